"""Host half of the device evaluation datasets (tokenhmr_amd/datasets.py) and of thmr_cropper_run_frames: the ABI surface, the refusals
(which need no device), the window rule against the warp's own source coordinates, and every non-image key of both datasets against
items the reference's ImageDataset / EMDBDataset produced (tests/golden/eval_dataset.npz, scripts/gen_golden_eval_dataset.py)."""
import ctypes as C
import os
import sys
import threading
import types

import numpy as np
import pytest
import torch

import _eval_dataset_fixture as F
from oracle import crop_oracle as CO


class RecordingCropper:
    """Stand-in for preprocess.Cropper on the host: records what it is asked for and returns zero crops."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.calls = []

    def warp_frames(self, frames, trans, sigmas=None, truncate=3.0, patch=256, mean=None, std=None, is_bgr=True, windows=True, out=None,
                    extra=None):
        self.calls.append({"n": len(frames), "shapes": [f.shape for f in frames], "trans": np.array(trans), "truncate": truncate,
                           "thread": threading.current_thread().name})
        img = torch.zeros(len(frames), 3, patch, patch)
        return img if extra is None else (img, torch.from_numpy(np.array(extra)))


def host_dataset(kind, tmp_path):
    ds = F.make_dataset(kind, tmp_path, "cpu", cropper=RecordingCropper())

    def no_meshes(batch, genders, joints24):
        n = len(genders)
        return torch.zeros(n, 6890, 3), (torch.zeros(n, 24, 3) if joints24 else None)

    ds._meshes = no_meshes
    return ds


def test_symbol_declared_bound_and_exported(built_lib):
    from tokenhmr_amd import _cabi
    assert _cabi.ABI_VERSION == 5 and built_lib.thmr_abi_version() == 5
    assert "thmr_cropper_run_frames" in _cabi.declared_symbols()
    # (exported and typed in both builds, like every declared function: tests/test_cabi_header.py)
    # the struct mirrors the header: 8 + 8 + 6*4 + 8*8
    assert C.sizeof(_cabi.FrameCrop) == 104 and _cabi.FrameCrop.M.offset == 40


def _one_item(lib, M, patch, H, W, win, sigma=0.0, truncate=3.0, ptr=4096, stride=None):
    """Calls the entry with a null cropper: every argument is checked before the handle, so the answer is the item's refusal or,
    for a valid item, 'null cropper' — no device is involved."""
    from tokenhmr_amd import _cabi
    it = (_cabi.FrameCrop * 1)()
    x0, y0, w, h = win
    it[0].win_dev, it[0].row_stride, it[0].H, it[0].W = ptr, (w * 3 if stride is None else stride), H, W
    it[0].win_x0, it[0].win_y0, it[0].win_w, it[0].win_h = x0, y0, w, h
    it[0].M[:] = np.asarray(M, dtype=np.float64).reshape(6).tolist()
    it[0].sigma, it[0].truncate = sigma, truncate
    one = (C.c_float * 3)(1, 1, 1)
    rc = lib.thmr_cropper_run_frames(None, it, 1, patch, 1, one, one, C.c_void_p(4096), None)
    return rc, lib.thmr_cropper_last_error(None).decode()


def test_entry_refuses_before_any_hip_call(built_lib):
    lib = built_lib
    rc = lib.thmr_cropper_run_frames(None, None, 0, 0, 0, None, None, None, None)
    assert rc != 0 and lib.thmr_cropper_last_error(None).decode() == "null buffer"
    M = CO.gen_trans_from_patch_cv(20, 20, 30, 30, 8, 8, 1.0, 0)
    assert _one_item(lib, M, 8, 48, 64, (0, 0, 64, 48))[1] == "null cropper"
    assert "does not lie inside the frame" in _one_item(lib, M, 8, 48, 64, (0, 0, 65, 48))[1]
    assert "does not lie inside the frame" in _one_item(lib, M, 8, 48, 64, (-1, 0, 64, 48))[1]
    assert "row_stride" in _one_item(lib, M, 8, 48, 64, (0, 0, 64, 48), stride=191)[1]
    assert "null window pointer" in _one_item(lib, M, 8, 48, 64, (0, 0, 64, 48), ptr=None)[1]
    assert "bad frame geometry" in _one_item(lib, M, 8, 0, 64, (0, 0, 0, 0))[1]
    assert "bad frame geometry" in _one_item(lib, M, 8, 48, 40000, (0, 0, 64, 48))[1]
    assert "non-finite affine" in _one_item(lib, np.full(6, np.inf), 8, 48, 64, (0, 0, 64, 48))[1]
    assert "sigma" in _one_item(lib, M, 8, 48, 64, (0, 0, 64, 48), sigma=-1.0)[1]
    rc, msg = _one_item(lib, M, 8, 48, 64, (0, 0, 10, 48))
    assert rc != 0 and msg.startswith("item 0: the window does not cover")
    # entirely outside: the box is empty, a null pointer and an empty window are fine
    Mo = CO.gen_trans_from_patch_cv(-500, -500, 30, 30, 8, 8, 1.0, 0)
    assert _one_item(lib, Mo, 8, 48, 64, (0, 0, 0, 0), ptr=None)[1] == "null cropper"
    # the blur radius int(truncate * sigma + 0.5) is compared in double before it is converted: 4096 is the largest, and a product
    # beyond int (or infinite) is a refusal like any other, not a conversion the weights are then sized from
    from tokenhmr_amd.preprocess import source_window
    full = (0, 0, 64, 48)
    for sigma, truncate in [(1e9, 3.0), (1e10, 3.0), (1e300, 3.0), (1.0, 1e300), (1e300, 1e300), (1366.0, 3.0)]:
        rc, msg = _one_item(lib, M, 8, 48, 64, full, sigma=sigma, truncate=truncate)
        assert rc != 0 and msg == "crop 0: blur radius too large", (sigma, truncate, msg)
        with pytest.raises(ValueError, match="blur radius too large"):
            source_window(M, 8, 48, 64, sigma, truncate)
    for sigma, truncate in [(1365.0, 3.0), (0.1, 3.0)]:          # radius 4095 and radius 0
        assert _one_item(lib, M, 8, 48, 64, full, sigma=sigma, truncate=truncate)[1] == "null cropper", (sigma, truncate)
        win = source_window(M, 8, 48, 64, sigma, truncate)
        assert win is not None and _one_item(lib, M, 8, 48, 64, win, sigma=sigma, truncate=truncate)[1] == "null cropper"
    assert source_window(M, 8, 48, 64, 1365.0, 3.0) == full and source_window(M, 8, 48, 64, 0.1, 3.0) == source_window(M, 8, 48, 64)


def _seeded_affines():
    rng = np.random.default_rng(4242)
    for t in range(200):
        H, W = int(rng.integers(5, 201)), int(rng.integers(7, 301))
        P = (8, 17, 256)[t % 3]
        box = P / rng.uniform(0.2, 8)
        where = t % 4                         # in | across an edge | outside | anywhere
        if where == 0:
            cx, cy = rng.uniform(0.3 * W, 0.7 * W), rng.uniform(0.3 * H, 0.7 * H)
        elif where == 1:
            cx, cy = rng.choice([0.0, W]) + rng.uniform(-2, 2), rng.choice([0.0, H]) + rng.uniform(-2, 2)
        elif where == 2:
            cx, cy = W + box + rng.uniform(2, 50), -box - rng.uniform(2, 50)
        else:
            cx, cy = rng.uniform(-box, W + box), rng.uniform(-box, H + box)
        rot = 0.0 if t % 2 else rng.uniform(-40, 40)
        sigma = rng.uniform(0.2, 2.5) if t % 5 == 0 else 0.0
        yield CO.gen_trans_from_patch_cv(cx, cy, box, box, P, P, 1.0, rot), P, H, W, sigma


def test_source_window_covers_the_sampled_texels(built_lib):
    """200 seeded affines: every in-frame texel the warp reads (oracle/crop_oracle.source_coords: sx, sx+1, sy, sy+1) lies inside
    source_window; blurred cases are wider by the kernel radius on every side, clipped; None exactly when no texel is in frame; and
    the C side holds the same rule: it accepts exactly this window and refuses it shrunk by one on any side."""
    from tokenhmr_amd.preprocess import source_window
    n_none = n_blur = 0
    for M, P, H, W, sigma in _seeded_affines():
        sx, sy, _, _ = CO.source_coords(M, (P, P))
        xs = np.concatenate([sx.ravel(), sx.ravel() + 1, sx.ravel(), sx.ravel() + 1])
        ys = np.concatenate([sy.ravel(), sy.ravel(), sy.ravel() + 1, sy.ravel() + 1])
        inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
        base = source_window(M, P, H, W)
        win = source_window(M, P, H, W, sigma, 3.0)
        assert (base is None) == (win is None)
        if not inside.any():
            # a crop that samples no texel may still get a (small) box: the rule is a bound, widened by one fixed-point step
            if base is None:
                n_none += 1
                assert _one_item(built_lib, M, P, H, W, (0, 0, 0, 0), sigma, ptr=None)[1] == "null cropper"
                continue
        else:
            assert base is not None
            x0, y0, w, h = base
            assert xs[inside].min() >= x0 and xs[inside].max() < x0 + w and ys[inside].min() >= y0 and ys[inside].max() < y0 + h
        if sigma > 0:
            n_blur += 1
            lw = int(3.0 * sigma + 0.5)
            x0, y0, w, h = base
            assert win == (max(x0 - lw, 0), max(y0 - lw, 0), min(x0 + w - 1 + lw, W - 1) - max(x0 - lw, 0) + 1,
                           min(y0 + h - 1 + lw, H - 1) - max(y0 - lw, 0) + 1)
        x0, y0, w, h = win
        assert _one_item(built_lib, M, P, H, W, win, sigma)[1] == "null cropper"
        for shrunk in ((x0 + 1, y0, w - 1, h), (x0, y0, w - 1, h), (x0, y0 + 1, w, h - 1), (x0, y0, w, h - 1)):
            assert _one_item(built_lib, M, P, H, W, shrunk, sigma)[1].startswith("item 0: the window does not cover"), (win, shrunk)
    assert n_none >= 20 and n_blur >= 20


def test_source_window_none_when_nothing_is_in_frame():
    """None <=> the warp reads no in-frame texel — exactly, except where the crop misses the frame by no more than the rule's own
    widening ([lo - 1, hi + 2]: up to 2 texels on an axis), where the box may be a sliver the warp never reads.  A window is never
    None while a texel is in frame (the safety direction, also held by the test above)."""
    from tokenhmr_amd.preprocess import source_window
    seen = {True: 0, False: 0}
    for M, P, H, W, _ in _seeded_affines():
        sx, sy, _, _ = CO.source_coords(M, (P, P))
        reads = (((sx + 1 >= 0) & (sx < W)) & ((sy + 1 >= 0) & (sy < H))).any()            # one of the four taps in frame
        near = (((sx + 3 >= 0) & (sx - 2 < W)) & ((sy + 3 >= 0) & (sy - 2 < H))).any()     # ... or within the widening of it
        win = source_window(M, P, H, W)
        if reads:
            assert win is not None
        elif not near:
            assert win is None
        if reads or not near:
            seen[bool(reads)] += 1
    assert seen[True] >= 50 and seen[False] >= 20, seen


@pytest.mark.parametrize("kind", ["image", "emdb", "bare"])
def test_host_half_matches_the_reference_items(kind, tmp_path, built_lib):
    _, meta = F.gold()
    ds = host_dataset(kind, tmp_path)
    n = meta["kinds"][kind]["n"]
    assert len(ds) == n
    skip = ()
    batch = ds.batch(range(n))
    inexact = F.check_host_keys(kind, list(range(n)), batch, skip)
    print(f"{kind}: keypoints_2d entries not bit-equal to the reference's: {inexact} of {n * 44 * 2}")
    # the crop the cropper was asked for: get_example's — one un-blurred crop per item, truncate 3.0, the frame of each item
    call = ds.cropper.calls[-1]
    g, _ = F.gold()
    fr = F.frames()
    assert call["n"] == n and call["truncate"] == 3.0
    assert call["shapes"] == [fr[str(nm)].shape for nm in g[f"in_{kind}/imgname"]]
    for i in range(n):
        r = F.ref_item(kind, i)
        M = CO.gen_trans_from_patch_cv(r["box_center"][0], r["box_center"][1], r["box_size"], r["box_size"], 256, 256, 1.0, 0)
        assert np.array_equal(call["trans"][i], M)
    # one item: the reference's keys, Python scalars where the reference has them
    it = ds[1]
    assert set(it) == set(batch) and isinstance(it["idx"], int) and it["idx"] == 1 and isinstance(it["imgname"], str)
    assert it["smpl_params_is_axis_angle"] == {"global_orient": True, "body_pose": True, "betas": False}
    assert torch.equal(it["keypoints_2d"], batch["keypoints_2d"][1])


def test_image_kind_rules(tmp_path, built_lib):
    g, _ = F.gold()
    img, emdb, bare = (host_dataset(k, tmp_path) for k in ("image", "emdb", "bare"))
    # scale / 200 for the image kind only, and the tiling to (n, 2)
    assert np.array_equal(img.scale, np.tile(g["in_image/scale"].reshape(-1, 1) / 200.0, (1, 2)))
    assert np.array_equal(emdb.scale, g["in_emdb/scale"])
    # the 3D confidences of body joints 1..14 are zeroed, the others kept
    k3 = img.keypoints_3d
    assert (k3[:, 1:15, -1] == 0).all() and np.array_equal(k3[:, 0, -1], g["in_image/body_keypoints_3d"][:, 0, -1].astype(np.float32))
    assert np.array_equal(k3[:, 15:25, -1], g["in_image/body_keypoints_3d"][:, 15:, -1].astype(np.float32))
    # gender parse and has_gender
    assert img.has_gender and img.gender.dtype == np.int32 and img.gender.tolist() == [0, 1, 0, 1, 1, 0]
    assert emdb.gender.tolist() == [1, 0, 1, 0]
    # the KeyError fallbacks: zeros for missing poses, betas and keypoints; no gender -> -1 and no vertices
    assert not bare.has_gender and bare.gender.tolist() == [-1, -1]
    assert bare.body_pose.shape == (2, 72) and not bare.body_pose.any() and not bare.has_body_pose.any()
    assert bare.betas.shape == (2, 10) and not bare.betas.any() and not bare.has_betas.any()
    assert bare.keypoints_2d.shape == (2, 44, 3) and bare.keypoints_2d.dtype == np.float32 and not bare.keypoints_2d.any()
    assert bare.keypoints_3d.shape == (2, 44, 4) and not bare.keypoints_3d.any()
    assert "vertices" not in bare.batch([0, 1])
    # EMDB keeps the file's float64 keypoints until the final astype
    assert emdb.keypoints_2d.dtype == np.float64 and emdb.batch([0])["keypoints_2d"].dtype == torch.float32
    assert emdb.batch([0])["orig_keypoints_2d"].dtype == torch.float64


def test_create_dataset_refusals_and_config(tmp_path):
    from tokenhmr_amd.datasets import create_dataset, dataset_eval_config
    cfg = F.model_cfg()
    with pytest.raises(NotImplementedError, match="train=True"):
        create_dataset(cfg, {"TYPE": "ImageDataset", "DATASET_FILE": "x", "IMG_DIR": "y"}, train=True)
    with pytest.raises(NotImplementedError, match="MoCapDataset"):
        create_dataset(cfg, {"TYPE": "MoCapDataset", "DATASET_FILE": "x"}, train=False)
    with pytest.raises(NotImplementedError, match="TYPE=None"):
        create_dataset(cfg, {"NPZ_FOLDER": "x"}, train=False)
    p = tmp_path / "datasets_eval.yaml"
    p.write_text("3DPW-TEST:\n    TYPE: ImageDataset\n    DATASET_FILE: 3dpw_test.npz\n    IMG_DIR: 3DPW/\n    KEYPOINT_LIST: [25, 26, 43]\n"
                 "    USE_HIPS: False\nEMDB:\n    TYPE: EMDBDataset\n    DATASET_FILE: EMDB/emdb.npz\n    IMG_DIR: EMDB\n    KEYPOINT_LIST: [0, 1]\n")
    dc = dataset_eval_config(str(p))
    assert dc["EMDB"].TYPE == "EMDBDataset" and dc["3DPW-TEST"].KEYPOINT_LIST == [25, 26, 43] and dc["3DPW-TEST"]["USE_HIPS"] is False
    assert "DATASET_FILE" in dc["EMDB"]
    # eval.py:61-64 edits the node in place, then hands it to create_dataset
    node = dc["3DPW-TEST"]
    node["DATASET_FILE"] = F.write_input("image", tmp_path)
    node["IMG_DIR"] = "imgs"
    ds = create_dataset(cfg, node, train=False, device="cpu", imread=F.imread, cropper=RecordingCropper())
    assert type(ds).__name__ == "ImageDataset" and len(ds) == 6 and ds.dataset_name == ""


def test_imread_fallback_order(tmp_path, monkeypatch):
    from tokenhmr_amd import datasets as DS
    from PIL import Image
    rgb = np.zeros((5, 7, 3), dtype=np.uint8)
    rgb[..., 0], rgb[..., 2] = 200, 30
    path = str(tmp_path / "a.png")
    Image.fromarray(rgb).save(path)
    # 1. cv2 where it imports: called with IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION
    seen = []
    fake = types.ModuleType("cv2")
    fake.IMREAD_COLOR, fake.IMREAD_IGNORE_ORIENTATION = 1, 128
    fake.imread = lambda p, flags: seen.append((p, flags)) or "cv2-frame"
    monkeypatch.setitem(sys.modules, "cv2", fake)
    assert DS.default_imread()(path) == "cv2-frame" and seen == [(path, 129)]
    # 2. PIL when cv2 does not import: RGB decoded, channel-reversed to BGR; an unreadable file gives None -> IOError in the dataset
    monkeypatch.setitem(sys.modules, "cv2", None)
    bgr = DS.default_imread()(path)
    assert bgr.dtype == np.uint8 and bgr.shape == (5, 7, 3) and bgr.flags.c_contiguous and np.array_equal(bgr, rgb[:, :, ::-1])
    assert DS.default_imread()(str(tmp_path / "missing.png")) is None
    ds = F.make_dataset("bare", tmp_path, "cpu", cropper=RecordingCropper())
    ds._imread = None
    with pytest.raises(IOError, match="Fail to read"):
        ds.read_frame(0)
    # 3. neither: ImportError naming both
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError, match="cv2.*PIL"):
        DS.default_imread()


def test_batches_keep_index_order_under_threads(tmp_path, built_lib):
    """ds.batches(4, num_workers=3) over 10 items: batches in index order, the last with 2 items, every item once, and no thread of
    the iterator alive afterwards — also when the consumer stops early."""
    g, _ = F.gold()
    arrays = {k.split("/", 1)[1]: g[k] for k in g if k.startswith("in_bare/")}
    names = ["f0.jpg", "f1.jpg", "f2.jpg", "f1.jpg", "f0.jpg", "f2.jpg", "f2.jpg", "f0.jpg", "f1.jpg", "f0.jpg"]
    rng = np.random.default_rng(3)
    path = os.path.join(str(tmp_path), "ten.npz")
    np.savez(path, imgname=np.array(names), center=rng.uniform(10, 40, size=(10, 2)), scale=rng.uniform(20, 60, size=10))
    from tokenhmr_amd.datasets import ImageDataset
    reads = []

    def slow_imread(p):
        reads.append((os.path.basename(p), threading.current_thread().name))
        return F.imread(p)

    before = set(threading.enumerate())
    crop = RecordingCropper()
    ds = ImageDataset(F.model_cfg(), path, "imgs", train=False, device="cpu", imread=slow_imread, cropper=crop)
    out = list(ds.batches(4, num_workers=3))
    assert [b["idx"].tolist() for b in out] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert [b["imgname_rel"] for b in out] == [names[0:4], names[4:8], names[8:10]]
    assert [c["n"] for c in crop.calls] == [4, 4, 2] and [r[0] for r in sorted(reads)] == sorted(names)
    assert all(t.startswith("thmr-decode") for _, t in reads) and len({t for _, t in reads}) <= 3
    assert set(threading.enumerate()) <= before, [t.name for t in set(threading.enumerate()) - before]
    # a consumer that stops after one batch: close() (or deletion) ends the producer and the decode threads
    it = ds.batches(2, num_workers=3, prefetch=1)
    assert next(it)["idx"].tolist() == [0, 1]
    it.close()
    assert set(threading.enumerate()) <= before
    # a decode error reaches the consumer, and the threads still end
    ds2 = ImageDataset(F.model_cfg(), path, "imgs", train=False, device="cpu", imread=lambda p: None, cropper=RecordingCropper())
    with pytest.raises(IOError, match="Fail to read"):
        list(ds2.batches(4, num_workers=2))
    assert set(threading.enumerate()) <= before
    # sharding of run_eval: a contiguous index range
    assert [b["idx"].tolist() for b in ds.batches(3, num_workers=1, start=3, stop=8)] == [[3, 4, 5], [6, 7]]
    with pytest.raises(NotImplementedError, match="shuffle"):
        ds.batches(4, shuffle=True)


def test_abandoned_iterator_and_failing_loop_leave_no_thread(tmp_path, built_lib):
    """The producer thread does not hold the iterator: one that is dropped without close() is collected and stops its threads; and
    run_eval closes the iterator when its loop ends by an exception (a failing model)."""
    import gc
    from tokenhmr_amd.eval_dp import run_eval
    before = set(threading.enumerate())
    ds = host_dataset("bare", tmp_path)
    it = ds.batches(1, num_workers=2, prefetch=1)
    assert next(it)["idx"].tolist() == [0]
    del it
    gc.collect()
    assert set(threading.enumerate()) <= before, [t.name for t in set(threading.enumerate()) - before]

    def failing_model(batch):
        raise RuntimeError("model failed")

    with pytest.raises(RuntimeError, match="model failed"):
        run_eval(failing_model, ds, lambda out, batch: None, batch_size=1, device="cpu", num_workers=2)
    assert set(threading.enumerate()) <= before, [t.name for t in set(threading.enumerate()) - before]


def test_smpl_constants_from_the_gendered_pickles(tmp_path):
    """Without smpl_male= / smpl_female= the constants come from SMPL.MODEL_PATH/SMPL_{MALE,FEMALE}.pkl through load_smpl_pkl, with the
    reference's '${SMPL.DATA_DIR}' -> '' replacement; SMPL.JOINT_REGRESSOR_EXTRA is optional (the meshes do not use it)."""
    import pickle
    from tokenhmr_amd.datasets import ImageDataset
    consts = F.smpl_constants()
    d = tmp_path / "smpl"
    d.mkdir()
    for name, c in (("SMPL_MALE.pkl", consts["male"]), ("SMPL_FEMALE.pkl", consts["female"])):
        kt = np.stack([np.array([2 ** 32 - 1] + [int(p) for p in c["parents"][1:]], dtype=np.uint32), np.arange(24, dtype=np.uint32)])
        with open(d / name, "wb") as f:
            pickle.dump({"v_template": c["v_template"].numpy(), "shapedirs": c["shapedirs"].numpy().astype(np.float64),
                         "posedirs": c["posedirs"].numpy().T.reshape(6890, 3, 207).astype(np.float64), "J_regressor": c["J_regressor"].numpy(),
                         "weights": c["lbs_weights"].numpy(), "kintree_table": kt, "f": np.zeros((13776, 3), dtype=np.uint32)}, f, protocol=2)
    with open(tmp_path / "j19.pkl", "wb") as f:
        pickle.dump(consts["male"]["J19_regressor"].numpy(), f, protocol=2)
    for with_j19 in (False, True):
        cfg = F.model_cfg()
        cfg.SMPL["MODEL_PATH"] = "${SMPL.DATA_DIR}" + str(d)
        if with_j19:
            cfg.SMPL["JOINT_REGRESSOR_EXTRA"] = "${SMPL.DATA_DIR}" + str(tmp_path / "j19.pkl")
        ds = ImageDataset(cfg, F.write_input("image", tmp_path), "imgs", device="cpu", imread=F.imread, cropper=RecordingCropper())
        for g, key in ((0, "male"), (1, "female")):
            got = ds.smpl_constants(g)
            for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "parents"):
                assert torch.equal(got[k], consts[key][k]), (key, k)
            assert got["J19_regressor"].shape == (19, 6890)
            assert torch.equal(got["J19_regressor"], consts["male"]["J19_regressor"]) if with_j19 else not got["J19_regressor"].any()
        assert ds.smpl_constants(0) is ds.smpl_constants(0)          # read once
