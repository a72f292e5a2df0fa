"""The device half of the evaluation datasets on the MI355X: thmr_cropper_run_frames against thmr_cropper_run item by item (bit-equal),
windows against whole frames, both datasets against the items the reference's code produced (tests/golden/eval_dataset.npz), and
run_eval over the drop-ins against the hand-written loop over the reference's items."""
import ctypes as C

import numpy as np
import pytest
import torch

import _eval_dataset_fixture as F
from oracle import crop_oracle as CO

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def crop_items():
    """(frame name, cx, cy, box, sigma): the six boxes of the fixture's image kind (inside, over the top-left corner on the same
    frame, over the bottom-right corner, entirely outside, 8x up-sampling, inside the smallest frame) and two blurred items: a 230 px
    box on the 200x150 frame, f = 230 / 64 > 1.1 -> sigma = (f - 1) / 2 = 1.297, kernel radius 4, region clipped on all four sides."""
    g, _ = F.gold()
    items = []
    for i in range(6):
        r = F.ref_item("image", i)
        items.append((str(g["in_image/imgname"][i]), float(r["box_center"][0]), float(r["box_center"][1]), float(r["box_size"]), 0.0))
    f = 230.0 / 64
    assert f > 1.1
    items.append(("f2.jpg", 100.0, 75.0, 230.0, (f - 1) / 2))
    # a second blurred item whose window lies STRICTLY inside its frame (non-zero window origin, window smaller than the frame in the
    # blur's rows pass): a 90 px box at (120, 80) on the 200x150 frame; at patch 64 this is f = box / patch = 1.41 > 1.1 as it stands
    f = 90.0 / 64
    assert f > 1.1
    items.append(("f2.jpg", 120.0, 80.0, 90.0, (f - 1) / 2))
    return items


INNER = 7          # index of the blurred item with an interior window


def affines(items, P):
    return np.stack([CO.gen_trans_from_patch_cv(cx, cy, b, b, P, P, 1.0, 0) for _, cx, cy, b, _ in items])


@pytest.fixture(scope="module")
def cropper(built_lib, cuda_dev):
    from tokenhmr_amd.preprocess import Cropper
    c = Cropper(cuda_dev)
    yield c
    c.close()


@pytest.mark.parametrize("P", [256, 64, 17, 8])
def test_frames_call_equals_single_frame_call(P, cropper, built_lib, cuda_dev):
    """Item i of thmr_cropper_run_frames is bit-equal to thmr_cropper_run on that item's frame alone; n = 1, 7 and 8; patch 256, 64
    (the blurred items' own patch), 17 (289 pixels: a ragged last workgroup) and 8 (less than one workgroup).  First whole frames as
    windows, the 181-wide frame with its rows padded to 576 bytes; then every item with exactly its source_window, each in a buffer of
    its own with rows padded by 13 bytes, so that window origin, window size and stride all differ from the frame's."""
    from tokenhmr_amd.preprocess import source_window
    from tokenhmr_amd import _cabi
    fr = F.frames()
    dev = {}
    for name, a in fr.items():
        H, W = a.shape[:2]
        stride = 576 if W == 181 else W * 3
        t = torch.full((H, stride), 255, dtype=torch.uint8, device=cuda_dev)
        t[:, :W * 3] = torch.from_numpy(a.reshape(H, W * 3)).to(cuda_dev)
        dev[name] = (t, stride)
    items = crop_items()
    T = affines(items, P)
    m = (C.c_float * 3)(*[np.float32(255.0 * v) for v in MEAN])
    s = (C.c_float * 3)(*[np.float32(255.0 * v) for v in STD])
    border = [(np.float32(0) - np.float32(255.0 * MEAN[c])) / np.float32(255.0 * STD[c]) for c in range(3)]
    single = [cropper.warp(fr[it[0]], T[i:i + 1], [it[4]], truncate=3.0, patch=P, mean=MEAN, std=STD)[0] for i, it in enumerate(items)]
    for sel in ([6], [INNER], list(range(7)), list(range(8))):
        n = len(sel)
        descs = (_cabi.FrameCrop * n)()
        for k, i in enumerate(sel):
            name, _, _, _, sigma = items[i]
            H, W = fr[name].shape[:2]
            d = descs[k]
            d.win_dev, d.row_stride, d.H, d.W = dev[name][0].data_ptr(), dev[name][1], H, W
            d.win_x0, d.win_y0, d.win_w, d.win_h = 0, 0, W, H
            d.M[:] = T[i].reshape(6).tolist()
            d.sigma, d.truncate = sigma, 3.0
        out = torch.full((n, 3, P, P), -7.0, device=cuda_dev)
        rc = built_lib.thmr_cropper_run_frames(cropper.h, descs, n, P, 1, m, s, C.c_void_p(out.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream(cuda_dev).cuda_stream))
        assert rc == 0, built_lib.thmr_cropper_last_error(cropper.h).decode()
        torch.cuda.synchronize()
        for k, i in enumerate(sel):
            assert torch.equal(out[k], single[i]), (P, n, i)
            name, cx, cy, b, sigma = items[i]
            if sigma == 0:
                ref = CO.example_item(fr[name], cx, cy, b, b, patch=P, mean=MEAN, std=STD)["img"]
                assert np.array_equal(out[k].cpu().numpy(), ref), (P, n, i)
            if i == 3:          # entirely outside the frame: (0 - mean) / std everywhere
                for c in range(3):
                    assert (out[k, c] == float(border[c])).all()
    # exact windows, own buffers, padded rows
    n = len(items)
    descs, keep = (_cabi.FrameCrop * n)(), []
    for i, (name, _, _, _, sigma) in enumerate(items):
        H, W = fr[name].shape[:2]
        win = source_window(T[i], P, H, W, sigma, 3.0)
        d = descs[i]
        d.H, d.W, d.sigma, d.truncate = H, W, sigma, 3.0
        d.M[:] = T[i].reshape(6).tolist()
        if win is None:
            assert i == 3
            continue
        x0, y0, w, h = win
        if i == INNER:
            assert x0 > 0 and y0 > 0 and x0 + w < W and y0 + h < H, win
        t = torch.full((h, w * 3 + 13), 255, dtype=torch.uint8, device=cuda_dev)
        t[:, :w * 3] = torch.from_numpy(np.ascontiguousarray(fr[name][y0:y0 + h, x0:x0 + w]).reshape(h, w * 3)).to(cuda_dev)
        keep.append(t)
        d.win_dev, d.row_stride = t.data_ptr(), w * 3 + 13
        d.win_x0, d.win_y0, d.win_w, d.win_h = x0, y0, w, h
    out = torch.full((n, 3, P, P), -7.0, device=cuda_dev)
    rc = built_lib.thmr_cropper_run_frames(cropper.h, descs, n, P, 1, m, s, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream(cuda_dev).cuda_stream))
    assert rc == 0, built_lib.thmr_cropper_last_error(cropper.h).decode()
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(out[i], single[i]), (P, "windows", i)


def test_windows_equal_whole_frames(cropper, cuda_dev):
    from tokenhmr_amd import _cabi
    from tokenhmr_amd.preprocess import source_window
    fr = F.frames()
    items = crop_items()
    frames = [fr[it[0]] for it in items]
    sig = [it[4] for it in items]
    for P in (256, 64, 17):
        T = affines(items, P)
        whole = cropper.warp_frames(frames, T, sig, truncate=3.0, patch=P, windows=False)
        b_whole = cropper.last_staged_bytes
        win = cropper.warp_frames(frames, T, sig, truncate=3.0, patch=P, windows=True)
        b_win = cropper.last_staged_bytes
        again = cropper.warp_frames(frames, T, sig, truncate=3.0, patch=P, windows=True)         # the other staging set
        third = cropper.warp_frames(frames, T, sig, truncate=3.0, patch=P, windows=True)         # the first set, reused
        assert torch.equal(win, whole) and torch.equal(again, win) and torch.equal(third, win)
        assert 0 < b_win < b_whole, (b_win, b_whole)
        print(f"patch {P}: staged bytes whole frames {b_whole}, windows {b_win}")
        # the same object three times / twice: whole frames are staged once each (3 frames, 256-byte aligned)
        assert b_whole == sum((f.size + 255) & ~255 for f in fr.values())
    # a window shrunk by one column is refused with the item's index before any launch: the output keeps its sentinel
    P = 256
    T = affines(items, P)
    wins = [source_window(T[i], P, frames[i].shape[0], frames[i].shape[1], sig[i], 3.0) for i in range(len(items))]
    assert wins[3] is None and all(w is not None for i, w in enumerate(wins) if i != 3)
    x0, y0, w, h = wins[INNER]
    assert x0 > 0 and y0 > 0 and x0 + w < 200 and y0 + h < 150, wins[INNER]
    for k in (2, 6, INNER):
        bad = list(wins)
        x0, y0, w, h = bad[k]
        bad[k] = (x0, y0, w - 1, h)
        out = torch.full((len(items), 3, P, P), -7.0, device=cuda_dev)
        with pytest.raises(_cabi.EngineError, match=f"item {k}: the window does not cover"):
            cropper.warp_frames(frames, T, sig, truncate=3.0, patch=P, windows=bad, out=out)
        torch.cuda.synchronize()
        assert (out == -7.0).all()
    # and the exact windows given explicitly are accepted
    ref = cropper.warp_frames(frames, T, sig, truncate=3.0, patch=P, windows=False)
    assert torch.equal(cropper.warp_frames(frames, T, sig, truncate=3.0, patch=P, windows=wins), ref)


def _vertex_bound():
    g, _ = F.gold()
    return max(2e-6, 2 * float(g["d_ref"]))


@pytest.mark.parametrize("kind", ["image", "emdb"])
def test_batches_match_reference_items(kind, tmp_path, built_lib, cuda_dev):
    from tokenhmr_amd.smpl import SMPL
    g, meta = F.gold()
    ds = F.make_dataset(kind, tmp_path, cuda_dev)
    n = meta["kinds"][kind]["n"]
    bound = _vertex_bound()
    consts = F.smpl_constants()
    direct = {0: SMPL(consts["male"], max_batch=64, device=cuda_dev), 1: SMPL(consts["female"], max_batch=64, device=cuda_dev)}
    seen = []
    for batch in ds.batches(4, num_workers=2):
        idxs = batch["idx"].tolist()
        seen += idxs
        assert all(t.device == cuda_dev for t in F.flat(batch).values() if torch.is_tensor(t))
        inexact = F.check_host_keys(kind, idxs, batch)
        print(f"{kind} {idxs}: keypoints_2d entries not bit-equal: {inexact}")
        refs = [F.ref_item(kind, i) for i in idxs]
        assert batch["img"].dtype == torch.float32 and batch["img"].shape == (len(idxs), 3, 256, 256)
        assert np.array_equal(batch["img"][:, :, ::4, ::4].cpu().numpy(), np.stack([r["img"] for r in refs]))
        v = batch["vertices"]
        assert v.dtype == torch.float32 and v.shape == (len(idxs), 6890, 3)
        d = np.linalg.norm(v[:, ::10].cpu().numpy().astype(np.float64) - np.stack([r["vertices"] for r in refs]), axis=-1).max()
        print(f"{kind} {idxs}: vertices vs the reference's fp32 CPU model: {d:.3e} m (bound {bound:.3e})")
        assert d <= bound
        # the parent's path, one call per gender group: the partition and the index_copy_ are what is under test
        gender = ds.gender[idxs]
        sp = batch["smpl_params"]
        for gg in (0, 1):
            rows = torch.as_tensor(np.nonzero((gender == 1) if gg == 1 else (gender != 1))[0], device=cuda_dev)
            if len(rows):
                want = direct[gg](sp["global_orient"][rows], sp["body_pose"][rows], sp["betas"][rows]).vertices
                assert torch.equal(v[rows], want), (kind, idxs, gg)
        if kind == "emdb":
            k3 = batch["keypoints_3d"]
            assert k3.dtype == torch.float32 and k3.shape == (len(idxs), 24, 3)
            v64 = v.cpu().numpy().astype(np.float64)
            for r, gi in enumerate(gender):
                J = consts["female" if gi == 1 else "male"]["J_regressor"].numpy().astype(np.float64)
                d3 = np.linalg.norm(k3[r].cpu().numpy() - J @ v64[r], axis=-1).max()
                dr = np.linalg.norm(k3[r].cpu().numpy().astype(np.float64) - refs[r]["keypoints_3d"], axis=-1).max()
                assert d3 <= bound and dr <= bound, (d3, dr)
    assert seen == list(range(n))
    for m in direct.values():
        m.close()


KP = [25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 43]      # 3DPW-TEST keypoint list (datasets_eval.yaml:12)


@pytest.fixture(scope="module")
def tiny_model(built_lib, cuda_dev):
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.model import TokenHMR
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    return TokenHMR.from_state(cfg, W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0),
                               max_batch=16, device=cuda_dev)


@pytest.mark.parametrize("kind", ["image", "emdb"])
def test_eval_loop_over_device_datasets(kind, tmp_path, tiny_model, cuda_dev):
    """run_eval over the drop-in (7 items: the fixture's, the first ones repeated; batch_size 4) against the hand loop over batches
    collated from the reference's items (img: the restated crop, which the generator holds bit-equal to the reference's on the full
    grid; keypoints_3d: the fixture's; vertices: the stand-in's fp32 CPU model run here, within the vertex bound of the fixture at every 10th
    vertex)."""
    import os
    from oracle import tokenhmr_oracle as O
    from tokenhmr_amd.datasets import create_dataset
    from tokenhmr_amd.evaluator import Evaluator
    from tokenhmr_amd.eval_dp import run_eval, recursive_to
    g, meta = F.gold()
    n0 = meta["kinds"][kind]["n"]
    order = (list(range(n0)) + list(range(n0)))[:7]
    arrays = {k.split("/", 1)[1]: g[k][order] for k in g if k.startswith(f"in_{kind}/")}
    path = os.path.join(str(tmp_path), "seven.npz")
    np.savez(path, **arrays)
    consts = F.smpl_constants()
    ds = create_dataset(F.model_cfg(), {"TYPE": "EMDBDataset" if kind == "emdb" else "ImageDataset", "DATASET_FILE": path, "IMG_DIR": "imgs"},
                        train=False, device=cuda_dev, imread=F.imread, smpl_male=consts["male"], smpl_female=consts["female"])
    assert len(ds) == 7
    fr = F.frames()
    ref = []
    for i in order:
        r = F.ref_item(kind, i)
        img = CO.example_item(fr[str(g[f"in_{kind}/imgname"][i])], r["box_center"][0], r["box_center"][1], r["box_size"], r["box_size"])["img"]
        assert np.array_equal(img[:, ::4, ::4], r["img"])
        c = consts["female" if ds.gender[order.index(i)] == 1 else "male"]
        with torch.no_grad():
            v, _ = O.smpl_forward_axis_angle(torch.from_numpy(r["smpl_params.global_orient"])[None], torch.from_numpy(r["smpl_params.body_pose"])[None],
                                             torch.from_numpy(r["smpl_params.betas"])[None], c)
        # the same fp32 CPU model as the generator's stand-in; its rounding depends on the host's CPU kernels, so not bit for bit
        assert np.linalg.norm(v[0, ::10].numpy().astype(np.float64) - r["vertices"], axis=-1).max() <= _vertex_bound()
        ref.append({"img": torch.from_numpy(img), "keypoints_3d": torch.from_numpy(r["keypoints_3d"]), "vertices": v[0],
                    "imgname": str(r["imgname"])})

    def make_ev():
        if kind == "emdb":
            return Evaluator(int(1e6), list(range(24)), 0, metrics=["mode_re", "mode_mpjpe", "mode_pve"], dataset="EMDB",
                             J_regressor_24_SMPL=consts["male"]["J_regressor"].to(cuda_dev))
        return Evaluator(int(1e6), KP, 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], dataset="3DPW-TEST")

    ev_a, ev_m = make_ev(), make_ev()
    a = run_eval(tiny_model, ds, ev_a, batch_size=4, device=cuda_dev, num_workers=2)
    for s in range(0, 7, 4):
        part = ref[s:s + 4]
        batch = recursive_to({"img": torch.stack([p["img"] for p in part]), "keypoints_3d": torch.stack([p["keypoints_3d"] for p in part]),
                              "vertices": torch.stack([p["vertices"] for p in part]), "imgname": [p["imgname"] for p in part]}, cuda_dev)
        with torch.no_grad():
            ev_m(tiny_model(batch), batch)
    m = ev_m.get_metrics_dict()
    assert ev_a.counter == 7 and ev_a.get_imgnames() == ev_m.get_imgnames() == [p["imgname"] for p in ref]
    for k in m:
        print(f"{kind} {k}: drop-in {a[k]!r}  reference items {m[k]!r}  |diff| {abs(a[k] - m[k]):.3e} mm")
    for k in m:
        if kind == "image" and k != "mode_pve":
            assert a[k] == m[k], (k, a[k], m[k])                  # same image bits, same ground-truth keypoints -> same bits
        else:
            assert abs(a[k] - m[k]) < 1e-3, (k, a[k], m[k])      # ground truth from the device mesh: regime differences, 1e-3 mm
    assert np.isfinite(list(m.values())).all() and m["mode_mpjpe"] > 0
    # a consumer that holds batch k while batch k+1 is produced still sees batch k unchanged
    it = ds.batches(4, num_workers=2, prefetch=1)
    first = next(it)
    keep = {k: v.clone() for k, v in F.flat(first).items() if torch.is_tensor(v)}
    second = next(it)
    torch.cuda.synchronize()
    assert second["idx"].tolist() == [4, 5, 6]
    with pytest.raises(StopIteration):
        next(it)
    torch.cuda.synchronize()
    for k, v in F.flat(first).items():
        if torch.is_tensor(v):
            assert torch.equal(v, keep[k]), k
