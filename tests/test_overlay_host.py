"""MeshRenderer's contract on the CPU (not-gpu): the draw list of the restatement (tests/overlay_numpy.py) pinned to the calls the
reference's render_openpose issues (tests/golden/openpose_calls.json, and live against the reference executed in place where it is
present); MeshRenderer's scene pinned to lib/utils/mesh_renderer.py (tests/golden/mesh_renderer_scene.npz, and live); the stated
coverage of a line and a circle on analytic cases; make_grid's geometry; argument checks that need no device."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import tests.test_render_host as TRH
from tests import overlay_numpy as ON

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(TRH.REF, "lib", "utils", "mesh_renderer.py")),
                               reason="reference tree not present (GPU box)")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_golden_overlay", os.path.join(ROOT, "scripts", "gen_golden_overlay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixture_cases():
    with open(os.path.join(GOLDEN, "openpose_calls.json")) as f:
        cases = json.load(f)
    nan = lambda rows: np.array([[np.nan if v == "nan" else v for v in row] for row in rows], np.float32)
    for c in cases:
        c["keypoints"] = nan(c["keypoints"])
        if c["keypoints_after"] is not None:
            c["keypoints_after"] = nan(c["keypoints_after"])
    return cases


def restated(case):
    """(records, keypoints as the call leaves them) of the restatement for one fixture case."""
    kp = case["keypoints"].copy()
    body = ON.body_from_pred(kp, case["res"]) if case["kind"] == "pred" else ON.body_from_gt(kp, case["res"])
    return ON.build_records(body, case["res"], case["res"]), kp


# ------------------------------------------------------------------------------------------------ 1. the draw list
def test_mesh_renderer_is_importable_and_has_the_reference_interface():
    import inspect
    from tokenhmr_amd.render import MeshRenderer
    assert list(inspect.signature(MeshRenderer.__call__).parameters)[1:] == [
        "vertices", "camera_translation", "image", "focal_length", "text", "resize", "side_view", "baseColorFactor", "rot_angle"]
    assert list(inspect.signature(MeshRenderer.visualize).parameters)[1:] == [
        "vertices", "camera_translation", "images", "focal_length", "nrow", "padding"]
    assert list(inspect.signature(MeshRenderer.visualize_tensorboard).parameters)[1:] == [
        "vertices", "camera_translation", "images", "pred_keypoints", "gt_keypoints", "focal_length", "nrow", "padding"]
    assert list(inspect.signature(MeshRenderer.__init__).parameters)[1:3] == ["cfg", "faces"]
    sig = inspect.signature(MeshRenderer.visualize_tensorboard).parameters
    assert sig["nrow"].default == 5 and sig["padding"].default == 2 and inspect.signature(MeshRenderer.visualize).parameters["nrow"].default == 3


def test_draw_list_reproduces_the_recorded_reference_calls():
    cases = fixture_cases()
    names = {c["name"] for c in cases}
    assert {"random_256", "random_1024", "outside_negative_256", "confidences_256", "single_keypoint_256", "collinear_256",
            "thin_rectangle_256", "beyond_range_256"} <= names
    for c in cases:
        rec, after = restated(c)
        assert ON.calls_of(rec) == ON.calls_in_range(c["calls"]), c["name"]
        if c["kind"] == "gt":
            np.testing.assert_array_equal(after, c["keypoints_after"], err_msg=c["name"])      # scaled and remapped in place
        else:
            np.testing.assert_array_equal(after, c["keypoints"])                               # predictions: the caller's array is untouched
    by = {c["name"]: c for c in cases}
    assert len(by["single_keypoint_256"]["calls"]) == 0 and len(by["collinear_256"]["calls"]) == 0 and len(by["nan_under_valid_256"]["calls"]) == 0
    assert len(by["random_256"]["calls"]) == len(by["random_1024"]["calls"]) == 49
    # the usual branch: line thickness 2, circle radius 1 / thickness 2; the ratioAreas <= 0.05 branch: circle thickness 1
    assert {(c[0], c[-1]) for c in by["random_1024"]["calls"]} == {("line", 2), ("circle", 2)}
    assert {(c[0], c[-1]) for c in by["thin_rectangle_256"]["calls"]} == {("line", 2), ("circle", 1)}
    assert {c[2] for c in by["thin_rectangle_256"]["calls"] if c[0] == "circle"} == {1}
    # truncation toward zero: (-0.6, -0.6) px is drawn at (0, 0); the contract drops what lies beyond +-16384 px, and only that
    assert ["circle", [0, 0], 1, [255.0, 0.0, 85.0], 2] in by["outside_negative_256"]["calls"]
    dropped = [k for k in by["beyond_range_256"]["calls"] if k not in ON.calls_in_range(by["beyond_range_256"]["calls"])]
    assert 0 < len(dropped) < 10 and all(max(abs(v) for v in k[1] + (k[2] if k[0] == "line" else [])) > ON.RANGE for k in dropped)
    # confidences on both sides of 0.1 appear among the drawn and the undrawn keypoints
    conf = by["confidences_256"]["keypoints_after"][:25, 2]
    assert (conf > np.float32(0.1)).any() and (conf <= np.float32(0.1)).any() and 0 < len(by["confidences_256"]["calls"]) < 49


def test_tables_are_openpose_body_25():
    assert ON.LIMBS.shape == (24, 2) and ON.PALETTE.shape == (25, 3) and len(ON.MATCHES) == 14
    assert sorted(a for a, _ in ON.MATCHES) == list(range(1, 15)) and sorted(b for _, b in ON.MATCHES) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14]


@needs_ref
def test_draw_list_matches_the_reference_executed_in_place():
    gen = _generator()
    cases = fixture_cases()
    with gen.reference_mesh_renderer(TRH.REF) as (mod, log):
        for c in cases:
            calls, after = gen.record_skeleton(mod, log, c["kind"], c["res"], c["keypoints"])
            assert calls == c["calls"], c["name"]                       # the committed fixture is what the reference does today
            rec, ours_after = restated(c)
            assert ON.calls_of(rec) == ON.calls_in_range(calls), c["name"]
            np.testing.assert_array_equal(ours_after, after if c["kind"] == "gt" else c["keypoints"])
        # skeletons the fixture does not hold
        rng = np.random.default_rng(77)
        for k in range(20):
            res = (256, 1024, 640)[k % 3]
            kp = np.concatenate([rng.uniform(-0.8, 0.8, (44, 2)), rng.choice([0.0, 0.05, 0.3, 1.0], (44, 1))], 1).astype(np.float32)
            kind = "gt" if k % 2 else "pred"
            case = {"kind": kind, "res": res, "keypoints": kp[:, :2].copy() if kind == "pred" else kp}
            calls, after = gen.record_skeleton(mod, log, kind, res, case["keypoints"])
            rec, ours_after = restated(case)
            assert ON.calls_of(rec) == ON.calls_in_range(calls)
            if kind == "gt":
                np.testing.assert_array_equal(ours_after, after)


# ------------------------------------------------------------------------------------------------ 2. the scene
def _check_scene(R, sc, ours_verts, g, tag, viewport, base):
    cam = TRH._Rec(**dict(zip(("fx", "fy", "cx", "cy"), g[tag + "_intrinsics"])))
    lights = list(zip(g[tag + "_light_kind"], g[tag + "_light_vec"], g[tag + "_light_color"], g[tag + "_light_intensity"]))
    TRH._assert_scene_matches(sc, cam, [g[tag + "_verts"]], lights, [ours_verts], tuple(int(v) for v in viewport))     # rtol 1e-6, as A1
    metallic, has_roughness, *colour = g[tag + "_material"]
    assert metallic == sc["metallic"] == 0.0 and not has_roughness and sc["roughness"] == 1.0      # pyrender's default roughness
    assert tuple(colour) == (*sc["base_color"], 1.0) == (*base, 1.0)
    assert tuple(g[tag + "_bg_ambient"]) == (*sc["bg"], 0.0, *sc["ambient"]) == (0, 0, 0, 0, 0.3, 0.3, 0.3)
    assert len(lights) == 3 and all(k == 0 for k, *_ in lights)                                    # ambient 0.3 + the three Raymond lights


def _scene_checks(g):
    from tokenhmr_amd import render as R
    mr = R.MeshRenderer(TRH._Ns(EXTRA=TRH._Ns(FOCAL_LENGTH=5000), MODEL=TRH._Ns(IMAGE_SIZE=int(g["res"]))), faces=g["faces"])
    W, H, t0 = int(g["width"]), int(g["height"]), g["cam_t"][0]
    # __call__, front: intrinsics of the image passed in, the focal length passed in, the caller's x negated in place
    sc = mr.scene(W, H, float(g["focal"]))
    _check_scene(R, sc, R.camera_frame_vertices(sc, g["verts"][0], t0), g, "front", g["front_viewport"], (1.0, 1.0, 0.9))
    np.testing.assert_array_equal(g["front_t_after"], t0 * [-1, 1, 1])
    # __call__, side view with its own angle and colour
    sc = mr.scene(W, H, float(g["focal"]), True, float(g["rot_angle"]), tuple(g["base"]))
    _check_scene(R, sc, R.camera_frame_vertices(sc, g["verts"][0], t0), g, "side", g["side_viewport"], tuple(g["base"][:3]))
    # visualize: front then side on the same camera_translation row — the side view sees x un-flipped, the array comes back restored,
    # the focal length argument is ignored in favour of cfg.EXTRA.FOCAL_LENGTH
    res = int(g["res"])
    for person in range(2):
        t = g["cam_t"][person]
        front, side = mr.scene(res, res, mr.focal_length), mr.scene(res, res, mr.focal_length, side_view=True)
        _check_scene(R, front, R.camera_frame_vertices(front, g["verts"][person], t), g, f"seq{2 * person}", g["seq_viewport"], (1.0, 1.0, 0.9))
        ts = R.side_translation(t)
        np.testing.assert_array_equal(ts, [-t[0], t[1], t[2]])
        _check_scene(R, side, R.camera_frame_vertices(side, g["verts"][person], ts), g, f"seq{2 * person + 1}", g["seq_viewport"], (1.0, 1.0, 0.9))
        assert g[f"seq{2 * person}_intrinsics"][0] == 5000 == mr.focal_length
        # the flipped translation would NOT match: the quirk is observable
        wrong = R.camera_frame_vertices(side, g["verts"][person], t)
        assert np.abs(wrong - g[f"seq{2 * person + 1}_verts"]).max() > 0.1
    np.testing.assert_array_equal(g["seq_t_after"], g["cam_t"])
    assert tuple(g["seq_grid"]) == (6, 3, 2)
    assert torch.equal(R.side_translation(torch.tensor([[1.0, 2.0, 3.0]])), torch.tensor([[-1.0, 2.0, 3.0]]))


def test_scene_matches_the_recorded_reference_scene():
    _scene_checks(dict(np.load(os.path.join(GOLDEN, "mesh_renderer_scene.npz"))))


@needs_ref
def test_scene_matches_the_reference_executed_in_place():
    live = _generator().record_scenes(TRH.REF)
    golden = dict(np.load(os.path.join(GOLDEN, "mesh_renderer_scene.npz")))
    assert sorted(live) == sorted(golden)
    for k in live:
        np.testing.assert_array_equal(np.asarray(live[k]), golden[k], err_msg=k)
    _scene_checks({k: np.asarray(v) for k, v in live.items()})


# ------------------------------------------------------------------------------------------------ 3. coverage
def _covered(rec, W=32, H=24):
    idx = ON.coverage_map(np.asarray(rec).reshape(-1, ON.N_WORDS), W, H)
    ys, xs = np.nonzero(idx >= 0)
    return set(zip(xs.tolist(), ys.tolist())), idx


def test_horizontal_line_of_thickness_2_is_a_capsule():
    pix, _ = _covered(ON.prim_record(ON.KIND_LINE, (10, 10), (20, 10), 0, 2, 0, 32, 24))
    expect = {(x, y) for x in range(10, 21) for y in (9, 10, 11)} | {(9, 10), (21, 10)}
    assert pix == expect and len(pix) == 35


def test_circles_cover_the_stated_rings():
    pix, _ = _covered(ON.prim_record(ON.KIND_CIRCLE, (15, 12), (15, 12), 1, 2, 0, 32, 24))
    assert pix == {(15 + dx, 12 + dy) for dx in range(-3, 4) for dy in range(-3, 4) if dx * dx + dy * dy <= 4} and len(pix) == 13
    pix, _ = _covered(ON.prim_record(ON.KIND_CIRCLE, (15, 12), (15, 12), 1, 1, 0, 32, 24))
    assert pix == {(15 + dx, 12 + dy) for dx in range(-2, 3) for dy in range(-2, 3) if dx * dx + dy * dy in (1, 2)} and len(pix) == 8
    assert (15, 12) not in pix
    pix, _ = _covered(ON.prim_record(ON.KIND_CIRCLE, (15, 12), (15, 12), 3, -1, 0, 32, 24))
    assert pix == {(15 + dx, 12 + dy) for dx in range(-4, 5) for dy in range(-4, 5) if dx * dx + dy * dy <= 9}


def test_slanted_and_degenerate_lines():
    pix, _ = _covered(ON.prim_record(ON.KIND_LINE, (4, 4), (12, 12), 0, 2, 0, 32, 24))
    # distance to the diagonal is |dx - dy| / sqrt 2 <= 1: the diagonal and its two neighbours, plus the cap pixels within 1 of an end
    assert {(k, k) for k in range(4, 13)} <= pix and (5, 4) in pix and (4, 6) not in pix and (3, 4) in pix and (3, 3) not in pix
    pix, _ = _covered(ON.prim_record(ON.KIND_LINE, (7, 7), (7, 7), 0, 2, 0, 32, 24))
    assert pix == {(7, 7), (6, 7), (8, 7), (7, 6), (7, 8)}                      # a == b: the disc of radius t / 2


def test_later_primitives_overwrite_and_outside_ones_change_nothing():
    a = ON.prim_record(ON.KIND_LINE, (2, 5), (20, 5), 0, 2, 3, 32, 24)
    b = ON.prim_record(ON.KIND_CIRCLE, (10, 5), (10, 5), 1, 2, 7, 32, 24)
    _, ab = _covered([a, b])
    _, ba = _covered([b, a])
    assert ab[5, 10] == 7 and ba[5, 10] == 3 and ab[5, 3] == 3 and ab[3, 10] == 7 and ba[3, 10] == 7
    far = [ON.prim_record(ON.KIND_LINE, (-300, -20), (-40, -9), 0, 2, 1, 32, 24), ON.prim_record(ON.KIND_CIRCLE, (40, 30), (40, 30), 1, 2, 1, 32, 24),
           ON.prim_record(ON.KIND_LINE, (16384, 16384), (16000, 16384), 0, 2, 1, 32, 24)]
    _, with_far = _covered([a] + far + [b])
    assert np.array_equal(with_far, ab)
    img = np.random.default_rng(0).random((3, 24, 32), dtype=np.float32)
    panel = ON.skeleton_panel(img, np.stack(far))
    assert np.array_equal(panel, (np.float32(255) * img) / np.float32(255)) and panel.dtype == np.float32
    drawn = ON.skeleton_panel(img, np.stack([a, b]))
    assert np.array_equal(drawn[:, 5, 10], (ON.PALETTE[7] / 255).astype(np.float32)) and np.array_equal(drawn[:, 0, 0], panel[:, 0, 0])


def test_coverage_at_the_range_bound_matches_python_integers():
    """Both ends at the +-16384 bound: the int64 formulation equals the same predicate in unbounded Python integers (4 cross^2 <= t^2 |ab|^2,
    which itself would pass 2^63 here)."""
    a, b, t = (-16384, -16384), (16384, 16380), 2
    pts = [(0, 0), (0, -2), (1, 0), (8191, 8189), (8191, 8191), (8191, 0), (0, 8191), (4096, 4095), (4096, 4097), (100, 101), (7, 5)]

    def exact(px, py):
        dx, dy, wx, wy = b[0] - a[0], b[1] - a[1], px - a[0], py - a[1]
        len2, dot = dx * dx + dy * dy, wx * dx + wy * dy
        if dot <= 0:
            return 4 * (wx * wx + wy * wy) <= t * t
        if dot >= len2:
            return 4 * ((px - b[0]) ** 2 + (py - b[1]) ** 2) <= t * t
        return 4 * (wx * dy - wy * dx) ** 2 <= t * t * len2
    got = ON.covers(ON.KIND_LINE, a[0], a[1], b[0], b[1], 0, t, np.array([p[0] for p in pts]), np.array([p[1] for p in pts]))
    assert got.tolist() == [exact(*p) for p in pts] and got.any() and not got.all()
    worst = 4 * ((8191 + 16384) * 32768 + (8191 + 16384) * 32768) ** 2
    assert worst > 2 ** 63 > worst // 4                            # why the kernel compares cross^2 with (t^2 |ab|^2) >> 2


# ------------------------------------------------------------------------------------------------ 4. the grid
@pytest.mark.parametrize("n,nrow,panels", [(3, 3, 3), (24, 3, 3), (40, 5, 5), (32, 4, 4), (24, 3, 3)])
def test_grid_geometry(n, nrow, panels):
    from tokenhmr_amd import render as R
    H, W, pad = 256, 256, 2
    xmaps, ymaps, Hg, Wg = R.sheet_geometry(n, nrow, pad, H, W)
    assert (xmaps, ymaps) == (min(nrow, n), -(-n // min(nrow, n)))
    assert (Hg, Wg) == (ymaps * 258 + 2, xmaps * 258 + 2) == ON.grid_geometry(n, nrow, pad, H, W)[:2]
    origins = ON.grid_geometry(n, nrow, pad, H, W)[2]
    assert origins[0] == (2, 2) and origins[-1] == (2 + ((n - 1) // xmaps) * 258, 2 + ((n - 1) % xmaps) * 258)
    tiles = [np.full((3, 8, 8), k + 1, np.float32) for k in range(n)]
    grid = ON.make_grid(tiles, nrow, pad)
    hg, wg, org = ON.grid_geometry(n, nrow, pad, 8, 8)
    assert grid.shape == (3, hg, wg)
    mask = np.zeros((hg, wg), bool)
    for k, (r, c) in enumerate(org):
        assert (grid[:, r:r + 8, c:c + 8] == k + 1).all()
        mask[r:r + 8, c:c + 8] = True
    assert (grid[:, ~mask] == 0).all() and (~mask).sum() == hg * wg - 64 * n        # padding is exactly 0


def test_nrow_shrinks_with_each_missing_keypoint_set():
    """visualize_tensorboard on 8 people: 5, 4, 4 and 3 tiles per person and row (both sets None: the (24, 3) sheet of visualize)."""
    from tokenhmr_amd import render as R
    for pred, gt, per in ((1, 1, 5), (1, 0, 4), (0, 1, 4), (0, 0, 3)):
        nrow = 5 - (not gt) - (not pred)
        assert R.sheet_geometry(8 * per, nrow, 2, 256, 256) == (per, 8, 8 * 258 + 2, per * 258 + 2)


# ------------------------------------------------------------------------------------------------ 5. arguments
def test_mesh_renderer_has_no_cpu_fallback():
    from tokenhmr_amd.render import MeshRenderer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MeshRenderer(TRH.CFG, np.zeros((1, 3), np.int64), device="cpu")


def test_bad_arguments_are_rejected_before_device_work(built_lib):
    from tokenhmr_amd import render as R
    faces = np.array([[0, 1, 2], [1, 2, 3]])
    mr = R.MeshRenderer(TRH.CFG, faces)                        # no device work until a call passes its checks
    v, t = np.zeros((2, 4, 3), np.float32), np.zeros((2, 3), np.float32)
    img = np.zeros((2, 3, 16, 16), np.float32)
    pred, gt = np.zeros((2, 44, 2), np.float32), np.zeros((2, 44, 3), np.float32)
    with pytest.raises(NotImplementedError, match="cv2.resize"):
        mr(v[0], t[0].copy(), np.zeros((16, 16, 3), np.float32), resize=(8, 8))
    with pytest.raises(ValueError):
        mr(v[0], t[0].copy(), np.zeros((3, 16, 16), np.float32))                    # CHW, not the reference's HWC
    with pytest.raises(ValueError):
        mr.visualize_tensorboard(v, t, img, pred[:, :25], gt)                       # wrong keypoint count
    with pytest.raises(ValueError):
        mr.visualize_tensorboard(v, t, img, pred, gt[:, :, :2])
    with pytest.raises(ValueError):
        mr.visualize_tensorboard(v, t, img, pred, gt.astype(np.int32))
    with pytest.raises(ValueError):
        mr.visualize(v, t, img[:1])
    with pytest.raises(ValueError):
        mr.visualize(v, t[:, :2], img)
    with pytest.raises(ValueError):
        mr.visualize(v[:, :3], t, img)                                              # the faces index vertex 3
    with pytest.raises(ValueError):
        mr.visualize(v, t, img, nrow=0)
    with pytest.raises(ValueError, match="every argument"):
        mr.visualize(torch.zeros(2, 4, 3), t, img)                                  # tensors and arrays mixed
    with pytest.raises(ValueError, match="every argument"):
        mr.visualize(torch.zeros(2, 4, 3), torch.zeros(2, 3), torch.zeros(2, 3, 16, 16))    # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="without faces"):
        R.MeshRenderer(TRH.CFG).visualize(v, t, img)                                # faces=None constructs, as in the reference
    assert not mr.renderer._handles and np.array_equal(gt, np.zeros((2, 44, 3), np.float32))
    # the C ABI validates too, before it touches a device
    L = built_lib
    import ctypes as C
    from tokenhmr_amd import _cabi
    assert "thmr_renderer_sheet" in _cabi.declared_symbols()
    d = _cabi.SheetDesc(1, 16, 16, 256, 7, 3, 2, 56, 20)
    one = C.c_void_p(16)
    assert L.thmr_renderer_sheet(None, C.byref(d), one, one, one, None, None, None, one, None) < 0
    assert b"null renderer" in L.thmr_renderer_last_error(None)
