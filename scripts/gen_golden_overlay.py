"""Record the fixtures that pin tokenhmr_amd.render.MeshRenderer to the reference:

  tests/golden/openpose_calls.json      the cv2.line / cv2.circle calls render_openpose issues (through visualize_tensorboard's
                                        keypoint remap) for a set of skeletons, and the ground-truth arrays as the call leaves them
  tests/golden/mesh_renderer_scene.npz  the pyrender scenes MeshRenderer.__call__ / visualize build, in the camera frame

The reference's files are executed IN PLACE (nothing of them is copied) with recording stand-ins for cv2, pyrender, trimesh and
torchvision — none of which exists where this project runs.  tests/test_overlay_host.py imports this module for its live comparison.

    python scripts/gen_golden_overlay.py [--reference /path/to/tokenhmr] [--check]
"""
import argparse
import contextlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
CALLS_JSON = os.path.join(GOLDEN, "openpose_calls.json")
SCENE_NPZ = os.path.join(GOLDEN, "mesh_renderer_scene.npz")
DEFAULT_REF = "/root/reference/tokenhmr"


@contextlib.contextmanager
def reference_mesh_renderer(ref=DEFAULT_REF):
    """lib/utils/mesh_renderer.py and render_openpose.py executed in place.  Yields (module, log): log["scenes"] / ["viewports"] as
    tests/test_render_host.py records them, log["calls"] the cv2 draw calls, log["grids"] make_grid's arguments."""
    import torch
    import tests.test_render_host as TRH
    log = {"scenes": [], "viewports": [], "calls": [], "grids": []}
    stubs = TRH._stubs(log)
    cv2 = stubs["cv2"]
    plain = lambda p: [int(v) for v in p]
    cv2.line = lambda img, p1, p2, color, thickness, lineType=8, shift=0: log["calls"].append(
        ["line", plain(p1), plain(p2), [float(v) for v in color], int(thickness)])
    cv2.circle = lambda img, c, radius, color, thickness, lineType=8, shift=0: log["calls"].append(
        ["circle", plain(c), int(radius), [float(v) for v in color], int(thickness)])
    tv, tvu = types.ModuleType("torchvision"), types.ModuleType("torchvision.utils")

    def make_grid(tensors, nrow=8, padding=2):
        log["grids"].append(([t.clone() for t in tensors], nrow, padding))
        return torch.zeros(3, 1, 1)
    tvu.make_grid = make_grid
    tv.utils = tvu
    pkg = types.ModuleType("_ref_lib_utils")
    pkg.__path__ = [os.path.join(ref, "lib", "utils")]
    stubs.update({"torchvision": tv, "torchvision.utils": tvu, "_ref_lib_utils": pkg})
    saved = {k: sys.modules.get(k) for k in list(stubs) + ["_ref_lib_utils.render_openpose", "_ref_lib_utils.mesh_renderer"]}
    saved_env = os.environ.get("PYOPENGL_PLATFORM")
    had_int = hasattr(np, "int")
    sys.modules.update(stubs)
    if not had_int:
        np.int = int                       # the reference predates numpy 1.24
    try:
        path = os.path.join(ref, "lib", "utils", "mesh_renderer.py")
        spec = importlib.util.spec_from_file_location("_ref_lib_utils.mesh_renderer", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["_ref_lib_utils.mesh_renderer"] = mod
        spec.loader.exec_module(mod)
        yield mod, log
    finally:
        if not had_int:
            del np.int
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        if saved_env is None:
            os.environ.pop("PYOPENGL_PLATFORM", None)
        else:
            os.environ["PYOPENGL_PLATFORM"] = saved_env


# ------------------------------------------------------------------------------------------------ the skeleton cases
def _norm(px, res):
    return (np.asarray(px, np.float64) / res - 0.5).astype(np.float32)


def skeleton_cases():
    """name -> (kind 'pred' | 'gt', image size, keypoints): (44, 2) normalised for 'pred', (44, 3) with confidences for 'gt'."""
    rng = np.random.default_rng(20240611)
    cases = []
    for res in (256, 1024):
        cases.append((f"random_{res}", "pred", res, rng.uniform(-0.45, 0.45, (44, 2)).astype(np.float32)))
    # outside the image and negative pixel coordinates; body keypoint 0 lands on (-0.6, -0.6) px, which truncates toward zero to (0, 0)
    k = rng.uniform(-1.5, 1.5, (44, 2)).astype(np.float32)
    k[0] = _norm([-0.6, -0.6], 256)
    cases.append(("outside_negative_256", "pred", 256, k))
    # confidences on both sides of 0.1 (and of the remap's 0): body and extra keypoints drawn from a small set
    g = np.concatenate([rng.uniform(-0.4, 0.4, (44, 2)), rng.choice([0.0, 0.05, 0.1, 0.10000001, 0.11, 0.5, 1.0], (44, 1))], 1).astype(np.float32)
    cases.append(("confidences_256", "gt", 256, g))
    g = np.concatenate([rng.uniform(-0.4, 0.4, (44, 2)), rng.choice([0.0, 0.0, 0.09, 0.2, 1.0], (44, 1))], 1).astype(np.float32)
    cases.append(("confidences_1024", "gt", 1024, g))
    # a single valid keypoint, and valid keypoints on one line: a rectangle of zero area draws nothing
    g = np.concatenate([rng.uniform(-0.4, 0.4, (44, 2)), np.zeros((44, 1))], 1).astype(np.float32)
    g[3, 2] = 1.0
    cases.append(("single_keypoint_256", "gt", 256, g))
    g = np.concatenate([rng.uniform(-0.4, 0.4, (44, 2)), np.ones((44, 1))], 1).astype(np.float32)
    g[:, 1] = np.float32(0.125)
    cases.append(("collinear_256", "gt", 256, g))
    # a rectangle under 12.8 px wide and under 0.15 px tall with positive area: ratioAreas <= 0.05, the other thickness branch
    px = np.stack([rng.uniform(100.0, 110.0, 44), rng.uniform(100.0, 100.1, 44)], 1)
    g = np.concatenate([_norm(px, 256), np.ones((44, 1), np.float32)], 1).astype(np.float32)
    cases.append(("thin_rectangle_256", "gt", 256, g))
    # coordinates beyond +-16384 px (dropped by the contract, issued by the reference), a NaN under an invalid and under a valid keypoint
    k = rng.uniform(-0.4, 0.4, (44, 2)).astype(np.float32)
    k[4] = [100.0, 0.1]
    k[25 + 3] = [0.2, -90.0]               # lands on body keypoint 12 through the remap
    cases.append(("beyond_range_256", "pred", 256, k))
    g = np.concatenate([rng.uniform(-0.4, 0.4, (44, 2)), np.ones((44, 1))], 1).astype(np.float32)
    g[17] = [np.nan, 0.1, 0.0]
    cases.append(("nan_under_invalid_256", "gt", 256, g))
    g = g.copy()
    g[17, 2] = 1.0
    cases.append(("nan_under_valid_256", "gt", 256, g))
    return cases


def record_skeleton(mod, log, kind, res, keypoints):
    """One person through the reference's visualize_tensorboard with only this keypoint set; returns (calls, gt array afterwards)."""
    cfg = types.SimpleNamespace(EXTRA=types.SimpleNamespace(FOCAL_LENGTH=5000), MODEL=types.SimpleNamespace(IMAGE_SIZE=res))
    r = mod.MeshRenderer(cfg, faces=np.array([[0, 1, 2]]))
    verts = np.array([[[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0]]], np.float32)
    images = np.zeros((1, 3, res, res), np.float32)
    kp = np.array(keypoints, np.float32)[None].copy()
    del log["calls"][:]
    with np.errstate(invalid="ignore", over="ignore"), _quiet():
        r.visualize_tensorboard(verts, np.array([[0.0, 0.0, 30.0]]), images, kp if kind == "pred" else None, kp if kind == "gt" else None)
    return [list(c) for c in log["calls"]], kp[0]


@contextlib.contextmanager
def _quiet():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def record_calls(ref=DEFAULT_REF):
    out = []
    with reference_mesh_renderer(ref) as (mod, log):
        for name, kind, res, kp in skeleton_cases():
            calls, after = record_skeleton(mod, log, kind, res, kp)
            out.append({"name": name, "kind": kind, "res": res, "keypoints": _tolist(kp), "calls": calls,
                        "keypoints_after": _tolist(after) if kind == "gt" else None})
    return out


def _tolist(a):
    """float32 values as JSON numbers that read back to the same float32 (NaN as the string 'nan')."""
    return [[("nan" if np.isnan(v) else float(v)) for v in row] for row in np.asarray(a, np.float32)]


def fromlist(rows):
    return np.array([[np.nan if v == "nan" else v for v in row] for row in rows], np.float32)


# ------------------------------------------------------------------------------------------------ the scenes
def scene_inputs():
    rng = np.random.default_rng(9)
    return {"verts": rng.normal(0, 0.4, (2, 50, 3)).astype(np.float32), "faces": rng.integers(0, 50, (30, 3)),
            "cam_t": np.array([[0.12, -0.3, 41.0], [-0.25, 0.2, 37.5]]), "width": 240, "height": 200, "res": 256,
            "focal": 1234.5, "base": np.array([0.2, 0.5, 0.9, 1.0]), "rot_angle": 60.0}


def record_scenes(ref=DEFAULT_REF):
    """The reference's scenes for __call__ (front; side with rot_angle and baseColorFactor) on a 240 x 200 image, and for visualize
    on two people (front then side on the same camera_translation row), reduced to the camera frame."""
    import tests.test_render_host as TRH
    inp = scene_inputs()
    out = dict(inp)
    H, W = inp["height"], inp["width"]
    cfg = types.SimpleNamespace(EXTRA=types.SimpleNamespace(FOCAL_LENGTH=5000), MODEL=types.SimpleNamespace(IMAGE_SIZE=inp["res"]))

    def capture(scene, tag):
        cam, verts, lights = TRH._captured(scene)
        out[tag + "_verts"] = verts[0]
        out[tag + "_intrinsics"] = np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float64)
        out[tag + "_light_kind"] = np.array([k for k, *_ in lights])
        out[tag + "_light_vec"] = np.array([v for _, v, _, _ in lights])
        out[tag + "_light_color"] = np.array([c for _, _, c, _ in lights], np.float64)
        out[tag + "_light_intensity"] = np.array([i for *_, i in lights], np.float64)
        m = scene.meshes[0].material
        out[tag + "_material"] = np.array([m.metallicFactor, float(hasattr(m, "roughnessFactor"))] + list(m.baseColorFactor), np.float64)
        out[tag + "_bg_ambient"] = np.array(list(scene.bg_color) + list(scene.ambient_light), np.float64)

    with reference_mesh_renderer(ref) as (mod, log):
        r = mod.MeshRenderer(cfg, faces=inp["faces"])
        img = np.zeros((H, W, 3), np.float32)
        t = inp["cam_t"][0].copy()
        r(inp["verts"][0], t, img, focal_length=inp["focal"])
        capture(log["scenes"][-1], "front")
        out["front_viewport"] = np.array(log["viewports"][-1])
        out["front_t_after"] = t.copy()
        t = inp["cam_t"][0].copy()
        r(inp["verts"][0], t, img, focal_length=inp["focal"], side_view=True, baseColorFactor=tuple(inp["base"]), rot_angle=inp["rot_angle"])
        capture(log["scenes"][-1], "side")
        out["side_viewport"] = np.array(log["viewports"][-1])
        n0 = len(log["scenes"])
        t2 = inp["cam_t"].copy()
        images = np.zeros((2, 3, inp["res"], inp["res"]), np.float32)
        r.visualize(inp["verts"], t2, images, focal_length=777.0)
        for k, s in enumerate(log["scenes"][n0:]):
            capture(s, f"seq{k}")                      # person 0 front, person 0 side, person 1 front, person 1 side
        out["seq_viewport"] = np.array(log["viewports"][-1])
        out["seq_t_after"] = t2
        out["seq_grid"] = np.array([len(log["grids"][-1][0]), log["grids"][-1][1], log["grids"][-1][2]])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=DEFAULT_REF, help="the reference's tokenhmr/ directory")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing them")
    a = ap.parse_args()
    calls, scenes = record_calls(a.reference), record_scenes(a.reference)
    if a.check:
        with open(CALLS_JSON) as f:
            assert json.load(f) == calls, "openpose_calls.json differs from the reference run"
        old = np.load(SCENE_NPZ)
        assert sorted(old.files) == sorted(scenes) and all(np.array_equal(old[k], scenes[k]) for k in scenes), "mesh_renderer_scene.npz differs"
        print("fixtures match the reference run")
        return
    with open(CALLS_JSON, "w") as f:
        json.dump(calls, f, separators=(",", ":"))
    np.savez_compressed(SCENE_NPZ, **scenes)
    for c in calls:
        print(f"{c['name']:26s} {c['kind']:4s} {c['res']:5d} px  {len(c['calls']):2d} calls")
    print(f"wrote {CALLS_JSON} ({os.path.getsize(CALLS_JSON)} B) and {SCENE_NPZ} ({os.path.getsize(SCENE_NPZ)} B)")


if __name__ == "__main__":
    main()
