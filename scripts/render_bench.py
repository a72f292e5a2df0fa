"""Time of the GPU mesh renderer (tokenhmr_amd.render, csrc/render.hip), HIP events around the device work of one call:
64 crops at 256x256 (4 samples, composited over the crops), one crop, and a 1920x1080 frame holding 8 people.  The meshes are
closed ellipsoids with SMPL's 6890 vertices / 13,776 faces, randomly rotated, framed as demo.py frames a crop.
    python scripts/render_bench.py [--steps K] [--warmup W]      -> one JSON line per case
    python scripts/render_bench.py --sheet                       -> MeshRenderer.visualize_tensorboard (eval.py --render's contact sheet)
                                                                    at 8 and 64 people beside the two RGBA renders it contains, timed alone
                                                                    in the same process; appended to profiles/eval_sheet_bench.jsonl"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests.render_numpy import uv_sphere
from tokenhmr_amd import _cabi
from tokenhmr_amd.render import MeshRenderer, Renderer, cam_crop_to_full, side_translation


class N(dict):
    __getattr__ = dict.__getitem__


def _rot(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(steps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def sheet_cases(cfg, faces, verts, cam_t, dev, steps, warmup):
    """visualize_tensorboard on device tensors (two RGBA renders + the draw-list builder + the sheet kernel), and the two renders alone."""
    rng = np.random.default_rng(1)
    mr = MeshRenderer(cfg, faces, device=dev)
    out = []
    for B in (8, 64):
        v, t = verts[:B].contiguous(), cam_t[:B].contiguous()
        imgs = torch.rand(B, 3, 256, 256, device=dev)
        pred = torch.tensor(rng.uniform(-0.45, 0.45, (B, 44, 2)), dtype=torch.float32, device=dev)
        gt0 = torch.tensor(np.c_[rng.uniform(-0.45, 0.45, (B * 44, 2)), rng.choice([0.0, 1.0], B * 44)].reshape(B, 44, 3), dtype=torch.float32, device=dev)
        gt = gt0.clone()
        front, side = mr.scene(256, 256, mr.focal_length), mr.scene(256, 256, mr.focal_length, side_view=True)

        def sheet():
            gt.copy_(gt0)                  # the call scales the ground truth in place: start every call from the same values (a 4 B x 132 B copy)
            return mr.visualize_tensorboard(v, t, imgs, pred, gt)

        def renders():
            mr.renderer._run(front, v, t, _cabi.RENDER_PER_IMAGE, 4)
            mr.renderer._run(side, v, side_translation(t), _cabi.RENDER_PER_IMAGE, 4)

        # interleaved: renders, sheet, renders — the two render timings bracket the sheet's
        r0, s0, r1 = _time(renders, steps, warmup), _time(sheet, steps, warmup), _time(renders, steps, warmup)
        rm = 0.5 * (r0[0] + r1[0])
        out.append({"case": f"contact sheet, {B} people, 256x256, 4 samples, 5 tiles per person", "sheet_median_ms": s0[0], "sheet_min_ms": s0[1],
                    "two_renders_median_ms": [r0[0], r1[0]], "two_renders_min_ms": [r0[1], r1[1]],
                    "sheet_over_renders": s0[0] / rm, "skeleton_and_assembly_ms": s0[0] - rm, "build": mr.renderer.lib.thmr_build_info().decode()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sheet", action="store_true", help="time MeshRenderer.visualize_tensorboard instead; appends to profiles/eval_sheet_bench.jsonl")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = N(EXTRA=N(FOCAL_LENGTH=5000), MODEL=N(IMAGE_SIZE=256, IMAGE_MEAN=[0.485, 0.456, 0.406], IMAGE_STD=[0.229, 0.224, 0.225]))
    v, f = uv_sphere(84, 83, 1.0)
    v = v * np.array([0.25, 0.8, 0.18])
    rng = np.random.default_rng(0)
    B = 64
    verts = torch.tensor(np.einsum("bij,vj->bvi", _rot(rng, B), v), dtype=torch.float32, device=dev)
    cam_t = torch.tensor(np.c_[rng.uniform(-0.2, 0.2, (B, 2)), np.full(B, 2 * 5000 / (256 * 0.9))], dtype=torch.float32, device=dev)
    imgs = torch.randn(B, 3, 256, 256, device=dev)
    if args.sheet:
        out = sheet_cases(cfg, f, verts, cam_t, dev, args.steps, args.warmup)
        with open(os.path.join(ROOT, "profiles", "eval_sheet_bench.jsonl"), "a") as fh:
            for o in out:
                o.update(steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
                print(json.dumps(o))
                fh.write(json.dumps(o) + "\n")
        return
    r = Renderer(cfg, f, device=dev)
    out = []
    ms = _time(lambda: r.render_batch(verts, cam_t, imgs), args.steps, args.warmup)
    out.append({"case": "64 crops 256x256, 4 samples, composited", "median_ms": ms[0], "min_ms": ms[1]})
    ms = _time(lambda: r.render_batch(verts[:1], cam_t[:1], imgs[:1]), args.steps, args.warmup)
    out.append({"case": "1 crop 256x256, 4 samples, composited", "median_ms": ms[0], "min_ms": ms[1]})
    n = 8
    cols, rows = np.arange(n) % 4, np.arange(n) // 4
    centers = torch.tensor(np.stack([240 + 480 * cols, 270 + 540 * rows], 1), dtype=torch.float32)
    cam = torch.tensor(np.c_[np.full(n, 0.9), rng.uniform(-0.1, 0.1, (n, 2))], dtype=torch.float32)
    focal = 5000 / 256 * 1920
    full_t = cam_crop_to_full(cam, centers, torch.full((n,), 400.0), torch.tensor([[1920.0, 1080.0]]).repeat(n, 1), focal).to(dev)
    ms = _time(lambda: r.render_scene(verts[:n], full_t, 1920, 1080, focal), args.steps, args.warmup)
    out.append({"case": "full frame 1920x1080, 8 people, 4 samples", "median_ms": ms[0], "min_ms": ms[1]})
    for o in out:
        o.update(steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
        print(json.dumps(o))


if __name__ == "__main__":
    main()
