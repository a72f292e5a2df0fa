"""Inputs shared by tests/test_jpeg_enc_host.py and tests/test_gpu_jpeg_enc.py: the golden archive (scripts/gen_golden_jpeg_enc.py) and a
few procedural images."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_enc_small.npz")
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (24, 8), (12, 20), (33, 64), (100, 75)]        # (W, H)
QUALITIES = [1, 30, 50, 75, 90, 95, 100]
SUBSAMPLING = {"444": "4:4:4", "420": "4:2:0", "grey": "4:2:0"}          # a grey image ignores it
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2}


@functools.lru_cache(maxsize=None)
def golden():
    """({name: case dict}, {key: array})."""
    with np.load(GOLDEN) as z:
        arrays = {k: z[k] for k in z.files}
    return json.loads(arrays["cases"].tobytes().decode()), arrays


def golden_input(name):
    """The image a golden case encodes: (H, W, 3) RGB, or (H, W) for a grey case."""
    table, arrays = golden()
    rgb = arrays[table[name]["input"]]
    return np.ascontiguousarray(rgb[:, :, 1]) if table[name]["mode"] == "grey" else rgb


def golden_file(name):
    return golden()[1][name + ".jpg"].tobytes()


def picture(kind, w, h, c=3, seed=0):
    """(h, w, c) uint8, or (h, w) for c = 0."""
    y, x = np.mgrid[0:h, 0:w]
    n = max(c, 1)
    if kind == "noise":
        img = np.random.default_rng(7919 * w + 31 * h + seed).integers(0, 256, (h, w, n), dtype=np.uint8)
    elif kind == "checker":
        img = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], n, axis=-1)
    elif kind == "smooth":
        img = np.stack([(255 * x // max(w - 1, 1) + 40 * k) % 256 if k % 2 == 0 else 255 * y // max(h - 1, 1) for k in range(n)], axis=-1).astype(np.uint8)
        img[(x - 0.6 * w) ** 2 + (y - 0.4 * h) ** 2 < (0.3 * min(h, w)) ** 2] = [230, 30, 60, 200][:n]
    else:
        img = np.full((h, w, n), {"black": 0, "white": 255}[kind], np.uint8)
    return img[..., 0] if c == 0 else img


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else n)
