"""The images of the PNG encoder's tests (tests/test_png_host.py, tests/test_gpu_png.py), generated from seeded NumPy generators, and the
host encoder's files for them, computed once per session."""
import functools

import numpy as np

SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (17, 33), (64, 64), (256, 192)]
KINDS = ["noise", "gradient", "flat", "render"]


def image(kind, h, w, c, seed=0):
    """(H, W, C) uint8."""
    rng = np.random.default_rng([seed, h, w, c])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(3 * x + 5 * y + 40 * k) & 255 for k in range(c)], axis=-1).astype(np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 31, 96, 255][:c], np.uint8), (h, w, c)).copy()
    assert kind == "render"
    # a white ground, a shaded disc, and a noisy "photographic" right half
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w, c), 255.0)
    r = np.hypot(x - 0.3 * w, y - 0.5 * h) / max(1.0, 0.22 * min(h, 2 * w))
    shade = np.clip(1.0 - r * r, 0.0, 1.0) ** 0.5
    for k in range(min(c, 3)):
        img[..., k] = np.where(r < 1.0, (60 + 50 * k) * shade + 30, img[..., k])
    photo = 128 + 60 * np.sin(x / 9.0)[..., None] * np.cos(y / 7.0)[..., None] + rng.normal(0, 12, (h, w, c))
    half = x >= w // 2
    img[half] = photo[half]
    if c == 4:
        img[..., 3] = 255
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def edge_shapes(S):
    """Grey (H, W) whose filtered size H * (1 + W) is exactly S - 1, S, S + 1, 2 S and 2 S + 1: H the largest factor up to 256."""
    out = []
    for n in (S - 1, S, S + 1, 2 * S, 2 * S + 1):
        h = max(k for k in range(1, 257) if n % k == 0 and n // k >= 2)
        out.append((h, n // h - 1))
        assert out[-1][0] * (1 + out[-1][1]) == n
    return out


def edge_image(kind, h, w):
    rng = np.random.default_rng([7, h, w])
    if kind == "constant":                     # one run across every segment boundary, far longer than 258
        return np.full((h, w, 1), 0, np.uint8)
    if kind in ("period2", "period3"):         # matches at a distance of whole rows
        k = int(kind[-1])
        rows = rng.integers(0, 256, (k, w, 1), dtype=np.uint8)
        return rows[np.arange(h) % k]
    assert kind == "noise"                     # incompressible: the stored fallback
    return rng.integers(0, 256, (h, w, 1), dtype=np.uint8)


EDGE_KINDS = ["constant", "period2", "period3", "noise"]


def roundtrip_cases():
    return [(f"{kind}-{h}x{w}x{c}", image(kind, h, w, c)) for (h, w) in SHAPES for c in (1, 3, 4) for kind in KINDS]


def edge_cases(S):
    return [(f"{kind}-{h}x{w}", edge_image(kind, h, w)) for (h, w) in edge_shapes(S) for kind in EDGE_KINDS]


def conversion_values():
    """float32 values whose conversion has an edge: halves, just outside the range, huge, infinite, NaN."""
    v = [k + 0.5 for k in range(255)] + [-0.6, -0.4, 255.4, 255.5, 256.0, 1e9, -1e9, np.inf, -np.inf, np.nan]
    return np.array(v, np.float32)


def convert_expected(v, scale, rounding):
    """v float32 -> uint8 as the contract states it: the product in fp32, then rint-and-clamp or clip-and-truncate; NaN -> 0."""
    p = (v.astype(np.float32) * np.float32(scale)).astype(np.float32)
    p = np.where(np.isnan(p), np.float32(0), p)
    if rounding == "nearest":
        return np.clip(np.rint(p), 0, 255).astype(np.uint8)
    return np.clip(p, 0, 255).astype(np.uint8)


def conversion_cases():
    """(name, float image (1, N, 1), scale, rounding)."""
    out = []
    for rounding in ("nearest", "trunc"):
        out.append((f"edges-{rounding}", conversion_values().reshape(1, -1, 1), 1.0, rounding))
        out.append((f"k255-{rounding}", (np.arange(256, dtype=np.float32) / np.float32(255)).reshape(1, -1, 1), 255.0, rounding))
    return out


def stride_cases():
    """(name, strided view, kwargs): each must give the file of np.ascontiguousarray(view)."""
    rng = np.random.default_rng(11)
    chw = rng.random((3, 20, 37), dtype=np.float32)
    sheet = image("render", 40, 120, 3)
    sheet4 = image("noise", 9, 50, 4)
    return [("chw-float", chw.transpose(1, 2, 0), dict(scale=255.0, rounding="trunc", bgr=False)),
            ("panel-of-sheet", sheet[5:33, 31:90, :], dict(bgr=True)),
            ("panel-of-sheet-rgba", sheet4[:, 7:30, :], dict(bgr=False)),
            ("grey-2d-slice", sheet[::2, 3:77, 1], dict())]


@functools.lru_cache(maxsize=None)
def host_file(group, name):
    """The host encoder's file of one named case, computed once."""
    from tokenhmr_amd import png as P
    S = P.segment_bytes()
    if group == "roundtrip":
        return P.encode_host(dict(roundtrip_cases())[name], bgr=False)
    if group == "edge":
        return P.encode_host(dict(edge_cases(S))[name], bgr=False)
    if group == "conversion":
        _, img, scale, rounding = next(c for c in conversion_cases() if c[0] == name)
        return P.encode_host(img, scale=scale, rounding=rounding)
    _, view, kw = next(c for c in stride_cases() if c[0] == name)
    return P.encode_host(view, **kw)
