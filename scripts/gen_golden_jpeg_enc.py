"""Writes tests/golden/jpeg_enc_small.npz: small input images and the JPEG files Pillow (libjpeg-turbo) writes for them.

    python scripts/gen_golden_jpeg_enc.py        # needs Pillow; the stored file was made with Pillow 12.2 / libjpeg-turbo 3.1

`in.KIND.WxH` is an (H, W, 3) uint8 RGB input (a grey case encodes its green channel); `NAME.jpg` the bytes of
Image.fromarray(input).save(format="JPEG", quality=q, subsampling=0 | 2) — baseline, Annex-K Huffman tables, no optimisation; `cases` a
JSON table NAME -> {input, width, height, kind, mode ("444", "420", "grey"), quality}; `versions` the Pillow and libjpeg-turbo versions
that wrote the files.  The images are procedural and small on purpose.  Sizes (W x H): 1x1, 7x9, 8x8, 16x16, 17x23 (a dummy luma column
and row in 4:2:0), 24x8 and 12x20 (the last chroma row is replicated: H even, no multiple of 16), 33x64, 100x75 (odd chroma width).
Every size x mode has a smooth and a noise image at two of the qualities 1 / 30 / 50 / 75 / 90 / 95 / 100 (the qualities rotate, so that each
meets every mode), a 0 / 255 checkerboard at q 100 (the largest DC and AC categories, the densest 0xFF stuffing) and an all-black and
an all-white image; 17x23 and 100x75 have noise at every quality.
"""
import io
import json
import os

import numpy as np
import PIL
from PIL import Image, features

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_enc_small.npz")
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (24, 8), (12, 20), (33, 64), (100, 75)]        # (W, H)
QUALITIES = [1, 30, 50, 75, 90, 95, 100]
MODES = ["444", "420", "grey"]
KINDS = ["smooth", "noise", "black", "white", "checker"]


def picture(kind, w, h):
    """(h, w, 3) uint8 RGB."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "smooth":
        img = np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 255 * (x + y) / max(w + h - 2, 1)], axis=-1)
        disc = (x - 0.6 * w) ** 2 + (y - 0.4 * h) ** 2 < (0.3 * min(h, w)) ** 2
        img[disc] = (230, 30, 60)
        return np.rint(img).astype(np.uint8)
    if kind == "checker":
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    return np.full((h, w, 3), 0 if kind == "black" else 255, np.uint8)


def cases():
    """[(name, kind, (w, h), mode, quality)]"""
    out = []
    for si, (w, h) in enumerate(SIZES):
        for mi, mode in enumerate(MODES):
            i = si * len(MODES) + mi
            picks = [("smooth", QUALITIES[i % 7]), ("noise", QUALITIES[(i + 3) % 7]), ("checker", 100), ("black", QUALITIES[(i + 1) % 7]), ("white", QUALITIES[(i + 5) % 7])]
            if (w, h) in ((17, 23), (100, 75)):
                picks += [("noise", q) for q in QUALITIES if q != QUALITIES[(i + 3) % 7]]
            out += [(f"{kind}_{w}x{h}_{mode}_q{q}", kind, (w, h), mode, q) for kind, q in picks]
    return out


def pillow_file(rgb, mode, quality):
    buf = io.BytesIO()
    if mode == "grey":
        Image.fromarray(np.ascontiguousarray(rgb[:, :, 1])).save(buf, "JPEG", quality=quality)
    else:
        Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling={"444": 0, "420": 2}[mode])
    return buf.getvalue()


def main():
    arrays, table = {}, {}
    for name, kind, (w, h), mode, q in cases():
        key = f"in.{kind}.{w}x{h}"
        if key not in arrays:
            arrays[key] = picture(kind, w, h)
        arrays[name + ".jpg"] = np.frombuffer(pillow_file(arrays[key], mode, q), dtype=np.uint8)
        table[name] = {"input": key, "width": w, "height": h, "kind": kind, "mode": mode, "quality": q}
    arrays["cases"] = np.frombuffer(json.dumps(table, indent=0).encode(), dtype=np.uint8)
    arrays["versions"] = np.array([PIL.__version__, str(features.version_feature("libjpeg_turbo"))])
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(table)} cases")


if __name__ == "__main__":
    main()
