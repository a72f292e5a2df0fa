"""Writes tests/golden/jpeg_small.npz: small JPEG files and the pixels Pillow (libjpeg-turbo) decodes from them.

    python scripts/gen_golden_jpeg.py            # needs Pillow; the stored file was made with Pillow 12.2 / libjpeg-turbo 3.1

Each case NAME has `NAME.jpg` (the file's bytes, uint8) and, where the decoder supports the file, `NAME.rgb` ((H, W, 3) uint8:
Image.open(...).convert('RGB'), i.e. libjpeg's default pipeline — JDCT_ISLOW, fancy upsampling, fixed-point YCbCr -> RGB).  `cases` is a
JSON table of what each file is: size, sampling, quality, and why it is there.  The images are procedural (seeded noise over gradients
and discs), small on purpose, and cover: 4:4:4 / 4:2:2 / 4:2:0 / grey; q 50 / 90 / 100 (q 100 on noise forces 0xFF00 stuffing);
optimize=True (non-default Huffman tables); restart intervals in MCU rows and in MCUs; sides that are no multiple of 8 or 16; chroma
planes at most 2 samples wide (where libjpeg replicates instead of interpolating); a progressive and a CMYK file for the refusals.
"""
import io
import json
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_small.npz")
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def picture(h, w, seed, noise):
    """Gradients, a disc and an edge, plus uniform noise of amplitude `noise`: smooth parts, sharp chroma edges and busy parts."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 255 * (x + y) / max(w + h - 2, 1)], axis=-1)
    disc = (x - 0.6 * w) ** 2 + (y - 0.4 * h) ** 2 < (0.3 * min(h, w)) ** 2
    img[disc] = (230, 30, 60)
    img[:, : w // 3][y[:, : w // 3] > 0.7 * h] = (10, 200, 240)
    img += g.uniform(-noise, noise, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# name, (H, W), mode, sampling, quality, extra save arguments, noise amplitude
CASES = [
    ("c420_1x1_q90", (1, 1), "RGB", "420", 90, {}, 0),
    ("c444_1x1_q90", (1, 1), "RGB", "444", 90, {}, 0),
    ("c420_3x4_q90", (3, 4), "RGB", "420", 90, {}, 40),
    ("c422_2x5_q90", (2, 5), "RGB", "422", 90, {}, 40),
    ("c420_8x8_q90", (8, 8), "RGB", "420", 90, {}, 40),
    ("c444_8x8_q100_noise", (8, 8), "RGB", "444", 100, {}, 255),
    ("grey_8x8_q50", (8, 8), "L", None, 50, {}, 30),
    ("c420_16x16_q50", (16, 16), "RGB", "420", 50, {}, 30),
    ("c422_16x16_q90_opt", (16, 16), "RGB", "422", 90, {"optimize": True}, 30),
    ("c444_16x16_q90", (16, 16), "RGB", "444", 90, {}, 30),
    ("c420_9x17_q90", (9, 17), "RGB", "420", 90, {}, 30),
    ("c422_9x17_q100_noise", (9, 17), "RGB", "422", 100, {}, 255),
    ("grey_9x17_q90_opt", (9, 17), "L", None, 90, {"optimize": True}, 30),
    ("c420_77x181_q90", (77, 181), "RGB", "420", 90, {}, 25),
    ("c420_77x181_q100_noise_rst3", (77, 181), "RGB", "420", 100, {"restart_marker_blocks": 3}, 255),
    ("c444_77x181_q50_opt_rstrow", (77, 181), "RGB", "444", 50, {"optimize": True, "restart_marker_rows": 1}, 25),
    ("grey_77x181_q100_noise", (77, 181), "L", None, 100, {}, 255),
    ("c422_150x200_q90", (150, 200), "RGB", "422", 90, {}, 25),
    ("c422_150x200_q50_rstrow", (150, 200), "RGB", "422", 50, {"restart_marker_rows": 1}, 25),
    ("c420_150x200_q90_opt_rst3", (150, 200), "RGB", "420", 90, {"optimize": True, "restart_marker_blocks": 3}, 60),
    ("progressive_16x16", (16, 16), "RGB", "420", 90, {"progressive": True}, 30),
    ("cmyk_16x16", (16, 16), "CMYK", None, 90, {}, 30),
    # the two sizes of the grow-and-reuse test (tests/test_gpu_jpeg.py): appended, so the seeds of the cases above stay
    ("grey_16x16_q90", (16, 16), "L", None, 90, {}, 30),
    ("c420_40x48_q90", (40, 48), "RGB", "420", 90, {}, 30),
]


def main():
    arrays, table = {}, {}
    for k, (name, (h, w), mode, samp, q, extra, noise) in enumerate(CASES):
        rgb = picture(h, w, 100 + k, noise)
        if mode == "L":
            im = Image.fromarray(rgb[:, :, 1], "L")
        elif mode == "CMYK":
            im = Image.fromarray(np.concatenate([rgb, rgb[:, :, :1]], axis=-1), "CMYK")
        else:
            im = Image.fromarray(rgb, "RGB")
        buf = io.BytesIO()
        kw = dict(extra)
        if samp is not None:
            kw["subsampling"] = SUBSAMPLING[samp]
        im.save(buf, "JPEG", quality=q, **kw)
        data = buf.getvalue()
        arrays[name + ".jpg"] = np.frombuffer(data, dtype=np.uint8)
        supported = mode != "CMYK" and not extra.get("progressive")
        if supported:
            with Image.open(io.BytesIO(data)) as dec:
                arrays[name + ".rgb"] = np.asarray(dec.convert("RGB")).copy()
        hs, vs = {"444": (1, 1), "422": (2, 1), "420": (2, 2), None: (1, 1)}[samp]
        table[name] = {"height": h, "width": w, "components": {"L": 1, "RGB": 3, "CMYK": 4}[mode], "h_samp": hs, "v_samp": vs, "quality": q,
                       "supported": supported, "save": extra, "stuffed_ff00": int(data.count(b"\xff\x00"))}
    arrays["cases"] = np.frombuffer(json.dumps(table, indent=0).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(table)} cases")


if __name__ == "__main__":
    main()
