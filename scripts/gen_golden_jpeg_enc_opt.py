"""Writes tests/golden/jpeg_enc_opt_small.npz: the JPEG files Pillow (libjpeg-turbo) writes with optimize=True — libjpeg's
optimize_coding, Huffman tables from the image's own statistics — for the cases of scripts/gen_golden_jpeg_enc.py.

    python scripts/gen_golden_jpeg_enc_opt.py    # needs Pillow; the stored file was made with Pillow 12.2 / libjpeg-turbo 3.1

The cases, their names and their inputs are those of tests/golden/jpeg_enc_small.npz (the same sizes x modes x kinds, the qualities
rotating through 1 / 30 / 50 / 75 / 90 / 95 / 100), and that archive is neither read nor written here: the inputs are procedural and are made
again, and this archive stores none — `cases` names each one's key `in.KIND.WxH` in the other archive.  `NAME.jpg` is the bytes of
Image.fromarray(input).save(format="JPEG", quality=q, subsampling=0 | 2, optimize=True); `versions` the Pillow and libjpeg-turbo versions
that wrote the files.  Among the cases: 1x1 and the flat 8x8 (every table holds one real symbol and the pseudo-symbol: one code of
length 1), 17x23 in 4:2:0 (dummy luma blocks, which are counted, and ragged chroma) and the grey images (two tables only).
"""
import io
import json
import os

import numpy as np
import PIL
from PIL import Image, features

from gen_golden_jpeg_enc import cases, picture

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_enc_opt_small.npz")


def pillow_file(rgb, mode, quality):
    buf = io.BytesIO()
    if mode == "grey":
        Image.fromarray(np.ascontiguousarray(rgb[:, :, 1])).save(buf, "JPEG", quality=quality, optimize=True)
    else:
        Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling={"444": 0, "420": 2}[mode], optimize=True)
    return buf.getvalue()


def main():
    arrays, table = {}, {}
    for name, kind, (w, h), mode, q in cases():
        arrays[name + ".jpg"] = np.frombuffer(pillow_file(picture(kind, w, h), mode, q), dtype=np.uint8)
        table[name] = {"input": f"in.{kind}.{w}x{h}", "width": w, "height": h, "kind": kind, "mode": mode, "quality": q}
    arrays["cases"] = np.frombuffer(json.dumps(table, indent=0).encode(), dtype=np.uint8)
    arrays["versions"] = np.array([PIL.__version__, str(features.version_feature("libjpeg_turbo"))])
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(table)} cases")


if __name__ == "__main__":
    main()
