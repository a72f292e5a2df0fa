"""Inputs shared by tests/test_jpeg_enc_optimize_host.py and tests/test_gpu_jpeg_enc_optimize.py: the golden archive of Pillow's
optimize=True files (scripts/gen_golden_jpeg_enc_opt.py; its inputs are those of the default-mode archive, _jpeg_enc_cases), the image
whose AC table needs the 16-bit limit, and a parser of a file's DHT segments."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_enc_opt_small.npz")


@functools.lru_cache(maxsize=None)
def golden():
    """({name: case dict}, {name + ".jpg": array})."""
    with np.load(GOLDEN) as z:
        arrays = {k: z[k] for k in z.files}
    return json.loads(arrays["cases"].tobytes().decode()), arrays


def golden_file(name):
    return golden()[1][name + ".jpg"].tobytes()


@functools.lru_cache(maxsize=None)
def long_code_image(seed=3):
    """(256, 256, 3) uint8 RGB: a horizontal 0 ... 255 gradient under heavy-tailed noise.  At q 95 in 4:2:0 its luma AC statistics have a
    long thin tail, and the unlimited Huffman code is longer than 16 bits — which the tests read from thmr_jpeg_optimal_table on the
    image's histogram, never assume."""
    rng = np.random.default_rng(seed)
    img = np.tile(np.arange(256, dtype=np.float64), (256, 1))[..., None] + rng.standard_cauchy((256, 256, 3)) * 3
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    img.setflags(write=False)               # shared by the tests that use it
    return img


def dht_segments(data):
    """[(class << 4 | id, the 16 counts, the symbols)] of a file's DHT segments, in order; one table per segment."""
    out, i = [], 2
    while data[i + 1] != 0xDA:
        n = data[i + 2] * 256 + data[i + 3]
        if data[i + 1] == 0xC4:
            counts = list(data[i + 5:i + 21])
            assert n == 2 + 1 + 16 + sum(counts), "one table per DHT segment"
            out.append((data[i + 4], counts, list(data[i + 21:i + 2 + n])))
        i += 2 + n
    return out


def markers(data):
    """The marker bytes of a file's segments before the scan, SOS included."""
    out, i = [], 2
    while True:
        out.append(data[i + 1])
        if data[i + 1] == 0xDA:
            return out
        i += 2 + data[i + 2] * 256 + data[i + 3]
