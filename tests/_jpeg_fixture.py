"""Shared by tests/test_jpeg_host.py and tests/test_gpu_jpeg.py: tests/golden/jpeg_small.npz (scripts/gen_golden_jpeg.py) read back, and
the window cases both files decode."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_small.npz")
_cache = {}

# the two frames the window cases use, and the cases: (x0, y0, w, h) given (W, H, MCU height)
WINDOW_FIXTURES = ("c420_77x181_q90", "c422_150x200_q90")


def gold():
    if not _cache:
        z = np.load(GOLD)
        _cache["cases"] = json.loads(z["cases"].tobytes())
        _cache["jpg"] = {k[:-4]: z[k].tobytes() for k in z.files if k.endswith(".jpg")}
        _cache["rgb"] = {k[:-4]: z[k] for k in z.files if k.endswith(".rgb")}
    return _cache["cases"], _cache["jpg"], _cache["rgb"]


def supported():
    cases, _, _ = gold()
    return [n for n, c in cases.items() if c["supported"]]


def window_cases(name):
    cases, _, _ = gold()
    c = cases[name]
    W, H, mcu_h = c["width"], c["height"], 8 * c["v_samp"]
    last = (H - 1) // mcu_h * mcu_h           # first pixel row of the last MCU row
    return {"whole": (0, 0, W, H), "one_pixel_odd": (37, 23, 1, 1), "off_grid": (19, 13, 50, 30), "right_bottom": (W - 45, H - 29, 45, 29),
            "last_mcu_row": (10, last + 2, 40, H - last - 2), "first_mcu_row": (10, 2, 40, 3)}
