"""Baseline JPEG decoding, the part that needs no device: the symbols, the probe, the CPU decode against the pixels Pillow stored in
tests/golden/jpeg_small.npz (scripts/gen_golden_jpeg.py), windows, robustness against truncated and corrupted files, the batch entry's
refusals, and the datasets' decode= argument on the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _eval_dataset_fixture as F

from _jpeg_fixture import GOLD, WINDOW_FIXTURES, gold, supported, window_cases


def test_fixture_covers_what_it_should():
    cases, jpg, rgb = gold()
    assert os.path.getsize(GOLD) < 1 << 20
    sizes = {(c["width"], c["height"]) for c in cases.values()}
    assert {(1, 1), (8, 8), (16, 16), (17, 9), (181, 77), (200, 150)} <= sizes
    sup = [c for c in cases.values() if c["supported"]]
    assert {(c["components"], c["h_samp"], c["v_samp"]) for c in sup} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert {50, 90, 100} <= {c["quality"] for c in sup}
    assert any(c["quality"] == 100 and c["stuffed_ff00"] > 0 for c in sup)
    assert any(c["save"].get("optimize") for c in sup)
    assert any("restart_marker_rows" in c["save"] for c in sup) and any("restart_marker_blocks" in c["save"] for c in sup)
    assert set(rgb) == set(supported()) and len(cases) - len(sup) == 2


def test_symbols_declared_bound_and_exported(built_lib):
    from tokenhmr_amd import _cabi
    assert _cabi.ABI_VERSION == 5 and built_lib.thmr_abi_version() == 5
    # (exported and typed in both builds, like every declared function: tests/test_cabi_header.py)
    assert {"thmr_jpeg_probe", "thmr_jpeg_entropy_decode", "thmr_jpeg_decode_host", "thmr_jpeg_create", "thmr_jpeg_destroy",
            "thmr_jpeg_last_error", "thmr_jpeg_decode_batch"} <= set(_cabi.declared_symbols())
    with open(_cabi.HEADER) as f:
        assert "THMR_ERR_UNSUPPORTED = -5" in f.read()
    # the structs mirror the header
    assert C.sizeof(_cabi.JpegInfo) == 32 and C.sizeof(_cabi.JpegPlan) == 496 and C.sizeof(_cabi.JpegItem) == 48
    assert _cabi.JpegPlan.quant.offset == 112 and _cabi.JpegItem.out_dev.offset == 32


def test_probe(built_lib):
    from tokenhmr_amd import _cabi, jpeg as J
    cases, jpg, _ = gold()
    for name, c in cases.items():
        if c["supported"]:
            info = J.probe(jpg[name])
            assert {k: info[k] for k in ("height", "width", "components", "h_samp", "v_samp")} == \
                   {k: c[k] for k in ("height", "width", "components", "h_samp", "v_samp")}, name
            rows, blocks = c["save"].get("restart_marker_rows"), c["save"].get("restart_marker_blocks")
            mcus_x = -(-c["width"] // (8 * c["h_samp"]))
            assert info["restart_interval"] == (rows * mcus_x if rows else blocks if blocks else 0), name
    info = _cabi.JpegInfo()
    for name, word in (("progressive_16x16", "progressive"), ("cmyk_16x16", "4 components")):
        d = jpg[name]
        rc = built_lib.thmr_jpeg_probe(d, len(d), C.byref(info))
        assert rc == _cabi.ERR_UNSUPPORTED == -5 and info.supported == 0 and (info.height, info.width) == (16, 16)
        assert word in built_lib.thmr_jpeg_last_error(None).decode() and word in built_lib.thmr_last_error(None).decode()
        with pytest.raises(J.JpegUnsupported, match=word):
            J.probe(d)
        with pytest.raises(J.JpegUnsupported, match=word):
            J.entropy_decode(d)
        with pytest.raises(J.JpegUnsupported, match=word):
            J.decode_host(d, window=(0, 0, 16, 16))
    png = b"\x89PNG\r\n\x1a\n" + bytes(64)
    assert built_lib.thmr_jpeg_probe(png, len(png), C.byref(info)) == _cabi.ERR_INVALID
    assert "not a JPEG" in built_lib.thmr_jpeg_last_error(None).decode()
    assert built_lib.thmr_jpeg_probe(None, 0, C.byref(info)) == _cabi.ERR_INVALID
    assert built_lib.thmr_jpeg_probe(b"", 0, C.byref(info)) == _cabi.ERR_INVALID
    with pytest.raises(J.JpegError) as e:
        J.probe(png)
    assert not isinstance(e.value, J.JpegUnsupported)


@pytest.mark.parametrize("name", supported())
def test_host_decode_is_bit_equal_to_pil(name, built_lib):
    """Whole frame, RGB and BGR order, against the stored Pillow pixels: all four formats (4:2:2 included) are bit-equal."""
    from tokenhmr_amd import jpeg as J
    _, jpg, rgb = gold()
    out = J.decode_host(jpg[name], bgr=False)
    assert out.shape == rgb[name].shape and np.array_equal(out, rgb[name])
    assert np.array_equal(J.decode_host(jpg[name], bgr=True), rgb[name][:, :, ::-1])


@pytest.mark.parametrize("name", WINDOW_FIXTURES)
def test_windows_equal_slices_and_decoding_stops_early(name, built_lib):
    from tokenhmr_amd import jpeg as J
    cases, jpg, rgb = gold()
    c = cases[name]
    mcus_y = -(-c["height"] // (8 * c["v_samp"]))
    plans = {}
    for key, (x0, y0, w, h) in window_cases(name).items():
        ref = rgb[name][y0:y0 + h, x0:x0 + w]
        # inside a canary frame with padded rows: nothing but win_w * 3 bytes of each row is written
        buf = np.full((h, w * 3 + 13), 0xA5, dtype=np.uint8)
        rc = built_lib.thmr_jpeg_decode_host(jpg[name], len(jpg[name]), (C.c_int32 * 4)(x0, y0, w, h), 0, C.c_void_p(buf.ctypes.data), w * 3 + 13)
        assert rc == 0, key
        assert np.array_equal(buf[:, :w * 3].reshape(h, w, 3), ref), key
        assert (buf[:, w * 3:] == 0xA5).all(), key
        plans[key] = J.entropy_decode(jpg[name], (x0, y0, w, h))
        assert plans[key].coef.shape == (plans[key].plan.n_blocks, 64)
    whole, last, first = plans["whole"].plan, plans["last_mcu_row"].plan, plans["first_mcu_row"].plan
    assert (whole.mcu_row0, whole.mcu_rows_kept, whole.mcu_rows_decoded) == (0, mcus_y, mcus_y)
    # the last row needs every MCU row decoded and keeps one; the first row stops after one
    assert (last.mcu_row0, last.mcu_rows_kept, last.mcu_rows_decoded) == (mcus_y - 1, 1, mcus_y)
    assert (first.mcu_row0, first.mcu_rows_kept, first.mcu_rows_decoded) == (0, 1, 1)
    assert 0 < last.n_blocks < whole.n_blocks and 0 < first.n_blocks < whole.n_blocks
    # an empty window keeps nothing and decodes nothing
    e = J.entropy_decode(jpg[name], (5, 5, 0, 0))
    assert e.plan.n_blocks == 0 and e.plan.mcu_rows_decoded == 0
    with pytest.raises(J.JpegError, match="does not lie inside"):
        J.entropy_decode(jpg[name], (0, 0, c["width"] + 1, 1))


def test_truncated_and_corrupted_files_are_refused_not_crashed_on(built_lib):
    """Every prefix of the small fixtures (every 97th of the larger ones) and every single-byte corruption of the first 700 bytes of
    the small ones (0x00, then 0xFF): each call returns 0 or a negative code.  Both the entropy decode of the whole frame (into a buffer
    of fixed capacity) and the CPU decode of a window of at most 32x32 run; a corrupted header may name any size."""
    from tokenhmr_amd import _cabi
    lib = built_lib
    cases, jpg, _ = gold()
    cap = 4096
    coef = np.empty((cap, 64), dtype=np.int16)
    out = np.empty((32, 32, 3), dtype=np.uint8)
    info, plan = _cabi.JpegInfo(), _cabi.JpegPlan()
    codes = set()

    def run(d):
        n = len(d)
        rc = lib.thmr_jpeg_probe(d, n, C.byref(info))
        assert rc <= 0
        codes.add(rc)
        rc2 = lib.thmr_jpeg_entropy_decode(d, n, None, C.c_void_p(coef.ctypes.data), cap, C.byref(plan))
        assert rc2 <= 0
        codes.add(rc2)
        if rc == 0:
            win = (C.c_int32 * 4)(0, 0, min(info.width, 32), min(info.height, 32))
            rc3 = lib.thmr_jpeg_decode_host(d, n, win, 1, C.c_void_p(out.ctypes.data), 96)
            assert rc3 <= 0
            codes.add(rc3)
        return rc2

    calls = 0
    for name, c in cases.items():
        d = jpg[name]
        small = c["width"] <= 16 and c["height"] <= 16
        for k in range(0, len(d), 1 if small else 97):
            rc = run(d[:k])
            calls += 1
            if c["supported"] and k < len(d) - 2:
                assert rc < 0, (name, k)                 # the whole frame needs every byte but the EOI marker's two
        if small:
            for k in range(min(700, len(d))):
                for v in (0x00, 0xFF):
                    b = bytearray(d)
                    b[k] = v
                    run(bytes(b))
                    calls += 1
    assert calls > 10000 and {0, _cabi.ERR_INVALID, _cabi.ERR_UNSUPPORTED} <= codes <= {0, _cabi.ERR_INVALID, _cabi.ERR_UNSUPPORTED}


def test_malformed_cases_are_invalid_not_unsupported(built_lib):
    from tokenhmr_amd import _cabi, jpeg as J
    _, jpg, _ = gold()
    d = jpg["c420_16x16_q50"]
    plan = _cabi.JpegPlan()
    coef = np.empty((64, 64), dtype=np.int16)

    def rc_of(b):
        return built_lib.thmr_jpeg_entropy_decode(bytes(b), len(b), None, C.c_void_p(coef.ctypes.data), 64, C.byref(plan)), \
               built_lib.thmr_jpeg_last_error(None).decode()

    assert rc_of(d)[0] == 0
    q = d.index(b"\xff\xdb")
    b = bytearray(d); b[q + 4] = 0x07                     # DQT table id 7
    assert rc_of(b) == (_cabi.ERR_INVALID, "DQT: table id 7 is above 3")
    t = d.index(b"\xff\xc4")
    b = bytearray(d); b[t + 4] = 0x05                     # DHT table id 5
    rc, msg = rc_of(b)
    assert rc == _cabi.ERR_INVALID and "DHT" in msg
    s = d.index(b"\xff\xda")
    rc, msg = rc_of(d[:s + 14] + b"\xff\xd9")             # EOI inside the rows the window needs
    assert rc == _cabi.ERR_INVALID and "entropy-coded data ends" in msg
    rc, msg = rc_of(d[:len(d) // 2])
    assert rc == _cabi.ERR_INVALID
    # a buffer that is too small is refused before anything is decoded
    rc = built_lib.thmr_jpeg_entropy_decode(d, len(d), None, C.c_void_p(coef.ctypes.data), 2, C.byref(plan))
    assert rc == _cabi.ERR_INVALID and "holds 2 blocks" in built_lib.thmr_jpeg_last_error(None).decode()
    with pytest.raises(J.JpegError):
        J.decode_host(d[:len(d) // 2])


def _batch(lib, planned, win=None, stride=None, out=4096, coef=True, plan=None, n=1, table=True, handle=None):
    from tokenhmr_amd import _cabi
    it = (_cabi.JpegItem * 1)()
    x0, y0, w, h = planned.window if win is None else win
    it[0].coef = planned.coef.ctypes.data if coef else None
    it[0].plan = C.pointer(planned.plan if plan is None else plan)
    it[0].win_x0, it[0].win_y0, it[0].win_w, it[0].win_h = x0, y0, w, h
    it[0].out_dev, it[0].row_stride = out, (w * 3 if stride is None else stride)
    rc = lib.thmr_jpeg_decode_batch(handle, it if table else None, n, 1, None)
    return rc, lib.thmr_jpeg_last_error(None).decode()


def test_batch_entry_refuses_before_any_hip_call(built_lib):
    """With a null handle: every argument is checked first, so the answer is the refusal or, for valid items, 'null handle'."""
    from tokenhmr_amd import _cabi, jpeg as J
    lib = built_lib
    _, jpg, _ = gold()
    name = "c420_77x181_q90"
    p = J.entropy_decode(jpg[name], (19, 13, 50, 30))
    assert _batch(lib, p) == (_cabi.ERR_INVALID, "null handle")
    assert _batch(lib, p, n=0)[1] == "n must be 1 ... 65535" and _batch(lib, p, n=-3)[0] == _cabi.ERR_INVALID
    assert _batch(lib, p, table=False)[1] == "null item table"
    assert _batch(lib, p, win=(150, 13, 50, 30))[1] == "item 0: the window does not lie inside the frame"
    assert _batch(lib, p, win=(-1, 13, 50, 30))[1] == "item 0: the window does not lie inside the frame"
    assert _batch(lib, p, stride=149)[1] == "item 0: row_stride is less than win_w * 3"
    assert _batch(lib, p, out=None)[1] == "item 0: null out_dev with a non-empty window"
    assert _batch(lib, p, coef=False)[1] == "item 0: null coefficients"
    # a window the plan's blocks do not cover: the plan was made for (19, 13, 50, 30)
    rc, msg = _batch(lib, p, win=(19, 13, 120, 30))
    assert rc == _cabi.ERR_INVALID and msg.startswith("item 0: the plan's block rectangle of component 0 does not cover the window")
    assert "does not cover the window" in _batch(lib, p, win=(19, 13, 50, 60))[1]
    # a smaller window inside the plan's blocks is fine; an empty one needs no pointer at all
    assert _batch(lib, p, win=(24, 16, 8, 8))[1] == "null handle"
    assert _batch(lib, p, win=(24, 16, 0, 0), out=None, coef=False)[1] == "null handle"
    # a doctored plan
    import copy
    bad = copy.deepcopy(p.plan); bad.bw[1] = 40
    assert "lies outside the component" in _batch(lib, p, plan=bad)[1]
    bad = copy.deepcopy(p.plan); bad.n_blocks += 1
    assert "block count" in _batch(lib, p, plan=bad)[1]
    bad = copy.deepcopy(p.plan); bad.h_samp = 3
    assert "geometry / sampling" in _batch(lib, p, plan=bad)[1]
    # the second item's index is named
    items = (_cabi.JpegItem * 2)()
    for k in range(2):
        items[k].coef, items[k].plan = p.coef.ctypes.data, C.pointer(p.plan)
        items[k].win_x0, items[k].win_y0, items[k].win_w, items[k].win_h = p.window
        items[k].out_dev, items[k].row_stride = 4096, 150 if k == 0 else 10
    assert lib.thmr_jpeg_decode_batch(None, items, 2, 1, None) == _cabi.ERR_INVALID
    assert lib.thmr_jpeg_last_error(None).decode() == "item 1: row_stride is less than win_w * 3"


class RecordingCropper:
    """Stand-in for preprocess.Cropper on the host: records what it is asked for and returns zero crops."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.calls = []

    def warp_frames(self, frames, trans, sigmas=None, truncate=3.0, patch=256, mean=None, std=None, is_bgr=True, windows=True, out=None,
                    extra=None):
        self.calls.append(("warp_frames", [f.shape for f in frames], np.array(trans).tobytes(), sigmas, truncate, patch, tuple(mean), tuple(std),
                           is_bgr, windows, np.array(extra).tobytes()))
        img = torch.zeros(len(frames), 3, patch, patch)
        return img if extra is None else (img, torch.from_numpy(np.array(extra)))

    def warp_device_windows(self, *a, **k):
        raise AssertionError("decode='host' must not take the device-window path")


def test_datasets_decode_argument_on_the_host(tmp_path, built_lib):
    from tokenhmr_amd.datasets import create_dataset, ImageDataset

    def no_meshes(batch, genders, joints24):
        n = len(genders)
        return torch.zeros(n, 6890, 3), (torch.zeros(n, 24, 3) if joints24 else None)

    recs = []
    for kw in ({}, {"decode": "host"}):
        crop = RecordingCropper()
        ds = F.make_dataset("image", tmp_path, "cpu", cropper=crop, **kw)
        ds._meshes = no_meshes
        assert ds.decode == "host" and ds.decode_stats == {"device": 0, "fallback": 0, "coef_bytes": 0}
        batches = list(ds.batches(4, num_workers=2))
        assert [len(b["imgname"]) for b in batches] == [4, 2]
        assert ds.decode_stats == {"device": 0, "fallback": 0, "coef_bytes": 0} and ds._jpeg is None
        recs.append(crop.calls)
    assert len(recs[0]) == 2 and recs[0] == recs[1]          # decode="host" makes exactly the default's calls
    with pytest.raises(ValueError, match="decode='gpu'"):
        F.make_dataset("image", tmp_path, "cpu", cropper=RecordingCropper(), decode="gpu")
    with pytest.raises(ValueError, match="decode="):
        create_dataset(F.model_cfg(), {"TYPE": "NoSuchType"}, decode="")
    with pytest.raises(ValueError, match="decode="):
        ImageDataset(F.model_cfg(), F.write_input("image", tmp_path), "imgs", device="cpu", imread=F.imread, cropper=RecordingCropper(),
                     decode=None)


def test_device_mode_host_half_plans_windows_and_falls_back(tmp_path, built_lib):
    """read_item with decode="device", no device involved: a baseline file becomes a PlannedItem for the crop's window, a progressive
    one and a non-JPEG go to imread, a malformed JPEG raises imread's error."""
    from PIL import Image
    from tokenhmr_amd import jpeg as J, preprocess as PP
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    fr = F.frames()
    Image.fromarray(fr["f0.jpg"][:, :, ::-1].copy()).save(str(imgs / "f0.jpg"), quality=90)
    Image.fromarray(fr["f1.jpg"][:, :, ::-1].copy()).save(str(imgs / "f1.jpg"), quality=90, progressive=True)
    Image.fromarray(fr["f2.jpg"][:, :, ::-1].copy()).save(str(imgs / "f2.jpg"), format="PNG")
    ds = F.make_dataset("image", tmp_path, "cpu", cropper=RecordingCropper(), decode="device", img_dir=str(imgs))
    ds._imread = None                       # the default decoder, on the files just written
    names = [os.path.basename(n) for n in ds._names(range(len(ds)))[1]]
    ke, k0, k1, k2 = 3, 5, names.index("f1.jpg"), names.index("f2.jpg")
    assert names[ke] == names[k0] == "f0.jpg"
    it = ds.read_item(ke)                   # this item's crop lies outside its frame: an empty window, nothing decoded
    assert isinstance(it, J.PlannedItem) and it.window == (0, 0, 0, 0) and it.coef.shape == (0, 64)
    it = ds.read_item(k0)
    assert isinstance(it, J.PlannedItem) and it.size == (48, 64)
    a, trans, _ = ds.host_batch([k0], [it.size])
    win = PP.source_window(trans[0], 256, 48, 64, 0.0, 3.0)
    assert it.window == tuple(win) and ds._item_window(k0, 48, 64) == tuple(win)
    with Image.open(str(imgs / "f0.jpg")) as im:
        ref = np.asarray(im.convert("RGB"))[:, :, ::-1]
    x0, y0, w, h = it.window
    with open(str(imgs / "f0.jpg"), "rb") as f:
        assert np.array_equal(J.decode_host(f.read(), it.window), ref[y0:y0 + h, x0:x0 + w])
    for k in (k1, k2):
        f = ds.read_item(k)
        assert isinstance(f, np.ndarray) and f.shape == fr[names[k]].shape
    with open(str(imgs / "f0.jpg"), "rb") as f:
        data = f.read()
    with open(str(imgs / "f0.jpg"), "wb") as f:
        f.write(data[:len(data) // 2])
    with pytest.raises(IOError, match="Fail to read"):
        ds.read_item(k0)
