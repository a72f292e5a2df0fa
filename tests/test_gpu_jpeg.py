"""Baseline JPEG decoding on the device: whole frames against the pixels Pillow stored (tests/golden/jpeg_small.npz), windows and
batches against the CPU decode with the same arithmetic (thmr_jpeg_decode_host, itself bit-equal to Pillow: tests/test_jpeg_host.py),
canaries around padded outputs, staging reuse, one captured call, and the datasets with decode="device" against decode="host"."""
import numpy as np
import pytest
import torch

import _eval_dataset_fixture as F
from _jpeg_fixture import WINDOW_FIXTURES, gold, supported, window_cases

pytestmark = pytest.mark.gpu

CANARY, PAD = 0xC3, 13


@pytest.fixture(scope="module")
def decoder(built_lib, cuda_dev):
    from tokenhmr_amd.jpeg import JpegDecoder
    d = JpegDecoder(cuda_dev)
    yield d
    d.close()


def mixed_items(n, seed):
    """n (fixture name, window) pairs cycling through every supported fixture (all formats and sizes); every other one gets a window
    drawn inside its frame instead of the whole frame, and one of them is empty."""
    rng = np.random.default_rng(seed)
    cases, _, _ = gold()
    names = supported()
    order = rng.permutation(len(names))
    out = []
    for k in range(n):
        name = names[order[k % len(names)]]
        W, H = cases[name]["width"], cases[name]["height"]
        if k % 2 == 0:
            win = (0, 0, W, H)
        else:
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            win = (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h)
        out.append((name, win))
    if n >= 7:
        out[5] = (out[5][0], (1, 1, 0, 0) if cases[out[5][0]]["width"] > 1 else (0, 0, 0, 0))
    return out


def host_reference(name, win, bgr=True):
    from tokenhmr_amd import jpeg as J
    _, jpg, _ = gold()
    return J.decode_host(jpg[name], win, bgr=bgr)


def decode_in_canaries(decoder, items, bgr=True):
    """One batch call; each output has rows padded by PAD bytes and sits inside a canary-filled buffer (64 bytes before, 64 after).
    Returns the windows as numpy arrays after checking that every canary byte is intact."""
    from tokenhmr_amd import jpeg as J
    _, jpg, _ = gold()
    planned = [J.entropy_decode(jpg[name], win) for name, win in items]
    bufs, outs, strides = [], [], []
    for p in planned:
        w, h = p.window[2], p.window[3]
        stride = w * 3 + PAD
        b = torch.full((64 + h * stride + 64,), CANARY, dtype=torch.uint8, device=decoder.device)
        bufs.append(b)
        outs.append(b[64:])
        strides.append(stride)
    # a view that starts 64 bytes in is contiguous; decode_planned takes its first byte as the window's
    decoder.decode_planned(planned, bgr=bgr, out=outs, row_strides=strides)
    torch.cuda.synchronize()
    res = []
    for p, b, stride in zip(planned, bufs, strides):
        w, h = p.window[2], p.window[3]
        a = b.cpu().numpy()
        assert (a[:64] == CANARY).all() and (a[64 + h * stride:] == CANARY).all()
        body = a[64:64 + h * stride].reshape(h, stride)
        assert (body[:, w * 3:] == CANARY).all()
        res.append(body[:, :w * 3].reshape(h, w, 3).copy())
    return res


def test_whole_frames_are_bit_equal_to_pil(decoder):
    _, jpg, rgb = gold()
    names = supported()
    for bgr in (False, True):
        outs = decoder.decode([jpg[n] for n in names], bgr=bgr)
        torch.cuda.synchronize()
        for n, o in zip(names, outs):
            ref = rgb[n][:, :, ::-1] if bgr else rgb[n]
            assert tuple(o.shape) == ref.shape and np.array_equal(o.cpu().numpy(), ref), (n, bgr)


@pytest.mark.parametrize("name", WINDOW_FIXTURES)
def test_windows_are_bit_equal_to_the_host_decode(name, decoder):
    _, jpg, rgb = gold()
    cases = window_cases(name)
    wins = list(cases.values())
    outs = decoder.decode([jpg[name]] * len(wins), windows=wins, bgr=True)
    torch.cuda.synchronize()
    for key, win, o in zip(cases, wins, outs):
        x0, y0, w, h = win
        got = o.cpu().numpy()
        assert np.array_equal(got, host_reference(name, win)), key
        assert np.array_equal(got, rgb[name][y0:y0 + h, x0:x0 + w, ::-1]), key


@pytest.mark.parametrize("n", [1, 7, 9])
def test_batches_of_mixed_items_keep_their_canaries(n, decoder):
    items = mixed_items(n, 50 + n)
    got = decode_in_canaries(decoder, items)
    for k, ((name, win), g) in enumerate(zip(items, got)):
        assert np.array_equal(g, host_reference(name, win)), (k, name, win)
        alone = decode_in_canaries(decoder, [(name, win)])[0]          # the same item decoded alone
        assert np.array_equal(g, alone), (k, name, win)


def test_an_empty_window_between_two_items(decoder):
    # the middle item has no blocks and shares its first block with its successor: every block past it belongs to the successor
    cases, _, _ = gold()
    names = supported()[:3]
    items = [(names[0], (0, 0, cases[names[0]]["width"], cases[names[0]]["height"])), (names[1], (0, 0, 0, 0)),
             (names[2], (0, 0, cases[names[2]]["width"], cases[names[2]]["height"]))]
    got = decode_in_canaries(decoder, items)
    assert got[1].size == 0
    for (name, win), g in zip(items, got):
        assert np.array_equal(g, host_reference(name, win)), (name, win)


def test_reuse_after_growth_and_on_the_alternate_staging_set(built_lib, cuda_dev):
    from tokenhmr_amd.jpeg import JpegDecoder
    d = JpegDecoder(cuda_dev)
    try:
        small, large = mixed_items(1, 7), mixed_items(9, 8)
        first = decode_in_canaries(d, small)              # set 0, small
        a = decode_in_canaries(d, large)                  # set 1, grown
        b = decode_in_canaries(d, large)                  # set 0, grown past the small batch
        c = decode_in_canaries(d, large)                  # set 1 again, no growth
        again = decode_in_canaries(d, small)              # set 0, smaller than its capacity
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        assert np.array_equal(first[0], again[0])
        for (name, win), x in zip(large, a):
            assert np.array_equal(x, host_reference(name, win))
    finally:
        d.close()


def test_one_handle_grown_then_reused_without_host_sync_equals_fresh_handles(built_lib, cuda_dev):
    """Reuse after growth, and the capacity bookkeeping: one handle, one stream, nothing waited for between the calls.  A 16x16 grey
    file, then a 40x48 4:2:0 file twice in a row (each of the two staging sets and the plane scratch grow), then the small file again
    inside the grown buffers.  Every result is bit-equal to the same call on a handle of its own, to the CPU decode and to the pixels
    Pillow stored.  (A missing synchronisation before the growth would not show here: hipFree waits for the device by itself.)"""
    from tokenhmr_amd import jpeg as J
    _, jpg, rgb = gold()
    small, large = J.entropy_decode(jpg["grey_16x16_q90"]), J.entropy_decode(jpg["c420_40x48_q90"])
    assert small.size == (16, 16) and large.size == (40, 48) and (large.plan.h_samp, large.plan.v_samp) == (2, 2)
    steps = [small, large, large, small]
    one = J.JpegDecoder(cuda_dev)
    got = [one.decode_planned([p])[0] for p in steps]
    torch.cuda.synchronize()
    one.close()
    for k, (p, g) in enumerate(zip(steps, got)):
        fresh = J.JpegDecoder(cuda_dev)
        want = fresh.decode_planned([p])[0].cpu()
        fresh.close()
        assert torch.equal(g.cpu(), want), k
        name = "grey_16x16_q90" if p is small else "c420_40x48_q90"
        assert np.array_equal(want.numpy(), host_reference(name, None)) and np.array_equal(want.numpy(), rgb[name][:, :, ::-1]), k


def test_one_captured_call_replays_the_same_bytes(built_lib, cuda_dev):
    """A decoder of its own (a captured call keeps reading its staging set), warmed up at the sizes, then one call captured at fixed
    sizes and replayed into cleared outputs.  The runtime's queue settings are left as they are."""
    from tokenhmr_amd import jpeg as J
    d = J.JpegDecoder(cuda_dev)
    try:
        _, jpg, _ = gold()
        items = mixed_items(7, 21)
        planned = [J.entropy_decode(jpg[name], win) for name, win in items]
        outs = [torch.zeros(max(p.window[2] * p.window[3] * 3, 1), dtype=torch.uint8, device=d.device) for p in planned]
        side = torch.cuda.Stream(cuda_dev)
        side.wait_stream(torch.cuda.current_stream(cuda_dev))
        with torch.cuda.stream(side):
            d.decode_planned(planned, out=outs)           # both staging sets grow to these sizes outside the capture
            d.decode_planned(planned, out=outs)
        torch.cuda.current_stream(cuda_dev).wait_stream(side)
        torch.cuda.synchronize()
        eager = [o.cpu().numpy().copy() for o in outs]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            d.decode_planned(planned, out=outs)
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for (name, win), p, o, e in zip(items, planned, outs, eager):
            w, h = p.window[2], p.window[3]
            got = o.cpu().numpy()
            assert np.array_equal(got, e), (name, win)
            if w * h:
                assert np.array_equal(got[:w * h * 3].reshape(h, w, 3), host_reference(name, win)), (name, win)
    finally:
        d.close()


def _tensors_equal(a, b, path=""):
    assert type(a) is type(b) or (torch.is_tensor(a) and torch.is_tensor(b)), path
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _tensors_equal(a[k], b[k], f"{path}.{k}")
    else:
        assert a == b, path


@pytest.mark.parametrize("kind", ["image", "emdb"])
def test_datasets_decode_device_equals_decode_host(kind, tmp_path, built_lib, cuda_dev):
    """The fixture's frames written as JPEG files (4:2:0, 4:2:2 and grey), one item's frame once more as a progressive file: batches(4)
    with decode="device" equal decode="host" in every key, bit for bit, and exactly the progressive item fell back."""
    from PIL import Image
    from tokenhmr_amd.datasets import create_dataset
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    fr = F.frames()
    Image.fromarray(fr["f0.jpg"][:, :, ::-1].copy()).save(str(imgs / "f0.jpg"), quality=90, subsampling=2)
    Image.fromarray(fr["f1.jpg"][:, :, ::-1].copy()).save(str(imgs / "f1.jpg"), quality=75, subsampling=1, optimize=True)
    Image.fromarray(fr["f2.jpg"][:, :, 1].copy()).save(str(imgs / "f2.jpg"), quality=90)
    Image.fromarray(fr["f2.jpg"][:, :, ::-1].copy()).save(str(imgs / "f2p.jpg"), quality=90, progressive=True)
    src = F.write_input(kind, tmp_path)
    z = dict(np.load(src, allow_pickle=True))
    names = [n.decode() if isinstance(n, bytes) else str(n) for n in z["imgname"]]
    prog = names.index("f2.jpg")
    names[prog] = "f2p.jpg"
    z["imgname"] = np.array(names)
    path = str(tmp_path / f"{kind}_files.npz")
    np.savez(path, **z)
    sm = F.smpl_constants()
    dcfg = {"TYPE": "EMDBDataset" if kind == "emdb" else "ImageDataset", "DATASET_FILE": path, "IMG_DIR": str(imgs), "KEYPOINT_LIST": [0]}
    got = {}
    for mode in ("host", "device"):
        ds = create_dataset(F.model_cfg(), dcfg, train=False, device=cuda_dev, smpl_male=sm["male"], smpl_female=sm["female"], decode=mode)
        got[mode] = list(ds.batches(4, num_workers=2))
        torch.cuda.synchronize()
        n = len(ds)
        if mode == "host":
            assert ds.decode_stats == {"device": 0, "fallback": 0, "coef_bytes": 0}
        else:
            assert ds.decode_stats["fallback"] == 1 and ds.decode_stats["device"] == n - 1 and ds.decode_stats["coef_bytes"] > 0
    assert len(got["host"]) == len(got["device"]) == -(-n // 4)
    for k, (a, b) in enumerate(zip(got["host"], got["device"])):
        assert a["img"].abs().max() > 0
        _tensors_equal(a, b, f"batch{k}")
