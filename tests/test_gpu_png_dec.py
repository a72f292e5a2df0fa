"""PNG decoding on the device: whole frames against the contract and Pillow (tests/_png_dec_cases.py writes the files by hand), windows
and batches against the CPU decode with the same arithmetic (thmr_png_decode_host, itself held to Pillow in tests/test_png_dec_host.py),
canaries around padded outputs, the un-filter kernel's band and strip boundaries, staging reuse, one captured call, the datasets with
decode="device+png" against decode="host", and tokenhmr_amd.imread.  Every comparison is bit-exact."""
import numpy as np
import pytest
import torch

import _eval_dataset_fixture as F
import _png_dec_cases as K

pytestmark = pytest.mark.gpu

CANARY, PAD = 0xC3, 13


@pytest.fixture(scope="module")
def decoder(built_lib, cuda_dev):
    from tokenhmr_amd.png import PNGDecoder
    d = PNGDecoder(cuda_dev)
    yield d
    d.close()


_files = {}


def files():
    """{name: (file, expected RGB)}: every supported kind at two sizes with mixed filters, made once."""
    if not _files:
        for k, (ctype, depth) in enumerate(K.KINDS):
            for h, w, f in ((23, 17, [4, 3, 2, 1, 0, 4, 4]), (70, 41, [1, 4, 4, 3, 3, 2, 4, 4, 4, 0, 4])):
                data, rgb, _ = K.case(h, w, ctype, depth, f, seed=k, idat=1 + k % 3, ancillary=bool(k % 2))
                _files[f"t{ctype}_d{depth}_{h}x{w}"] = (data, rgb)
    return _files


def host_reference(name, win, bgr=True):
    from tokenhmr_amd import png as P
    return P.decode_host(files()[name][0], win, bgr=bgr)


def mixed_items(n, seed):
    """n (file name, window) pairs cycling through every kind and size; every other one gets a window drawn inside its frame instead
    of the whole frame, and (from 7 items on) one in the middle is empty."""
    rng = np.random.default_rng(seed)
    names = list(files())
    order = rng.permutation(len(names))
    out = []
    for k in range(n):
        name = names[order[k % len(names)]]
        H, W = files()[name][1].shape[:2]
        if k % 2 == 0:
            win = (0, 0, W, H)
        else:
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            win = (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h)
        out.append((name, win))
    if n >= 7:
        out[n // 2] = (out[n // 2][0], (1, 1, 0, 0))
    return out


def decode_in_canaries(decoder, planned, bgr=True):
    """One batch call; each output has rows padded by PAD bytes and sits inside a canary-filled buffer (64 bytes before, 64 after).
    Returns the windows as numpy arrays after checking that every canary byte is intact."""
    bufs, outs, strides = [], [], []
    for p in planned:
        w, h = p.window[2], p.window[3]
        stride = w * 3 + PAD
        b = torch.full((64 + h * stride + 64,), CANARY, dtype=torch.uint8, device=decoder.device)
        bufs.append(b)
        outs.append(b[64:])
        strides.append(stride)
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


def plan(items):
    from tokenhmr_amd import png as P
    return [P.inflate_window(files()[name][0], win) for name, win in items]


def test_whole_frames_of_every_kind_in_both_channel_orders(decoder):
    names = list(files())
    for bgr in (False, True):
        outs = decoder.decode([files()[n][0] for n in names], bgr=bgr)
        torch.cuda.synchronize()
        for n, o in zip(names, outs):
            ref = files()[n][1][:, :, ::-1] if bgr else files()[n][1]
            assert tuple(o.shape) == ref.shape and np.array_equal(o.cpu().numpy(), ref), (n, bgr)
            assert np.array_equal(ref, host_reference(n, None, bgr)), n


@pytest.mark.parametrize("n", [1, 7, 9])
def test_batches_of_mixed_items_keep_their_canaries(n, decoder):
    items = mixed_items(n, 50 + n)
    got = decode_in_canaries(decoder, plan(items))
    for k, ((name, win), g) in enumerate(zip(items, got)):
        assert np.array_equal(g, host_reference(name, win)), (k, name, win)
        x0, y0, w, h = win
        assert np.array_equal(g, files()[name][1][y0:y0 + h, x0:x0 + w, ::-1]), (k, name, win)
    assert n < 7 or got[n // 2].size == 0
    alone = decode_in_canaries(decoder, plan(items[-1:]))[0]          # the last item decoded alone
    assert np.array_equal(got[-1], alone)


def test_band_boundaries(decoder, built_lib):
    """Heights around the kernel's rows per band at widths 3 ... 9, and widths around a wave at height 3, all with Paeth and Avg rows
    (every row needs the row above, so a dependency missed at a band or lane boundary shows), one batch call."""
    from tokenhmr_amd import png as P
    B = P.band_rows()
    assert B == built_lib.thmr_png_decode_band_rows() and B >= 2
    cases = [(h, w) for h in (1, 2, B - 1, B, B + 1, 2 * B + 1) for w in range(3, 10)] + [(3, w) for w in (1, 2, 63, 64, 65, 257)]
    datas, want = [], []
    for k, (h, w) in enumerate(cases):
        ctype, depth = K.KINDS[k % len(K.KINDS)]
        data, rgb, _ = K.case(h, w, ctype, depth, [4, 3, 4, 4, 3] if k % 2 else [3, 4], seed=100 + k, smooth=bool(k % 3))
        datas.append(data)
        want.append(rgb)
    got = decode_in_canaries(decoder, [P.inflate_window(d) for d in datas], bgr=False)
    for (h, w), g, r, d in zip(cases, got, want, datas):
        assert np.array_equal(g, r), (h, w)
        assert np.array_equal(g, P.decode_host(d, bgr=False)), (h, w)


def test_one_strip_and_a_strip_per_row_and_a_window_below_a_restart(decoder):
    from tokenhmr_amd import png as P
    B = P.band_rows()
    H, W = 2 * B + 9, 21
    one, _, _ = K.case(H, W, 2, 8, 4, seed=1)                          # one strip of three bands
    per_row, _, _ = K.case(H, W, 6, 8, [1, 0], seed=2)                 # every row its own strip: units of B single-row strips
    mixed = np.full(H, 2, np.uint8)
    mixed[[0, 5, 6, B + 3]] = [1, 0, 1, 1]                             # strips of 5, 1, B - 3 and the rest, Up rows between
    strips, _, _ = K.case(H, W, 4, 16, mixed, seed=3)
    wins = [None, (3, B + 5, 10, B), (0, H - 1, W, 1), (W - 1, 0, 1, H)]
    planned = [P.inflate_window(d, w) for d in (one, per_row, strips) for w in wins]
    assert planned[1].plan.row0 == 0 and planned[5].plan.row0 == B + 5 and planned[9].plan.row0 == B + 3
    got = decode_in_canaries(decoder, planned)
    k = 0
    for d in (one, per_row, strips):
        for w in wins:
            assert np.array_equal(got[k], P.decode_host(d, w)), (k, w)
            k += 1


def test_one_row_of_32767_grey_bytes(decoder):
    from tokenhmr_amd import png as P
    for f in (4, 1):
        data, rgb, _ = K.case(1, 32767, 0, 8, f, seed=4, level=1)
        got = decode_in_canaries(decoder, [P.inflate_window(data), P.inflate_window(data, (32000, 0, 767, 1))], bgr=False)
        assert np.array_equal(got[0], rgb) and np.array_equal(got[1], rgb[:, 32000:])


def test_reuse_after_growth_and_on_the_alternate_staging_set(built_lib, cuda_dev):
    from tokenhmr_amd.png import PNGDecoder
    d = PNGDecoder(cuda_dev)
    try:
        small, large = mixed_items(1, 7), mixed_items(9, 8)
        ps, pl = plan(small), plan(large)
        first = decode_in_canaries(d, ps)              # set 0, small
        a = decode_in_canaries(d, pl)                  # set 1, grown
        b = decode_in_canaries(d, pl)                  # set 0, grown past the small batch
        c = decode_in_canaries(d, pl)                  # set 1 again, no growth
        again = decode_in_canaries(d, ps)              # set 0, smaller than its capacity
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[0], host_reference(*small[0]))
        for (name, win), x in zip(large, a):
            assert np.array_equal(x, host_reference(name, win))
        # nothing waited for between the calls: small, large, large, small on one stream
        steps = [ps[0], pl[0], pl[2], ps[0]]
        got = [d.decode_planned([p])[0] for p in steps]
        torch.cuda.synchronize()
        for p, g, (name, win) in zip(steps, got, [small[0], large[0], large[2], small[0]]):
            assert np.array_equal(g.cpu().numpy(), host_reference(name, win))
    finally:
        d.close()


def test_one_captured_call_replays_the_same_bytes(built_lib, cuda_dev):
    """A decoder of its own (a captured call keeps reading its staging set), warmed up at the sizes, then one call captured at fixed
    sizes and replayed into cleared outputs.  The runtime's queue settings are left as they are."""
    from tokenhmr_amd import png as P
    d = P.PNGDecoder(cuda_dev)
    try:
        items = mixed_items(7, 21)
        planned = plan(items)
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


def test_datasets_decode_device_png_equals_decode_host(tmp_path, built_lib, cuda_dev):
    """The fixture's frames written as a PNG by Pillow, a PNG by this project's encoder, a baseline JPEG, and one item's frame once more
    as an Adam7-interlaced PNG: batches(4) with decode="device+png" equal decode="host" in every key, bit for bit; the JPEG is counted
    in decode_stats, the PNGs in png_stats, and exactly the interlaced item fell back (it is in both fallback counts)."""
    from PIL import Image
    from tokenhmr_amd import png as P
    from tokenhmr_amd.datasets import create_dataset
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    fr = F.frames()
    Image.fromarray(fr["f0.jpg"][:, :, ::-1].copy()).save(str(imgs / "f0.jpg"), format="PNG")
    Image.fromarray(fr["f1.jpg"][:, :, ::-1].copy()).save(str(imgs / "f1.jpg"), quality=90, subsampling=2)
    with open(str(imgs / "f2.jpg"), "wb") as f:
        f.write(P.encode_host(fr["f2.jpg"], compression="dynamic"))
    with open(str(imgs / "f2i.jpg"), "wb") as f:
        f.write(K.write_interlaced(fr["f2.jpg"][:, :, ::-1]))
    with Image.open(str(imgs / "f2i.jpg")) as im:
        assert im.info.get("interlace") == 1 and np.array_equal(np.asarray(im.convert("RGB")), fr["f2.jpg"][:, :, ::-1])
    src = F.write_input("image", tmp_path)
    z = dict(np.load(src, allow_pickle=True))
    names = [n.decode() if isinstance(n, bytes) else str(n) for n in z["imgname"]]
    lace = names.index("f2.jpg")
    names[lace] = "f2i.jpg"
    z["imgname"] = np.array(names)
    path = str(tmp_path / "image_files.npz")
    np.savez(path, **z)
    sm = F.smpl_constants()
    dcfg = {"TYPE": "ImageDataset", "DATASET_FILE": path, "IMG_DIR": str(imgs), "KEYPOINT_LIST": [0]}
    n_png = sum(n in ("f0.jpg", "f2.jpg") for n in names)
    n_jpeg = sum(n == "f1.jpg" for n in names)
    assert n_png >= 2 and n_jpeg >= 1 and n_png + n_jpeg + 1 == len(names)
    got = {}
    for mode in ("host", "device+png", "device"):
        ds = create_dataset(F.model_cfg(), dcfg, train=False, device=cuda_dev, smpl_male=sm["male"], smpl_female=sm["female"], decode=mode)
        got[mode] = list(ds.batches(4, num_workers=2))
        torch.cuda.synchronize()
        assert set(ds.decode_stats) == {"device", "fallback", "coef_bytes"}
        if mode == "host":
            assert ds.decode_stats == {"device": 0, "fallback": 0, "coef_bytes": 0} and ds.png_stats == {"device": 0, "fallback": 0, "stream_bytes": 0}
        elif mode == "device+png":
            assert ds.decode_stats["device"] == n_jpeg and ds.decode_stats["fallback"] == 1 and ds.decode_stats["coef_bytes"] > 0
            assert ds.png_stats["device"] == n_png and ds.png_stats["fallback"] == 1 and ds.png_stats["stream_bytes"] > 0
        else:               # "device" keeps sending every PNG to imread
            assert ds.decode_stats["device"] == n_jpeg and ds.decode_stats["fallback"] == n_png + 1
            assert ds.png_stats == {"device": 0, "fallback": 0, "stream_bytes": 0} and ds._png is None
    assert len(got["host"]) == len(got["device+png"]) == -(-len(names) // 4)
    for k, (a, b, c) in enumerate(zip(got["host"], got["device+png"], got["device"])):
        assert a["img"].abs().max() > 0
        _tensors_equal(a, b, f"batch{k}")
        _tensors_equal(a, c, f"batch{k}")


def test_imread_and_vitdet_dataset_from_its_tensor(tmp_path, built_lib, cuda_dev):
    from PIL import Image
    import tokenhmr_amd
    from tokenhmr_amd import jpeg as J, png as P, preprocess as PP
    fr = F.frames()["f0.jpg"]
    rgb = fr[:, :, ::-1].copy()
    Image.fromarray(rgb).save(str(tmp_path / "a.png"))
    Image.fromarray(rgb).save(str(tmp_path / "b.jpg"), quality=90)
    Image.fromarray(rgb).save(str(tmp_path / "c.jpg"), quality=90, progressive=True)
    with open(str(tmp_path / "d.png"), "wb") as f:
        f.write(open(str(tmp_path / "a.png"), "rb").read()[:200])
    with open(str(tmp_path / "a.png"), "rb") as f:
        want_png = P.decode_host(f.read())
    with open(str(tmp_path / "b.jpg"), "rb") as f:
        want_jpg = J.decode_host(f.read())
    with Image.open(str(tmp_path / "c.jpg")) as im:
        want_prog = np.asarray(im.convert("RGB"))[:, :, ::-1]
    assert np.array_equal(want_png, fr)
    for name, want in (("a.png", want_png), ("b.jpg", want_jpg), ("c.jpg", want_prog)):
        t = tokenhmr_amd.imread(str(tmp_path / name), device=cuda_dev)
        assert t.device == cuda_dev and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), want), name
        t = tokenhmr_amd.imread(str(tmp_path / name), device=cuda_dev, bgr=False)
        assert np.array_equal(t.cpu().numpy(), want[:, :, ::-1]), name
    assert tokenhmr_amd.imread(str(tmp_path / "missing.png"), device=cuda_dev) is None
    assert tokenhmr_amd.imread(str(tmp_path / "d.png"), device=cuda_dev) is None
    frame = tokenhmr_amd.imread(str(tmp_path / "a.png"), device=cuda_dev)
    boxes = np.array([[5.0, 4.0, 40.0, 44.0], [20.0, 10.0, 63.0, 47.0]])
    a = PP.ViTDetDataset(F.model_cfg(), frame, boxes, device=cuda_dev).batch()
    b = PP.ViTDetDataset(F.model_cfg(), fr, boxes, device=cuda_dev).batch()
    torch.cuda.synchronize()
    _tensors_equal(a, b)
    assert a["img"].abs().max() > 0
