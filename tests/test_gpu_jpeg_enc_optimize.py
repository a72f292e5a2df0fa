"""The optimised mode of the JPEG encoder on the device (optimize=True: the symbol histogram, the table build and the count / pack kernels
reading an image's own code words) against the CPU restatement (thmr_jpeg_encode_host_flags, itself held to Pillow's optimize=True
bytes by tests/test_jpeg_enc_optimize_host.py): the same files byte for byte at the edge sizes, one block past each workgroup / segment
boundary the new kernels add or reuse, in batches that mix flagged and unflagged images inside canary-guarded buffers, twice over and
across staging growth, on the image whose code needs the 16-bit limit and on the one-symbol images; imwrite / imwrite_batch read back
by Pillow; the refusal inside a stream capture.  The largest shape is one 256x512 panel."""
import io
import os
import re

import numpy as np
import pytest
import torch

import _jpeg_enc_cases as K
import _jpeg_enc_opt_cases as KO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J(built_lib):
    from tokenhmr_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def encoder(J, cuda_dev):
    e = J.JpegEncoder(cuda_dev)
    yield e
    e.close()


def kernel_constants():
    """TRANSFORM_BLOCKS and SEG_BLOCKS as csrc/jpegenc.hip defines them."""
    from tokenhmr_amd import _cabi
    with open(os.path.join(os.path.dirname(_cabi.__file__), "csrc", "jpegenc.hip")) as f:
        text = f.read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, text).group(1)) for n in ("TRANSFORM_BLOCKS", "SEG_BLOCKS"))


def check(J, encoder, dev, images, **kw):
    """The device files of one batch call; each equals the host file of the same image and arguments."""
    files = encoder.encode([torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in images], **kw)
    for i, (a, data) in enumerate(zip(images, files)):
        one = {k: (v[i] if isinstance(v, (list, tuple)) else v) for k, v in kw.items()}
        want = J.encode_host(a, **one)
        assert data == want, (i, a.shape, one, K.first_difference(data, want))
    return files


@pytest.mark.parametrize("mode", ["444", "420", "grey"])
def test_edge_sizes_equal_the_host_files_and_pillows(J, encoder, cuda_dev, mode):
    table, _ = KO.golden()
    names = [n for n, c in table.items() if c["mode"] == mode]
    assert {(table[n]["width"], table[n]["height"]) for n in names} == set(K.SIZES)
    files = check(J, encoder, cuda_dev, [K.golden_input(n) for n in names], quality=[table[n]["quality"] for n in names],
                  subsampling=K.SUBSAMPLING[mode], optimize=True, bgr=False)
    for n, data in zip(names, files):
        assert data == KO.golden_file(n), n
        assert data != K.golden_file(n), n          # and not the default mode's


def test_one_block_past_each_boundary(J, encoder, cuda_dev):
    T, S = kernel_constants()
    assert (T, S) == (32, 256)
    images, kw = [], {"quality": [], "subsampling": []}

    def add(img, q, sub):
        images.append(img); kw["quality"].append(q); kw["subsampling"].append(sub)

    # grey has one block per MCU.  S + 1 blocks: the image's histogram is the sum of two workgroups', the second with one live lane;
    # 2 S + 1 = 27 x 19 blocks: of three; T + 1: the transform's boundary, inside one segment
    add(K.picture("noise", 8 * (S + 1), 8, 0), 90, "4:2:0")
    add(K.picture("smooth", 8 * 27, 8 * 19, 0), 75, "4:2:0")
    assert 27 * 19 == 2 * S + 1
    add(K.picture("noise", 8 * (T + 1), 8, 0), 90, "4:2:0")
    add(K.picture("noise", 8 * S, 8, 0), 90, "4:2:0")                   # exactly one full segment
    # a segment boundary INSIDE an MCU (258 blocks): both classes' counters get parts from two workgroups, and the DC difference of
    # the first block of the second reaches into the segment before
    add(K.picture("noise", 8 * 86, 8), 90, "4:4:4")
    add(K.picture("noise", 16 * 43, 16), 90, "4:2:0")
    add(K.picture("smooth", 16 * 43 - 9, 16 + 7), 50, "4:2:0")          # 43 x 2 MCUs with a dummy column and row: 516 blocks, dummies counted
    check(J, encoder, cuda_dev, images, optimize=True, bgr=False, **kw)


def guarded(img, dev, pad=(3, 5), fill=0xA5):
    """The image inside a larger device buffer of `fill`: (the buffer, the view of the image in it)."""
    h, w = img.shape[:2]
    buf = torch.full((h + 2 * pad[0], w + 2 * pad[1]) + img.shape[2:], fill, dtype=torch.from_numpy(img[:1]).dtype, device=dev)
    view = buf[pad[0]:pad[0] + h, pad[1]:pad[1] + w]
    view.copy_(torch.from_numpy(np.ascontiguousarray(img)).to(dev))
    return buf, view


def mixed_items(n, seed):
    """n images of different sizes, channel counts, dtypes and layouts: (image, quality, subsampling, optimize).  The flags interleave
    (two flagged, one not, ...), so flagged and unflagged images alternate as neighbours in the batch."""
    rng = np.random.default_rng(seed)
    kinds = ["noise", "smooth", "checker", "smooth", "noise", "white", "smooth", "noise", "black"]
    sizes = [(17, 23), (100, 75), (33, 64), (1, 1), (24, 8), (12, 20), (7, 9), (16, 16), (8, 8)]
    out = []
    for i in range(n):
        (w, h), c = sizes[(i + seed) % 9], (3, 0, 4, 3, 1)[i % 5]
        img = K.picture(kinds[i % 9], w, h, c, seed=seed + i)
        if i % 3 == 1:
            img = img.astype(np.float32) / np.float32(255)
        out.append((img, int(rng.choice(K.QUALITIES)), ("4:2:0", "4:4:4")[i % 2], i % 3 != 2))
    return out


@pytest.mark.parametrize("n", [3, 9])
def test_mixed_batches_of_flagged_and_unflagged_in_guarded_buffers(J, encoder, cuda_dev, n):
    items = mixed_items(n, 20 + n)
    held = [guarded(img, cuda_dev) for img, _, _, _ in items]
    views = [v for _, v in held]
    flags = [o for _, _, _, o in items]
    assert any(flags) and not all(flags)
    kw = dict(quality=[q for _, q, _, _ in items], subsampling=[s for _, _, s, _ in items], scale=255.0, rounding="trunc", bgr=True)
    together = encoder.encode(views, optimize=flags, **kw)
    today = encoder.encode(views, **kw)                 # the call as it was before the mode existed
    for i, (img, q, s, o) in enumerate(items):
        want = J.encode_host(img, quality=q, subsampling=s, optimize=o, scale=255.0, rounding="trunc", bgr=True)
        assert together[i] == want, (i, img.shape, img.dtype, q, s, o, K.first_difference(together[i], want))
        if not o:
            assert together[i] == today[i], i
        else:
            assert together[i] != today[i] and len(together[i]) < len(today[i]), i
    for (buf, view), (img, _, _, _) in zip(held, items):          # the buffers are as they were
        assert torch.equal(view.cpu(), torch.from_numpy(np.ascontiguousarray(img)))
        frame = buf.clone()
        frame[3:3 + img.shape[0], 5:5 + img.shape[1]] = 0xA5
        assert bool((frame == 0xA5).all())
    # a second call, the flags inverted, and the batch reversed
    assert encoder.encode(views, optimize=flags, **kw) == together
    inverted = encoder.encode(views, optimize=[not o for o in flags], **kw)
    for i, (img, q, s, o) in enumerate(items):
        assert inverted[i] == J.encode_host(img, quality=q, subsampling=s, optimize=not o, scale=255.0, rounding="trunc", bgr=True), i
    rev = dict(kw, quality=kw["quality"][::-1], subsampling=kw["subsampling"][::-1])
    assert encoder.encode(views[::-1], optimize=flags[::-1], **rev) == together[::-1]


def test_twice_then_a_larger_batch_and_a_smaller_one(J, cuda_dev):
    # the histograms are grow-only scratch zeroed by every call: a second call that added to the first one's counts would build other
    # tables; then every buffer grows, and the grown buffers hold a smaller call whose histograms lie where other data lay
    e = J.JpegEncoder(cuda_dev)
    try:
        small, panel, noise = K.picture("smooth", 17, 23), K.picture("smooth", 512, 256), K.picture("noise", 100, 75)
        ds, dp, dn = (torch.from_numpy(a).to(cuda_dev) for a in (small, panel, noise))
        hs, hp, hn = (J.encode_host(a, optimize=True) for a in (small, panel, noise))
        assert e.encode([ds, dn], optimize=True) == [hs, hn]
        assert e.encode([ds, dn], optimize=True) == [hs, hn]
        assert e.encode([dp, ds, dn, dn], optimize=[True, True, False, True]) == [hp, hs, J.encode_host(noise), hn]
        assert e.encode([dn], optimize=True) == [hn]
        assert e.encode([ds, dn], optimize=True) == [hs, hn]
        assert e.encode([dn, ds]) == [J.encode_host(noise), J.encode_host(small)]           # and no flag at all
    finally:
        e.close()


def test_the_image_whose_code_needs_the_16_bit_limit(J, encoder, cuda_dev):
    img = np.array(KO.long_code_image())          # a copy: the shared one is read-only
    hist = J.symbol_histogram(img, quality=95, subsampling="4:2:0", bgr=False)
    bits, _ = J.optimal_table(hist[1])
    assert bits[0] > 16 and bits[16] > 0           # the limiter ran on the luma AC table
    files = check(J, encoder, cuda_dev, [img], quality=95, subsampling="4:2:0", optimize=True, bgr=False)
    assert KO.dht_segments(files[0])[1][1][15] == bits[16]


def test_single_symbol_images_beside_a_noise_image(J, encoder, cuda_dev):
    # 1 x 1 and flat 8 x 8: every table holds one real symbol and the pseudo-symbol, one code of length 1
    images = [K.picture("noise", 1, 1, 0), K.picture("white", 8, 8), K.picture("noise", 40, 56), K.picture("black", 8, 8, 0), K.picture("noise", 1, 1)]
    files = check(J, encoder, cuda_dev, images, quality=[95, 95, 95, 50, 75], subsampling=["4:2:0", "4:4:4", "4:2:0", "4:2:0", "4:2:0"], optimize=True, bgr=False)
    for data in (files[1], files[3]):
        for _, counts, symbols in KO.dht_segments(data):
            assert counts == [1] + [0] * 15 and len(symbols) == 1


def test_imwrite_and_imwrite_batch(J, cuda_dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    bgr = K.picture("smooth", 80, 48)
    path = tmp_path / "device.jpg"
    assert J.imwrite(str(path), torch.from_numpy(bgr).to(cuda_dev), [J.IMWRITE_JPEG_OPTIMIZE, 1]) is True
    assert path.read_bytes() == J.encode_host(bgr, quality=95, subsampling="4:2:0", optimize=True, bgr=True)
    default = J.encode_host(bgr)
    assert len(path.read_bytes()) < len(default)
    assert np.array_equal(np.asarray(Image.open(path)), np.asarray(Image.open(io.BytesIO(default))))      # the same pixels
    path = tmp_path / "host.JPEG"
    assert J.imwrite(str(path), bgr, [J.IMWRITE_JPEG_QUALITY, 40, J.IMWRITE_JPEG_OPTIMIZE, 1], device=cuda_dev) is True
    assert path.read_bytes() == J.encode_host(bgr, quality=40, optimize=True)
    assert J.imwrite(str(path), bgr, [J.IMWRITE_JPEG_OPTIMIZE, 0], device=cuda_dev) is True
    assert path.read_bytes() == default
    grey = K.picture("smooth", 17, 33, 0)
    images = [torch.from_numpy(bgr).to(cuda_dev), grey, torch.from_numpy(K.picture("noise", 9, 9, 4)).to(cuda_dev)]
    paths = [str(tmp_path / f"b{i}.jpg") for i in range(3)]
    assert J.imwrite_batch(paths, images, quality=[95, 75, 100], optimize=True, device=cuda_dev) is True
    for p, img, q in zip(paths, images, (95, 75, 100)):
        a = img.cpu().numpy() if torch.is_tensor(img) else img
        with open(p, "rb") as f:
            data = f.read()
        assert data == J.encode_host(a, quality=q, optimize=True)
        opened = Image.open(io.BytesIO(data))
        assert opened.size == (a.shape[1], a.shape[0]) and opened.mode == ("L" if a.ndim == 2 else "RGB")
        assert np.array_equal(np.asarray(opened.convert("RGB")), J.decode_host(data, bgr=False))
    assert J.imwrite_batch(paths[:2], images[:2], optimize=[False, True], device=cuda_dev) is True
    with open(paths[0], "rb") as f:
        assert f.read() == default


def test_refused_inside_a_stream_capture_and_usable_after(J, cuda_dev):
    from tokenhmr_amd import _cabi
    e = J.JpegEncoder(cuda_dev)
    try:
        img = K.picture("smooth", 33, 64)
        dev = torch.from_numpy(img).to(cuda_dev)
        want = J.encode_host(img, optimize=True)
        assert e.encode([dev], optimize=True)[0] == want
        x = torch.zeros(8, device=cuda_dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = x + 1           # the graph is not empty
            with pytest.raises(J.JpegError, match=r"error %d: .*stream capture" % _cabi.ERR_STATE):
                e.encode([dev], optimize=True)
        torch.cuda.synchronize()
        assert y.shape == x.shape
        with pytest.raises(J.JpegUnsupported, match="item 1.*2 channels"):
            e.encode([dev, torch.zeros(4, 4, 2, dtype=torch.uint8, device=cuda_dev)], optimize=True)
        assert e.encode([dev], optimize=True)[0] == want
    finally:
        e.close()
