"""The JPEG encoder on the device against the CPU restatement (thmr_jpeg_encode_host, itself held to Pillow's bytes by
tests/test_jpeg_enc_host.py): the same files byte for byte at the edge sizes, one block past each kernel's workgroup / segment / chunk
boundary, on the stuffing-dense checkerboard, in mixed batches inside canary-guarded buffers, across staging growth, and twice over;
the refusal inside a stream capture; imwrite / imwrite_batch read back by Pillow.  The largest shape is one 256x512 panel."""
import io
import os
import re

import numpy as np
import pytest
import torch

import _jpeg_enc_cases as K

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
    """TRANSFORM_BLOCKS, SEG_BLOCKS and CHUNK as csrc/jpegenc.hip defines them."""
    from tokenhmr_amd import _cabi
    with open(os.path.join(os.path.dirname(_cabi.__file__), "csrc", "jpegenc.hip")) as f:
        text = f.read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, text).group(1)) for n in ("TRANSFORM_BLOCKS", "SEG_BLOCKS", "CHUNK"))


def check(J, encoder, dev, images, **kw):
    """The device files of one batch call; each equals the host file of the same image."""
    files = encoder.encode([torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in images], **kw)
    for i, (a, data) in enumerate(zip(images, files)):
        one = {k: (v[i] if isinstance(v, (list, tuple)) else v) for k, v in kw.items()}
        want = J.encode_host(a, **one)
        assert data == want, (i, a.shape, one, K.first_difference(data, want))
    return files


@pytest.mark.parametrize("mode", ["444", "420", "grey"])
def test_edge_sizes_equal_the_host_files(J, encoder, cuda_dev, mode):
    table, _ = K.golden()
    names = [n for n, c in table.items() if c["mode"] == mode]
    assert {(table[n]["width"], table[n]["height"]) for n in names} == set(K.SIZES)
    files = check(J, encoder, cuda_dev, [K.golden_input(n) for n in names], quality=[table[n]["quality"] for n in names],
                  subsampling=K.SUBSAMPLING[mode], bgr=False)
    for n, data in zip(names, files):          # and with that, Pillow's
        assert data == K.golden_file(n), n


def test_one_block_past_each_boundary(J, encoder, cuda_dev):
    T, S, CH = kernel_constants()
    assert (T, S, CH) == (32, 256, 1024)
    images, kw = [], {"quality": [], "subsampling": []}

    def add(img, q, sub):
        images.append(img); kw["quality"].append(q); kw["subsampling"].append(sub)

    # grey has one block per MCU: T + 1 and S + 1 blocks as one row of blocks, 2 S + 1 = 27 x 19 blocks as a rectangle
    add(K.picture("noise", 8 * (T + 1), 8, 0), 90, "4:2:0")
    add(K.picture("noise", 8 * (S + 1), 8, 0), 90, "4:2:0")
    add(K.picture("smooth", 8 * 27, 8 * 19, 0), 75, "4:2:0")
    assert 27 * 19 == 2 * S + 1
    # 4:4:4 has three blocks per MCU, 4:2:0 six: the first MCU counts past S blocks are 86 (258 blocks) and 43 (258 blocks); a segment
    # boundary then falls INSIDE an MCU (block 256 is MCU 85's Cb / MCU 42's Cb), and the DC predictor reaches into the segment before
    add(K.picture("noise", 8 * 86, 8), 90, "4:4:4")
    add(K.picture("noise", 16 * 43, 16), 90, "4:2:0")
    add(K.picture("smooth", 16 * 43 - 9, 16 + 7), 50, "4:2:0")         # 43 x 2 MCUs with a dummy column and row: 516 blocks
    # the unstuffed scan one block past a chunk of the stuffing kernels: the narrowest noise strip whose scan is longer than CH bytes
    for w in range(8, 8 * 64, 8):
        strip = K.picture("noise", w, 8, 0, seed=5)
        data = J.encode_host(strip, quality=100)
        scan = data[328:-2]
        if len(scan) - scan.count(b"\xff\x00") > CH:
            break
    before = J.encode_host(strip[:, :-8], quality=100)[328:-2]
    assert len(before) - before.count(b"\xff\x00") <= CH < len(scan) - scan.count(b"\xff\x00")
    add(strip, 100, "4:2:0")
    add(np.ascontiguousarray(strip[:, :-8]), 100, "4:2:0")
    check(J, encoder, cuda_dev, images, bgr=False, **kw)


def test_items_of_one_three_and_twelve_blocks(J, encoder, cuda_dev):
    # 1 x 1 grey, 17 x 23 at 4:2:0 and 8 x 8 at 4:4:4 have 1, 2 x 6 = 12 and 3 blocks, and each item starts a segment of its own:
    # their first blocks are 0, 256 and 512, so nearly every lane that searches for its item finds one whose blocks it lies past
    _, S, _ = kernel_constants()
    assert S == 256
    images = [K.picture("noise", 1, 1, 0), K.picture("noise", 17, 23), K.picture("smooth", 8, 8)]
    check(J, encoder, cuda_dev, images, quality=[90, 75, 100], subsampling=["4:2:0", "4:2:0", "4:4:4"], bgr=False)


def test_stuffing_dense_and_large_scans(J, encoder, cuda_dev):
    # 0 / 255 checkerboards at q 100: the largest categories and a 0xFF in most bytes' neighbourhood; the noise panel's scan has more
    # than 256 chunks, so the scan over the chunks takes a second round; an all-white image stuffs nothing
    images = [K.picture("checker", 100, 75), K.picture("checker", 100, 75, 0), K.picture("checker", 255, 129), K.picture("noise", 512, 256),
              K.picture("white", 64, 48)]
    files = check(J, encoder, cuda_dev, images, quality=100, subsampling=["4:4:4", "4:2:0", "4:2:0", "4:4:4", "4:2:0"], bgr=False)
    assert files[0].count(b"\xff\x00") > 50 and files[2].count(b"\xff\x00") > 200
    assert len(files[3]) > 256 * 1024 + 623
    for data, img in zip(files, images):
        c = 1 if img.ndim == 2 else 3
        assert len(data) <= J.encode_bound(img.shape[1], img.shape[0], c, "4:4:4")


def guarded(img, dev, pad=(3, 5), fill=0xA5):
    """The image inside a larger device buffer of `fill` (165 as uint8, 165.0 as float32): (the buffer, the view of the image in it)."""
    h, w = img.shape[:2]
    shape = (h + 2 * pad[0], w + 2 * pad[1]) + img.shape[2:]
    buf = torch.full(shape, fill, dtype=torch.from_numpy(img[:1]).dtype, device=dev)
    view = buf[pad[0]:pad[0] + h, pad[1]:pad[1] + w]
    view.copy_(torch.from_numpy(np.ascontiguousarray(img)).to(dev))
    return buf, view


def mixed_items(n, seed):
    """n images of different sizes, channel counts, dtypes and layouts with their quality and subsampling."""
    rng = np.random.default_rng(seed)
    kinds = ["noise", "smooth", "checker", "smooth", "noise", "white", "smooth", "noise", "black"]
    sizes = [(17, 23), (100, 75), (33, 64), (1, 1), (24, 8), (12, 20), (7, 9), (16, 16), (8, 8)]
    out = []
    for i in range(n):
        (w, h), c = sizes[(i + seed) % 9], (3, 0, 4, 3, 1)[i % 5]
        img = K.picture(kinds[i % 9], w, h, c, seed=seed + i)
        if i % 3 == 1:
            img = img.astype(np.float32) / np.float32(255)
        out.append((img, int(rng.choice(K.QUALITIES)), ("4:2:0", "4:4:4")[i % 2]))
    return out


@pytest.mark.parametrize("n", [1, 7, 9])
def test_mixed_batches_in_guarded_buffers(J, encoder, cuda_dev, n):
    items = mixed_items(n, 10 + n)
    held = [guarded(img, cuda_dev) for img, _, _ in items]
    views = [v for _, v in held]
    assert n == 1 or not all(v.is_contiguous() for v in views)
    kw = dict(quality=[q for _, q, _ in items], subsampling=[s for _, _, s in items], scale=255.0, rounding="trunc", bgr=True)
    together = encoder.encode(views, **kw)
    for i, (img, q, s) in enumerate(items):
        want = J.encode_host(img, quality=q, subsampling=s, scale=255.0, rounding="trunc", bgr=True)
        assert together[i] == want, (i, img.shape, img.dtype, q, s, K.first_difference(together[i], want))
        assert encoder.encode([views[i]], quality=q, subsampling=s, scale=255.0, rounding="trunc", bgr=True)[0] == want, i
    for (buf, view), (img, _, _) in zip(held, items):          # the buffers are as they were
        assert torch.equal(view.cpu(), torch.from_numpy(np.ascontiguousarray(img)))
        frame = buf.clone()
        frame[3:3 + img.shape[0], 5:5 + img.shape[1]] = 0xA5
        assert bool((frame == 0xA5).all())
    # a second call, and the batch reversed
    assert encoder.encode(views, **kw) == together
    rev = dict(kw, quality=kw["quality"][::-1], subsampling=kw["subsampling"][::-1])
    assert encoder.encode(views[::-1], **rev) == together[::-1]


def test_float_chw_view_and_channel_swap(J, encoder, cuda_dev):
    rng = np.random.default_rng(2)
    chw = rng.random((3, 40, 56), dtype=np.float32)
    dev = torch.from_numpy(chw).to(cuda_dev).permute(1, 2, 0)
    assert not dev.is_contiguous()
    for rounding in ("nearest", "trunc"):
        for bgr in (True, False):
            got = encoder.encode([dev], quality=90, scale=255.0, rounding=rounding, bgr=bgr)[0]
            assert got == J.encode_host(chw.transpose(1, 2, 0), quality=90, scale=255.0, rounding=rounding, bgr=bgr), (rounding, bgr)
    rgba = K.picture("smooth", 19, 23, 4)
    d = torch.from_numpy(rgba).to(cuda_dev)
    assert encoder.encode([d], bgr=True)[0] == J.encode_host(rgba, bgr=True) != encoder.encode([d], bgr=False)[0]


def test_staging_grows_and_is_reused(J, cuda_dev):
    e = J.JpegEncoder(cuda_dev)
    try:
        small, large = K.picture("smooth", 17, 23), K.picture("smooth", 512, 256)
        ds, dl = torch.from_numpy(small).to(cuda_dev), torch.from_numpy(large).to(cuda_dev)
        hs, hl = J.encode_host(small), J.encode_host(large)
        assert e.encode([ds])[0] == hs
        assert e.encode([dl, ds]) == [hl, hs]               # every buffer grows
        assert e.encode([ds])[0] == hs                      # the grown buffers hold a smaller call
        assert e.encode([ds, dl, ds], quality=[95, 95, 30])[:2] == [hs, hl]
    finally:
        e.close()


def test_refused_inside_a_stream_capture_and_usable_after(J, cuda_dev):
    from tokenhmr_amd import _cabi
    e = J.JpegEncoder(cuda_dev)
    try:
        img = K.picture("smooth", 33, 64)
        dev = torch.from_numpy(img).to(cuda_dev)
        want = J.encode_host(img)
        assert e.encode([dev])[0] == want
        x = torch.zeros(8, device=cuda_dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = x + 1           # the graph is not empty
            with pytest.raises(J.JpegError, match=r"error %d: .*stream capture" % _cabi.ERR_STATE):
                e.encode([dev])
        torch.cuda.synchronize()
        assert y.shape == x.shape
        with pytest.raises(J.JpegUnsupported, match="item 1.*2 channels"):
            e.encode([dev, torch.zeros(4, 4, 2, dtype=torch.uint8, device=cuda_dev)])
        assert e.encode([dev])[0] == want
    finally:
        e.close()


def test_imwrite_and_imwrite_batch(J, cuda_dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    bgr = K.picture("smooth", 80, 48)
    path = tmp_path / "device.jpg"
    assert J.imwrite(str(path), torch.from_numpy(bgr).to(cuda_dev)) is True
    assert path.read_bytes() == J.encode_host(bgr, quality=95, subsampling="4:2:0", bgr=True)        # cv2's defaults
    assert np.abs(np.asarray(Image.open(path)).astype(int) - bgr[..., ::-1]).mean() < 6
    path = tmp_path / "host.JPEG"
    assert J.imwrite(str(path), bgr, [J.IMWRITE_JPEG_QUALITY, 40], device=cuda_dev) is True
    assert path.read_bytes() == J.encode_host(bgr, quality=40)
    grey = K.picture("smooth", 17, 33, 0)
    images = [torch.from_numpy(bgr).to(cuda_dev), grey, torch.from_numpy(K.picture("noise", 9, 9, 4)).to(cuda_dev)]
    paths = [str(tmp_path / f"b{i}.jpg") for i in range(3)]
    assert J.imwrite_batch(paths, images, quality=[95, 75, 100], device=cuda_dev) is True
    for p, img, q in zip(paths, images, (95, 75, 100)):
        a = img.cpu().numpy() if torch.is_tensor(img) else img
        with open(p, "rb") as f:
            data = f.read()
        assert data == J.encode_host(a, quality=q)
        opened = Image.open(io.BytesIO(data))
        assert opened.size == (a.shape[1], a.shape[0]) and opened.mode == ("L" if a.ndim == 2 else "RGB")
        assert np.array_equal(np.asarray(opened.convert("RGB")), J.decode_host(data, bgr=False))
