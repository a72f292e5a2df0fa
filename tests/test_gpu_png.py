"""The PNG encoder on the device against the CPU restatement (thmr_png_encode_host, itself checked by tests/test_png_host.py): the same
files byte for byte for every case of the host test, one call on a mixed batch against each image alone and against a second call,
imwrite / imwrite_batch read back by tests/_png_reader.py and Pillow, and the grow path of the handle's buffers."""
import io

import numpy as np
import pytest
import torch

import _png_cases as K
import _png_reader as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P(built_lib):
    from tokenhmr_amd import png
    return png


@pytest.fixture(scope="module")
def encoder(P, cuda_dev):
    e = P.PNGEncoder(cuda_dev)
    yield e
    e.close()


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else n)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_round_trip_cases_equal_the_host_files(P, encoder, cuda_dev, c):
    cases = [(n, img) for n, img in K.roundtrip_cases() if img.shape[2] == c]
    files = encoder.encode([torch.from_numpy(img).to(cuda_dev) for _, img in cases], bgr=False)
    for (name, _), data in zip(cases, files):
        want = K.host_file("roundtrip", name)
        assert data == want, (name, first_difference(data, want))


@pytest.mark.parametrize("kind", K.EDGE_KINDS)
def test_segment_edge_cases_equal_the_host_files(P, encoder, cuda_dev, kind):
    cases = [(n, img) for n, img in K.edge_cases(P.segment_bytes()) if n.startswith(kind)]
    assert len(cases) == 5
    files = encoder.encode([torch.from_numpy(img).to(cuda_dev) for _, img in cases], bgr=False)
    for (name, _), data in zip(cases, files):
        want = K.host_file("edge", name)
        assert data == want, (name, first_difference(data, want))


def test_constant_and_render_like_equal_the_host_files(P, encoder, cuda_dev):
    for img in (K.image("flat", 256, 256, 3), K.image("render", 256, 512, 3)):
        data = encoder.encode([torch.from_numpy(img).to(cuda_dev)], bgr=False)[0]
        want = P.encode_host(img, bgr=False)
        assert data == want, first_difference(data, want)


def test_conversion_cases_equal_the_host_files(P, encoder, cuda_dev):
    for name, img, scale, rounding in K.conversion_cases():
        data = encoder.encode([torch.from_numpy(img).to(cuda_dev)], scale=scale, rounding=rounding)[0]
        want = K.host_file("conversion", name)
        assert data == want, (name, first_difference(data, want))
        assert np.array_equal(R.read(data)[0], K.convert_expected(img, scale, rounding))


def test_stride_cases_equal_the_host_files(P, encoder, cuda_dev):
    for name, view, kw in K.stride_cases():
        base = view.base if view.base is not None else view
        dev = torch.from_numpy(np.ascontiguousarray(base)).to(cuda_dev)
        # the same view of the device copy: strides and offset carried over in elements
        off = (view.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // view.itemsize
        tview = torch.as_strided(dev, view.shape, [s // view.itemsize for s in view.strides], off)
        assert not tview.is_contiguous()
        data = encoder.encode([tview], **kw)[0]
        want = K.host_file("stride", name)
        assert data == want, (name, first_difference(data, want))
    img = K.image("render", 19, 23, 4)
    dev = torch.from_numpy(img).to(cuda_dev)
    assert encoder.encode([dev], bgr=True)[0] == P.encode_host(img, bgr=True) != encoder.encode([dev], bgr=False)[0]


def mixed_batch(cuda_dev):
    rng = np.random.default_rng(5)
    chw = torch.from_numpy(rng.random((3, 40, 56), dtype=np.float32) * 255).to(cuda_dev)
    sheet = torch.from_numpy(K.image("render", 64, 200, 3)).to(cuda_dev)
    return [torch.from_numpy(K.image("render", 256, 512, 3)).to(cuda_dev),
            chw.permute(1, 2, 0),
            sheet[3:50, 20:133, :],
            torch.from_numpy(K.image("noise", 17, 33, 4)).to(cuda_dev),
            torch.from_numpy(K.image("gradient", 7, 1, 1)).to(cuda_dev)[..., 0],
            torch.from_numpy(K.image("flat", 130, 129, 1)).to(cuda_dev),
            (sheet[:, :64, :].float() / 255).contiguous()]


def test_mixed_batch_equals_each_alone_and_a_second_call(P, encoder, cuda_dev):
    images = mixed_batch(cuda_dev)
    together = encoder.encode(images, rounding="trunc")
    for i, img in enumerate(images):
        assert encoder.encode([img], rounding="trunc")[0] == together[i], i
        host = P.encode_host(img.cpu().numpy(), rounding="trunc")
        assert together[i] == host, (i, first_difference(together[i], host))
    assert encoder.encode(images, rounding="trunc") == together
    assert encoder.encode(images[::-1], rounding="trunc") == together[::-1]


def test_one_filter_workgroup_spans_three_items(P, encoder, cuda_dev):
    # heights 1, 2 and 5: rows 0 ... 3 of the batch, one 4-row workgroup of the filter kernel, belong to items 0, 1, 1 and 2, so the
    # search for a row's item ends at every item inside one workgroup; widths below, at and one past the 64 lanes of a row's wave
    images = [K.image("noise", 1, 3, 3), K.image("render", 2, 64, 1), K.image("noise", 5, 65, 4)]
    files = encoder.encode([torch.from_numpy(img).to(cuda_dev) for img in images], bgr=False)
    for i, (img, data) in enumerate(zip(images, files)):
        want = P.encode_host(img, bgr=False)
        assert data == want, (i, first_difference(data, want))


def test_imwrite_and_imwrite_batch(P, cuda_dev, tmp_path):
    bgr = K.image("render", 48, 80, 3)
    rgb = bgr[..., ::-1]
    path = tmp_path / "device.png"
    assert P.imwrite(str(path), torch.from_numpy(bgr).to(cuda_dev)) is True
    assert np.array_equal(R.read(path.read_bytes())[0], rgb)
    path = tmp_path / "host.PNG"
    assert P.imwrite(str(path), bgr, device=cuda_dev) is True
    assert np.array_equal(R.read(path.read_bytes())[0], rgb)
    grey = K.image("gradient", 33, 17, 1)[..., 0]
    images = [torch.from_numpy(bgr).to(cuda_dev), grey, torch.from_numpy(K.image("noise", 9, 9, 4)).to(cuda_dev)]
    paths = [str(tmp_path / f"b{i}.png") for i in range(3)]
    assert P.imwrite_batch(paths, images, device=cuda_dev) is True
    want = [rgb, grey[..., None], K.image("noise", 9, 9, 4)[..., [2, 1, 0, 3]]]
    for p, w in zip(paths, want):
        with open(p, "rb") as f:
            data = f.read()
        assert np.array_equal(R.read(data)[0], w)
    Image = pytest.importorskip("PIL.Image")
    for p, w in zip(paths, want):
        assert np.array_equal(np.asarray(Image.open(p)).reshape(w.shape), w)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO((tmp_path / "device.png").read_bytes()))), rgb)


def test_larger_images_after_smaller_on_one_handle(P, cuda_dev):
    e = P.PNGEncoder(cuda_dev)
    try:
        small = K.image("render", 17, 33, 3)
        large = K.image("render", 256, 512, 3)
        assert e.encode([torch.from_numpy(small).to(cuda_dev)])[0] == P.encode_host(small)
        files = e.encode([torch.from_numpy(large).to(cuda_dev), torch.from_numpy(small).to(cuda_dev)])
        assert files[0] == P.encode_host(large) and files[1] == P.encode_host(small)
        assert e.encode([torch.from_numpy(small).to(cuda_dev)])[0] == P.encode_host(small)
    finally:
        e.close()


def test_large_streams_copied_out_in_chunks(P, encoder, cuda_dev):
    # three incompressible panels: each stream is longer than one chunk of the copy-out (its CRC is combined from the chunks'), and the
    # call is large enough for the chunks to be shared among threads
    images = [np.random.default_rng(40 + i).integers(0, 256, (256, 512, 3), dtype=np.uint8) for i in range(3)]
    files = encoder.encode([torch.from_numpy(a).to(cuda_dev) for a in images], bgr=False)
    assert sum(map(len, files)) > 1 << 20
    for a, data in zip(images, files):
        assert data == P.encode_host(a, bgr=False)
        assert np.array_equal(R.read(data)[0], a)


def test_refusal_leaves_the_handle_usable(P, encoder, cuda_dev):
    with pytest.raises(P.PngUnsupported, match="item 1.*2 channels"):
        encoder.encode([torch.zeros(4, 4, 3, dtype=torch.uint8, device=cuda_dev), torch.zeros(4, 4, 2, dtype=torch.uint8, device=cuda_dev)])
    img = K.image("noise", 3, 5, 3)
    assert encoder.encode([torch.from_numpy(img).to(cuda_dev)])[0] == P.encode_host(img)
