"""compression="dynamic" on the device against the CPU restatement (thmr_png_encode_host in the dynamic mode, itself read by zlib, Pillow
and a block walker in tests/test_png_dynamic_host.py): the same files byte for byte at the segment edges, over shapes x channels x
kinds, on wide images whose row matches give tokens of more than 33 bits, for strided and float images, and for one call that mixes
fixed and dynamic items (a batch with a dynamic item runs the DYNAMIC instantiation of png_deflate_kernel for all of its segments; a
batch without one runs the other).  tests/test_gpu_png.py stays the proof that the fixed mode is unchanged."""
import numpy as np
import pytest
import torch

import _png_cases as K
from test_gpu_png import first_difference, mixed_batch
from test_png_dynamic_host import dynamic_file, wide_cases, wide_file

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (17, 33), (256, 192)]


@pytest.fixture(scope="module")
def P(built_lib):
    from tokenhmr_amd import png
    return png


@pytest.fixture(scope="module")
def encoder(P, cuda_dev):
    e = P.PNGEncoder(cuda_dev)
    yield e
    e.close()


@pytest.mark.parametrize("kind", K.EDGE_KINDS)
def test_segment_edge_cases_equal_the_host_files(P, encoder, cuda_dev, kind):
    cases = [(n, img) for n, img in K.edge_cases(P.segment_bytes()) if n.startswith(kind)]
    assert len(cases) == 5
    files = encoder.encode([torch.from_numpy(img).to(cuda_dev) for _, img in cases], bgr=False, compression="dynamic")
    for (name, _), data in zip(cases, files):
        want = dynamic_file("edge", name)
        assert data == want, (name, first_difference(data, want))


@pytest.mark.parametrize("c", [1, 3, 4])
def test_round_trip_cases_equal_the_host_files(P, encoder, cuda_dev, c):
    cases = [(n, img) for n, img in K.roundtrip_cases() if img.shape[2] == c and img.shape[:2] in SHAPES]
    assert len(cases) == len(SHAPES) * len(K.KINDS)
    files = encoder.encode([torch.from_numpy(img).to(cuda_dev) for _, img in cases], bgr=False, compression="dynamic")
    for (name, _), data in zip(cases, files):
        want = dynamic_file("roundtrip", name)
        assert data == want, (name, first_difference(data, want))


def test_wide_images_equal_the_host_files(P, encoder, cuda_dev):
    # row distances of 5761 and 11521 bytes (11 and 12 extra bits), and tokens of more than 33 bits that start at bit 30 or 31 of a word
    cases = wide_cases()
    files = encoder.encode([torch.from_numpy(img).to(cuda_dev) for _, img in cases], bgr=False, compression="dynamic")
    for (name, _), data in zip(cases, files):
        want = wide_file(name)
        assert data == want, (name, first_difference(data, want))


def test_conversion_cases_equal_the_host_files(P, encoder, cuda_dev):
    for name, img, scale, rounding in K.conversion_cases():
        data = encoder.encode([torch.from_numpy(img).to(cuda_dev)], scale=scale, rounding=rounding, compression="dynamic")[0]
        want = dynamic_file("conversion", name)
        assert data == want, (name, first_difference(data, want))


def test_stride_cases_equal_the_host_files(P, encoder, cuda_dev):
    for name, view, kw in K.stride_cases():
        base = view.base if view.base is not None else view
        dev = torch.from_numpy(np.ascontiguousarray(base)).to(cuda_dev)
        off = (view.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // view.itemsize
        tview = torch.as_strided(dev, view.shape, [s // view.itemsize for s in view.strides], off)
        assert not tview.is_contiguous()
        data = encoder.encode([tview], compression="dynamic", **kw)[0]
        want = dynamic_file("stride", name)
        assert data == want, (name, first_difference(data, want))


def test_one_call_mixing_fixed_and_dynamic_items(P, encoder, cuda_dev):
    images = mixed_batch(cuda_dev)
    modes = ["dynamic" if i % 2 == 0 else "fixed" for i in range(len(images))]
    host = {m: [P.encode_host(img.cpu().numpy(), rounding="trunc", compression=m) for img in images] for m in ("fixed", "dynamic")}
    assert host["fixed"][0] != host["dynamic"][0]
    for order in (modes, modes[::-1], ["dynamic"] * len(images), ["fixed"] * len(images)):
        together = encoder.encode(images, rounding="trunc", compression=order)
        for i, m in enumerate(order):
            assert together[i] == host[m][i], (order, i, first_difference(together[i], host[m][i]))
    # each image alone, through the kernel its own mode selects
    for i, img in enumerate(images):
        for m in ("fixed", "dynamic"):
            assert encoder.encode([img], rounding="trunc", compression=m)[0] == host[m][i], (i, m)
    with pytest.raises(ValueError, match="compression"):
        encoder.encode(images, compression=["dynamic"])
    for bad in ("best", None, 1, ["best"], [None]):
        with pytest.raises(ValueError, match="compression"):
            encoder.encode(images[:1], compression=bad)


def test_imwrite_and_imwrite_batch_take_the_mode(P, cuda_dev, tmp_path):
    bgr = K.image("render", 48, 80, 3)
    dev = torch.from_numpy(bgr).to(cuda_dev)
    assert P.imwrite(str(tmp_path / "a.png"), dev, [16, 9], compression="dynamic") is True        # cv2's params: accepted and ignored
    assert (tmp_path / "a.png").read_bytes() == P.encode_host(bgr, compression="dynamic")
    paths = [str(tmp_path / f"b{i}.png") for i in range(2)]
    assert P.imwrite_batch(paths, [dev, bgr], compression="dynamic", device=cuda_dev) is True
    for p in paths:
        with open(p, "rb") as f:
            assert f.read() == P.encode_host(bgr, compression="dynamic")
    assert P.imwrite(str(tmp_path / "c.png"), dev) is True
    assert (tmp_path / "c.png").read_bytes() == P.encode_host(bgr)
