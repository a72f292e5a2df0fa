"""Renderer on the GPU (-m gpu): csrc/render.hip through tokenhmr_amd.render against the NumPy restatement of the contract
(tests/render_numpy.py) — exact coverage / alpha, winning faces equal up to depth ties, RGB within one 8-bit step — on synthetic
scenes, on 64 crops from a real forward, on a full frame, and along demo.py's rendering loop."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import render_numpy as RN

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
LIGHT_BLUE = (0.65098039, 0.74117647, 0.85882353)


class _N(dict):
    __getattr__ = dict.__getitem__


def _cfg(focal=5000, res=256):
    return _N(EXTRA=_N(FOCAL_LENGTH=focal), MODEL=_N(IMAGE_SIZE=res, IMAGE_MEAN=MEAN, IMAGE_STD=STD, BBOX_SHAPE=[192, 256]))


def _compare(gpu, gpu_ids, ref, faces, S, rgb_channels=3):
    """alpha / coverage exact; a different winner only where the two depths tie within 1e-5 relative; RGB within 1/255 of
    the restatement's — resolved with the GPU's winners where a tie went the other way (two faces at one depth, e.g. across a
    fold, need not share a colour)."""
    gpu, gpu_ids = np.asarray(gpu), np.asarray(gpu_ids).astype(np.int64)
    ref_ids = ref["ids"]
    assert gpu_ids.shape == ref_ids.shape
    np.testing.assert_array_equal(gpu_ids >= 0, ref_ids >= 0)
    if gpu.shape[-1] == 4:
        np.testing.assert_array_equal(gpu[..., 3], ref["out"][..., 3])
    diff = np.nonzero(gpu_ids != ref_ids)
    if len(diff[0]):
        _, py, px, s = diff
        dg = np.array([RN.sample_depth(ref["fix"], ref["Z"], faces, g, x, y, k, S) for g, x, y, k in zip(gpu_ids[diff], px, py, s)])
        dr = ref["depth"][diff]
        assert (np.abs(dg - dr) <= 1e-5 * np.abs(dr)).all(), (len(dr), np.abs(dg - dr).max())
    expect = ref["out"] if not len(diff[0]) else RN.resolve(ref, gpu_ids)
    err = np.abs(gpu[..., :rgb_channels] - expect[..., :rgb_channels])
    assert err.max(initial=0) <= 1 / 255 + 1e-6, err.max()
    return len(diff[0])


def _scene_meshes(kind):
    if kind == "sphere":
        v, f = RN.uv_sphere(40, 20, 1.0)
        return f, v[None], np.array([[0.1, -0.05, 6.0]])
    if kind == "torus":
        v, f = RN.torus()
        R = np.array([[1, 0, 0], [0, np.cos(1.0), -np.sin(1.0)], [0, np.sin(1.0), np.cos(1.0)]])
        return f, (v @ R.T)[None], np.array([[0.0, 0.1, 5.0]])
    v, f = RN.uv_sphere(40, 20, 1.0)
    return f, np.stack([v, v * 0.8]), np.array([[-0.4, 0.0, 6.0], [0.5, 0.2, 6.3]])      # two interpenetrating spheres


@pytest.mark.parametrize("size", [(256, 256), (640, 480)])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("kind", ["sphere", "torus", "two_spheres"])
def test_synthetic_scenes_match_the_restatement(built_lib, cuda_dev, kind, S, size):
    from tokenhmr_amd import render as R
    W, H = size
    faces, verts, cam_t = _scene_meshes(kind)
    r = R.Renderer(_cfg(focal=600, res=W), faces, device=cuda_dev, samples=S)
    # one image holding every mesh (render_rgba_multiple's scene)
    out, ids = r.render_scene(verts, cam_t, W, H, rot_axis=[0, 1, 0], rot_angle=15, mesh_base_color=(0.9, 0.6, 0.3), scene_bg_color=(0.2, 0.3, 0.4),
                              return_ids=True)
    sc = R.build_scene("rgba", W, H, 600, rot_angle=15, rot_axis=[0, 1, 0], mesh_base_color=(0.9, 0.6, 0.3), scene_bg_color=(0.2, 0.3, 0.4))
    ref = RN.render(sc, faces, verts, cam_t, samples=S, one_image=True)
    assert (ref["ids"] >= 0).sum() > 1000
    _compare(out.cpu().numpy()[None], ids.cpu().numpy()[None], ref, faces, S)
    # per-image crops (Renderer.__call__'s scene), composited over a crop, with and without the side view
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(verts.shape[0], 3, H, W, generator=g)
    for side in (False, True):
        out, ids = r.render_batch(torch.as_tensor(verts, dtype=torch.float32), torch.as_tensor(cam_t, dtype=torch.float32), imgs, side_view=side,
                                  mesh_base_color=(0.3, 0.8, 0.5), scene_bg_color=(1, 1, 1), return_ids=True)
        sc = R.build_scene("call", W, H, 600, np.zeros(3), side, 90, mesh_base_color=(0.3, 0.8, 0.5), scene_bg_color=(1, 1, 1))
        ref = RN.render(sc, faces, verts, cam_t, samples=S, images=None if side else imgs.numpy(), mean=MEAN, std=STD)
        _compare(out.cpu().numpy(), ids.cpu().numpy(), ref, faces, S)


def _forward_crops(cuda_dev, B=64):
    """B crops of a real forward (synthetic weights) over a synthetic body: an ellipsoid with exactly SMPL's 6890 vertices and
    13,776 faces (a closed genus-0 triangulation) skinned rigidly to the root, so the forward's vertices form a closed surface."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.model import TokenHMR
    cfg = HMRConfig(vit_depth=2, dec_depth=2)
    sd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    v, f = RN.uv_sphere(84, 83, 1.0)
    assert v.shape[0] == 6890 and f.shape[0] == 13776
    smpl["v_template"] = torch.as_tensor(v * np.array([0.25, 0.8, 0.18]), dtype=torch.float32)
    smpl["shapedirs"] = smpl["shapedirs"] * 0.05
    smpl["posedirs"] = smpl["posedirs"] * 0.0
    w = torch.zeros_like(smpl["lbs_weights"])
    w[:, 0] = 1.0
    smpl["lbs_weights"] = w
    smpl["faces"] = torch.as_tensor(f)
    model = TokenHMR.from_state(cfg, sd, tok, smpl, max_batch=B, device=cuda_dev)
    g = torch.Generator().manual_seed(11)
    img = torch.randn(B, 3, 256, 256, generator=g)
    with torch.no_grad():
        out = model({"img": img.to(cuda_dev)})
    verts = out["pred_vertices"].float()
    # synthetic weights give an arbitrary camera: keep the predicted offsets, bounded, at a depth that frames the body
    t = out["pred_cam_t"].float().clone()
    t[:, :2] = t[:, :2].clamp(-0.3, 0.3)
    t[:, 2] = 2 * 5000 / (256 * 0.9)
    return model, f, verts, t, img, out


def test_64_crops_equal_their_single_calls_and_the_restatement(built_lib, cuda_dev):
    from tokenhmr_amd import render as R
    model, faces, verts, cam_t, img, _ = _forward_crops(cuda_dev)
    r = R.Renderer(_cfg(), model.smpl.faces, device=cuda_dev)
    batch, ids = r.render_batch(verts, cam_t, img.to(cuda_dev), mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1), return_ids=True)
    batch, ids = batch.cpu().numpy(), ids.cpu().numpy()
    for n in range(verts.shape[0]):
        t = cam_t[n].cpu().numpy().astype(np.float64)
        one = r(verts[n].cpu().numpy(), t, img[n], mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1))
        assert one.dtype == np.float32 and one.shape == (256, 256, 3)
        assert np.array_equal(one, batch[n]), n
    sc = R.build_scene("call", 256, 256, 5000, np.zeros(3), mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1))
    ref = RN.render(sc, faces, verts.cpu().numpy(), cam_t.cpu().numpy(), images=img.numpy(), mean=MEAN, std=STD)
    assert (ref["ids"] >= 0).mean() > 0.05
    _compare(batch, ids, ref, faces, 4)


def _frame_placement(cam_t_crop_cam, n=8):
    from tokenhmr_amd.render import cam_crop_to_full
    cols = np.arange(n) % 4
    rows = np.arange(n) // 4
    centers = torch.tensor(np.stack([240 + 480 * cols, 270 + 540 * rows], 1), dtype=torch.float32)
    sizes = torch.full((n,), 400.0)
    img_size = torch.tensor([[1920.0, 1080.0]]).repeat(n, 1)
    cam = cam_t_crop_cam.clone()
    cam[:, 0] = 0.9
    cam[:, 1:] = cam[:, 1:].clamp(-0.2, 0.2)
    focal = 5000 / 256 * 1920
    return cam_crop_to_full(cam, centers, sizes, img_size, focal), focal


def test_full_frame_matches_the_restatement_and_is_order_free(built_lib, cuda_dev):
    from tokenhmr_amd import render as R
    model, faces, verts, _, _, out = _forward_crops(cuda_dev, B=8)
    cam_full, focal = _frame_placement(out["pred_cam"].float().cpu())
    r = R.Renderer(_cfg(), model.smpl.faces, device=cuda_dev)
    v = verts.cpu().numpy()
    t = cam_full.numpy()
    img, ids = r.render_scene(v, t, 1920, 1080, focal, mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1), return_ids=True)
    img, ids = img.cpu().numpy(), ids.cpu().numpy()
    assert img.shape == (1080, 1920, 4) and img.dtype == np.float32
    sc = R.build_scene("rgba", 1920, 1080, focal, mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1))
    ref = RN.render(sc, faces, v, t, one_image=True)
    touched = np.unique(ref["ids"][ref["ids"] >= 0] // faces.shape[0])
    assert len(touched) == 8
    _compare(img[None], ids[None], ref, faces, 4)
    again = r.render_scene(v, t, 1920, 1080, focal, mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1)).cpu().numpy()
    assert np.array_equal(again, img)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    permuted = r.render_scene(v[perm], t[perm], 1920, 1080, focal, mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1)).cpu().numpy()
    assert np.array_equal(permuted, img)


def test_demo_rendering_loop(built_lib, cuda_dev, tmp_path):
    """demo.py:71-143 without the reference: ViTDetDataset -> model(batch) -> cam_crop_to_full -> Renderer.__call__ (+ side view)
    -> render_rgba_multiple -> the overlay -> vertices_to_trimesh(...).export(.obj)."""
    from tokenhmr_amd import render as R
    from tokenhmr_amd.preprocess import ViTDetDataset
    model, faces, _, _, _, _ = _forward_crops(cuda_dev, B=8)
    mcfg = _cfg()
    rng = np.random.default_rng(2)
    H, Wd = 480, 640
    img_cv2 = rng.integers(0, 255, (H, Wd, 3), dtype=np.uint8)
    boxes = np.array([[40, 60, 260, 460], [330, 40, 600, 470]], float)
    batch = ViTDetDataset(mcfg, img_cv2, boxes, device=cuda_dev).batch()
    with torch.no_grad():
        out = model(batch)
    renderer = R.Renderer(mcfg, faces=model.smpl.faces, device=cuda_dev)
    img_size = batch["img_size"].float()
    scaled_focal_length = mcfg.EXTRA.FOCAL_LENGTH / mcfg.MODEL.IMAGE_SIZE * img_size.max()
    pred_cam = out["pred_cam"].clone()
    pred_cam[:, 0] = 0.9                                     # synthetic weights: a camera that frames the body
    pred_cam_t_full = R.cam_crop_to_full(pred_cam, batch["box_center"].float(), batch["box_size"].float(), img_size,
                                         scaled_focal_length).detach().cpu().numpy()
    DEFAULT_MEAN, DEFAULT_STD = 255. * np.array(MEAN), 255. * np.array(STD)
    all_verts, all_cam_t = [], []
    for n in range(batch["img"].shape[0]):
        white_img = (torch.ones_like(batch["img"][n]).cpu() - torch.tensor(DEFAULT_MEAN)[:, None, None] / 255) / (torch.tensor(DEFAULT_STD)[:, None, None] / 255)
        verts = out["pred_vertices"][n].detach().cpu().numpy()
        cam_t = out["pred_cam_t"][n].detach().cpu().numpy().copy()
        cam_t[2] = 2 * 5000 / (256 * 0.9)
        before = cam_t.copy()
        regression_img = renderer(verts, cam_t, batch["img"][n], mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1))
        assert cam_t[0] == -before[0] and cam_t[1] == before[1]            # the reference's in-place negation, kept
        side_img = renderer(verts, before.copy(), white_img, mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1), side_view=True)
        assert regression_img.shape == side_img.shape == (256, 256, 3) and regression_img.dtype == side_img.dtype == np.float32
        assert (side_img != 1.0).any() and (regression_img != batch["img"][n].cpu().numpy().transpose(1, 2, 0)).any()
        all_verts.append(verts)
        all_cam_t.append(pred_cam_t_full[n])
        path = str(tmp_path / f"p{n}.obj")
        renderer.vertices_to_trimesh(verts, pred_cam_t_full[n].copy(), LIGHT_BLUE).export(path)
        vs, fs = [], []
        for line in open(path):
            if line.startswith("v "):
                vs.append([float(x) for x in line.split()[1:]])
            elif line.startswith("f "):
                fs.append([int(x) for x in line.split()[1:]])
        vs, fs = np.array(vs), np.array(fs)
        expect = (verts.astype(np.float64) + pred_cam_t_full[n]) * np.array([1.0, -1.0, -1.0])
        np.testing.assert_allclose(vs[:, :3], expect, atol=1e-6)
        np.testing.assert_allclose(vs[:, 3:], np.tile(np.round(np.array(LIGHT_BLUE) * 255) / 255, (len(vs), 1)), atol=1e-7)
        np.testing.assert_array_equal(fs, np.asarray(faces) + 1)
    cam_view = renderer.render_rgba_multiple(all_verts, cam_t=all_cam_t, render_res=img_size[0], mesh_base_color=LIGHT_BLUE,
                                             scene_bg_color=(1, 1, 1), focal_length=scaled_focal_length)
    assert cam_view.shape == (H, Wd, 4) and cam_view.dtype == np.float32 and (cam_view[..., 3] > 0).sum() > 500
    input_img = img_cv2.astype(np.float32)[:, :, ::-1] / 255.0
    input_img = np.concatenate([input_img, np.ones_like(input_img[:, :, :1])], axis=2)
    overlay = input_img[:, :, :3] * (1 - cam_view[:, :, 3:]) + cam_view[:, :, :3] * cam_view[:, :, 3:]
    assert overlay.shape == (H, Wd, 3) and np.isfinite(overlay).all()
    sc = R.build_scene("rgba", Wd, H, float(scaled_focal_length), mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1))
    ref = RN.render(sc, faces, np.stack(all_verts), np.stack(all_cam_t), one_image=True)
    np.testing.assert_array_equal(cam_view[..., 3], ref["out"][0, ..., 3])


def test_scratch_growth_and_errors(built_lib, cuda_dev):
    from tokenhmr_amd import _cabi
    from tokenhmr_amd import render as R
    faces, verts, cam_t = _scene_meshes("two_spheres")
    grown = R.Renderer(_cfg(focal=600), faces, device=cuda_dev)
    small = grown.render_scene(verts, cam_t, 320, 240, 300).cpu().numpy()
    big = grown.render_scene(verts, cam_t, 1280, 960, 1200).cpu().numpy()
    fresh = R.Renderer(_cfg(focal=600), faces, device=cuda_dev)
    assert np.array_equal(fresh.render_scene(verts, cam_t, 1280, 960, 1200).cpu().numpy(), big)
    assert np.array_equal(grown.render_scene(verts, cam_t, 320, 240, 300).cpu().numpy(), small)
    # invalid descriptors come back as THMR_ERR_INVALID with text, and the handle keeps working
    L = grown.lib
    h = grown._handle(verts.shape[1])
    v = torch.as_tensor(verts, dtype=torch.float32, device=cuda_dev).contiguous()
    t = torch.as_tensor(cam_t, dtype=torch.float32, device=cuda_dev).contiguous()
    o = torch.empty(1, 240, 320, 4, device=cuda_dev)
    sc = R.build_scene("rgba", 320, 240, 300.0)
    for field, value, text in (("samples", 2, b"samples"), ("width", 0, b"image size"), ("height", 9000, b"image size"),
                               ("out_channels", 5, b"out_channels"), ("n_lights", 17, b"n_lights"), ("mode", 7, b"mode")):
        d = R.make_desc(sc, 4, _cabi.RENDER_ONE_IMAGE, 4)
        setattr(d, field, value)
        assert L.thmr_renderer_run(h, C.byref(d), v.data_ptr(), t.data_ptr(), 2, None, o.data_ptr(), None) == -1
        assert text in L.thmr_renderer_last_error(h), L.thmr_renderer_last_error(h)
    d = R.make_desc(sc, 4, _cabi.RENDER_ONE_IMAGE, 4)
    assert L.thmr_renderer_run(h, C.byref(d), v.data_ptr(), t.data_ptr(), 0, None, o.data_ptr(), None) == -1
    assert L.thmr_renderer_run(h, C.byref(d), v.data_ptr(), t.data_ptr(), 2, o.data_ptr(), o.data_ptr(), None) == -1   # bg needs 3 channels
    torch.cuda.synchronize()
    assert np.array_equal(grown.render_scene(verts, cam_t, 320, 240, 300).cpu().numpy(), small)


def test_one_handle_grown_then_reused_without_host_sync_equals_fresh_handles(built_lib, cuda_dev):
    """Reuse after growth, and the capacity bookkeeping: one handle, one stream, no host synchronisation between the calls.  1 mesh,
    then 3 (every scratch buffer grows), then 1 again inside the grown buffers.  64x64 images, 1 sample.  Every result, colours and
    winning ids, is bit-equal to the same call on a renderer of its own.  (A missing synchronisation before the growth would not
    show here: hipFree waits for the device by itself.)"""
    from tokenhmr_amd import _cabi
    from tokenhmr_amd import render as R
    faces, verts, cam_t = _scene_meshes("sphere")
    v3 = torch.as_tensor(np.repeat(verts, 3, axis=0) * np.array([1.0, 0.7, 1.3])[:, None, None], dtype=torch.float32).to(cuda_dev)
    t3 = torch.as_tensor(cam_t + np.array([[0.0, 0.0, 0.0], [0.8, -0.6, 1.0], [-1.2, 0.9, -2.0]]), dtype=torch.float32).to(cuda_dev)
    sc = R.build_scene("call", 64, 64, 120.0, np.zeros(3), mesh_base_color=(0.9, 0.6, 0.3), scene_bg_color=(0.2, 0.3, 0.4))
    steps = [slice(0, 1), slice(0, 3), slice(2, 3)]
    torch.cuda.synchronize()

    def call(r, k):
        return r._run(sc, v3[k], t3[k], _cabi.RENDER_PER_IMAGE, 4, return_ids=True)

    one = R.Renderer(_cfg(focal=120, res=64), faces, device=cuda_dev, samples=1)
    got = [call(one, k) for k in steps]
    torch.cuda.synchronize()
    one.close()
    for i, (k, (out, ids)) in enumerate(zip(steps, got)):
        fresh = R.Renderer(_cfg(focal=120, res=64), faces, device=cuda_dev, samples=1)
        want, want_ids = call(fresh, k)
        assert torch.equal(out.cpu(), want.cpu()) and torch.equal(ids.cpu(), want_ids.cpu()), i
        fresh.close()
        assert (ids >= 0).sum() > 100 * ids.shape[0] and (ids < 0).any(), i          # every image shows its mesh against background
    assert torch.equal(got[2][0][0], got[1][0][2])                                    # the same mesh, alone or third of three
