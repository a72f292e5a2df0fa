"""MeshRenderer on the GPU (-m gpu): thmr_renderer_sheet through tokenhmr_amd.render.MeshRenderer against the NumPy restatement
(tests/overlay_numpy.py).  Everything is compared for EQUALITY: the draw-list records, the skeleton panels, the hard-mask mesh
panels (against the same handle's own RGBA output, which tests/test_gpu_render.py holds to tests/render_numpy.py) and the whole
contact sheet along eval.py's render_predictions."""
import numpy as np
import pytest
import torch

import tests.test_gpu_render as TGR
from tests import overlay_numpy as ON
from tests.test_overlay_host import fixture_cases

pytestmark = pytest.mark.gpu

TRI = np.array([[0, 1, 2]])


def _renderer(cuda_dev, res=256, faces=TRI):
    from tokenhmr_amd import render as R
    return R.MeshRenderer(TGR._cfg(res=res), faces, device=cuda_dev)


def _skeleton_sheet(mr, images, pred, gt):
    """Image + skeleton panels only (no mesh): (canvas (3, H, tiles W) numpy, records numpy); gt is changed in place on the device."""
    from tokenhmr_amd import _cabi
    n = 1 + (pred is not None) + (gt is not None)
    canvas, rec = mr._sheet(3, images, None, None, _cabi.SHEET_IMAGE, pred, gt, nrow=n * images.shape[0], padding=0)
    return canvas.cpu().numpy(), rec.cpu().numpy()


def _expected_records(pred, gt, res, W, H):
    """Restatement: records in the device's order (predicted skeletons first, then ground truth) and the gt array afterwards."""
    recs = []
    if pred is not None:
        recs += [ON.build_records(ON.body_from_pred(p, res), W, H) for p in pred]
    gt_after = None
    if gt is not None:
        gt_after = gt.copy()
        recs += [ON.build_records(ON.body_from_gt(g, res), W, H) for g in gt_after]
    return (np.stack(recs) if recs else np.zeros((0, ON.N_REC, ON.N_WORDS), np.int32)), gt_after


def test_fixture_skeletons_give_the_restatements_records_and_panels(built_lib, cuda_dev):
    g = torch.Generator().manual_seed(5)
    for c in fixture_cases():
        res = c["res"]
        mr = _renderer(cuda_dev, res)
        img = torch.rand(1, 3, res, res, generator=g)
        kp = torch.as_tensor(c["keypoints"][None]).to(cuda_dev)
        pred, gt = (kp, None) if c["kind"] == "pred" else (None, kp)
        canvas, rec = _skeleton_sheet(mr, img.to(cuda_dev), pred, gt)
        want, gt_after = _expected_records(c["keypoints"][None] if pred is not None else None, c["keypoints"][None] if gt is not None else None, res, res, res)
        np.testing.assert_array_equal(rec, want, err_msg=c["name"])
        assert ON.calls_of(rec[0]) == ON.calls_in_range(c["calls"]), c["name"]          # and so the reference's recorded calls
        if gt is not None:
            np.testing.assert_array_equal(kp.cpu().numpy()[0], c["keypoints_after"], err_msg=c["name"])
        assert np.array_equal(canvas[:, :, :res], img[0].numpy()), c["name"]
        assert np.array_equal(canvas[:, :, res:], ON.skeleton_panel(img[0].numpy(), want[0])), c["name"]
        mr.close()


@pytest.mark.parametrize("res,B", [(256, 64), (1024, 1)])
def test_random_skeleton_panels_are_bit_identical_to_the_restatement(built_lib, cuda_dev, res, B):
    rng = np.random.default_rng(res + B)
    mr = _renderer(cuda_dev, res)
    img = rng.random((B, 3, res, res), dtype=np.float32)
    pred = rng.uniform(-0.7, 0.7, (B, 44, 2)).astype(np.float32)
    gt = np.concatenate([rng.uniform(-0.6, 0.6, (B, 44, 2)), rng.choice([0.0, 0.05, 0.1, 0.3, 1.0], (B, 44, 1))], 2).astype(np.float32)
    dev = lambda a: torch.as_tensor(a).to(cuda_dev)
    gt_dev = dev(gt)
    canvas, rec = _skeleton_sheet(mr, dev(img), dev(pred), gt_dev)
    want, gt_after = _expected_records(pred, gt, res, res, res)
    np.testing.assert_array_equal(rec, want)
    np.testing.assert_array_equal(gt_dev.cpu().numpy(), gt_after)
    assert (want[:, :, 0] != 0).sum() > 40 * B                                        # the skeletons are drawn
    tiles = canvas.reshape(3, res, B, 3, res)
    for b in range(B):
        assert np.array_equal(tiles[:, :, b, 0], img[b])
        assert np.array_equal(tiles[:, :, b, 1], ON.skeleton_panel(img[b], want[b])), b
        assert np.array_equal(tiles[:, :, b, 2], ON.skeleton_panel(img[b], want[B + b])), b
    again, rec2 = _skeleton_sheet(mr, dev(img), dev(pred), dev(gt))
    assert np.array_equal(again, canvas) and np.array_equal(rec2, rec)                # run to run
    mr.close()


def test_odd_sizes_and_a_ragged_last_row(built_lib, cuda_dev):
    """50 x 37 images, keypoints scaled by another img_res, padding 1, 9 tiles 2 to a row (the last row holds one tile): a canvas whose
    width is no multiple of 4 and cells that start at odd columns."""
    from tokenhmr_amd import _cabi
    rng = np.random.default_rng(8)
    B, H, W, res = 3, 37, 50, 64
    mr = _renderer(cuda_dev, res)
    img = rng.random((B, 3, H, W), dtype=np.float32)
    pred = rng.uniform(-0.5, 0.4, (B, 44, 2)).astype(np.float32)
    gt = np.concatenate([rng.uniform(-0.5, 0.3, (B, 44, 2)), rng.choice([0.0, 1.0], (B, 44, 1))], 2).astype(np.float32)
    dev = lambda a: torch.as_tensor(a).to(cuda_dev)
    for nrow, pad in ((2, 1), (4, 0), (9, 5), (100, 2)):
        canvas, rec = mr._sheet(3, dev(img), None, None, _cabi.SHEET_IMAGE, dev(pred), dev(gt), nrow=nrow, padding=pad)
        want, _ = _expected_records(pred, gt, res, W, H)
        np.testing.assert_array_equal(rec.cpu().numpy(), want)
        tiles = []
        for b in range(B):
            tiles += [img[b], ON.skeleton_panel(img[b], want[b]), ON.skeleton_panel(img[b], want[B + b])]
        assert np.array_equal(canvas.cpu().numpy(), ON.make_grid(tiles, nrow, pad)), (nrow, pad)
    mr.close()


@pytest.fixture(scope="module")
def people(built_lib, cuda_dev):
    """8 people from a real forward of a synthetic-weight engine, images in 0 ... 1, random ground-truth keypoints."""
    model, faces, verts, cam_t, _, out = TGR._forward_crops(cuda_dev, B=8)
    g = torch.Generator().manual_seed(21)
    images = torch.rand(8, 3, 256, 256, generator=g).to(cuda_dev)
    rng = np.random.default_rng(21)
    gt = np.concatenate([rng.uniform(-0.45, 0.45, (8, 44, 2)), rng.choice([0.0, 0.05, 0.5, 1.0], (8, 44, 1))], 2).astype(np.float32)
    pred = out["pred_keypoints_2d"].float().reshape(8, -1, 2).contiguous()
    assert pred.shape == (8, 44, 2) and torch.isfinite(pred).all()
    return {"model": model, "verts": verts.contiguous(), "cam_t": cam_t.contiguous(), "images": images, "pred": pred, "gt": gt}


def _mesh_panels(mr, p):
    """where(alpha > 0.8, rgb, bg) from the handle's own RGBA renders: front over the image, side (x un-flipped) over ones."""
    from tokenhmr_amd import render as R
    front = mr.renderer.render_batch(p["verts"], p["cam_t"], return_rgba=True, width=256, height=256).cpu().numpy()
    side = mr.renderer.render_batch(p["verts"], R.side_translation(p["cam_t"]), side_view=True, return_rgba=True, width=256, height=256).cpu().numpy()
    img = p["images"].cpu().numpy()
    assert ((front[..., 3] > 0.8).mean() > 0.02) and ((side[..., 3] > 0.8).mean() > 0.01)
    assert set(np.unique(front[..., 3])) <= {np.float32(v / 255) for v in (0, 64, 127, 128, 191, 255)}     # 4 samples, 8-bit alpha
    return [ON.mesh_panel(front[b], img[b]) for b in range(8)], [ON.mesh_panel(side[b], None) for b in range(8)]


def _expected_sheet(mr, p, with_pred=True, with_gt=True, nrow=5, padding=2):
    img = p["images"].cpu().numpy()
    front, side = _mesh_panels(mr, p)
    rec, gt_after = _expected_records(p["pred"].cpu().numpy() if with_pred else None, p["gt"] if with_gt else None, 256, 256, 256)
    tiles = []
    for b in range(8):
        tiles += [img[b], front[b], side[b]]
        if with_pred:
            tiles.append(ON.skeleton_panel(img[b], rec[b]))
        if with_gt:
            tiles.append(ON.skeleton_panel(img[b], rec[(8 if with_pred else 0) + b]))
    nrow = nrow - (not with_pred) - (not with_gt)
    return ON.make_grid(tiles, nrow, padding), gt_after


def test_call_is_the_hard_mask_over_the_handles_own_rgba(people, cuda_dev):
    p = people
    mr = _renderer(cuda_dev, faces=p["model"].smpl.faces)
    front, side = _mesh_panels(mr, p)
    img = p["images"].cpu().numpy()
    for b in (0, 5):
        v = p["verts"][b].cpu().numpy()
        t = p["cam_t"][b].cpu().numpy().astype(np.float64)
        before = t.copy()
        one = mr(v, t, img[b].transpose(1, 2, 0), focal_length=5000)
        assert one.shape == (256, 256, 3) and one.dtype == np.float32
        assert np.array_equal(one.transpose(2, 0, 1), front[b])
        assert t[0] == -before[0] and t[1] == before[1] and t[2] == before[2]        # the reference's in-place negation
        two = mr(v, t, img[b].transpose(1, 2, 0), focal_length=5000, side_view=True)        # the second call sees (-tx, ty, tz) ...
        assert np.array_equal(two.transpose(2, 0, 1), side[b])
        assert np.array_equal(t, before)                                                # ... and restores the caller's array
    mr.close()


def test_contact_sheets_are_bit_identical_to_the_assembled_restatement(people, cuda_dev):
    p = people
    mr = _renderer(cuda_dev, faces=p["model"].smpl.faces)
    want, gt_after = _expected_sheet(mr, p)
    # device tensors in, device tensor out, nothing copied to the host
    gt_dev = torch.as_tensor(p["gt"]).to(cuda_dev)
    cam_before = p["cam_t"].clone()
    sheet = mr.visualize_tensorboard(p["verts"], p["cam_t"], p["images"], p["pred"], gt_dev)
    assert torch.is_tensor(sheet) and sheet.device == cuda_dev and sheet.dtype == torch.float32 and tuple(sheet.shape) == (3, 8 * 258 + 2, 5 * 258 + 2)
    assert np.array_equal(sheet.cpu().numpy(), want)
    assert np.array_equal(gt_dev.cpu().numpy(), gt_after) and torch.equal(p["cam_t"], cam_before)
    # the reference's NumPy arguments: the same values, the caller's arrays changed exactly as the reference changes them
    v_np, t_np, img_np, pred_np = (a.cpu().numpy() for a in (p["verts"], p["cam_t"], p["images"], p["pred"]))
    gt_np = p["gt"].copy()
    t_copy, pred_copy = t_np.copy(), pred_np.copy()
    sheet_np = mr.visualize_tensorboard(v_np, t_np, img_np, pred_np, gt_np, focal_length=np.full((8, 2), 123.0))
    assert torch.is_tensor(sheet_np) and sheet_np.device == cuda_dev and torch.equal(sheet_np, sheet)
    assert np.array_equal(gt_np, gt_after) and np.array_equal(t_np, t_copy) and np.array_equal(pred_np, pred_copy)
    # a keypoint set left out drops its column; both left out is visualize's sheet
    want_p, _ = _expected_sheet(mr, p, with_gt=False)
    assert np.array_equal(mr.visualize_tensorboard(p["verts"], p["cam_t"], p["images"], p["pred"], None).cpu().numpy(), want_p)
    want_g, _ = _expected_sheet(mr, p, with_pred=False)
    assert np.array_equal(mr.visualize_tensorboard(v_np, t_np, img_np, None, p["gt"].copy()).cpu().numpy(), want_g)
    want_0, _ = _expected_sheet(mr, p, with_pred=False, with_gt=False)
    assert want_0.shape == (3, 8 * 258 + 2, 3 * 258 + 2)
    assert np.array_equal(mr.visualize_tensorboard(p["verts"], p["cam_t"], p["images"], None, None).cpu().numpy(), want_0)
    assert np.array_equal(mr.visualize(v_np, t_np, img_np).cpu().numpy(), want_0)
    assert np.array_equal(mr.visualize(p["verts"], p["cam_t"], p["images"], focal_length=1.0).cpu().numpy(), want_0)
    # another nrow: 40 tiles, 4 to a row
    tiles_per_row = mr.visualize_tensorboard(p["verts"], p["cam_t"], p["images"], p["pred"], torch.as_tensor(p["gt"]).to(cuda_dev), nrow=4, padding=3)
    assert tuple(tiles_per_row.shape) == (3, 10 * 259 + 3, 4 * 259 + 3)                # a canvas width that is no multiple of 4
    assert np.array_equal(tiles_per_row.cpu().numpy(), _expected_sheet(mr, p, nrow=4, padding=3)[0])
    mr.close()


def test_eval_render_predictions_call_shape(people, cuda_dev):
    """eval.py:69-112 re-enacted: de-normalised batch images, .cpu().numpy() arguments, two sheets, the second one's columns 256 ... 1024
    appended to the first, 8-bit conversion."""
    p = people
    mesh_renderer = _renderer(cuda_dev, faces=p["model"].smpl.faces)
    mean = torch.tensor([0.485, 0.456, 0.406], device=cuda_dev).reshape(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=cuda_dev).reshape(1, 3, 1, 1)
    B = 8
    batch = {"img": (p["images"] - mean) / std, "keypoints_2d": torch.as_tensor(p["gt"]).to(cuda_dev)}
    output = {"pred_vertices": p["verts"], "pred_cam_t": p["cam_t"], "pred_keypoints_2d": p["pred"].reshape(B, -1),
              "focal_length": torch.full((B, 2), 5000.0, device=cuda_dev),
              "pred_vertices_gt": p["verts"].flip(0).contiguous(), "pred_keypoints_2d_gt": p["pred"].flip(0).contiguous()}
    batch_size = batch["keypoints_2d"].shape[0]
    images = batch["img"] * std + mean
    gt_keypoints_2d = batch["keypoints_2d"]
    num_images = min(batch_size, 8)
    sheets = []
    for vk, kk in (("pred_vertices", "pred_keypoints_2d"), ("pred_vertices_gt", "pred_keypoints_2d_gt")):
        pred_vertices = output[vk].detach().reshape(batch_size, -1, 3)
        focal_length = output["focal_length"].detach().reshape(batch_size, 2)
        pred_cam_t = output["pred_cam_t"].detach().reshape(batch_size, 3)
        pred_keypoints_2d = output[kk].detach().reshape(batch_size, -1, 2)
        predictions = mesh_renderer.visualize_tensorboard(pred_vertices[:num_images].cpu().numpy(), pred_cam_t[:num_images].cpu().numpy(),
                                                          images[:num_images].cpu().numpy(), pred_keypoints_2d[:num_images].cpu().numpy(),
                                                          gt_keypoints_2d[:num_images].cpu().numpy(),
                                                          focal_length=focal_length[:num_images].cpu().numpy())
        predictions = predictions.cpu().numpy().transpose(1, 2, 0) * 255
        sheets.append(np.clip(predictions, 0, 255).astype(np.uint8))
    predictions = np.concatenate([sheets[0], sheets[1][:, 256:256 * 4]], 1)
    assert predictions.shape == (8 * 258 + 2, 5 * 258 + 2 + 768, 3) and predictions.dtype == np.uint8
    assert np.array_equal(gt_keypoints_2d.cpu().numpy(), p["gt"])                    # the batch itself is untouched: .cpu().numpy() copies
    q = dict(p, images=images)
    want0, _ = _expected_sheet(mesh_renderer, q)
    want1, _ = _expected_sheet(mesh_renderer, dict(q, verts=output["pred_vertices_gt"], pred=output["pred_keypoints_2d_gt"]))
    to8 = lambda a: np.clip(a.transpose(1, 2, 0) * 255, 0, 255).astype(np.uint8)
    assert np.array_equal(predictions[:, :5 * 258 + 2], to8(want0)) and np.array_equal(predictions[:, 5 * 258 + 2:], to8(want1)[:, 256:1024])
    assert (sheets[0] != sheets[1]).any()
    mesh_renderer.close()


def test_sheet_descriptor_errors_leave_the_handle_usable(built_lib, cuda_dev):
    import ctypes as C
    from tokenhmr_amd import _cabi
    mr = _renderer(cuda_dev)
    img = torch.rand(2, 3, 32, 48, device=cuda_dev)
    pred = torch.zeros(2, 44, 2, device=cuda_dev)
    good, _ = _skeleton_sheet(mr, img, pred, None)
    L, h = mr.renderer.lib, mr.renderer._handle(3)
    canvas = torch.empty(3, 32, 4 * 48, device=cuda_dev)
    rec = torch.empty(2, 49, 12, dtype=torch.int32, device=cuda_dev)
    for field, value, text in (("n", 0, b"people"), ("width", 9000, b"image size"), ("nrow", 0, b"nrow"), ("panels", 8, b"panel"),
                               ("canvas_width", 100, b"canvas must be"), ("img_res", 0, b"img_res")):
        d = _cabi.SheetDesc(2, 48, 32, 256, _cabi.SHEET_IMAGE, 4, 0, 4 * 48, 32)
        setattr(d, field, value)
        assert L.thmr_renderer_sheet(h, C.byref(d), img.data_ptr(), None, None, pred.data_ptr(), None, rec.data_ptr(), canvas.data_ptr(), None) == -1
        assert text in L.thmr_renderer_last_error(h), L.thmr_renderer_last_error(h)
    d = _cabi.SheetDesc(2, 48, 32, 256, _cabi.SHEET_IMAGE | _cabi.SHEET_FRONT, 4, 0, 6 * 48, 32)
    assert L.thmr_renderer_sheet(h, C.byref(d), img.data_ptr(), None, None, None, None, None, canvas.data_ptr(), None) == -1      # no front render
    d = _cabi.SheetDesc(2, 48, 32, 256, _cabi.SHEET_IMAGE, 4, 0, 4 * 48, 32)
    assert L.thmr_renderer_sheet(h, C.byref(d), img.data_ptr(), None, None, pred.data_ptr(), None, None, canvas.data_ptr(), None) == -1   # no records
    torch.cuda.synchronize()
    again, _ = _skeleton_sheet(mr, img, pred, None)
    assert np.array_equal(again, good)
    mr.close()
