"""Renderer on the GPU (-m gpu) where tests/test_gpu_render.py never looks: meshes that leave the frame through every border and
corner, meshes at, across and behind the near plane and the guard band, faces far larger and far smaller than a tile, images
narrower than a tile or of a ragged tile count, an empty image between full ones, face lists at exact multiples of the raster
kernel's 256-face chunk, exact depth ties, non-finite vertices and zero-area faces.

Every scene is rendered by csrc/render.hip through tokenhmr_amd.render.Renderer and compared with the NumPy restatement
(tests/render_numpy.py) by test_gpu_render._compare: coverage and alpha exact, RGB within 1/255, another winner only at a depth tie.
Each scene first asserts, on the restatement alone, that it still takes the path it is here for (`_regime`): the counts are
equalities with what the restatement gave when the scene was chosen, the fractions a band of 0.01.

Sub-pixel faces at 4 samples (`far`, `speck`, `tiny`, `near_wide` with its 0.3 px faces, and the sweep cases `_subpixel` names): the shading point is the pixel centre,
which lies far outside a face smaller than a pixel (centre barycentrics up to +-26), so the kernel's fp32 shading and the
restatement's fp64 one are not bound to 1/255 by the contract; ids and alpha stay exact there and RGB must be finite and in [0, 1].
"""
import functools

import numpy as np
import pytest
import torch

from tests import render_numpy as RN
from tests.test_gpu_render import MEAN, STD, _cfg, _compare

pytestmark = pytest.mark.gpu

BASE, BG = (0.9, 0.6, 0.3), (0.2, 0.3, 0.4)
TILE, SMALL_TILES, CHUNK = 16, 4, 256          # render.hip: tile side, tiles a binned face may span, faces staged per pass


# ------------------------------------------------------------------------------------------------ scenes and their regimes
def _sphere():
    return RN.uv_sphere(40, 20, 1.0)


def _call_scene(W, H, f, znear=None):
    from tokenhmr_amd import render as R
    sc = R.build_scene("call", W, H, f, np.zeros(3), mesh_base_color=BASE, scene_bg_color=BG)
    if znear is not None:
        sc["znear"] = znear
    return sc


def _regime(sc, faces, verts, cam_t):
    """Per mesh, what the restatement's projection and setup make of it: the paths of render.hip the scene reaches."""
    W, H = sc["width"], sc["height"]
    P, fix, ok = RN.project(sc, verts, cam_t)
    tx, ty = -(-W // TILE), -(-H // TILE)
    out = []
    for m in range(len(verts)):
        acc, corners, _, lo, hi = RN.setup(fix[m], ok[m], P[m, :, 2], faces, W, H)
        raw_lo, raw_hi = corners.min(1) >> 8, corners.max(1) >> 8
        clamped = acc & ((raw_lo < 0).any(1) | (raw_hi[:, 0] >= W) | (raw_hi[:, 1] >= H))
        tl, th = lo // TILE, hi // TILE
        large = acc & ((th - tl + 1).prod(1) > SMALL_TILES)
        bins = np.zeros((ty, tx), int)
        for i in np.nonzero(acc & ~large)[0]:
            bins[tl[i, 1]:th[i, 1] + 1, tl[i, 0]:th[i, 0] + 1] += 1
        okf = ok[m][faces]
        with np.errstate(invalid="ignore"):
            guard = (P[m, :, 2] >= np.float32(sc["znear"])) & ~ok[m]
        out.append(dict(acc=int(acc.sum()), clamped=int(clamped.sum()), large=int(large.sum()), maxbin=int(bins.max()),
                        unusable=int((~ok[m]).sum()), guard=int(guard.sum()), mixed=int((okf.any(1) & ~okf.all(1)).sum()),
                        masks=dict(acc=acc, large=large, clamped=clamped, tl=tl, th=th, bins=bins)))
    return out


def _borders(ids):
    """Which borders of one image (H, W, S) the coverage touches, as a string out of "LRTB"."""
    cov = (ids >= 0).any(-1)
    return "".join(k for k, hit in zip("LRTB", (cov[:, 0].any(), cov[:, -1].any(), cov[0].any(), cov[-1].any())) if hit)


# name -> mesh ("sphere", "half": scaled x0.5, "inside": the finer sphere wound inwards), cam_t, (W, H), f, the sample counts,
# and the preconditions on the restatement: _regime counts (equalities), "borders", "cov" (fraction, +-0.01), "full" / "empty", "covered" (the number of covered samples per sample count: `speck` is missed by every pixel
# centre, and hit by exactly one of the 28,000 samples of the 4x pattern)
_B = dict(size=(100, 70), f=120.0, S=(1, 4), mesh="sphere")
SCENES = {
    "left": dict(_B, t=(-2.2, 0, 5), pre=dict(acc=236, clamped=49, borders="L")),
    "right": dict(_B, t=(2.2, 0.1, 5), pre=dict(acc=236, clamped=51, borders="R")),
    "top": dict(_B, t=(0, -1.5, 5), pre=dict(acc=269, clamped=55, borders="T")),
    "bottom": dict(_B, t=(0.3, 1.5, 5), pre=dict(acc=270, clamped=53, borders="B")),
    "corner": dict(_B, t=(2.0, 1.4, 5), pre=dict(acc=174, clamped=47, borders="RB")),
    "closeup": dict(_B, t=(0.1, -0.05, 1.3), pre=dict(acc=60, large=34, full=True)),
    "near": dict(_B, mesh="half", t=(0.8, 0.1, 0.3), f=30.0, pre=dict(unusable=241, mixed=80, acc=97, cov=0.20)),
    # the near plane inside the frame: faces with a corner at 0 < Z < znear project on screen and must leave a hole — at the default
    # znear = 0.05 under a very wide lens, and at a znear of 4.5 that cuts the front cap off a sphere 5 away
    "near_wide": dict(_B, mesh="half", t=(0.8, 0.1, 0.3), f=3.0, pre=dict(unusable=241, mixed=80, acc=142, cov=0.028), subpixel=True),
    "znear_cut": dict(_B, t=(0.1, -0.05, 5), znear=4.5, pre=dict(unusable=241, mixed=80, acc=160, cov=0.020)),
    "guard": dict(_B, t=(0, 0, 1.3), f=3.0e6, pre=dict(guard=320, unusable=320, mixed=192, acc=40, large=40, full=True)),
    "far": dict(_B, t=(0.3, 0.2, 40), pre=dict(acc=760, maxbin=756), subpixel=True),
    "speck": dict(_B, t=(0.3, 0.2, 400), pre=dict(acc=746, covered={1: 0, 4: 1}), subpixel=True),
    "behind": dict(_B, t=(0, 0, -5), pre=dict(unusable=762, acc=0, empty=True)),
    "tiny": dict(_B, t=(0, 0, 4), size=(7, 5), f=20.0, pre=dict(acc=280, full=True), subpixel=True),
    "tiny1x1": dict(_B, t=(0, 0, 4), size=(1, 1), f=20.0, pre=dict(acc=40, full=True), subpixel=True),
    "inside": dict(_B, mesh="inside", t=(0, 0, 0), size=(640, 480), f=400.0, S=(1,), pre=dict(acc=854, large=764, unusable=1025, full=True)),
}
TABLE = [(name, S) for name, sc in SCENES.items() for S in sc["S"]]


def _mesh(kind):
    if kind == "inside":
        v, f = RN.uv_sphere(64, 32, 1.0)
        return v, f[:, ::-1].copy()
    v, f = _sphere()
    return (v * 0.5 if kind == "half" else v), f


@functools.lru_cache(maxsize=None)
def _table_ref(name, S):
    """(scene, faces, verts (1, V, 3), cam_t (1, 3), restatement) of one table scene — computed once, shared, never modified."""
    d = SCENES[name]
    v, f = _mesh(d["mesh"])
    sc = _call_scene(*d["size"], d["f"], d.get("znear"))
    verts, cam_t = v[None].astype(np.float32), np.array([d["t"]], np.float64)
    return sc, f, verts, cam_t, RN.render(sc, f, verts, cam_t, samples=S)


def _check_preconditions(pre, regime, ids, S):
    for k, want in pre.items():
        if k == "borders":
            assert _borders(ids) == want, (k, _borders(ids))
        elif k == "cov":
            assert abs((ids >= 0).mean() - want) <= 0.01, (k, (ids >= 0).mean())
        elif k == "full":
            assert (ids >= 0).all()
        elif k == "empty":
            assert (ids < 0).all()
        elif k == "covered":
            assert (ids >= 0).sum() == want[S], (k, (ids >= 0).sum())
        else:
            assert regime[k] == want, (k, regime[k], want)


def _run(r, sc, verts, cam_t, per_image=True, **kw):
    from tokenhmr_amd import _cabi
    out, ids = r._run(sc, verts, cam_t, _cabi.RENDER_PER_IMAGE if per_image else _cabi.RENDER_ONE_IMAGE, 4, return_ids=True, **kw)
    return out.cpu().numpy(), ids.cpu().numpy()


def _exact_ids_and_alpha(out, ids, ref):
    np.testing.assert_array_equal(ids.astype(np.int64), ref["ids"])
    np.testing.assert_array_equal(out[..., 3], ref["out"][..., 3])


def _check(out, ids, ref, faces, S, subpixel=False, single_front=True):
    """The comparison of one render.  subpixel (4 samples only): ids and alpha exact, RGB finite and in [0, 1].  single_front: every
    sample is covered by at most one front face (a convex mesh from outside, a star-shaped one from inside), so depth decides
    nothing and no winner may differ."""
    assert np.isfinite(out).all()
    if subpixel and S == 4:
        _exact_ids_and_alpha(out, ids, ref)
        assert out.min() >= 0.0 and out.max() <= 1.0
        return
    n = _compare(out, ids, ref, faces, S)
    if single_front:
        assert n == 0, n


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("name,S", TABLE, ids=[f"{n}-S{s}" for n, s in TABLE])
def test_table_scene_matches_the_restatement(built_lib, cuda_dev, name, S):
    from tokenhmr_amd import render as R
    sc, faces, verts, cam_t, ref = _table_ref(name, S)
    pre = SCENES[name]["pre"]
    _check_preconditions(pre, _regime(sc, faces, verts, cam_t)[0], ref["ids"][0], S)
    r = R.Renderer(_cfg(focal=SCENES[name]["f"]), faces, device=cuda_dev, samples=S)
    out, ids = _run(r, sc, verts, cam_t)
    r.close()
    _check(out, ids, ref, faces, S, subpixel=SCENES[name].get("subpixel", False))
    if pre.get("empty") or "covered" in pre:                   # the background exactly, wherever no sample is covered
        untouched = (ref["ids"] < 0).all(-1)
        assert untouched.sum() >= untouched.size - 1
        np.testing.assert_array_equal(out[untouched], np.broadcast_to(np.append(RN.to8(np.array(BG)), np.float32(0)), out[untouched].shape))


# ------------------------------------------------------------------------------------------------ chunk boundaries of the two lists
KS = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1]


def _first_k(name, which, k):
    """The scene `name` with its face array cut down to the first k faces the restatement puts into the fullest bin ("bin") or into
    the large-face list ("large")."""
    sc, faces, verts, cam_t, _ = _table_ref(name, SCENES[name]["S"][0])
    m = _regime(sc, faces, verts, cam_t)[0]["masks"]
    if which == "large":
        member = m["large"]
    else:
        ty, tx = np.unravel_index(m["bins"].argmax(), m["bins"].shape)
        member = m["acc"] & ~m["large"] & (m["tl"][:, 0] <= tx) & (tx <= m["th"][:, 0]) & (m["tl"][:, 1] <= ty) & (ty <= m["th"][:, 1])
    keep = np.nonzero(member)[0][:k]
    assert len(keep) == k
    return sc, np.ascontiguousarray(faces[keep]), verts, cam_t


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,which,S", [("far", "bin", 1), ("far", "bin", 4), ("inside", "large", 1)])
def test_lists_of_exactly_k_faces_around_the_chunk_size(built_lib, cuda_dev, name, which, S, k):
    from tokenhmr_amd import render as R
    sc, faces, verts, cam_t = _first_k(name, which, k)
    reg = _regime(sc, faces, verts, cam_t)[0]
    assert reg["acc"] == k and (reg["maxbin"] == k and reg["large"] == 0 if which == "bin" else reg["large"] == k)
    ref = RN.render(sc, faces, verts, cam_t, samples=S)
    assert (ref["ids"] >= 0).any()
    r = R.Renderer(_cfg(focal=sc["fx"]), faces, device=cuda_dev, samples=S)
    out, ids = _run(r, sc, verts, cam_t)
    r.close()
    _exact_ids_and_alpha(out, ids, ref)
    assert np.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ one batch, every regime
BATCH = ["closeup", "behind", "left", "far", "behind", "corner"]


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("composite", [True, False])
def test_batch_mixing_regimes_equals_single_renders_and_the_restatement(built_lib, cuda_dev, composite, S):
    from tokenhmr_amd import render as R
    v, faces = _sphere()
    W, H = 100, 70
    verts = np.stack([v] * len(BATCH)).astype(np.float32)
    cam_t = np.array([SCENES[n]["t"] for n in BATCH], np.float32)
    imgs = torch.randn(len(BATCH), 3, H, W, generator=torch.Generator().manual_seed(3))
    kw = dict(mesh_base_color=BASE, scene_bg_color=BG, return_ids=True)
    if not composite:
        kw.update(return_rgba=True, width=W, height=H)
    r = R.Renderer(_cfg(focal=120.0), faces, device=cuda_dev, samples=S)

    def render(sel):
        out, ids = r.render_batch(torch.as_tensor(verts[sel]), torch.as_tensor(cam_t[sel]), imgs[sel] if composite else None, **kw)
        return out.cpu().numpy(), ids.cpu().numpy()

    every = np.arange(len(BATCH))
    out, ids = render(every)
    assert out.shape == (len(BATCH), H, W, 3 if composite else 4) and np.isfinite(out).all()
    sc = _call_scene(W, H, 120.0)
    ref = RN.render(sc, faces, verts, cam_t, samples=S, images=imgs.numpy() if composite else None, mean=MEAN, std=STD)
    shown = imgs.numpy().transpose(0, 2, 3, 1) * np.asarray(STD, np.float32) + np.asarray(MEAN, np.float32)
    for n, name in enumerate(BATCH):
        one = dict(ref, ids=ref["ids"][n:n + 1], depth=ref["depth"][n:n + 1], out=ref["out"][n:n + 1],
                   images=ref["images"][n:n + 1] if composite else None)      # mesh n of the batch: its ids stay n * F + face
        if name == "far" and S == 4:                           # sub-pixel faces: ids exact (alpha is their count), RGB finite
            np.testing.assert_array_equal(ids[n], ref["ids"][n])
        else:
            assert _compare(out[n:n + 1], ids[n:n + 1], one, faces, S) == 0, name
        if name == "behind":
            assert (ids[n] < 0).all()
            if composite:
                np.testing.assert_array_equal(out[n], shown[n])
            else:
                np.testing.assert_array_equal(out[n], np.broadcast_to(np.append(RN.to8(np.array(BG)), np.float32(0)), out[n].shape))
    for n in every:                                            # image for image what the mesh gives alone
        alone, alone_ids = render(np.array([n]))
        in_batch = np.where(ids[n] >= 0, ids[n] - n * len(faces), -1)      # alone, the mesh is mesh 0
        assert np.array_equal(alone[0], out[n]) and np.array_equal(alone_ids[0], in_batch), BATCH[n]
    back, back_ids = render(every[::-1].copy())                # and in the reverse order, on the same handle
    face = lambda i: np.where(i >= 0, i % len(faces), -1)      # the mesh index in an id is the mesh's place in the batch
    assert np.array_equal(back[::-1], out) and np.array_equal(face(back_ids[::-1]), face(ids))
    r.close()


# ------------------------------------------------------------------------------------------------ several meshes in one image
def _scene_render(cuda_dev, faces, verts, cam_t, S, colors, W=100, H=70, f=120.0):
    """render_scene and its restatement: (out (1, H, W, 4), ids (1, H, W, S), scene, ref)."""
    from tokenhmr_amd import render as R
    r = R.Renderer(_cfg(focal=f), faces, device=cuda_dev, samples=S)
    out, ids = r.render_scene(verts, cam_t, W, H, f, mesh_base_color=BASE, scene_bg_color=BG, mesh_colors=colors, return_ids=True)
    r.close()
    sc = R.build_scene("rgba", W, H, f, mesh_base_color=BASE, scene_bg_color=BG)
    ref = RN.render(sc, faces, verts, cam_t, samples=S, one_image=True, mesh_colors=colors)
    return out.cpu().numpy()[None], ids.cpu().numpy()[None], sc, ref


COLORS = np.array([(0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9), (0.9, 0.9, 0.1), (0.1, 0.9, 0.9)], np.float32)


@pytest.mark.parametrize("S", [1, 4])
def test_five_border_spheres_in_one_image(built_lib, cuda_dev, S):
    v, faces = _sphere()
    names = ["left", "right", "top", "bottom", "corner"]
    verts = np.stack([v] * 5).astype(np.float32)
    cam_t = np.array([SCENES[n]["t"] for n in names], np.float64)
    out, ids, sc, ref = _scene_render(cuda_dev, faces, verts, cam_t, S, COLORS)
    assert abs((ref["ids"] >= 0).mean() - 0.51) <= 0.01 and _borders(ref["ids"][0]) == "LRTB"
    assert len(np.unique(ref["ids"][ref["ids"] >= 0] // len(faces))) == 5
    _check(out, ids, ref, faces, S, single_front=False)


@pytest.mark.parametrize("S", [1, 4])
def test_near_mesh_in_front_of_a_far_mesh(built_lib, cuda_dev, S):
    v, faces = _sphere()
    verts = np.stack([v, v * 3]).astype(np.float32)
    cam_t = np.array([(0.9, 0.0, 1.5), (0.0, 0.0, 8.0)])
    out, ids, sc, ref = _scene_render(cuda_dev, faces, verts, cam_t, S, COLORS[:2])
    reg = _regime(sc, faces, verts, cam_t)
    assert abs((ref["ids"] >= 0).mean() - 0.94) <= 0.01
    assert reg[0]["large"] + reg[1]["large"] == 9 and reg[0]["clamped"] > 0 and reg[1]["clamped"] > 0
    _check(out, ids, ref, faces, S, single_front=False)
    # where both meshes cover a sample, the near one wins
    W, H = sc["width"], sc["height"]
    ok = RN.project(sc, verts, cam_t)[2]
    cover = [RN.rasterize(ref["fix"], ok, ref["Z"], faces, W, H, S, [m])[0] >= 0 for m in range(2)]
    both = cover[0] & cover[1]
    assert both.sum() > 100 and (ids[0][both] >= 0).all() and (ids[0][both] < len(faces)).all()


@pytest.mark.parametrize("S", [1, 4])
def test_coincident_meshes_tie_to_the_lower_id(built_lib, cuda_dev, S):
    v, faces = _sphere()
    verts = np.stack([v, v]).astype(np.float32)
    cam_t = np.array([(0.1, 0.0, 5.0), (0.1, 0.0, 5.0)])
    out, ids, sc, ref = _scene_render(cuda_dev, faces, verts, cam_t, S, COLORS[:2])
    assert (ref["ids"] >= 0).sum() > 500 and (ref["ids"] < len(faces)).all()
    np.testing.assert_array_equal(ids.astype(np.int64), ref["ids"])                 # every tie goes to mesh 0, as the total order says
    _check(out, ids, ref, faces, S)
    swapped, ids2, _, ref2 = _scene_render(cuda_dev, faces, verts, cam_t, S, COLORS[1::-1].copy())
    np.testing.assert_array_equal(ids2, ids)
    _check(swapped, ids2, ref2, faces, S)
    covered = (ids[0] >= 0).all(-1)
    assert covered.sum() > 100 and (np.abs(swapped[0] - out[0])[covered][:, :3].max(-1) > 0.1).all()   # the colour is mesh 0's


# ------------------------------------------------------------------------------------------------ non-finite and degenerate input
@pytest.mark.parametrize("S", [1, 4])
def test_non_finite_vertices_and_zero_area_faces(built_lib, cuda_dev, S):
    """No address in render.hip is formed from a coordinate (every index is a face's vertex index, checked at create, or a thread
    id), a non-finite vertex fails `Z >= znear && |u|, |v| <= guard` and is marked unusable, a face with a non-finite or zero normal
    length adds nothing to its corners' normals, and a face of zero doubled area is not a front face."""
    from tokenhmr_amd import render as R
    v, f = _sphere()
    v = v.copy()
    v[[5, 100, 333]] = [[np.nan, 0, 0], [np.inf, 1, 1], [0, 0, -np.inf]]
    v[401] = v[400]                                                        # a collapsed edge: zero-area faces on both sides of it
    faces = np.concatenate([f, [[7, 7, 9], [10, 11, 10], [20, 20, 20]]])
    R.check_faces(faces)
    sc = _call_scene(100, 70, 120.0)
    verts, cam_t = v[None].astype(np.float32), np.array([(0.1, 0.0, 3.0)])
    reg = _regime(sc, faces, verts, cam_t)[0]
    ref = RN.render(sc, faces, verts, cam_t, samples=S)
    assert reg["unusable"] == 3 and reg["mixed"] == 17 and abs((ref["ids"] >= 0).mean() - 0.74) <= 0.01
    assert np.isfinite(ref["out"]).all() and np.isfinite(ref["N"]).all()
    r = R.Renderer(_cfg(focal=120.0), faces, device=cuda_dev, samples=S)
    out, ids = _run(r, sc, verts, cam_t)
    r.close()
    assert np.isfinite(out).all()
    np.testing.assert_array_equal(ids.astype(np.int64), ref["ids"])
    _check(out, ids, ref, faces, S)


# ------------------------------------------------------------------------------------------------ seeded sweep on one handle
SWEEP_SEED, SWEEP_CASES = 0, 24


def _sweep():
    rng = np.random.default_rng(SWEEP_SEED)
    cases = []
    for _ in range(SWEEP_CASES):
        W, H = (int(x) for x in rng.integers(1, 131, 2))
        f = float(rng.uniform(20, 400))
        x, y = rng.uniform(-3, 3, 2)
        z = rng.uniform(-1, 12)
        S = (1, 4)[int(rng.integers(2))]
        cases.append((W, H, f, np.array([(x, y, z)]), S))
    return cases


def _subpixel(f, z):
    """The sphere's faces are 2 pi / 40 wide at the equator: below one pixel once f 2 pi / 40 < z — the regime of `far` (0.47 px) and
    `tiny` (0.79 px), where RGB at 4 samples is not bound to 1/255; `left` ... `corner` (3.8 px) are held to it."""
    return z > 0 and f * 2 * np.pi / 40 < z


def test_seeded_sweep_on_one_handle(built_lib, cuda_dev):
    """Random image sizes (1 ... 130: below a tile, ragged in both directions), focal lengths and placements, in front of, across and
    behind the camera, on ONE renderer: its grow-only scratch is reused across shrinking and growing sizes."""
    from tokenhmr_amd import render as R
    v, faces = _sphere()
    verts = v[None].astype(np.float32)
    r = R.Renderer(_cfg(focal=120.0), faces, device=cuda_dev)
    with_cov = without = unusable = 0
    for W, H, f, cam_t, S in _sweep():
        sc = _call_scene(W, H, f)
        ref = RN.render(sc, faces, verts, cam_t, samples=S)
        reg = _regime(sc, faces, verts, cam_t)[0]
        with_cov += bool((ref["ids"] >= 0).any())
        without += not (ref["ids"] >= 0).any()
        unusable += reg["unusable"] > 0
        r.samples = S
        out, ids = _run(r, sc, verts, cam_t)
        _check(out, ids, ref, faces, S, subpixel=_subpixel(f, cam_t[0, 2]))
    r.close()
    assert with_cov >= 8 and without >= 3 and unusable >= 3, (with_cov, without, unusable)
