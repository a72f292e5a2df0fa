"""Renderer contract on the CPU (not-gpu): the host scene builder of tokenhmr_amd.render pinned against the reference's
lib/utils/renderer.py executed in place with recording stand-ins for pyrender / trimesh / cv2 / yacs; cam_crop_to_full against
the reference function; the NumPy restatement's own coverage properties; argument checks that need no device."""
import ast
import contextlib
import ctypes as C
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import render_numpy as RN

REF = "/root/reference/tokenhmr"
RENDERER = os.path.join(REF, "lib", "utils", "renderer.py")
needs_ref = pytest.mark.skipif(not os.path.exists(RENDERER), reason="reference tree not present (GPU box)")


# ------------------------------------------------------------------------------------------------ recording stand-ins
def _rotation_matrix(angle, direction, point=None):
    """trimesh.transformations.rotation_matrix (4x4, about the origin) — Rodrigues in float64."""
    s, c = np.sin(angle), np.cos(angle)
    d = np.asarray(direction[:3], dtype=np.float64)
    d = d / np.linalg.norm(d)
    K = np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]])
    M = np.eye(4)
    M[:3, :3] = c * np.eye(3) + (1 - c) * np.outer(d, d) + s * K
    return M


class _Rec:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _stubs(log):
    class Trimesh:
        def __init__(self, vertices, faces, vertex_colors=None, **kw):
            self.vertices = np.asarray(vertices, dtype=np.float64).copy()
            self.faces, self.vertex_colors = faces, vertex_colors

        def apply_transform(self, M):
            self.vertices = self.vertices @ M[:3, :3].T + M[:3, 3]

    class Scene:
        def __init__(self, bg_color=None, ambient_light=None):
            self.bg_color, self.ambient_light, self.nodes, self.meshes, self.camera = bg_color, ambient_light, [], [], None
            log["scenes"].append(self)

        def add(self, obj, name=None, pose=None):
            if isinstance(obj, _Rec) and getattr(obj, "kind", "") == "camera":
                self.camera = (obj, np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64))
            else:
                self.meshes.append(obj)

        def add_node(self, node):
            if node.camera is not None:
                self.camera = (node.camera, np.asarray(node.matrix, dtype=np.float64))
            self.nodes.append(node)

        def get_pose(self, node):
            return np.asarray(node.matrix, dtype=np.float64)

        def has_node(self, node):
            return any(n is node for n in self.nodes)

    class OffscreenRenderer:
        def __init__(self, viewport_width, viewport_height, point_size=1.0):
            self.w, self.h = viewport_width, viewport_height
            log["viewports"].append((viewport_width, viewport_height))

        def render(self, scene, flags=None):
            return np.zeros((self.h, self.w, 4), np.uint8), np.zeros((self.h, self.w), np.float32)

        def delete(self):
            pass

    def Node(name=None, light=None, camera=None, matrix=None, **kw):
        return _Rec(name=name, light=light, camera=camera, matrix=np.eye(4) if matrix is None else np.asarray(matrix, dtype=np.float64))

    pyrender = types.ModuleType("pyrender")
    pyrender.OffscreenRenderer, pyrender.Scene, pyrender.Node = OffscreenRenderer, Scene, Node
    pyrender.MetallicRoughnessMaterial = lambda **kw: _Rec(kind="material", **kw)
    pyrender.Mesh = types.SimpleNamespace(from_trimesh=lambda mesh, material=None: _Rec(kind="mesh", vertices=mesh.vertices.copy(),
                                                                                         material=material, vertex_colors=mesh.vertex_colors))
    pyrender.IntrinsicsCamera = lambda fx, fy, cx, cy, zfar=None, znear=0.05: _Rec(kind="camera", fx=fx, fy=fy, cx=cx, cy=cy, znear=znear)
    pyrender.DirectionalLight = lambda color=None, intensity=1.0: _Rec(kind="directional", color=np.asarray(color), intensity=intensity)
    pyrender.PointLight = lambda color=None, intensity=1.0: _Rec(kind="point", color=np.asarray(color), intensity=intensity)
    pyrender.RenderFlags = types.SimpleNamespace(RGBA=1)
    trimesh = types.ModuleType("trimesh")
    trimesh.Trimesh = Trimesh
    trimesh.transformations = types.SimpleNamespace(rotation_matrix=_rotation_matrix)
    yacs, yacs_config = types.ModuleType("yacs"), types.ModuleType("yacs.config")
    yacs_config.CfgNode = dict
    yacs.config = yacs_config
    return {"pyrender": pyrender, "trimesh": trimesh, "cv2": types.ModuleType("cv2"), "yacs": yacs, "yacs.config": yacs_config}


@contextlib.contextmanager
def _reference_renderer():
    log = {"scenes": [], "viewports": []}
    stubs = _stubs(log)
    saved = {k: sys.modules.get(k) for k in stubs}
    saved_env = os.environ.get("PYOPENGL_PLATFORM")
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("_ref_renderer", RENDERER)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        yield mod, log
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        if saved_env is None:
            os.environ.pop("PYOPENGL_PLATFORM", None)      # the module sets it at import
        else:
            os.environ["PYOPENGL_PLATFORM"] = saved_env


class _Ns(dict):
    __getattr__ = dict.__getitem__


CFG = _Ns(EXTRA=_Ns(FOCAL_LENGTH=5000), MODEL=_Ns(IMAGE_SIZE=256, IMAGE_MEAN=[0.485, 0.456, 0.406], IMAGE_STD=[0.229, 0.224, 0.225]))
_FL = np.diag([1.0, -1.0, -1.0])


def _captured(scene):
    """A recorded pyrender scene in the camera frame (x right, y down, z forward)."""
    cam, pose = scene.camera
    Rc, pc = pose[:3, :3], pose[:3, 3]
    to_cam = lambda p: _FL @ (Rc.T @ (p - pc))
    verts = [(m.vertices - pc) @ Rc @ _FL for m in scene.meshes]
    lights = []
    for n in scene.nodes:
        if n.light is None:
            continue
        if n.light.kind == "directional":
            lights.append((0, _FL @ (Rc.T @ (-n.matrix[:3, 2])), n.light.color, n.light.intensity))
        else:
            lights.append((1, to_cam(n.matrix[:3, 3]), n.light.color, n.light.intensity))
    return cam, verts, lights


def _assert_scene_matches(ours, cam, verts_ref, lights_ref, ours_verts, viewport):
    assert (ours["width"], ours["height"]) == viewport
    assert (ours["fx"], ours["fy"], ours["cx"], ours["cy"]) == (cam.fx, cam.fy, cam.cx, cam.cy)
    for a, b in zip(ours_verts, verts_ref):
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6 * np.abs(b).max())
    assert len(ours["lights"]) == len(lights_ref)
    for (k1, v1, c1, i1), (k2, v2, c2, i2) in zip(ours["lights"], lights_ref):
        assert k1 == k2
        np.testing.assert_allclose(v1, v2, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(c1, c2)
        assert i1 == i2


@needs_ref
@pytest.mark.parametrize("side_view", [False, True])
def test_scene_of_call_matches_the_reference(side_view):
    from tokenhmr_amd import render as R
    rng = np.random.default_rng(3)
    verts = rng.normal(0, 0.4, (50, 3)).astype(np.float32)
    faces = rng.integers(0, 50, (30, 3))
    cam_t = np.array([0.12, -0.3, 41.0])
    img = torch.zeros(3, 200, 240)
    with _reference_renderer() as (mod, log):
        ref_t = cam_t.copy()
        mod.Renderer(CFG, faces)(verts, ref_t, img, side_view=side_view, rot_angle=90, mesh_base_color=(0.2, 0.5, 0.9), scene_bg_color=(1, 1, 1))
        scene = log["scenes"][-1]
        cam, vref, lref = _captured(scene)
        material = scene.meshes[0].material
        viewport = log["viewports"][-1]
    assert ref_t[0] == -cam_t[0] and ref_t[1] == cam_t[1]                 # the side effect a drop-in keeps
    ours = R.build_scene("call", 240, 200, 5000, cam_t, side_view, 90, mesh_base_color=(0.2, 0.5, 0.9), scene_bg_color=(1, 1, 1))
    _assert_scene_matches(ours, cam, vref, lref, [R.camera_frame_vertices(ours, verts, cam_t)], viewport)
    assert material.metallicFactor == ours["metallic"] == 0.0 and not hasattr(material, "roughnessFactor")   # pyrender default 1.0
    assert ours["roughness"] == 1.0 and material.alphaMode == "OPAQUE"
    assert tuple(material.baseColorFactor) == (*ours["base_color"], 1.0)
    assert tuple(scene.bg_color) == (*ours["bg"], 0.0) and tuple(scene.ambient_light) == ours["ambient"]


@needs_ref
def test_scene_of_render_rgba_matches_the_reference():
    from tokenhmr_amd import render as R
    rng = np.random.default_rng(4)
    verts = rng.normal(0, 0.4, (40, 3)).astype(np.float32)
    faces = rng.integers(0, 40, (20, 3))
    cam_t = np.array([0.3, 0.1, 30.0])
    with _reference_renderer() as (mod, log):
        mod.Renderer(CFG, faces).render_rgba(verts, cam_t=cam_t, rot_axis=[0, 1, 0], rot_angle=30, mesh_base_color=(0.9, 0.4, 0.1),
                                            scene_bg_color=(0.1, 0.2, 0.3), render_res=[320, 240])
        scene = log["scenes"][-1]
        cam, vref, lref = _captured(scene)
        viewport = log["viewports"][-1]
    ours = R.build_scene("rgba", 320, 240, 5000, rot_angle=30, rot_axis=[0, 1, 0], mesh_base_color=(0.9, 0.4, 0.1), scene_bg_color=(0.1, 0.2, 0.3))
    _assert_scene_matches(ours, cam, vref, lref, [R.camera_frame_vertices(ours, verts, cam_t)], viewport)
    assert scene.meshes[0].material is None                          # pyrender's default vertex-colour material
    np.testing.assert_allclose(scene.meshes[0].vertex_colors, np.tile([0.9, 0.4, 0.1, 1.0], (40, 1)))
    assert tuple(scene.bg_color) == (*ours["bg"], 0.0) and tuple(scene.ambient_light) == ours["ambient"]
    assert [k for k, *_ in lref] == [1] * 6 + [0] * 9                # 6 point lights, 6 + 3 directional


@needs_ref
def test_scene_of_render_rgba_multiple_matches_the_reference():
    from tokenhmr_amd import render as R
    rng = np.random.default_rng(5)
    verts = [rng.normal(0, 0.4, (30, 3)).astype(np.float32) for _ in range(3)]
    cam_t = [np.array([0.5 * i - 0.5, 0.2, 25.0 + i]) for i in range(3)]
    faces = rng.integers(0, 30, (10, 3))
    with _reference_renderer() as (mod, log):
        mod.Renderer(CFG, faces).render_rgba_multiple(verts, cam_t, render_res=[640, 480], focal_length=1200.0)
        scene = log["scenes"][-1]
        cam, vref, lref = _captured(scene)
        viewport = log["viewports"][-1]
    ours = R.build_scene("rgba", 640, 480, 1200.0)
    _assert_scene_matches(ours, cam, vref, lref, [R.camera_frame_vertices(ours, v, t) for v, t in zip(verts, cam_t)], viewport)
    # the .obj path: vertices_to_trimesh is (v + t), rotated, then flipped — the GL world the scene holds
    with _reference_renderer() as (mod, log):
        ref_mesh = mod.Renderer(CFG, faces).vertices_to_trimesh(verts[1], cam_t[1], (0.3, 0.6, 0.9), [0, 0, 1], 20)
    ours_mesh = R.Renderer.vertices_to_trimesh(types.SimpleNamespace(faces=faces), verts[1], cam_t[1], (0.3, 0.6, 0.9), [0, 0, 1], 20)
    np.testing.assert_allclose(ours_mesh.vertices, ref_mesh.vertices, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(ours_mesh.faces, faces)


def _reference_function(rel, fname, glb):
    with open(os.path.join(REF, rel)) as f:
        tree = ast.parse(f.read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == fname)
    ns = dict(glb)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), os.path.join(REF, rel), "exec"), ns)
    return ns[fname]


@needs_ref
@pytest.mark.parametrize("focal", [5000.0, 1234.5])
def test_cam_crop_to_full_is_the_reference_bit_for_bit(focal):
    from tokenhmr_amd.render import cam_crop_to_full
    ref = _reference_function("lib/utils/renderer.py", "cam_crop_to_full", {"torch": torch})
    g = torch.Generator().manual_seed(7)
    cam = torch.randn(16, 3, generator=g) * torch.tensor([0.3, 0.2, 0.2]) + torch.tensor([0.9, 0.0, 0.0])
    center = torch.rand(16, 2, generator=g) * 1000
    size = torch.rand(16, generator=g) * 500 + 20
    img = torch.tensor([[1920.0, 1080.0]]).repeat(16, 1)
    assert torch.equal(cam_crop_to_full(cam, center, size, img, focal), ref(cam, center, size, img, focal))
    assert torch.equal(cam_crop_to_full(cam, center, size, img), ref(cam, center, size, img))


# ------------------------------------------------------------------------------------------------ the restatement's own checks
def _flat_scene(W, H):
    return {"width": W, "height": H, "fx": 100.0, "fy": 100.0, "cx": W / 2, "cy": H / 2, "znear": 0.05, "R": np.eye(3),
            "translate_first": False, "metallic": 0.0, "roughness": 1.0, "ambient": (0.3, 0.3, 0.3), "bg": (0, 0, 0),
            "base_color": (1, 1, 1), "lights": []}


def _screen_quad(x0, y0, x1, y1, W, H, diag_flip=False):
    """A quad at Z = 1 whose corners project to exactly (x0, y0) ... (x1, y1) px (fx = 100), front-facing."""
    sc = _flat_scene(W, H)
    to3 = lambda u, v: ((u - W / 2) / 100.0, (v - H / 2) / 100.0, 1.0)
    verts = np.array([to3(x0, y0), to3(x1, y0), to3(x1, y1), to3(x0, y1)])
    # front = negative doubled area in the image frame: (0, 3, 2) and (0, 2, 1) wind that way
    faces = np.array([[0, 3, 1], [1, 3, 2]]) if diag_flip else np.array([[0, 3, 2], [0, 2, 1]])
    return sc, verts[None], faces


@pytest.mark.parametrize("S", [1, 4])
def test_axis_aligned_quad_covers_the_analytic_sample_count(S):
    W, H = 32, 24
    x0, y0, x1, y1 = 3.25, 2.5, 20.75, 17.0
    sc, verts, faces = _screen_quad(x0, y0, x1, y1, W, H)
    r = RN.render(sc, faces, verts, np.zeros((1, 3)), samples=S)
    P, fix, ok = RN.project(sc, verts, np.zeros((1, 3)))
    assert ok.all() and set(np.unique(fix[0, :, 0] % 64)) <= {0}            # corners land on the grid exactly
    ox = np.array([128]) if S == 1 else RN.OX
    oy = np.array([128]) if S == 1 else RN.OY
    expect = 0
    for s in range(S):
        xs = np.arange(W) * 256 + ox[s]
        ys = np.arange(H) * 256 + oy[s]
        # top-left: the left and top edges own their samples, the right and bottom ones do not
        expect += ((xs >= x0 * 256) & (xs < x1 * 256)).sum() * ((ys >= y0 * 256) & (ys < y1 * 256)).sum()
    assert (r["ids"] >= 0).sum() == expect


@pytest.mark.parametrize("flip", [False, True])
def test_shared_diagonal_covers_each_sample_exactly_once(flip):
    W, H = 16, 16
    sc, verts, faces = _screen_quad(2.0, 2.0, 14.0, 14.0, W, H, diag_flip=flip)    # the diagonal passes through sample points
    P, fix, ok = RN.project(sc, verts, np.zeros((1, 3)))
    hits = np.zeros((H, W, 4), int)
    for f in range(2):
        win, _ = RN.rasterize(fix, ok, P[..., 2], faces[f:f + 1], W, H, 4, [0])
        hits += win >= 0
    assert hits.max() == 1
    full, _ = RN.rasterize(fix, ok, P[..., 2], faces, W, H, 4, [0])
    assert ((full >= 0) == (hits == 1)).all() and (hits == 1).sum() == 12 * 12 * 4


def test_inside_out_sphere_renders_empty():
    """Seen from its centre, a sphere with outward normals shows only back faces: nothing.  Its inside-out twin (the windings
    reversed) covers the whole view; the same sphere seen from outside shows its near half."""
    v, f = RN.uv_sphere(48, 24, 10.0)
    sc = _flat_scene(64, 64)
    inside, outside = np.zeros((1, 3)), np.array([[0.0, 0.0, 50.0]])
    assert (RN.render(sc, f, v[None], inside)["ids"] >= 0).sum() == 0
    assert (RN.render(sc, f[:, ::-1], v[None], inside)["ids"] >= 0).all()
    r = RN.render(sc, f, v[None], outside)
    hit = r["ids"][r["ids"] >= 0]
    assert hit.size > 1000 and (r["P"][0, f[hit], 2].mean(1) < 50.0).all()         # every visible face is on the near half


def test_triangle_behind_znear_is_rejected():
    sc = _flat_scene(32, 32)
    verts = np.array([[[-0.5, -0.5, 1.0], [-0.5, 0.5, 1.0], [0.5, 0.0, 1.0]]])
    faces = np.array([[0, 1, 2]])
    assert (RN.render(sc, faces, verts, np.zeros((1, 3)))["ids"] >= 0).sum() > 0
    verts2 = verts.copy()
    verts2[0, 2, 2] = 0.04                                   # one corner in front of znear
    assert (RN.render(sc, faces, verts2, np.zeros((1, 3)))["ids"] >= 0).sum() == 0
    verts2[0, 2, 2] = -1.0                                   # one corner behind the camera: its projection flips, the face still goes
    assert (RN.render(sc, faces, verts2, np.zeros((1, 3)))["ids"] >= 0).sum() == 0


def test_triangle_with_a_corner_beyond_the_guard_band_is_rejected():
    sc = _flat_scene(32, 32)
    faces = np.array([[0, 1, 2]])
    verts = np.array([[[-0.5, -0.5, 1.0], [-0.5, 0.5, 1.0], [2.0e4, 0.0, 1.0]]])       # u = 2,000,016 px: inside 2^21 = 2,097,152
    P, fix, ok = RN.project(sc, verts, np.zeros((1, 3)))
    assert ok.all() and fix[0, 2, 0] == 2000016 * 256
    assert (RN.render(sc, faces, verts, np.zeros((1, 3)))["ids"] >= 0).sum() > 0
    verts[0, 2, 0] = 2.1e4                                   # u = 2,100,016 px: beyond it
    assert list(RN.project(sc, verts, np.zeros((1, 3)))[2][0]) == [True, True, False]
    assert (RN.render(sc, faces, verts, np.zeros((1, 3)))["ids"] >= 0).sum() == 0
    verts[0, 2] = [0.0, -2.1e4, 1.0]                         # the same in v
    for winding in (faces, faces[:, ::-1]):
        assert (RN.render(sc, winding, verts, np.zeros((1, 3)))["ids"] >= 0).sum() == 0


def _analytic_quad_count(x0, y0, x1, y1, W, H, S):
    """Samples of a W x H image inside [x0, x1) x [y0, y1) px — top-left rule: the left and top edges own their samples."""
    ox = np.array([128]) if S == 1 else RN.OX
    oy = np.array([128]) if S == 1 else RN.OY
    n = 0
    for s in range(S):
        xs, ys = np.arange(W) * 256 + ox[s], np.arange(H) * 256 + oy[s]
        n += int(((xs >= x0 * 256) & (xs < x1 * 256)).sum() * ((ys >= y0 * 256) & (ys < y1 * 256)).sum())
    return n


# a quad over each border and each corner of a 37 x 23 image (neither a multiple of the 16-pixel tile), corners on the 1/4 px grid
_OVERHANG = {"left": (-6.25, 4.5, 9.75, 15.25), "right": (30.5, 3.25, 44.0, 19.75), "top": (5.25, -7.5, 28.75, 6.25),
             "bottom": (8.5, 17.25, 21.25, 31.0), "top_left": (-3.75, -9.25, 11.5, 8.75), "top_right": (25.25, -2.5, 51.0, 10.25),
             "bottom_left": (-12.0, 14.75, 7.25, 40.5), "bottom_right": (29.75, 12.5, 37.25, 23.5),
             "all_round": (-5.0, -4.0, 41.0, 30.0), "last_column_only": (36.75, 2.0, 50.0, 20.0)}


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("where", sorted(_OVERHANG))
def test_overhanging_quad_covers_the_analytic_count_of_its_visible_part(where, S):
    W, H = 37, 23
    x0, y0, x1, y1 = _OVERHANG[where]
    sc, verts, faces = _screen_quad(x0, y0, x1, y1, W, H)
    _, fix, ok = RN.project(sc, verts, np.zeros((1, 3)))
    assert ok.all() and sorted(map(tuple, fix[0])) == sorted((int(x * 256), int(y * 256)) for x in (x0, x1) for y in (y0, y1))
    ids = RN.render(sc, faces, verts, np.zeros((1, 3)), samples=S)["ids"][0]
    expect = _analytic_quad_count(x0, y0, x1, y1, W, H, S)
    assert expect > 0 or where == "last_column_only"
    assert (ids >= 0).sum() == expect
    # and it is the right samples: every covered pixel lies inside the quad's pixel box, clipped to the image
    py, px = np.nonzero((ids >= 0).any(-1))
    if len(px):
        assert px.min() >= max(int(np.floor(x0)), 0) and px.max() <= min(int(np.ceil(x1)) - 1, W - 1)
        assert py.min() >= max(int(np.floor(y0)), 0) and py.max() <= min(int(np.ceil(y1)) - 1, H - 1)


@pytest.mark.parametrize("size", [(37, 23), (1, 1)])
@pytest.mark.parametrize("S", [1, 4])
def test_one_huge_triangle_covers_every_sample(S, size):
    W, H = size
    sc = _flat_scene(W, H)
    to3 = lambda u, v: ((u - W / 2) / 100.0, (v - H / 2) / 100.0, 1.0)
    verts = np.array([[to3(-300, -200), to3(-300, 900), to3(1200, -200)]])      # the image is deep inside: 337/1500 + 223/1100 < 1
    faces = np.array([[0, 1, 2]])                                                # negative doubled area in the image frame: front
    ids = RN.render(sc, faces, verts, np.zeros((1, 3)), samples=S)["ids"]
    assert ids.shape == (1, H, W, S) and (ids == 0).all()
    assert (RN.render(sc, faces[:, ::-1], verts, np.zeros((1, 3)), samples=S)["ids"] == -1).all()     # its back covers nothing


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("box", [(-20.0, 3.0, -2.25, 18.0), (4.0, -30.5, 30.0, -1.0), (37.0, 2.0, 60.0, 20.0), (3.0, 23.0, 30.0, 45.5),
                                 (-9.0, -9.0, 0.0, 0.0), (37.25, 23.5, 50.0, 40.0)])
def test_quad_outside_the_image_covers_nothing(box, S):
    """Left of, above, right of and below a 37 x 23 image, and touching it only at a corner or an edge it does not own."""
    sc, verts, faces = _screen_quad(*box, 37, 23)
    assert (RN.render(sc, faces, verts, np.zeros((1, 3)), samples=S)["ids"] >= 0).sum() == 0


# ------------------------------------------------------------------------------------------------ arguments and errors
def test_renderer_has_no_cpu_fallback():
    from tokenhmr_amd.render import Renderer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Renderer(CFG, np.zeros((1, 3), np.int64), device="cpu")


def test_bad_arguments_are_rejected_before_device_work(built_lib):
    from tokenhmr_amd import render as R
    faces = np.array([[0, 1, 2]])
    r = R.Renderer(CFG, faces, device="cuda:0")              # no device work until a call passes its checks
    v, t = torch.zeros(2, 3, 3), torch.zeros(2, 3)
    with pytest.raises(ValueError):
        r.render_batch(v[:, :, :2], t)
    with pytest.raises(ValueError):
        r.render_batch(v, t[:1])
    with pytest.raises(ValueError):
        r.render_batch(v, t, images=torch.zeros(3, 3, 8, 8))
    with pytest.raises(ValueError):
        r.render_scene(v, t, 9000, 10)
    with pytest.raises(ValueError):
        r.render_scene(torch.zeros(1, 2, 3), t[:1], 64, 64)   # faces index vertex 2
    with pytest.raises(ValueError):
        R.Renderer(CFG, faces, samples=2)
    with pytest.raises(ValueError):
        R.check_faces(np.zeros((4, 2), np.int64))
    with pytest.raises(ValueError):
        R.build_scene("wireframe", 8, 8, 100.0)
    assert not r._handles
    # the C ABI validates too, before it touches a device
    L = built_lib
    h = C.c_void_p()
    bad = np.array([[0, 1, 5]], np.int32)
    assert L.thmr_renderer_create(0, bad.ctypes.data, 1, 3, C.byref(h)) < 0 and not h.value
    assert b"outside [0, 3)" in L.thmr_renderer_last_error(None)
    d = R.make_desc(R.build_scene("rgba", 8, 8, 100.0), 4, 0, 4)
    one = C.c_void_p(1)
    assert L.thmr_renderer_run(None, C.byref(d), one, one, 1, None, one, None) < 0
    assert b"null renderer" in L.thmr_renderer_last_error(None)


def test_rgba_scene_fits_the_light_list():
    from tokenhmr_amd import render as R
    s = R.build_scene("rgba", 256, 256, 5000.0)
    assert len(s["lights"]) == 15 <= 16
    d = R.make_desc(s, 4, 1, 4)
    assert d.n_lights == 15 and d.lights[0].type == 1 and d.lights[14].type == 0
