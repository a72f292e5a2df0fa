"""Mesh rendering on the GPU — drop-in for the reference's pyrender Renderer (tokenhmr/lib/utils/renderer.py).

    from tokenhmr_amd.render import Renderer, cam_crop_to_full        # instead of lib.utils.renderer (demo.py:13)
    renderer = Renderer(model_cfg, faces=model.smpl.faces)            # demo.py:52
    regression_img = renderer(verts, cam_t, batch['img'][n], mesh_base_color=LIGHT_BLUE, scene_bg_color=(1, 1, 1))

Same names, signatures, defaults and return types as the reference (numpy float32 images), without pyrender, EGL or trimesh.
The reference's scenes are reduced here, on the host, to one camera frame (x right, y down, z forward — the frame of
perspective_projection), a light list and a material, written into a thmr_render_desc; rasterisation, visibility, shading,
resolve and compositing run in csrc/render.hip.  The batched device entry points the per-person calls wrap are
`Renderer.render_batch` (B crops / side views in one launch) and `Renderer.render_scene` (one frame holding N meshes).

    from tokenhmr_amd.render import MeshRenderer                      # instead of lib.utils (eval.py:19)
    mesh_renderer = MeshRenderer(model_cfg, faces=smpl.faces)         # eval.py --render

`MeshRenderer` is the drop-in for lib/utils/mesh_renderer.py: its contact sheets (the image, the mesh from the front and from the side,
the predicted and the ground-truth OpenPose skeleton per person, tiled as make_grid tiles them) are two RGBA renders plus
thmr_renderer_sheet, which builds the skeletons' draw lists and writes the whole canvas on the device.
There is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _cabi

ZNEAR = 0.05            # faces with a vertex nearer than this are rejected (no clipping: DESIGN.md §3.6)
AMBIENT = (0.3, 0.3, 0.3)
MAX_SIZE = 8192
_NEEDS_GPU = "Renderer needs a GPU device: the render kernels have no CPU fallback"


# ------------------------------------------------------------------------------------------------ the reference's scene arithmetic
def cam_crop_to_full(cam_bbox, box_center, box_size, img_size, focal_length=5000.):
    """renderer.py:13-23, in torch, on the device the arguments live on."""
    img_w, img_h = img_size[:, 0], img_size[:, 1]
    cx, cy, b = box_center[:, 0], box_center[:, 1], box_size
    w_2, h_2 = img_w / 2., img_h / 2.
    bs = b * cam_bbox[:, 0] + 1e-9
    tz = 2 * focal_length / bs
    tx = (2 * (cx - w_2) / bs) + cam_bbox[:, 1]
    ty = (2 * (cy - h_2) / bs) + cam_bbox[:, 2]
    return torch.stack([tx, ty, tz], dim=-1)


def rotation_matrix(angle, direction):
    """trimesh.transformations.rotation_matrix about the origin (Rodrigues, float64), 3x3."""
    sina, cosa = math.sin(angle), math.cos(angle)
    d = np.asarray(direction, dtype=np.float64)[:3]
    d = d / np.sqrt(np.dot(d, d))
    M = np.diag([cosa, cosa, cosa])
    M += np.outer(d, d) * (1.0 - cosa)
    d = d * sina
    M += np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return M


def _rot(axis, theta):
    c, s = np.cos(theta), np.sin(theta)
    m = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return torch.tensor(m, dtype=torch.float32)


def get_light_poses(n_lights=5, elevation=np.pi / 3, dist=12):
    """renderer.py:25-34 (make_rotation(rx=-theta, ry=phi, order='xyz') @ make_translation([0, 0, dist]), float32)."""
    poses = []
    trans = torch.eye(4)
    trans[2, 3] = float(dist)
    for phi in 2 * np.pi * np.arange(n_lights) / n_lights:
        rot = torch.eye(4)
        rot[:3, :3] = _rot("z", 0) @ _rot("y", phi) @ _rot("x", -elevation)
        poses.append((rot @ trans).numpy())
    return poses


def create_raymond_lights():
    """renderer.py:106-135: three directional lights as (4x4 pose, colour, intensity)."""
    out = []
    for phi, theta in zip(np.pi * np.array([0.0, 2.0 / 3.0, 4.0 / 3.0]), np.pi * np.array([1.0 / 6.0] * 3)):
        z = np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])
        z = z / np.linalg.norm(z)
        x = np.array([-z[1], z[0], 0.0])
        if np.linalg.norm(x) == 0:
            x = np.array([1.0, 0.0, 0.0])
        x = x / np.linalg.norm(x)
        y = np.cross(z, x)
        m = np.eye(4)
        m[:3, :3] = np.c_[x, y, z]
        out.append(m)
    return out


_FLIP = np.diag([1.0, -1.0, -1.0])        # GL camera axes (y up, looking down -z) -> the image frame


def _to_camera(kind, pose, cam_pos):
    """A light node's world pose -> (type, vec) in the camera frame; the camera rotation is the identity in every scene."""
    if kind == _cabi.LIGHT_DIRECTIONAL:
        return kind, _FLIP @ (-pose[:3, 2])          # pyrender: a directional light shines along its node's -z axis
    return kind, _FLIP @ (pose[:3, 3] - cam_pos)


def build_scene(kind, width, height, focal_length, cam_t=None, side_view=False, rot_angle=None, rot_axis=(1, 0, 0),
                mesh_base_color=(1.0, 1.0, 0.9), scene_bg_color=(0, 0, 0)):
    """The reference's scene for one call, in the camera frame.  kind = "call" (Renderer.__call__) or "rgba"
    (render_rgba / render_rgba_multiple).  For "call", cam_t is the camera_translation the caller passed (before the
    reference's in-place negation); the camera-frame vertices are R v + t.  For "rgba" they are R (v + t)."""
    W, H = int(width), int(height)
    s = {"width": W, "height": H, "fx": float(focal_length), "fy": float(focal_length), "cx": W / 2., "cy": H / 2., "znear": ZNEAR,
         "ambient": AMBIENT, "bg": tuple(float(c) for c in scene_bg_color), "base_color": tuple(float(c) for c in mesh_base_color)}
    lights = []
    if rot_angle is None:
        rot_angle = 90 if kind == "call" else 0
    if kind == "call":
        s["R"] = rotation_matrix(np.radians(rot_angle), [0, 1, 0]) if side_view else np.eye(3)
        s["translate_first"] = False
        t = np.asarray(cam_t, dtype=np.float64)
        cam_pos = np.array([-t[0], t[1], t[2]])          # camera_translation[0] *= -1 (renderer.py:189), then the camera pose
        s["metallic"], s["roughness"] = 0.0, 1.0         # MetallicRoughnessMaterial(metallicFactor=0.0): roughness defaults to 1
        for m in create_raymond_lights():
            lights.append(_to_camera(_cabi.LIGHT_DIRECTIONAL, m, cam_pos) + (np.ones(3), 1.0))
    elif kind == "rgba":
        s["R"] = rotation_matrix(np.radians(rot_angle), rot_axis)
        s["translate_first"] = True
        cam_pos = np.zeros(3)
        s["metallic"], s["roughness"] = 0.2, 0.8         # pyrender's default material for a vertex-coloured trimesh
        cam_pose = np.eye(4)
        for p in get_light_poses(dist=0.5) + [np.eye(4)]:                 # add_point_lighting (renderer.py:379-396)
            lights.append(_to_camera(_cabi.LIGHT_POINT, cam_pose @ p, cam_pos) + (np.ones(3), 1.0))
        for p in get_light_poses() + [np.eye(4)]:                         # add_lighting (renderer.py:361-377)
            lights.append(_to_camera(_cabi.LIGHT_DIRECTIONAL, cam_pose @ p, cam_pos) + (np.ones(3), 1.0))
        for m in create_raymond_lights():
            lights.append(_to_camera(_cabi.LIGHT_DIRECTIONAL, m, cam_pos) + (np.ones(3), 1.0))
    else:
        raise ValueError(f"unknown scene kind {kind!r}")
    s["lights"] = lights
    return s


def camera_frame_vertices(scene, vertices, cam_t):
    """float64 restatement of what the kernel computes in fp32: R v + t, or R (v + t)."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(cam_t, dtype=np.float64)
    return (v + t) @ scene["R"].T if scene["translate_first"] else v @ scene["R"].T + t


def make_desc(scene, samples, mode, out_channels, mesh_colors=None, mean=(0, 0, 0), std=(1, 1, 1), ids=None):
    d = _cabi.RenderDesc()
    d.width, d.height = scene["width"], scene["height"]
    d.fx, d.fy, d.cx, d.cy, d.znear = scene["fx"], scene["fy"], scene["cx"], scene["cy"], scene["znear"]
    d.samples, d.mode, d.translate_first = samples, mode, int(scene["translate_first"])
    d.rot[:] = [float(x) for x in np.asarray(scene["R"], dtype=np.float32).reshape(9)]
    d.base_color[:] = scene["base_color"]
    d.mesh_colors = mesh_colors.ctypes.data_as(C.POINTER(C.c_float)) if mesh_colors is not None else None
    d.bg_color[:] = scene["bg"]
    d.metallic, d.roughness = scene["metallic"], scene["roughness"]
    d.ambient[:] = scene["ambient"]
    if len(scene["lights"]) > _cabi.RENDER_MAX_LIGHTS:
        raise ValueError("too many lights")
    d.n_lights = len(scene["lights"])
    for i, (kind, vec, color, inten) in enumerate(scene["lights"]):
        d.lights[i].type = kind
        d.lights[i].vec[:] = [float(x) for x in vec]
        d.lights[i].color[:] = [float(x) for x in color]
        d.lights[i].intensity = float(inten)
    d.out_channels = out_channels
    d.img_mean[:] = [float(x) for x in mean]
    d.img_std[:] = [float(x) for x in std]
    d.ids_dev = ids.data_ptr() if ids is not None else None
    return d


def _get(cfg, *path):
    for k in path:
        cfg = getattr(cfg, k) if hasattr(cfg, k) else cfg[k]
    return cfg


def check_faces(faces):
    f = np.asarray(faces.cpu().numpy() if torch.is_tensor(faces) else faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"faces must be an (F, 3) integer array, got {f.dtype} {f.shape}")
    if f.min() < 0:
        raise ValueError("faces hold a negative vertex index")
    return np.ascontiguousarray(f, dtype=np.int32)


def check_meshes(vertices, cam_t, n_verts=None):
    """(N, V, 3) and (N, 3) floating arrays / tensors; raises ValueError before any device work."""
    v_shape, t_shape = tuple(vertices.shape), tuple(cam_t.shape)
    if len(v_shape) != 3 or v_shape[2] != 3 or v_shape[0] < 1:
        raise ValueError(f"vertices must be (N, V, 3), got {v_shape}")
    if t_shape != (v_shape[0], 3):
        raise ValueError(f"cam_t must be ({v_shape[0]}, 3), got {t_shape}")
    if n_verts is not None and v_shape[1] <= n_verts:
        raise ValueError(f"the faces index {n_verts + 1} vertices, the meshes have {v_shape[1]}")


def check_size(width, height):
    if not (1 <= int(width) <= MAX_SIZE and 1 <= int(height) <= MAX_SIZE):
        raise ValueError(f"render size {width}x{height} outside 1 ... {MAX_SIZE}")


class Mesh:
    """What vertices_to_trimesh returns: .vertices (V, 3) float64, .faces (F, 3), .visual.vertex_colors / .vertex_colors (V, 4)
    RGBA uint8 (trimesh's storage), and .export(path) to Wavefront .obj with per-vertex colours."""

    class _Visual:
        def __init__(self, c):
            self.vertex_colors = c

    def __init__(self, vertices, faces, vertex_colors):
        self.vertices, self.faces = vertices, faces
        self.vertex_colors = np.clip(np.round(np.asarray(vertex_colors, dtype=np.float64) * 255), 0, 255).astype(np.uint8)
        self.visual = Mesh._Visual(self.vertex_colors)

    def export(self, file_obj, file_type=None):
        lines = []
        for v, c in zip(self.vertices, self.vertex_colors):
            lines.append("v %.8f %.8f %.8f %.8f %.8f %.8f" % (v[0], v[1], v[2], c[0] / 255.0, c[1] / 255.0, c[2] / 255.0))
        for f in self.faces:
            lines.append("f %d %d %d" % (f[0] + 1, f[1] + 1, f[2] + 1))
        text = "\n".join(lines) + "\n"
        if file_obj is None:
            return text
        with open(file_obj, "w") as fh:
            fh.write(text)
        return text


# ------------------------------------------------------------------------------------------------ the renderer
class _Handle(_cabi.Handle):
    """One thmr_renderer: the vertex -> face lists of `faces` for meshes of V vertices, and its grow-only scratch."""

    def __init__(self, device, faces, V):
        super().__init__(device, "thmr_renderer", _NEEDS_GPU)
        self._open(self._index(), faces.ctypes.data, faces.shape[0], V)


class Renderer:
    """renderer.py:137-396 on the GPU.  Owns one thmr_renderer handle per vertex count (the vertex -> face lists)."""

    def __init__(self, cfg, faces, device="cuda:0", samples=4):
        dev = _Handle.cuda_device(device, _NEEDS_GPU, resolve=False)
        if samples not in (1, 4):
            raise ValueError("samples must be 1 or 4")
        self.cfg = cfg
        self.focal_length = _get(cfg, "EXTRA", "FOCAL_LENGTH")
        self.img_res = _get(cfg, "MODEL", "IMAGE_SIZE")
        self.camera_center = [self.img_res // 2, self.img_res // 2]
        self.faces = faces
        self.samples = samples
        self._faces32 = check_faces(faces)
        self._max_index = int(self._faces32.max())
        self.device = _Handle.cuda_device(dev, _NEEDS_GPU, resolve=True)
        self.lib = _cabi.load()
        self._handles = {}

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles = {}

    def _owner(self, V):
        """The _Handle for meshes of V vertices, created on first use; it is destroyed by close() or with this object."""
        if V not in self._handles:
            self._handles[V] = _Handle(self.device, self._faces32, V)
        return self._handles[V]

    def _handle(self, V):
        return self._owner(V).h

    def _run(self, scene, vertices, cam_t, mode, out_channels, images=None, mesh_colors=None, mean=(0, 0, 0), std=(1, 1, 1),
             return_ids=False):
        check_meshes(vertices, cam_t, self._max_index)
        v = torch.as_tensor(vertices).to(self.device, torch.float32).contiguous()
        t = torch.as_tensor(cam_t).to(self.device, torch.float32).contiguous()
        N, V = v.shape[0], v.shape[1]
        n_img = 1 if mode == _cabi.RENDER_ONE_IMAGE else N
        H, W = scene["height"], scene["width"]
        out = torch.empty(n_img, H, W, out_channels, device=self.device, dtype=torch.float32)
        ids = torch.empty(n_img, H, W, self.samples, device=self.device, dtype=torch.int32) if return_ids else None
        img = None
        if images is not None:
            img = torch.as_tensor(images).to(self.device, torch.float32).contiguous()
        colors = None
        if mesh_colors is not None:
            colors = np.ascontiguousarray(np.broadcast_to(np.asarray(mesh_colors, dtype=np.float32), (N, 3)))
        d = make_desc(scene, self.samples, mode, out_channels, colors, mean, std, ids)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            owner = self._owner(V)
            rc = self.lib.thmr_renderer_run(owner.h, C.byref(d), v.data_ptr(), t.data_ptr(), N, img.data_ptr() if img is not None else None,
                                            out.data_ptr(), stream)
        owner._check(rc, "thmr_renderer_run")
        return (out, ids) if return_ids else out

    # ---- batched device paths
    def render_batch(self, vertices, cam_t, images=None, side_view=False, rot_angle=90, mesh_base_color=(1.0, 1.0, 0.9),
                     scene_bg_color=(0, 0, 0), return_rgba=False, width=None, height=None, return_ids=False):
        """B crops (or side views) in one launch: what B calls of __call__ compute, image for image.  vertices (B, V, 3),
        cam_t (B, 3) as the reference's camera_translation (NOT negated here: the caller's arrays are not touched), images
        (B, 3, H, W) normalised crops or None (then width x height, default IMAGE_SIZE squared).  Returns a (B, H, W, 3) CUDA
        tensor — the overlay, or the colour alone for side views — or (B, H, W, 4) RGBA with return_rgba.  return_ids adds the
        (B, H, W, samples) int32 winning face ids (mesh * F + face, -1 = background)."""
        check_meshes(vertices, cam_t)
        B = vertices.shape[0]
        if images is not None:
            if tuple(images.shape[:2]) != (B, 3) or len(images.shape) != 4:
                raise ValueError(f"images must be ({B}, 3, H, W), got {tuple(images.shape)}")
            height, width = int(images.shape[2]), int(images.shape[3])
        width = int(width if width is not None else self.img_res)
        height = int(height if height is not None else self.img_res)
        check_size(width, height)
        ct = cam_t.detach().cpu().numpy() if torch.is_tensor(cam_t) else np.asarray(cam_t)
        scene = build_scene("call", width, height, self.focal_length, np.zeros(3), side_view, rot_angle, mesh_base_color=mesh_base_color,
                            scene_bg_color=scene_bg_color)
        composite = images is not None and not side_view and not return_rgba
        mean = [float(np.float32(x)) for x in _get(self.cfg, "MODEL", "IMAGE_MEAN")] if composite else (0, 0, 0)
        std = [float(np.float32(x)) for x in _get(self.cfg, "MODEL", "IMAGE_STD")] if composite else (1, 1, 1)
        return self._run(scene, vertices, torch.as_tensor(np.asarray(ct, dtype=np.float32)), _cabi.RENDER_PER_IMAGE,
                         4 if return_rgba else 3, images if composite else None, None, mean, std, return_ids)

    def render_scene(self, vertices, cam_t, width, height, focal_length=None, rot_axis=(1, 0, 0), rot_angle=0,
                     mesh_base_color=(1.0, 1.0, 0.9), scene_bg_color=(0, 0, 0), mesh_colors=None, return_ids=False):
        """One width x height frame holding N meshes (render_rgba_multiple's scene): vertices (N, V, 3), cam_t (N, 3).
        Returns the (H, W, 4) RGBA CUDA tensor (and the (H, W, samples) ids with return_ids).  mesh_colors (N, 3) overrides
        mesh_base_color per mesh."""
        check_meshes(vertices, cam_t)
        check_size(width, height)
        scene = build_scene("rgba", width, height, self.focal_length if focal_length is None else focal_length, rot_angle=rot_angle,
                            rot_axis=rot_axis, mesh_base_color=mesh_base_color, scene_bg_color=scene_bg_color)
        r = self._run(scene, vertices, cam_t, _cabi.RENDER_ONE_IMAGE, 4, mesh_colors=mesh_colors, return_ids=return_ids)
        return (r[0][0], r[1][0]) if return_ids else r[0]

    # ---- the reference's per-person calls (renderer.py:153-359)
    def __call__(self, vertices, camera_translation, image, full_frame=False, imgname=None, side_view=False, rot_angle=90,
                 mesh_base_color=(1.0, 1.0, 0.9), scene_bg_color=(0, 0, 0), return_rgba=False):
        if full_frame:
            import cv2                    # the reference reads the frame here; image decoding stays with cv2
            frame = cv2.imread(imgname).astype(np.float32)[:, :, ::-1] / 255.
            H, W = frame.shape[:2]
        else:
            if not torch.is_tensor(image) or image.dim() != 3 or image.shape[0] != 3:
                raise ValueError("image must be a (3, H, W) tensor of normalised pixel values")
            H, W = int(image.shape[1]), int(image.shape[2])
        v = np.asarray(vertices, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError(f"vertices must be (V, 3), got {v.shape}")
        t = np.array(camera_translation, dtype=np.float64).reshape(3)
        camera_translation[0] *= -1.                  # renderer.py:189 — an in-place side effect on the caller's array
        if full_frame:
            rgba = self.render_batch(v[None], t[None], None, side_view, rot_angle, mesh_base_color, scene_bg_color, True, W, H)
            color = rgba[0].cpu().numpy()
            if return_rgba:
                return color
            if side_view:
                return color[:, :, :3].astype(np.float32)
            a = color[:, :, -1][:, :, None]
            return (color[:, :, :3] * a + (1 - a) * frame).astype(np.float32)
        out = self.render_batch(v[None], t[None], image[None], side_view, rot_angle, mesh_base_color, scene_bg_color, return_rgba)
        return out[0].cpu().numpy()

    def vertices_to_trimesh(self, vertices, camera_translation, mesh_base_color=(1.0, 1.0, 0.9), rot_axis=[1, 0, 0], rot_angle=0):
        """renderer.py:233-251: (v + t), rotated about the origin, then 180 degrees about x — in float64, on the host."""
        vertex_colors = np.array([(*mesh_base_color, 1.0)] * vertices.shape[0])
        v = np.asarray(vertices, dtype=np.float64) + np.asarray(camera_translation, dtype=np.float64)
        v = v @ rotation_matrix(np.radians(rot_angle), rot_axis).T
        v = v @ rotation_matrix(np.radians(180), [1, 0, 0]).T
        return Mesh(v, np.asarray(self.faces).copy(), vertex_colors)

    def render_rgba(self, vertices, cam_t=None, rot=None, rot_axis=[1, 0, 0], rot_angle=0, camera_z=3, mesh_base_color=(1.0, 1.0, 0.9),
                    scene_bg_color=(0, 0, 0), render_res=[256, 256]):
        if cam_t is not None:
            camera_translation = np.array(cam_t, dtype=np.float64).copy()
        else:
            camera_translation = np.array([0, 0, camera_z * self.focal_length / render_res[1]])
        return self.render_rgba_multiple([vertices], [camera_translation], rot_axis, rot_angle, mesh_base_color, scene_bg_color, render_res)

    def render_rgba_multiple(self, vertices, cam_t, rot_axis=[1, 0, 0], rot_angle=0, mesh_base_color=(1.0, 1.0, 0.9), scene_bg_color=(0, 0, 0),
                             render_res=[256, 256], focal_length=None):
        if len(vertices) != len(cam_t) or len(vertices) == 0:
            raise ValueError("one camera translation per mesh, at least one mesh")
        v = np.stack([np.asarray(x, dtype=np.float32) for x in vertices])
        t = np.stack([np.asarray(x, dtype=np.float32).reshape(3) for x in cam_t])
        out = self.render_scene(v, t, render_res[0], render_res[1], focal_length, rot_axis, rot_angle, mesh_base_color, scene_bg_color)
        return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the contact sheets of eval.py --render
def sheet_geometry(n_tiles, nrow, padding, height, width):
    """torchvision.utils.make_grid(list of n_tiles (3, height, width) tensors, nrow, padding): (xmaps, ymaps, canvas height,
    canvas width).  Tile k starts at row padding + (k // xmaps) (height + padding), column padding + (k % xmaps) (width + padding)."""
    xmaps = min(int(nrow), int(n_tiles))
    ymaps = -(-int(n_tiles) // xmaps)
    return xmaps, ymaps, ymaps * (height + padding) + padding, xmaps * (width + padding) + padding


def side_translation(cam_t):
    """The translation the reference's side view sees in visualize*: __call__ negates camera_translation[i][0] in place on both of
    its calls, so the second one (the side view) runs on (-tx, ty, tz) in this project's frame and leaves the caller's array restored."""
    if torch.is_tensor(cam_t):
        return torch.cat([-cam_t[..., :1], cam_t[..., 1:]], dim=-1)
    return np.asarray(cam_t) * np.array([-1.0, 1.0, 1.0], dtype=np.asarray(cam_t).dtype)


class MeshRenderer:
    """lib/utils/mesh_renderer.py:44-157 on the GPU: same constructor, __call__, visualize and visualize_tensorboard.  The arguments
    are the reference's NumPy arrays or torch tensors already on the device (all of one kind); the sheets come back as a
    (3, Hg, Wg) float32 tensor on the device, __call__ as a NumPy (H, W, 3) image.  With device tensors nothing is copied to the
    host and nothing synchronises."""

    def __init__(self, cfg, faces=None, device="cuda:0", samples=4):
        dev = _Handle.cuda_device(device, "MeshRenderer needs a GPU device: the render kernels have no CPU fallback", resolve=False)
        if samples not in (1, 4):
            raise ValueError("samples must be 1 or 4")
        self.cfg = cfg
        self.focal_length = _get(cfg, "EXTRA", "FOCAL_LENGTH")
        self.img_res = _get(cfg, "MODEL", "IMAGE_SIZE")
        self.camera_center = [self.img_res // 2, self.img_res // 2]
        self.faces = faces
        self._device, self._samples = dev, samples
        self._renderer = None

    @property
    def renderer(self):
        """The Renderer that owns the device handle; faces=None is accepted at construction, as in the reference, and fails here."""
        if self._renderer is None:
            if self.faces is None:
                raise ValueError("MeshRenderer was constructed without faces: nothing to render")
            self._renderer = Renderer(self.cfg, self.faces, self._device, self._samples)
        return self._renderer

    def close(self):
        if self._renderer is not None:
            self._renderer.close()

    def scene(self, width, height, focal_length, side_view=False, rot_angle=90, baseColorFactor=(1.0, 1.0, 0.9, 1.0)):
        """mesh_renderer.py:109-146 in the camera frame: Renderer.__call__'s scene with a transparent black background."""
        return build_scene("call", width, height, focal_length, np.zeros(3), side_view, rot_angle,
                           mesh_base_color=tuple(baseColorFactor)[:3], scene_bg_color=(0, 0, 0))

    def _sheet(self, n_verts, images, front, side, panels, pred=None, gt=None, nrow=1, padding=0):
        """thmr_renderer_sheet on device tensors; returns (canvas, records or None)."""
        r = self.renderer
        B, _, H, W = images.shape
        n_skel = (pred is not None) + (gt is not None)
        n_panels = bin(panels).count("1") + n_skel
        _, _, Hg, Wg = sheet_geometry(B * n_panels, nrow, padding, H, W)
        canvas = torch.empty(3, Hg, Wg, device=r.device, dtype=torch.float32)
        records = torch.empty(n_skel * B, _cabi.SHEET_RECORDS, _cabi.SHEET_RECORD_WORDS, device=r.device, dtype=torch.int32) if n_skel else None
        d = _cabi.SheetDesc(B, W, H, int(self.img_res), panels, int(nrow), int(padding), Wg, Hg)
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(r.device):
            stream = torch.cuda.current_stream(r.device).cuda_stream
            owner = r._owner(n_verts)                  # the handle the two renders ran on
            rc = r.lib.thmr_renderer_sheet(owner.h, C.byref(d), images.data_ptr(), ptr(front), ptr(side), ptr(pred), ptr(gt), ptr(records),
                                           canvas.data_ptr(), stream)
        owner._check(rc, "thmr_renderer_sheet")
        return canvas, records

    def __call__(self, vertices, camera_translation, image, focal_length=5000, text=None, resize=None, side_view=False,
                 baseColorFactor=(1.0, 1.0, 0.9, 1.0), rot_angle=90):
        """One person over one (H, W, 3) image with values in 0 ... 1 (the side view over ones): the mesh where all samples of a pixel
        are covered (alpha > 0.8), the background elsewhere.  `text` is unused, as in the reference."""
        if resize is not None:
            raise NotImplementedError("resize= needs cv2.resize, which this renderer does not restate; resize the returned image")
        img = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"image must be (H, W, 3), got {img.shape}")
        v = vertices.detach().cpu().numpy() if torch.is_tensor(vertices) else np.asarray(vertices)
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError(f"vertices must be (V, 3), got {v.shape}")
        H, W = int(img.shape[0]), int(img.shape[1])
        check_size(W, H)
        r = self.renderer
        t = np.array(camera_translation, dtype=np.float64).reshape(3)
        check_meshes(v[None], t[None], r._max_index)
        camera_translation[0] *= -1.                  # mesh_renderer.py:118 — in place, on the caller's array
        rgba = r._run(self.scene(W, H, focal_length, side_view, rot_angle, baseColorFactor), v[None].astype(np.float32), t[None],
                      _cabi.RENDER_PER_IMAGE, 4)
        images = torch.as_tensor(np.ascontiguousarray(img.transpose(2, 0, 1)[None], dtype=np.float32)).to(r.device)
        canvas, _ = self._sheet(v.shape[0], images, None if side_view else rgba, rgba if side_view else None,
                                _cabi.SHEET_SIDE if side_view else _cabi.SHEET_FRONT)
        return np.ascontiguousarray(canvas.permute(1, 2, 0).cpu().numpy())

    def _sheet_arguments(self, vertices, camera_translation, images, pred_keypoints=None, gt_keypoints=None):
        """Every check of visualize / visualize_tensorboard, before any device work.  Returns on_device."""
        args = [a for a in (vertices, camera_translation, images, pred_keypoints, gt_keypoints) if a is not None]
        tensors = [a for a in args if torch.is_tensor(a)]
        if tensors and (len(tensors) != len(args) or any(a.device != self.renderer.device for a in tensors)):
            raise ValueError("pass every argument as a NumPy array, or every argument as a tensor on the renderer's device")
        check_meshes(vertices, camera_translation, self.renderer._max_index)
        B = int(vertices.shape[0])
        if len(images.shape) != 4 or tuple(images.shape[:2]) != (B, 3):
            raise ValueError(f"images must be ({B}, 3, H, W), got {tuple(images.shape)}")
        check_size(images.shape[3], images.shape[2])
        if pred_keypoints is not None and tuple(pred_keypoints.shape) != (B, _cabi.SHEET_KEYPOINTS, 2):
            raise ValueError(f"pred_keypoints must be ({B}, {_cabi.SHEET_KEYPOINTS}, 2), got {tuple(pred_keypoints.shape)}")
        if gt_keypoints is not None:
            if tuple(gt_keypoints.shape) != (B, _cabi.SHEET_KEYPOINTS, 3):
                raise ValueError(f"gt_keypoints must be ({B}, {_cabi.SHEET_KEYPOINTS}, 3), got {tuple(gt_keypoints.shape)}")
            floating = gt_keypoints.dtype.is_floating_point if tensors else np.issubdtype(gt_keypoints.dtype, np.floating)
            if not floating:
                raise ValueError("gt_keypoints are scaled in place: they must be a floating-point array")
        return bool(tensors)

    def _sheets(self, vertices, camera_translation, images, pred_keypoints, gt_keypoints, nrow, padding):
        on_device = self._sheet_arguments(vertices, camera_translation, images, pred_keypoints, gt_keypoints)
        if int(nrow) < 1 or int(padding) < 0:
            raise ValueError("nrow must be >= 1 and padding >= 0")
        r = self.renderer
        dev = lambda a: None if a is None else torch.as_tensor(a).detach().to(r.device, torch.float32).contiguous()
        v, t, img, pred, gt = dev(vertices), dev(camera_translation), dev(images), dev(pred_keypoints), dev(gt_keypoints)
        H, W = int(img.shape[2]), int(img.shape[3])
        # the reference calls __call__ twice on the same camera_translation[i], which it negates in place each time: the front view
        # sees t, the side view (-tx, ty, tz), and the caller's array ends up as it was.  visualize* ignore their focal_length.
        front = r._run(self.scene(W, H, self.focal_length), v, t, _cabi.RENDER_PER_IMAGE, 4)
        side = r._run(self.scene(W, H, self.focal_length, side_view=True), v, side_translation(t), _cabi.RENDER_PER_IMAGE, 4)
        canvas, _ = self._sheet(int(v.shape[1]), img, front, side, _cabi.SHEET_IMAGE | _cabi.SHEET_FRONT | _cabi.SHEET_SIDE, pred, gt, nrow, padding)
        if gt_keypoints is not None:                   # scaled and remapped in place, like the reference's caller array
            if not on_device:
                gt_keypoints[...] = gt.cpu().numpy()
            elif gt.data_ptr() != gt_keypoints.data_ptr():
                gt_keypoints.copy_(gt)
        return canvas

    def visualize(self, vertices, camera_translation, images, focal_length=None, nrow=3, padding=2):
        """mesh_renderer.py:57-68: per person the image, the front and the side view, tiled nrow to a row."""
        return self._sheets(vertices, camera_translation, images, None, None, nrow, padding)

    def visualize_tensorboard(self, vertices, camera_translation, images, pred_keypoints, gt_keypoints, focal_length=None, nrow=5, padding=2):
        """mesh_renderer.py:70-107: visualize's tiles plus the predicted and the ground-truth OpenPose skeleton over the image; nrow
        shrinks by one for each keypoint set that is None.  gt_keypoints is scaled to pixels and remapped in place."""
        nrow = nrow - 1 if gt_keypoints is None else nrow
        nrow = nrow - 1 if pred_keypoints is None else nrow
        return self._sheets(vertices, camera_translation, images, pred_keypoints, gt_keypoints, nrow, padding)
