"""NumPy restatement of the renderer contract — test infrastructure for tests/test_render_host.py and
tests/test_gpu_render.py / tests/test_gpu_render_edges.py.

  * transform + projection: the kernel's fp32 operations in the kernel's order (numpy float32 arithmetic is IEEE, no fused
    multiply-add), snapped to 1/256 px with round-half-even — bit for bit what csrc/render.hip computes
  * coverage: exact int64 edge functions, top-left rule, back-face / degenerate / znear / guard-band rejection — bit for bit
  * visibility: smallest (depth, mesh * F + face) per sample, depth perspective-correct in float64
  * shading, resolve, compositing: float64, then the 8-bit rounding and the fp32 composite of the contract
"""
import numpy as np

OX = np.array([96, 224, 32, 160])
OY = np.array([32, 96, 160, 224])
GUARD = np.float32(2097152.0)
F32 = np.float32


def project(scene, verts, cam_t):
    """(N, V, 3), (N, 3) -> camera-frame positions (float32), snapped (N, V, 2) int64, usable (N, V) bool."""
    v = np.asarray(verts, dtype=F32)
    t = np.asarray(cam_t, dtype=F32)[:, None, :]
    R = np.asarray(scene["R"], dtype=F32)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    if scene["translate_first"]:
        x, y, z = x + t[..., 0], y + t[..., 1], z + t[..., 2]
    X = R[0, 0] * x + R[0, 1] * y + R[0, 2] * z
    Y = R[1, 0] * x + R[1, 1] * y + R[1, 2] * z
    Z = R[2, 0] * x + R[2, 1] * y + R[2, 2] * z
    if not scene["translate_first"]:
        X, Y, Z = X + t[..., 0], Y + t[..., 1], Z + t[..., 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = X / Z * F32(scene["fx"]) + F32(scene["cx"])
        w = Y / Z * F32(scene["fy"]) + F32(scene["cy"])
        ok = (Z >= F32(scene["znear"])) & (np.abs(u) <= GUARD) & (np.abs(w) <= GUARD)
        fix = np.stack([np.where(ok, np.rint(u * F32(256)), 0), np.where(ok, np.rint(w * F32(256)), 0)], -1).astype(np.int64)
    return np.stack([X, Y, Z], -1), fix, ok


def edge(a, b, p):
    return (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])


def _inside(e, a, b):
    dx, dy = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    return (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def vertex_normals(P, faces):
    """trimesh-style smooth normals: unit face normals weighted by the corner angle, summed, normalised (float64)."""
    P = np.asarray(P, dtype=np.float64)
    a, b, c = P[faces[:, 0]], P[faces[:, 1]], P[faces[:, 2]]
    fn = np.cross(b - a, c - a)
    fl = np.linalg.norm(fn, axis=1)
    good = fl > 0
    fn = np.where(good[:, None], fn / np.where(good, fl, 1)[:, None], 0)
    n = np.zeros_like(P)
    for k in range(3):
        o, q, r = P[faces[:, k]], P[faces[:, (k + 1) % 3]], P[faces[:, (k + 2) % 3]]
        e1, e2 = q - o, r - o
        l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
        ok = good & (l1 > 0) & (l2 > 0)
        cs = np.clip(np.sum(e1 * e2, 1) / np.where(ok, l1 * l2, 1), -1, 1)
        w = np.where(ok, np.arccos(cs), 0)
        np.add.at(n, faces[:, k], fn * w[:, None])
    ln = np.linalg.norm(n, axis=1)
    return n / np.where(ln > 0, ln, 1)[:, None]


def setup(fix, ok, Z, faces, W, H):
    """per face of one mesh: accepted mask, oriented corners (F, 3, 2), their Z (F, 3), pixel box."""
    a, b, c = fix[faces[:, 0]], fix[faces[:, 1]], fix[faces[:, 2]]
    za, zb, zc = Z[faces[:, 0]].astype(np.float64), Z[faces[:, 1]].astype(np.float64), Z[faces[:, 2]].astype(np.float64)
    acc = ok[faces[:, 0]] & ok[faces[:, 1]] & ok[faces[:, 2]] & (edge(a, b, c) < 0)
    corners = np.stack([a, c, b], 1)              # oriented positively (the kernel swaps corners 1 and 2)
    zs = np.stack([za, zc, zb], 1)
    lo, hi = corners.min(1) >> 8, corners.max(1) >> 8
    acc &= (hi[:, 0] >= 0) & (hi[:, 1] >= 0) & (lo[:, 0] < W) & (lo[:, 1] < H)
    lo = np.maximum(lo, 0)
    hi = np.minimum(hi, [W - 1, H - 1])
    return acc, corners, zs, lo, hi


def rasterize(fix, ok, Z, faces, W, H, S, meshes):
    """winning id (H, W, S) (-1 = none) and its depth (float64) for one image holding `meshes` (indices into fix / ok / Z)."""
    F = faces.shape[0]
    cand = []
    for m in meshes:
        acc, corners, zs, lo, hi = setup(fix[m], ok[m], Z[m], faces, W, H)
        idx = np.nonzero(acc)[0]
        cand.append((m * F + idx, corners[idx], zs[idx], lo[idx], hi[idx]))
    ids = np.concatenate([c[0] for c in cand])
    corners = np.concatenate([c[1] for c in cand])
    zs = np.concatenate([c[2] for c in cand])
    lo = np.concatenate([c[3] for c in cand])
    hi = np.concatenate([c[4] for c in cand])
    win = np.full(H * W * S, -1, np.int64)
    dep = np.full(H * W * S, np.inf)
    if len(ids) == 0:
        return win.reshape(H, W, S), dep.reshape(H, W, S)
    w, h = hi[:, 0] - lo[:, 0] + 1, hi[:, 1] - lo[:, 1] + 1
    n = w * h
    keys, depths, fids = [], [], []
    step = 1 << 22
    starts = np.concatenate([[0], np.cumsum(n)])
    # expand (face, pixel) pairs in bounded chunks of faces
    f0 = 0
    while f0 < len(ids):
        f1 = int(np.searchsorted(starts, starts[f0] + step, side="right")) - 1
        f1 = max(f1, f0 + 1)
        sel = np.arange(f0, f1)
        rep = np.repeat(sel, n[sel])
        local = np.arange(len(rep)) - np.repeat(starts[sel] - starts[f0], n[sel])
        px = lo[rep, 0] + local % w[rep]
        py = lo[rep, 1] + local // w[rep]
        A, B, Cc = corners[rep, 0], corners[rep, 1], corners[rep, 2]
        area = edge(A, B, Cc).astype(np.float64)
        for s in range(S):
            sp = np.stack([px * 256 + (128 if S == 1 else OX[s]), py * 256 + (128 if S == 1 else OY[s])], -1)
            e0, e1, e2 = edge(B, Cc, sp), edge(Cc, A, sp), edge(A, B, sp)
            cov = _inside(e0, B, Cc) & _inside(e1, Cc, A) & _inside(e2, A, B)
            iz = (e0 / area / zs[rep, 0] + e1 / area / zs[rep, 1] + e2 / area / zs[rep, 2])
            keys.append(((py * W + px) * S + s)[cov])
            depths.append((1.0 / iz)[cov])
            fids.append(ids[rep][cov])
        f0 = f1
    keys, depths, fids = np.concatenate(keys), np.concatenate(depths), np.concatenate(fids)
    order = np.lexsort((fids, depths, keys))
    keys, depths, fids = keys[order], depths[order], fids[order]
    first = np.ones(len(keys), bool)
    first[1:] = keys[1:] != keys[:-1]
    win[keys[first]] = fids[first]
    dep[keys[first]] = depths[first]
    return win.reshape(H, W, S), dep.reshape(H, W, S)


def sample_depth(fix, Z, faces, fid, px, py, s, S):
    """float64 depth of face `fid` (mesh * F + face) at sample s of pixel (px, py); arrays broadcast."""
    F = faces.shape[0]
    m, f = fid // F, fid % F
    a, b, c = (fix[m, faces[f, k]] for k in range(3))
    sp = np.stack([px * 256 + (128 if S == 1 else OX[s]), py * 256 + (128 if S == 1 else OY[s])], -1)
    area = edge(a, b, c).astype(np.float64)
    iz = (edge(b, c, sp) / area / Z[m, faces[f, 0]] + edge(c, a, sp) / area / Z[m, faces[f, 1]]
          + edge(a, b, sp) / area / Z[m, faces[f, 2]])
    return 1.0 / iz


def shade(scene, P, N, fix, faces, fid, px, py, colors):
    """shaded colour (K, 3) of faces fid (K,) at the centres of pixels (px, py), float64."""
    F = faces.shape[0]
    m, f = fid // F, fid % F
    vi = faces[f]
    sp = np.stack([px * 256 + 128, py * 256 + 128], -1)
    a, b, c = fix[m, vi[:, 0]], fix[m, vi[:, 1]], fix[m, vi[:, 2]]
    area = edge(a, b, c).astype(np.float64)
    l0, l1 = edge(b, c, sp) / area, edge(c, a, sp) / area
    l = np.stack([l0, l1, 1.0 - l0 - l1], -1)
    Pv = P[m[:, None], vi].astype(np.float64)
    Nv = N[m[:, None], vi]
    w = l / Pv[..., 2]
    w = w / w.sum(1, keepdims=True)
    p = np.einsum("kj,kjc->kc", w, Pv)
    n = np.einsum("kj,kjc->kc", w, Nv)
    nl = np.linalg.norm(n, axis=1, keepdims=True)
    n = n / np.where(nl > 0, nl, 1)
    v = -p / np.linalg.norm(p, axis=1, keepdims=True)
    base = np.asarray(colors, dtype=np.float64)[m]
    met, alpha = scene["metallic"], scene["roughness"] ** 2
    a2 = alpha * alpha
    cdiff = base * (1 - 0.04) * (1 - met)
    f0 = 0.04 * (1 - met) + base * met
    f90 = np.clip(f0.max(1, keepdims=True) * 25, 0, 1)
    ndv = np.clip(np.abs(np.sum(n * v, 1, keepdims=True)), 0.001, 1)
    col = np.asarray(scene["ambient"]) * base
    for kind, vec, color, inten in scene["lights"]:
        vec = np.asarray(vec, dtype=np.float64)
        if kind == 0:
            L, att = np.broadcast_to(-vec, p.shape), 1.0
        else:
            L = vec - p
            att = 1.0 / np.sum(L * L, 1, keepdims=True)
        L = L / np.linalg.norm(L, axis=1, keepdims=True)
        h = L + v
        h = h / np.linalg.norm(h, axis=1, keepdims=True)
        ndl = np.clip(np.sum(n * L, 1, keepdims=True), 0.001, 1)
        ndh = np.clip(np.sum(n * h, 1, keepdims=True), 0, 1)
        vdh = np.clip(np.sum(v * h, 1, keepdims=True), 0, 1)
        Fr = f0 + (f90 - f0) * (1 - vdh) ** 5
        G = (2 * ndl / (ndl + np.sqrt(a2 + (1 - a2) * ndl * ndl))) * (2 * ndv / (ndv + np.sqrt(a2 + (1 - a2) * ndv * ndv)))
        D = a2 / (np.pi * (ndh * ndh * (a2 - 1) + 1) ** 2)
        col = col + att * np.asarray(color) * inten * ndl * ((1 - Fr) * cdiff / np.pi + Fr * G * D / (4 * ndl * ndv))
    return np.clip(np.maximum(col, 0) ** (1 / 2.2), 0, 1)


def to8(x):
    return (np.rint(np.clip(x, 0, 1) * 255).astype(F32) / F32(255)).astype(F32)


def render(scene, faces, verts, cam_t, samples=4, one_image=False, images=None, mean=None, std=None, mesh_colors=None):
    """The whole contract.  Returns dict(out=(n_img, H, W, 3|4) float32, ids=(n_img, H, W, S) int64, depth, fix, Z, P, N, and
    what resolve() needs).
    images (n_img, 3, H, W) normalised -> the __call__ composite (3 channels); else RGBA."""
    faces = np.asarray(faces, dtype=np.int64)
    verts = np.asarray(verts, dtype=F32)
    Nm = verts.shape[0]
    P, fix, ok = project(scene, verts, cam_t)
    Nrm = np.stack([vertex_normals(P[m], faces) for m in range(Nm)])
    W, H, S = scene["width"], scene["height"], samples
    colors = np.broadcast_to(np.asarray(scene["base_color"] if mesh_colors is None else mesh_colors, dtype=F32).astype(np.float64), (Nm, 3))
    groups = [list(range(Nm))] if one_image else [[m] for m in range(Nm)]
    wins, deps = [], []
    for meshes in groups:
        win, dep = rasterize(fix, ok, P[..., 2], faces, W, H, S, meshes)
        wins.append(win)
        deps.append(dep)
    r = {"ids": np.stack(wins), "depth": np.stack(deps), "fix": fix, "Z": P[..., 2], "P": P, "N": Nrm, "scene": scene, "faces": faces,
         "colors": colors, "images": images, "mean": mean, "std": std, "S": S}
    r["out"] = resolve(r, r["ids"])
    return r


def resolve(r, ids):
    """shade + resolve + composite for given per-sample winners (n_img, H, W, S) — the restatement's own, or another
    renderer's, so that a depth tie decided the other way can be checked for its colour too."""
    scene, S = r["scene"], r["S"]
    H, W = ids.shape[1:3]
    outs = []
    for gi in range(ids.shape[0]):
        win = ids[gi]
        k = (win >= 0).sum(-1)
        acc = np.zeros((H, W, 3))
        cov = np.nonzero(win >= 0)
        if len(cov[0]):
            col = shade(scene, r["P"], r["N"], r["fix"], r["faces"], win[cov], cov[1], cov[0], r["colors"])
            np.add.at(acc, (cov[0], cov[1]), col)
        rgb = to8((acc + (S - k)[..., None] * np.asarray(scene["bg"])) / S)
        a = to8(k / S)
        if r["images"] is not None:
            im = np.asarray(r["images"][gi], dtype=F32).transpose(1, 2, 0) * np.asarray(r["std"], dtype=F32) + np.asarray(r["mean"], dtype=F32)
            av = a[..., None]
            o = rgb * av + (F32(1) - av) * im
        else:
            o = np.concatenate([rgb, a[..., None]], -1)
        outs.append(o.astype(F32))
    return np.stack(outs)


# ------------------------------------------------------------------------------------------------ synthetic meshes
def uv_sphere(n_lon=32, n_lat=16, r=1.0, center=(0, 0, 0)):
    """Closed sphere, faces counter-clockwise seen from outside (outward normals)."""
    verts = [(0, 0, r), (0, 0, -r)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            verts.append((r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)))
    ring = lambda i, j: 2 + (i - 1) * n_lon + (j % n_lon)
    faces = []
    for j in range(n_lon):
        faces.append((0, ring(1, j), ring(1, j + 1)))
        faces.append((1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            faces += [(a, c, d), (a, d, b)]
    return np.asarray(verts, np.float64) + np.asarray(center), np.asarray(faces, np.int64)


def torus(n_major=48, n_minor=24, R=1.0, r=0.35):
    verts, faces = [], []
    for i in range(n_major):
        u = 2 * np.pi * i / n_major
        for j in range(n_minor):
            v = 2 * np.pi * j / n_minor
            verts.append(((R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)))
    idx = lambda i, j: (i % n_major) * n_minor + (j % n_minor)
    for i in range(n_major):
        for j in range(n_minor):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1)
            faces += [(a, b, d), (a, d, c)]
    return np.asarray(verts, np.float64), np.asarray(faces, np.int64)
