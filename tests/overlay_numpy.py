"""NumPy restatement of the contact-sheet contract (include/tokenhmr_hip.h: thmr_renderer_sheet): the draw list of
the reference's render_openpose and of visualize_tensorboard's keypoint remap (pinned to the reference by
tests/golden/openpose_calls.json), the stated pixel coverage of a thick line and a circle (cv2's rasteriser is not pinned: the wheel
is absent), the skeleton panel, the hard-mask mesh panel and make_grid's layout.  All coverage arithmetic is exact in int64; every
float is one fp32 rounding per operation, so the device must match bit for bit."""
import numpy as np

RANGE = 16384                       # a primitive with a coordinate beyond +-RANGE after truncation is not drawn (stated deviation)
N_KP, N_BODY, N_REC, N_WORDS = 44, 25, 49, 12
KIND_NONE, KIND_LINE, KIND_CIRCLE = 0, 1, 2

# OpenPose BODY_25 as published (pose/poseParametersRender.hpp): the rendered limbs and the palette
LIMBS = np.array([1, 8, 1, 2, 1, 5, 2, 3, 3, 4, 5, 6, 6, 7, 8, 9, 9, 10, 10, 11, 8, 12, 12, 13, 13, 14, 1, 0, 0, 15, 15, 17, 0, 16, 16, 18,
                  14, 19, 19, 20, 14, 21, 11, 22, 22, 23, 11, 24]).reshape(-1, 2)
PALETTE = np.array([255, 0, 85, 255, 0, 0, 255, 85, 0, 255, 170, 0, 255, 255, 0, 170, 255, 0, 85, 255, 0, 0, 255, 0, 255, 0, 0, 0, 255, 85,
                    0, 255, 170, 0, 255, 255, 0, 170, 255, 0, 85, 255, 0, 0, 255, 255, 0, 170, 170, 0, 255, 255, 0, 255, 85, 0, 255,
                    0, 0, 255, 0, 0, 255, 0, 0, 255, 0, 255, 255, 0, 255, 255, 0, 255, 255], dtype=np.float64).reshape(-1, 3)
# visualize_tensorboard: body keypoint -> the one of the 19 extra keypoints that replaces it
MATCHES = [(1, 12), (2, 8), (3, 7), (4, 6), (5, 9), (6, 10), (7, 11), (8, 14), (9, 2), (10, 1), (11, 0), (12, 3), (13, 4), (14, 5)]


# ------------------------------------------------------------------------------------------------ keypoints -> body skeleton
def body_from_pred(pred, img_res):
    """(44, 2) normalised predicted keypoints -> the (25, 3) float32 body skeleton in pixels, confidence 1, remapped unconditionally."""
    kp = np.concatenate([np.asarray(pred, np.float32), np.ones((N_KP, 1), np.float32)], axis=-1)
    kp = (np.float32(img_res) * (kp + np.float32(0.5))).astype(np.float32)
    for a, b in MATCHES:
        kp[a] = kp[N_BODY + b]
    return kp[:N_BODY].copy()


def body_from_gt(gt, img_res):
    """(44, 3) ground-truth keypoints, changed IN PLACE as the reference changes its caller's array (x, y scaled to pixels, a body
    keypoint of confidence 0 replaced by its extra keypoint of confidence > 0); returns the (25, 3) body skeleton."""
    assert gt.dtype == np.float32 and gt.shape == (N_KP, 3)
    gt[:, :2] = np.float32(img_res) * (gt[:, :2] + np.float32(0.5))
    for a, b in MATCHES:
        if gt[N_BODY + b, 2] > 0 and gt[a, 2] == 0:
            gt[a] = gt[N_BODY + b]
    return gt[:N_BODY].copy()


# ------------------------------------------------------------------------------------------------ the draw list
def _in_range(v):
    return bool(np.isfinite(v) and abs(float(v)) < RANGE + 1)


def build_records(body, width, height):
    """render_keypoints' draw list for one (25, 3) float32 skeleton over a (height, width, 3) image, as the (49, 12) int32 records of
    thmr_renderer_sheet: 24 limbs then 25 joints; {kind, x0, y0, x1, y1, radius, thickness, colour index, box x0, y0, x1, y1}."""
    body = np.asarray(body, np.float32)
    rec = np.zeros((N_REC, N_WORDS), np.int32)
    x, y, c = body[:, 0], body[:, 1], body[:, 2]
    over = c > np.float32(0.1)
    if not over.any():
        return rec
    with np.errstate(invalid="ignore", over="ignore"):
        pw = np.float32(x[over].max() - x[over].min())
        ph = np.float32(y[over].max() - y[over].min())
        area = np.float32(pw * ph)
        if not area > 0:
            return rec
        # the reference reads width, height = img.shape[1], img.shape[2] of an HWC image: its "height" is the 3 channels
        rw, rh = np.float32(pw / np.float32(width)), np.float32(ph / np.float32(3))
    m = rh if rh > rw else rw
    ratio = m if m < 1 else np.float32(1)
    tr = max(np.round(np.sqrt(float(width * 3)) * (1.0 / 75.0) * float(ratio)), 2.0)          # float64, half to even
    t_circle = int(tr if ratio > np.float32(0.05) else 1.0)
    t_line = int(max(1.0, np.round(tr * 0.75)))
    radius = int(np.round(tr / 2))

    def put(slot, kind, x0, y0, x1, y1, r, t, colour, ext):
        rec[slot] = [kind, x0, y0, x1, y1, r, t, colour, max(min(x0, x1) - ext, 0), max(min(y0, y1) - ext, 0),
                     min(max(x0, x1) + ext, width - 1), min(max(y0, y1) + ext, height - 1)]

    for k, (i, j) in enumerate(LIMBS):
        if over[i] and over[j] and all(_in_range(v) for v in (x[i], y[i], x[j], y[j])):
            put(k, KIND_LINE, int(x[i]), int(y[i]), int(x[j]), int(y[j]), 0, t_line, int(j), (t_line + 1) // 2)
    for i in range(N_BODY):
        if over[i] and _in_range(x[i]) and _in_range(y[i]):
            put(24 + i, KIND_CIRCLE, int(x[i]), int(y[i]), int(x[i]), int(y[i]), radius, t_circle, i, radius + (t_circle + 1) // 2)
    return rec


def calls_of(rec):
    """Records -> the cv2 calls they stand for, in draw order, as the fixture lists them."""
    out = []
    for r in rec:
        colour = [float(v) for v in PALETTE[r[7]]]
        if r[0] == KIND_LINE:
            out.append(["line", [int(r[1]), int(r[2])], [int(r[3]), int(r[4])], colour, int(r[6])])
        elif r[0] == KIND_CIRCLE:
            out.append(["circle", [int(r[1]), int(r[2])], int(r[5]), colour, int(r[6])])
    return out


def calls_in_range(calls):
    """The reference's calls without those the contract drops (a coordinate beyond +-RANGE)."""
    keep = []
    for c in calls:
        pts = c[1] + (c[2] if c[0] == "line" else [])
        if all(abs(int(v)) <= RANGE for v in pts):
            keep.append(c)
    return keep


# ------------------------------------------------------------------------------------------------ coverage
def covers(kind, x0, y0, x1, y1, radius, thick, px, py):
    """Is the pixel centred on the integer point (px, py) covered?  px, py int64 arrays; exact.  cross^2 is compared with
    (t^2 |ab|^2) >> 2 instead of 4 cross^2 with t^2 |ab|^2 (the same predicate for integers) so that nothing exceeds int64
    with |coordinates| <= 16384 and pixels below 8192."""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    t = np.int64(thick)
    wx, wy = px - np.int64(x0), py - np.int64(y0)
    d2 = wx * wx + wy * wy
    if kind == KIND_LINE:
        dx, dy = np.int64(x1) - np.int64(x0), np.int64(y1) - np.int64(y0)
        len2, dot = dx * dx + dy * dy, wx * dx + wy * dy
        ux, uy = px - np.int64(x1), py - np.int64(y1)
        cr = wx * dy - wy * dx
        return np.where(dot <= 0, 4 * d2 <= t * t, np.where(dot >= len2, 4 * (ux * ux + uy * uy) <= t * t, cr * cr <= ((t * t * len2) >> 2)))
    r = np.int64(radius)
    if t < 0:
        return d2 <= r * r
    lo, hi = 2 * r - t, 2 * r + t
    return (4 * d2 <= hi * hi) & ((lo <= 0) | (lo * lo <= 4 * d2))


def coverage_map(rec, width, height):
    """(height, width) int: the colour index of the last covering record per pixel, -1 where none covers."""
    out = np.full((height, width), -1, np.int64)
    for r in rec:                                  # painter's order: later records overwrite earlier ones
        if r[0] == KIND_NONE or r[8] > r[10] or r[9] > r[11]:
            continue
        ys, xs = np.mgrid[r[9]:r[11] + 1, r[8]:r[10] + 1]
        hit = covers(int(r[0]), r[1], r[2], r[3], r[4], r[5], r[6], xs, ys)
        out[r[9]:r[11] + 1, r[8]:r[10] + 1][hit] = r[7]
    return out


def prim_record(kind, p0, p1, radius, thick, colour, width, height):
    """One record for a free-standing primitive (the analytic coverage cases)."""
    ext = (thick + 1) // 2 if kind == KIND_LINE else radius + ((thick + 1) // 2 if thick > 0 else 0)
    x0, y0, x1, y1 = p0[0], p0[1], p1[0], p1[1]
    return np.array([kind, x0, y0, x1, y1, radius, thick, colour, max(min(x0, x1) - ext, 0), max(min(y0, y1) - ext, 0),
                     min(max(x0, x1) + ext, width - 1), min(max(y0, y1) + ext, height - 1)], np.int32)


# ------------------------------------------------------------------------------------------------ panels and the grid
def skeleton_panel(image, rec):
    """render_openpose(255 * img) / 255 over a (3, H, W) float32 image: fl(fl(255 x) / 255) where nothing is drawn, colour / 255 else."""
    image = np.asarray(image, np.float32)
    _, H, W = image.shape
    out = ((np.float32(255) * image).astype(np.float32) / np.float32(255)).astype(np.float32)
    idx = coverage_map(rec, W, H)
    colours = (PALETTE.astype(np.float32) / np.float32(255)).astype(np.float32)
    hit = idx >= 0
    for ch in range(3):
        out[ch][hit] = colours[idx[hit], ch]
    return out


def mesh_panel(rgba, background):
    """where(alpha > 0.8, rgb, bg): rgba (H, W, 4), background (3, H, W) or None for ones; returns (3, H, W)."""
    rgba = np.asarray(rgba, np.float32)
    bg = np.ones((3,) + rgba.shape[:2], np.float32) if background is None else np.asarray(background, np.float32)
    return np.where(rgba[None, :, :, 3] > np.float32(0.8), rgba[:, :, :3].transpose(2, 0, 1), bg).astype(np.float32)


def grid_geometry(n, nrow, padding, H, W):
    """make_grid: (canvas height, canvas width, [(row, col) origin of tile k])."""
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    origins = [(padding + (k // xmaps) * (H + padding), padding + (k % xmaps) * (W + padding)) for k in range(n)]
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, origins


def make_grid(tiles, nrow, padding=2):
    tiles = [np.asarray(t, np.float32) for t in tiles]
    _, H, W = tiles[0].shape
    Hg, Wg, origins = grid_geometry(len(tiles), nrow, padding, H, W)
    out = np.zeros((3, Hg, Wg), np.float32)
    for t, (r, c) in zip(tiles, origins):
        out[:, r:r + H, c:c + W] = t
    return out
