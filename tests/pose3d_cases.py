"""Planted scenes for the 3-D pose route (TEST INFRASTRUCTURE): 64 x 96 frames whose class regions carry a known rigid pose.

Every class pixel has a depth on a tilted plane, quantised to uint16 at factor 10000; an INLIER pixel's object coordinate is
R^T (eye - t) of its own (quantised) camera point, scaled into `vertex_pred` — exact up to the f32 rounding of the scaling,
about 1e-7 m. OUTLIER pixels have their object point moved by 5 to 15 cm; HOLES have depth 0; EMPTY pixels hold exactly 0.5
on the three axes, which unscales to the reference's "empty prediction" (0, 0, 0). The object centre lies 10 cm behind the
plane, so an empty pixel is itself at least 10 cm off under the planted pose.

Classes (C = 7): 1: 2500 pixels (above two batches of 1000), 2: 900 (below one batch), 3: 401 (just live), 4: 400 (not live:
the test is `> min_area`), 5: 448 pixels that are all holes (live, but no hypothesis can be drawn), 6: absent.
A few background pixels carry labels outside [0, C)."""
import numpy as np

F, D = np.float32, np.float64
H, W, C = 64, 96, 7
FACTOR = 10000.0
EXTENT = 0.3
SIZES = {1: 2500, 2: 900, 3: 401, 4: 400, 5: 448, 6: 0}
LIVE = (1, 2, 3, 5)
POSED = (1, 2, 3)
INTRINSICS = ((120.0, 118.0, 48.0, 32.0), (131.5, 127.25, 45.5, 30.25), (110.0, 112.0, 50.0, 33.5))


def _regions():
    lab = np.zeros((H, W), np.int32)
    lab[0:50, 0:50] = 1
    lab[0:30, 52:82] = 2
    lab[32:52, 52:72] = 3
    lab[32, 72] = 3
    lab[32:52, 75:95] = 4
    lab[50:64, 0:32] = 5
    lab[60, 90], lab[61, 91], lab[62, 92], lab[63, 93] = 7, 99, -1, -5
    return lab


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def eye_points(depth, K):
    """the header's f32 camera points of a whole frame: [H,W,3]"""
    fx, fy, px, py = (F(v) for v in K)
    d = depth.astype(F)
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    e = np.stack([(x - px) * d / fx / F(FACTOR), (y - py) * d / fy / F(FACTOR), d / F(FACTOR)], axis=-1).astype(F)
    e[depth == 0] = 0
    return e


def make_frame(seed, K=INTRINSICS[0]):
    """-> dict(label, depth, vertex_pred, extents, K, factor, poses {c: (R, t)}, inlier {c: bool over the class's records in
    raster order}, kind [H,W] 0 inlier / 1 outlier / 2 hole / 3 empty)"""
    rng = np.random.RandomState(seed)
    label = _regions()
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    depth = np.rint((0.8 + 0.0006 * x + 0.0004 * y) * FACTOR).astype(np.uint16)
    kind = np.zeros((H, W), np.int8)
    u = rng.uniform(size=(H, W))
    kind[u < 0.20] = 1
    kind[(u >= 0.20) & (u < 0.25)] = 2
    kind[(u >= 0.25) & (u < 0.27)] = 3
    kind[label == 5] = 2
    depth[kind == 2] = 0
    eye = eye_points(depth, K).astype(D)
    extents = np.zeros((C, 3), F)
    extents[1:] = EXTENT
    a, b = F(1.0 / D(F(EXTENT))), F(0.5)
    vertex = rng.uniform(size=(H, W, 3 * C)).astype(F)
    poses, inlier = {}, {}
    for c in range(1, C):
        m = label == c
        if not m.any():
            continue
        centre = eye[m & (depth > 0)].mean(axis=0) if (m & (depth > 0)).any() else np.array([0.0, 0.0, 0.9])
        R, t = _rotation(rng), centre + np.array([0.0, 0.0, 0.1])
        obj = (eye - t) @ R                                    # rows: R^T (eye - t)
        off = rng.normal(size=(H, W, 3))
        off *= (rng.uniform(0.05, 0.15, size=(H, W)) / np.linalg.norm(off, axis=-1))[..., None]
        obj = np.where((kind == 1)[..., None], obj + off, obj)
        v = (obj.astype(F) * a + b).astype(F)
        v[kind == 3] = b
        vertex[m, 3 * c:3 * c + 3] = v[m]
        poses[c] = (R, t)
        inlier[c] = (kind[m] == 0)
    return dict(label=label, depth=depth, vertex_pred=vertex, extents=extents, K=tuple(K), factor=FACTOR, poses=poses,
                inlier=inlier, kind=kind)


def box_corners(extent):
    h = np.asarray(extent, dtype=D) * 0.5
    return np.array([[sx * h[0], sy * h[1], sz * h[2]] for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)])


def corner_displacement(P, R, t, extent):
    """the largest distance between a box corner under P (12 or 3 x 4) and under the planted (R, t)"""
    P = np.asarray(P, dtype=D).reshape(3, 4)
    c = box_corners(extent)
    return float(np.linalg.norm((c @ P[:, :3].T + P[:, 3]) - (c @ R.T + t), axis=1).max())


def batch(seeds, intrinsics):
    """frames stacked for ops.estimate_poses_3d: (label [B,H,W], depth, vertex_pred, extents, K [B,4], frames)"""
    frames = [make_frame(s, k) for s, k in zip(seeds, intrinsics)]
    return (np.stack([f["label"] for f in frames]), np.stack([f["depth"] for f in frames]),
            np.stack([f["vertex_pred"] for f in frames]), frames[0]["extents"], np.array([f["K"] for f in frames], dtype=F), frames)


# ---- a residual exactly at the threshold ------------------------------------------------------------------------------------
THRESHOLD = dict(inlier_threshold=0.25, min_dist=0.01, min_area=0, hypotheses=13)


def threshold_frame():
    """An 8 x 8 frame, C = 2, whose arithmetic is exact: fx = fy = 1, px = py = 0, factor 4, extent 1, so that
    eye = (x d / 4, y d / 4, d / 4) and obj = v - 0.5 without rounding. Class 1 has four pixels: (1,1), (2,4), (3,1) at d = 8
    with obj = eye - (0, 0, 2) — coordinate sums divisible by 3, so every three-point fit is exactly R = I, t = (0, 0, 2)
    whatever the order —, and pixel (0,0) at d = 9 with the empty prediction (obj = 0, never sampled, but counted): its
    residual under that pose is |2.25 - 2| = 0.25, EXACTLY the inlier threshold of THRESHOLD. With `<` the pose has 3
    inliers in every round (never refitted, ref_steps still reaches ref_it); with `<=` it has 4 and is refitted.
    -> dict(label, depth, vertex_pred, extents, K, factor)"""
    label = np.zeros((8, 8), np.int32)
    depth = np.full((8, 8), 8, np.uint16)
    vertex = np.full((8, 8, 6), 0.25, F)
    for x, y in ((1, 1), (2, 4), (3, 1)):
        label[y, x] = 1
        vertex[y, x, 3:] = (2 * x + 0.5, 2 * y + 0.5, 0.5)
    label[0, 0], depth[0, 0] = 1, 9
    vertex[0, 0, 3:] = 0.5
    extents = np.array([[0, 0, 0], [1, 1, 1]], F)
    return dict(label=label, depth=depth, vertex_pred=vertex, extents=extents, K=(1.0, 1.0, 0.0, 0.0), factor=4.0)


THRESHOLD_POSE = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 2.0])
