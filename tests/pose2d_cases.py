"""Planted scenes for the RGB-only pose route (TEST INFRASTRUCTURE): 64 x 96 frames with the regions and class sizes of
tests/pose3d_cases.py, whose class pixels carry a known rigid pose — and no depth.

Every class pixel has a point on a virtual tilted plane along its own ray (not quantised); an INLIER pixel's object coordinate
is R^T (ray z - t), scaled into `vertex_pred` — exact up to the f32 rounding of the scaling. OUTLIER pixels have that point
moved ACROSS their ray by 5 to 15 cm (a move along the ray would not change where the point projects); EMPTY pixels hold
exactly 0.5 on the three axes, which unscales to the "empty prediction" (0, 0, 0) — the object centre, so pixels within
CLEAR pixels of the centre's projection are never empty.

Scene condition (asserted by `make_frame`): under the planted pose every inlier reprojects within 1e-3 pixel and every
outlier and every empty pixel at >= 3 x INLIER_THRESHOLD.

Classes (C = 7): 1: 2500 pixels, 2: 900, 3: 401 (just live), 4: 400 (not live: the test is `> min_area`), 5: 448 pixels that
are all empty (live, but no hypothesis can be drawn), 6: absent. A few background pixels carry labels outside [0, C)."""
import numpy as np

import pose3d_cases as C3

F, D = np.float32, np.float64
H, W, C = C3.H, C3.W, C3.C
EXTENT = C3.EXTENT
SIZES, LIVE, POSED, INTRINSICS = C3.SIZES, C3.LIVE, C3.POSED, C3.INTRINSICS
INLIER_THRESHOLD, MIN_DIST2D = 1.0, 3.0
PARAMS = dict(inlier_threshold=INLIER_THRESHOLD, min_dist2d=MIN_DIST2D)
CLEAR = 6.0
box_corners, corner_displacement = C3.box_corners, C3.corner_displacement


def project(R, t, obj, K):
    q = obj @ R.T + t
    return np.stack([K[0] * q[..., 0] / q[..., 2] + K[2], K[1] * q[..., 1] / q[..., 2] + K[3]], axis=-1)


def make_frame(seed, K=INTRINSICS[0]):
    """-> dict(label, vertex_pred, extents, K, poses {c: (R, t)}, inlier {c: bool over the class's records in raster order},
    kind [H,W] 0 inlier / 1 outlier / 3 empty)"""
    rng = np.random.RandomState(seed)
    label = C3._regions()
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    ray = np.stack([(x - K[2]) / K[0], (y - K[3]) / K[1], np.ones((H, W))], axis=-1)
    eye = ray * (0.8 + 0.0006 * x + 0.0004 * y)[..., None]
    kind = np.zeros((H, W), np.int8)
    u = rng.uniform(size=(H, W))
    kind[u < 0.20] = 1
    kind[(u >= 0.20) & (u < 0.22)] = 3
    extents = np.zeros((C, 3), F)
    extents[1:] = EXTENT
    a, b = F(1.0 / D(F(EXTENT))), F(0.5)
    vertex = rng.uniform(size=(H, W, 3 * C)).astype(F)
    pix = np.stack([x, y], axis=-1).astype(D)
    poses, inlier = {}, {}
    for c in range(1, C):
        m = label == c
        if not m.any():
            continue
        R, t = C3._rotation(rng), eye[m].mean(axis=0) + np.array([0.0, 0.0, 0.1])
        off = rng.normal(size=(H, W, 3))
        unit = ray / np.linalg.norm(ray, axis=-1, keepdims=True)
        off -= (off * unit).sum(axis=-1, keepdims=True) * unit                 # across the ray
        off *= (rng.uniform(0.05, 0.15, size=(H, W)) / np.linalg.norm(off, axis=-1))[..., None]
        k = kind.copy()
        if c == 5:
            k[m] = 3
        else:
            centre = project(R, t, np.zeros(3), K)
            k[(k == 3) & (np.linalg.norm(pix - centre, axis=-1) < CLEAR)] = 0
        obj = (np.where((k == 1)[..., None], eye + off, eye) - t) @ R           # rows: R^T (point - t)
        v = (obj.astype(F) * a + b).astype(F)
        v[k == 3] = b
        vertex[m, 3 * c:3 * c + 3] = v[m]
        kind[m] = k[m]
        poses[c] = (R, t)
        inlier[c] = (k[m] == 0)
        if c in POSED:                                                          # the scene condition, on what the route reads
            o = ((vertex[m, 3 * c:3 * c + 3] - b) / a).astype(D)
            d = np.linalg.norm(project(R, t, o, K) - pix[m], axis=-1)
            assert d[inlier[c]].max() < 1e-3 and d[~inlier[c]].min() >= 3 * INLIER_THRESHOLD, (c, d[inlier[c]].max(), d[~inlier[c]].min())
    return dict(label=label, vertex_pred=vertex, extents=extents, K=tuple(K), poses=poses, inlier=inlier, kind=kind)


def batch(seeds, intrinsics):
    """frames stacked for ops.estimate_poses_2d: (label [B,H,W], vertex_pred, extents, K [B,4], frames)"""
    frames = [make_frame(s, k) for s, k in zip(seeds, intrinsics)]
    return (np.stack([f["label"] for f in frames]), np.stack([f["vertex_pred"] for f in frames]), frames[0]["extents"],
            np.array([f["K"] for f in frames], dtype=F), frames)


# ---- a reprojection distance exactly at the threshold -----------------------------------------------------------------------
THRESHOLD = 1.25
THRESHOLD_POSE = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 2.0])
THRESHOLD_K = (1.0, 1.0, 0.0, 0.0)


def threshold_frame():
    """An 8 x 8 frame, C = 2, whose arithmetic is exact: fx = fy = 1, px = py = 0, extent 1 (obj = v - 0.5 without rounding),
    the pose R = I, t = (0, 0, 2). Class 1 has four pixels: (1,1), (2,4), (6,2) with obj = (2 x, 2 y, 0) — q.z = 2, they
    reproject exactly onto themselves, so a Gauss-Newton increment over them is exactly zero —, and pixel (4,3) with
    obj = (9.5, 8, 0), which reprojects at (4.75, 4): offsets (0.75, 1.0), distance sqrt(0.5625 + 1) = 1.25, EXACTLY the
    threshold. With `<` the pose has 3 inliers and is not refitted; with `<=` it has 4, is refitted and moves.
    -> dict(label, vertex_pred, extents, K)"""
    label = np.zeros((8, 8), np.int32)
    vertex = np.full((8, 8, 6), 0.25, F)
    for x, y in ((1, 1), (2, 4), (6, 2)):
        label[y, x] = 1
        vertex[y, x, 3:] = (2 * x + 0.5, 2 * y + 0.5, 0.5)
    label[3, 4] = 1
    vertex[3, 4, 3:] = (10.0, 8.5, 0.5)
    extents = np.array([[0, 0, 0], [1, 1, 1]], F)
    return dict(label=label, vertex_pred=vertex, extents=extents, K=THRESHOLD_K)
