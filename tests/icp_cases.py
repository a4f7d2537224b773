"""Edge cases of the pose-refinement kernels (posecnn_amd/csrc/icp.hip): gates, degenerate systems and block boundaries.
Shared by tests/test_icp_edges_cpu.py (needs no GPU: the oracle against the expectations below, the constants, the regimes)
and tests/test_gpu_icp_edges.py (the library against the oracle, bit for bit, and against the same expectations).

Every case builds its inputs directly as arrays (no rendered scene), records the regime it claims, and carries an expectation
derived BY CONSTRUCTION — independent of the library and of oracle/:
  - integer counts and masks come from the flags the builder starts from (the arrays are made from the flags, never the
    flags from the arrays), or are stated literally in the case table;
  - sums, normal equations (numpy.linalg.lstsq) and energies are float64 numpy over the float32 inputs.

BOUNDS holds, per float64 comparison, the distance measured on the CPU between the ORACLE and the float64 value and the
bound asserted (4 x that distance; the margin covers nothing more than the case list growing). No bound comes from the
GPU's output: the library has to equal the oracle bit for bit anyway.
"""
import functools
import os
import re

import numpy as np

F = np.float32
D = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICP_HIP = os.path.join(ROOT, "posecnn_amd", "csrc", "icp.hip")

# ---- the constants restated (tests/test_icp_edges_cpu.py reads their values out of icp.hip) ---------------------------
ICP_BLOCK = 256          # pixels per workgroup of the terms / centre kernels = one partial row
ICP_NSEG = 8             # segments of the f64 sum of the partial rows
NM_LANES = 1024          # threads of the polish workgroup = stride of a thread's walk through the label's box
ICP_CH = 8               # candidates of a window row fetched per trip of the score scan
BACKPROJECT_GRID_CAP = 4096   # workgroups of icp_backproject_kernel at most: a second grid-stride trip above 4096 * 256 pixels
CONSTANTS = {"ICP_BLOCK": ICP_BLOCK, "ICP_NSEG": ICP_NSEG, "NM_LANES": NM_LANES, "ICP_CH": ICP_CH}


def parse_backproject_grid_cap(path=ICP_HIP):
    """the literal cap of `std::min<long long>((P + 255) / 256, CAP)` in pcnn_icp_backproject_fwd"""
    with open(path) as fh:
        text = fh.read()
    body = text[text.index("pcnn_icp_backproject_fwd"):]
    m = re.search(r"std::min<long long>\(\(P \+ 255\) / 256,\s*(\d+)\)", body)
    return int(m.group(1)) if m else None


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def intrinsics(fx, fy, px, py):
    return np.array([[fx, 0, px], [0, fy, py], [0, 0, 1]], D)


def nblocks(H, W):
    return (H * W + ICP_BLOCK - 1) // ICP_BLOCK


def segment_length(nb):
    return (nb + ICP_NSEG - 1) // ICP_NSEG


def pad4(a, fill=1.0):
    return np.concatenate([a, np.full(a.shape[:-1] + (1,), fill, F)], axis=-1)


# =====================================================================================================================
# measured |oracle - float64| per comparison and the bound asserted (= 4 x measured), filled from
# `python tests/icp_cases.py` (which prints this table from the oracle on the CPU)
BOUNDS = {
    # refine, first iteration: relative distance of sum r^2, max abs distance of the 3x4 update
    "refine/16x16": {"sum_r2": (5.3e-08, 2.12e-07), "update": (9.9e-07, 3.96e-06)},
    "refine/16x17": {"sum_r2": (7.7e-08, 3.08e-07), "update": (1.3e-06, 5.2e-06)},
    "refine/28x64": {"sum_r2": (4.3e-08, 1.72e-07), "update": (5.1e-07, 2.04e-06)},
    "refine/32x64": {"sum_r2": (3.2e-08, 1.28e-07), "update": (3.8e-07, 1.52e-06)},
    "refine/33x64": {"sum_r2": (4.4e-08, 1.76e-07), "update": (9.4e-07, 3.76e-06)},
    "refine/126x128": {"sum_r2": (3.8e-08, 1.52e-07), "update": (1.6e-08, 6.4e-08)},
    "refine/128x128": {"sum_r2": (2.5e-08, 1e-07), "update": (1.5e-08, 6e-08)},
    "refine/129x128": {"sum_r2": (6.1e-08, 2.44e-07), "update": (5.1e-08, 2.04e-07)},
    # degenerate systems: max abs distance of the 3x4 update from exp(float64 solution of the reduced system)
    "degenerate/single-inlier": {"update": (0, 0)},
    "degenerate/plane": {"update": (1.1e-09, 4.4e-09)},
    # centre: max abs distance of the three coordinate sums
    "center/P1": {"sums": (1.9e-08, 7.6e-08)},
    "center/P255": {"sums": (2.8e-06, 1.12e-05)},
    "center/P256": {"sums": (1.6e-05, 6.4e-05)},
    "center/P257": {"sums": (7.6e-06, 3.04e-05)},
    "center/P2049": {"sums": (1.5e-05, 6e-05)},
    # polish at a budget of 8: abs distance of the returned energy from the float64 minimum over the initial simplex
    "polish/w1023": {"energy": (1.3e-10, 5.2e-10)},
    "polish/w1024": {"energy": (1.9e-10, 7.6e-10)},
    "polish/w1025": {"energy": (2.6e-10, 1.04e-09)},
    "polish/one-pixel-first": {"energy": (1.7e-10, 6.8e-10)},
    "polish/one-pixel-last": {"energy": (6.3e-12, 2.52e-11)},
    "polish/no-valid": {"energy": (0, 0)},
    "polish/nan-background": {"energy": (2e-11, 8e-11)},
}


def bound(case_id, what):
    return BOUNDS[case_id][what][1]


# =====================================================================================================================
# 1. backproject
BACKPROJECT_K = intrinsics(1066.778, 1067.487, 312.9869, 241.3109)
BACKPROJECT_FACTOR = 10000.0          # not a power of two: the division rounds
BACKPROJECT_CASES = [
    dict(id="1025x1024-label", H=1025, W=1024, masked=True, trips=2),
    dict(id="1025x1024-nolabel", H=1025, W=1024, masked=False, trips=2),
    dict(id="1x1-label-65535", H=1, W=1, masked=True, trips=1, depth=65535),
    dict(id="1x1-nolabel-0", H=1, W=1, masked=False, trips=1, depth=0),
]
BACKPROJECT_OBJ = 3


def backproject_trips(H, W):
    """trips of the grid-stride loop the busiest thread takes"""
    grid = min((H * W + 255) // 256, BACKPROJECT_GRID_CAP)
    return -(-(H * W) // (grid * 256))


@functools.lru_cache(maxsize=None)
def _backproject_frame(H, W):
    rng = np.random.default_rng(1025)
    depth = rng.integers(0, 65536, (H, W), dtype=np.int64).astype(np.uint16)
    label = rng.choice(np.array([0, BACKPROJECT_OBJ, 5], np.int32), (H, W))
    if H * W >= 4:     # the extreme readings in the first trip and in the last block of the second, all on the object
        depth.flat[0], depth.flat[1], depth.flat[-1], depth.flat[-2] = 0, 65535, 65535, 0
        for i in (0, 1, -1, -2):
            label.flat[i] = BACKPROJECT_OBJ
    return depth, label


def backproject_inputs(case):
    """-> depth uint16 [H,W], label int32 [H,W] or None"""
    if "depth" in case:
        depth = np.full((case["H"], case["W"]), case["depth"], np.uint16)
        label = np.full((case["H"], case["W"]), BACKPROJECT_OBJ, np.int32)
    else:
        depth, label = _backproject_frame(case["H"], case["W"])
    return depth, (label if case["masked"] else None)


def backproject_expected(case):
    """the three expressions in numpy float32 (each operation correctly rounded, no contraction)"""
    depth, label = backproject_inputs(case)
    H, W = depth.shape
    K = BACKPROJECT_K
    fx, fy, px, py = F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])
    d = depth.astype(F) / F(BACKPROJECT_FACTOR)
    if label is not None:
        d = np.where(label == BACKPROJECT_OBJ, d, F(0))
    x = np.arange(W, dtype=F)[None, :]
    y = np.arange(H, dtype=F)[:, None]
    out = np.empty((H, W, 3), F)
    out[..., 0] = (x - px) / fx * d
    out[..., 1] = (y - py) / fy * d
    out[..., 2] = d
    return out


# =====================================================================================================================
# 2. the six gates of icp_terms_kernel: one planted pixel per gate side, each its own object of ONE call
GATE_H, GATE_W = 24, 32
GATE_K = intrinsics(64.0, 64.0, 16.0, 12.0)       # powers of two and integers: projections are exact
GATE_RANGE = (0.25, 6.0)
GATE_MAX_ERROR = 2.0 ** -7
_NAN = float("nan")


def _axis(z):
    return (0.0, 0.0, z)


def _col(proj):     # a predicted vertex at depth 1 that projects to column `proj`, row 12
    return ((proj - 16.0) / 64.0, 0.0, 1.0)


def _row(proj):
    return (0.0, (proj - 12.0) / 64.0, 1.0)


_DOWN = (0.0, 0.0, -1.0)
# id, the gate (line of the reference's icp.cu the kernel cites), quantity planted, its value, the threshold it sits at or
# one ulp beside, inlier expected (the side the reference's test puts the value on), predicted vertex, normal, live pixel
# (v, u) and live vertex. Every other gate of a planted pixel passes with room to spare, so a gate that moved shows as 0 <-> 1.
GATE_ROWS = [
    # icp.cu:60  `if (predDepth < near || predDepth > far) return` — equality and NaN pass
    ("pvz=znear", ":60", "pvz", F(0.25), F(0.25), 1, _axis(0.25), _DOWN, (12, 16), _axis(0.25)),
    ("pvz=znear-ulp", ":60", "pvz", down(0.25), F(0.25), 0, _axis(down(0.25)), _DOWN, (12, 16), _axis(0.25)),
    ("pvz=zfar", ":60", "pvz", F(6.0), F(6.0), 1, _axis(6.0), _DOWN, (12, 16), _axis(6.0)),
    ("pvz=zfar+ulp", ":60", "pvz", up(6.0), F(6.0), 0, _axis(up(6.0)), _DOWN, (12, 16), _axis(6.0)),
    # a NaN passes :60 and dies at the border test: (int)(NaN + 0.5) is 0 on the device
    ("pvz=nan", ":60/:81", "pvz", F(_NAN), F(_NAN), 0, _axis(_NAN), _DOWN, (12, 16), _axis(1.0)),
    # icp.cu:78-81  u = (int)(proj + 0.5); `if (u <= border || u >= W - 1 - border ...) return`, border = 2:
    # proj = k + 0.5 lands on k + 1 (truncation after + 0.5, not round-to-even); 2 and W - 3 are out, 3 and W - 4 are in
    ("u=2", ":81", "projx", F(1.5), F(1.5), 0, _col(1.5), _DOWN, (12, 2), _col(1.5)),
    ("u=3", ":81", "projx", F(2.5), F(2.5), 1, _col(2.5), _DOWN, (12, 3), _col(2.5)),
    ("u=W-4", ":81", "projx", F(27.5), F(27.5), 1, _col(27.5), _DOWN, (12, 28), _col(27.5)),
    ("u=W-3", ":81", "projx", F(28.5), F(28.5), 0, _col(28.5), _DOWN, (12, 29), _col(28.5)),
    ("v=2", ":81", "projy", F(1.5), F(1.5), 0, _row(1.5), _DOWN, (2, 16), _row(1.5)),
    ("v=3", ":81", "projy", F(2.5), F(2.5), 1, _row(2.5), _DOWN, (3, 16), _row(2.5)),
    ("v=H-4", ":81", "projy", F(19.5), F(19.5), 1, _row(19.5), _DOWN, (20, 16), _row(19.5)),
    ("v=H-3", ":81", "projy", F(20.5), F(20.5), 0, _row(20.5), _DOWN, (21, 16), _row(20.5)),
    # icp.cu:92  `if (liveDepth < near || liveDepth > far) return` — equality passes. The depth-0 pixel is seen along an
    # oblique ray with the normal (-1, 0, 0), so its residual n . (live - pred) is 0 whatever the live depth: only :92 stops it
    ("live=0", ":92", "ldepth", F(0.0), F(0.25), 0, (0.1875, 0.0, 1.0), (-1.0, 0.0, 0.0), (12, 28), (0.1875, 0.0, 0.0)),
    ("live=znear", ":92", "ldepth", F(0.25), F(0.25), 1, _axis(0.25 + 2.0 ** -8), _DOWN, (12, 16), _axis(0.25)),
    ("live=znear-ulp", ":92", "ldepth", down(0.25), F(0.25), 0, _axis(0.25), _DOWN, (12, 16), _axis(down(0.25))),
    ("live=zfar", ":92", "ldepth", F(6.0), F(6.0), 1, _axis(6.0 - 2.0 ** -8), _DOWN, (12, 16), _axis(6.0)),
    ("live=zfar+ulp", ":92", "ldepth", up(6.0), F(6.0), 0, _axis(6.0), _DOWN, (12, 16), _axis(up(6.0))),
    # icp.cu:104  `if (-ray.dot(normal) < 0.1f) return` — equality passes. On the axis at depth 1 the ray is (0, 0, 1) exactly
    ("nz=-0.1f", ":104", "negdot", F(0.1), F(0.1), 1, _axis(1.0), (0.0, 0.0, F(-0.1)), (12, 16), _axis(1.0)),
    ("nz=-0.1f+ulp", ":104", "negdot", down(0.1), F(0.1), 0, _axis(1.0), (0.0, 0.0, -down(0.1)), (12, 16), _axis(1.0)),
    # icp.cu:115  `if (fabsf(error) > maxError) return` — equality passes (the centre kernel's test is the strict one)
    ("err=max", ":115", "abserr", F(2.0 ** -7), F(2.0 ** -7), 1, _axis(1.0), _DOWN, (12, 16), _axis(1.0 - 2.0 ** -7)),
    ("err=max+ulp", ":115", "abserr", up(2.0 ** -7), F(2.0 ** -7), 0, _axis(1.0), (0.0, 0.0, -up(1.0)), (12, 16), _axis(1.0 - 2.0 ** -7)),
    # nothing planted at all
    ("empty", "-", None, None, None, 0, None, None, None, None),
]
GATE_IDS = [r[0] for r in GATE_ROWS]
GATE_EXPECT = np.array([r[5] for r in GATE_ROWS], np.int64)


def gate_pixel(n):
    """where object n's predicted vertex sits in its map: spread over the three blocks of the 768 pixels"""
    return (n * 101 + 7) % (GATE_H * GATE_W)


@functools.lru_cache(maxsize=None)
def gate_inputs():
    """-> live [N,H,W,3], pred_v [N,H,W,3], pred_n [N,H,W,3]; everything but the planted pixels is zero (predicted depth 0
    fails :60, live depth 0 fails :92)"""
    N = len(GATE_ROWS)
    live = np.zeros((N, GATE_H, GATE_W, 3), F)
    pv = np.zeros((N, GATE_H * GATE_W, 3), F)
    pn = np.zeros((N, GATE_H * GATE_W, 3), F)
    for n, row in enumerate(GATE_ROWS):
        if row[6] is None:
            continue
        pv[n, gate_pixel(n)] = row[6]
        pn[n, gate_pixel(n)] = row[7]
        live[n, row[8][0], row[8][1]] = row[9]
    return live, pv.reshape(N, GATE_H, GATE_W, 3), pn.reshape(N, GATE_H, GATE_W, 3)


def gate_quantities(n):
    """the six compared quantities of object n's planted pixel at the identity pose, in float32 numpy with the kernel's
    expression order (the identity leaves the vertex unchanged bit for bit)"""
    live, pv, pn = gate_inputs()
    row = GATE_ROWS[n]
    x, y, z = pv[n].reshape(-1, 3)[gate_pixel(n)]
    nx, ny, nz = pn[n].reshape(-1, 3)[gate_pixel(n)]
    K = GATE_K
    with np.errstate(all="ignore"):
        projx = (x / z) * F(K[0, 0]) + F(K[0, 2])
        projy = (y / z) * F(K[1, 1]) + F(K[1, 2])
        lx, ly, lz = live[n, row[8][0], row[8][1]]
        nrm = np.sqrt(x * x + (y * y + z * z))
        rx, ry, rz = x / nrm, y / nrm, z / nrm
        negdot = -(rx * nx + (ry * ny + rz * nz))
        err = nx * (lx - x) + (ny * (ly - y) + nz * (lz - z))
    return dict(pvz=z, projx=projx, projy=projy, ldepth=lz, negdot=negdot, abserr=np.abs(err))


IDENTITY34 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], D)


# =====================================================================================================================
# float64 statement of one Gauss-Newton step of df::icp at the identity pose
def se3_exp(x):
    """Sophus::SE3::exp in float64: x = (upsilon, omega) -> 3x4"""
    x = np.asarray(x, D)
    w = x[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 0.1:      # series: no cancellation in (th - sin th) / th^3
        A = 1 - th2 / 6 + th2 ** 2 / 120 - th2 ** 3 / 5040 + th2 ** 4 / 362880
        B = 0.5 - th2 / 24 + th2 ** 2 / 720 - th2 ** 3 / 40320 + th2 ** 4 / 3628800
        C = 1.0 / 6 - th2 / 120 + th2 ** 2 / 5040 - th2 ** 3 / 362880 + th2 ** 4 / 39916800
    else:
        A, B, C = np.sin(th) / th, (1 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    Wm = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], D)
    out = np.zeros((3, 4), D)
    out[:, :3] = np.eye(3) + A * Wm + B * (Wm @ Wm)
    out[:, 3] = (np.eye(3) + B * Wm + C * (Wm @ Wm)) @ x[:3]
    return out


def refine_f64(live, pv, pn, K, depth_range, max_error, columns=None):
    """live [H,W,3], pv / pn [H,W,3|4] (float32 data) -> dict: inlier mask, count, sum r^2, the solution of the normal
    equations (numpy.linalg.lstsq of the weighted Jacobian rows; over `columns` only for a rank-deficient system, the other
    variables 0), exp(solution), and per gate the smallest relative distance of any pixel that reaches it from its threshold"""
    H, W = live.shape[:2]
    fx, fy, px, py = D(F(K[0, 0])), D(F(K[1, 1])), D(F(K[0, 2])), D(F(K[1, 2]))
    znear, zfar, me = D(F(depth_range[0])), D(F(depth_range[1])), D(F(max_error))
    v = pv[..., :3].astype(D).reshape(-1, 3)
    n = pn[..., :3].astype(D).reshape(-1, 3)
    margins = {}
    with np.errstate(all="ignore"):
        z = v[:, 2]
        margins["pvz"] = float(np.min(np.minimum(np.abs(z - znear) / znear, np.abs(z - zfar) / zfar)))
        ok = ~((z < znear) | (z > zfar))
        idx = np.flatnonzero(ok)
        v, n = v[idx], n[idx]
        tx, ty = v[:, 0] / v[:, 2] * fx + px + 0.5, v[:, 1] / v[:, 2] * fy + py + 0.5
        margins["proj"] = float(np.min(np.minimum(np.abs(tx - np.rint(tx)), np.abs(ty - np.rint(ty)))))   # in pixels
        u, w = np.trunc(tx).astype(np.int64), np.trunc(ty).astype(np.int64)
        ok = ~((u <= 2) | (u >= W - 3) | (w <= 2) | (w >= H - 3))
        idx, v, n, u, w = idx[ok], v[ok], n[ok], u[ok], w[ok]
        lv = live.astype(D)[w, u]
        lz = lv[:, 2]
        margins["ldepth"] = float(np.min(np.minimum(np.abs(lz - znear) / znear, np.abs(lz - zfar) / zfar)))
        ok = ~((lz < znear) | (lz > zfar))
        idx, v, n, lv = idx[ok], v[ok], n[ok], lv[ok]
        ray = v / np.linalg.norm(v, axis=1, keepdims=True)
        negdot = -np.sum(ray * n, axis=1)
        margins["negdot"] = float(np.min(np.abs(negdot - D(F(0.1))) / 0.1))
        ok = ~(negdot < D(F(0.1)))
        idx, v, n, lv = idx[ok], v[ok], n[ok], lv[ok]
        err = np.sum(n * (lv - v), axis=1)
        margins["abserr"] = float(np.min(np.abs(np.abs(err) - me) / me))
        ok = ~(np.abs(err) > me)
        idx, v, n, lv, err = idx[ok], v[ok], n[ok], lv[ok], err[ok]
    wgt = 1.0 / lv[:, 2]
    J = wgt[:, None] * np.concatenate([n, np.cross(v, n)], axis=1)
    r = wgt * err
    cols = list(range(6)) if columns is None else list(columns)
    x = np.zeros(6, D)
    if len(idx):
        x[cols] = np.linalg.lstsq(J[:, cols], r, rcond=None)[0]
    inl = np.zeros(H * W, bool)
    inl[idx] = True
    return dict(inliers=inl.reshape(H, W), count=int(len(idx)), sum_r2=float(r @ r), x=x, update=se3_exp(x), margins=margins)


# =====================================================================================================================
# 3. the reduction: dense noisy surfaces, block counts around ICP_NSEG and around 8 * ICP_NSEG
REDUCTION_SHAPES = [(16, 16), (16, 17), (28, 64), (32, 64), (33, 64), (126, 128), (128, 128), (129, 128)]
# nblocks and L = ceil(nblocks / ICP_NSEG) each shape claims: empty segments below 8 blocks, no tail at L = 8, a tail of one row at L = 9
REDUCTION_CLAIMS = {(16, 16): (1, 1), (16, 17): (2, 1), (28, 64): (7, 1), (32, 64): (8, 1), (33, 64): (9, 2),
                    (126, 128): (63, 8), (128, 128): (64, 8), (129, 128): (65, 9)}
REDUCTION_N = 3
REDUCTION_RANGE = (0.25, 6.0)
REDUCTION_MAX_ERROR = 0.01


def reduction_id(H, W):
    return "refine/%dx%d" % (H, W)


def reduction_K(H, W):
    return intrinsics(float(W), float(W), (W - 1) / 2.0, (H - 1) / 2.0)


def _surface(H, W, K, coef):
    """a quadric depth map over the pixel rays (no symmetry: all six directions constrained): points and unit normals, f64"""
    z0, a, b, c, d, e = coef
    s = ((np.arange(W, dtype=D) - K[0, 2]) / K[0, 0])[None, :] + np.zeros((H, 1))
    t = ((np.arange(H, dtype=D) - K[1, 2]) / K[1, 1])[:, None] + np.zeros((1, W))
    z = z0 + a * s * s + b * t * t + c * s * t + d * s + e * t
    zs, zt = 2 * a * s + c * t + d, 2 * b * t + c * s + e
    Ps = np.stack([z + s * zs, t * zs, zs], -1)
    Pt = np.stack([s * zt, z + t * zt, zt], -1)
    nrm = np.cross(Ps, Pt)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    nrm[nrm[..., 2] > 0] *= -1
    return s, t, z, nrm


@functools.lru_cache(maxsize=None)
def reduction_inputs(H, W):
    """-> live [3,H,W,3], pred_v [3,H,W,3], pred_n [3,H,W,3]: per object a quadric seen along the pixel rays, the live depth
    a few millimetres off it (smooth offset + noise), 2 % clear outliers (5 cm off) and 2 % holes (depth 0)"""
    K = reduction_K(H, W)
    rng = np.random.default_rng(1000 * H + W)
    lives, pvs, pns = [], [], []
    for k in range(REDUCTION_N):
        coef = (0.8 + 0.1 * k, 0.6 - 0.2 * k, -0.4 + 0.3 * k, 0.3, 0.1 * (k - 1), -0.15)
        s, t, z, nrm = _surface(H, W, K, coef)
        dz = 0.002 + 0.004 * s - 0.003 * t + 0.002 * s * t + rng.uniform(-0.0012, 0.0012, (H, W))
        kind = rng.random((H, W))
        dz = np.where(kind < 0.02, 0.05, dz)
        zl = np.where(kind > 0.98, 0.0, z + dz)
        lives.append(np.stack([s * zl, t * zl, zl], -1).astype(F))
        pvs.append(np.stack([s * z, t * z, z], -1).astype(F))
        pns.append(nrm.astype(F))
    return np.stack(lives), np.stack(pvs), np.stack(pns)


@functools.lru_cache(maxsize=None)
def reduction_expected(H, W):
    live, pv, pn = reduction_inputs(H, W)
    return [refine_f64(live[k], pv[k], pn[k], reduction_K(H, W), REDUCTION_RANGE, REDUCTION_MAX_ERROR) for k in range(REDUCTION_N)]


# =====================================================================================================================
# 4. degenerate systems (24 x 32, the gate camera)
def degenerate_empty_inputs():
    """three objects without a single usable pixel"""
    z = np.zeros((3, GATE_H, GATE_W, 3), F)
    return z, z.copy(), z.copy()


def degenerate_single_inputs():
    """one inlier on the optical axis, 2^-8 in front of the predicted surface: the only constrained variable is t_z"""
    live = np.zeros((1, GATE_H, GATE_W, 3), F)
    pv, pn = np.zeros_like(live), np.zeros_like(live)
    pv[0, 5, 9] = _axis(1.0)
    pn[0, 5, 9] = _DOWN
    live[0, 12, 16] = _axis(1.0 - 2.0 ** -8)
    return live, pv, pn


def degenerate_single_expected():
    """J = w (0, 0, -1, 0, 0, 0), r = w 2^-8: x = (0, 0, -2^-8, 0, 0, 0) whatever w — the update is a pure translation"""
    upd = IDENTITY34.copy()
    upd[2, 3] = -(2.0 ** -8)
    return upd


PLANE_COLUMNS = (2, 3, 4)       # t_z and the two tilts; t_x, t_y and the roll have an all-zero Jacobian column


@functools.lru_cache(maxsize=None)
def degenerate_plane_inputs():
    """a fronto-parallel plane at 0.8 m, every normal (0, 0, -1); the live plane is a few millimetres off and slightly tilted"""
    H, W, K = GATE_H, GATE_W, GATE_K
    rng = np.random.default_rng(77)
    lives, pvs, pns = [], [], []
    for k in range(2):
        s = ((np.arange(W, dtype=D) - K[0, 2]) / K[0, 0])[None, :] + np.zeros((H, 1))
        t = ((np.arange(H, dtype=D) - K[1, 2]) / K[1, 1])[:, None] + np.zeros((1, W))
        z = np.full((H, W), 0.8)
        zl = z + 0.003 - 0.001 * k + 0.004 * s - 0.002 * t + rng.uniform(-0.0005, 0.0005, (H, W))
        lives.append(np.stack([s * zl, t * zl, zl], -1).astype(F))
        pvs.append(np.stack([s * z, t * z, z], -1).astype(F))
        pns.append(np.broadcast_to(np.array(_DOWN, F), (H, W, 3)).copy())
    return np.stack(lives), np.stack(pvs), np.stack(pns)


@functools.lru_cache(maxsize=None)
def degenerate_plane_expected():
    live, pv, pn = degenerate_plane_inputs()
    return [refine_f64(live[k], pv[k], pn[k], GATE_K, GATE_RANGE, GATE_MAX_ERROR, columns=PLANE_COLUMNS) for k in range(2)]


# =====================================================================================================================
# 5. centre
CENTER_SHAPES = {1: (1, 1), 255: (15, 17), 256: (16, 16), 257: (1, 257), 2049: (3, 683)}     # P -> (H, W)
CENTER_OBJ = 4
CENTER_MAX_ERROR = 2.0 ** -7
# planted pixels (P >= 255), at pixel indices 0, 1, ...: label ok, live depth, canonical point, its model coordinate vx =
# cx - roundf(cx) stated by hand, |error| as a multiple of max_error through (normal z, depth offset), expected (valid, votes)
_E = CENTER_MAX_ERROR
CENTER_PLANTS = [
    # id                 label  dz          canonical (cx, cy, cz)         vx        nz           dz - pvz  valid votes
    ("wrong-label",      False, 1.0,        (2.25, 0.0, 0.0),              0.25,     1.0,         0.0,      0, 0),
    ("dz=0",             True,  0.0,        (2.25, 0.0, 0.0),              0.25,     1.0,         0.0,      0, 0),
    ("dz=denorm-min",    True,  1e-45,      (2.25, 0.0, 0.0),              0.25,     1.0,         4 * _E,   1, 0),
    ("nan-cx",           True,  1.0,        (_NAN, 0.0, 0.0),              _NAN,     1.0,         0.0,      0, 0),
    ("nan-cy",           True,  1.0,        (2.25, _NAN, 0.0),             0.25,     1.0,         0.0,      0, 0),
    ("nan-cz",           True,  1.0,        (2.25, 0.0, _NAN),             0.25,     1.0,         0.0,      0, 0),
    ("cx=3.5",           True,  1.0,        (3.5, 0.01, 0.02),             -0.5,     1.0,         0.0,      1, 1),     # roundf: halves away from zero -> 4
    ("cx=-2.5",          True,  1.0,        (-2.5, 0.01, 0.02),            0.5,      1.0,         0.0,      1, 1),     # -> -3
    ("cx=7+2^-20",       True,  1.0,        (7.0 + 2.0 ** -20, 0.01, 0.02), 2.0 ** -20, 1.0,      0.0,      1, 1),
    ("err=max",          True,  1.0,        (2.25, 0.01, 0.02),            0.25,     1.0,         _E,       1, 0),     # `fabsf(error) < max_error` is strict: a pair, no vote
    ("err=max-ulp",      True,  1.0,        (2.25, 0.01, 0.02),            0.25,     float(down(1.0)), _E,  1, 1),
    ("err=-max",         True,  1.0,        (2.25, 0.01, 0.02),            0.25,     -1.0,        _E,       1, 0),
]


@functools.lru_cache(maxsize=None)
def center_case(P):
    """-> dict(inputs..., mask, pairs, votes, sums f64 [3]); the arrays are built FROM the flags (label ok, depth ok, canonical
    ok, votes), so mask and both counts are exact by construction"""
    H, W = CENTER_SHAPES[P]
    rng = np.random.default_rng(P)
    lab_ok = rng.random(P) < 0.9
    depth_ok = rng.random(P) < 0.95
    canon_ok = rng.random(P) < 0.97
    votes = rng.random(P) < 0.7
    live = np.stack([rng.uniform(-0.3, 0.3, P), rng.uniform(-0.3, 0.3, P), rng.uniform(0.5, 1.5, P)], -1)
    live[~depth_ok, 2] = 0.0
    idx = rng.integers(0, 21, P).astype(D)                       # the model index riding in canonical x
    vx = rng.uniform(-0.4, 0.4, P)
    canon = np.stack([idx + vx, rng.uniform(-0.1, 0.1, P), rng.uniform(-0.1, 0.1, P)], -1)
    bad = np.flatnonzero(~canon_ok)
    canon[bad, rng.integers(0, 3, len(bad))] = np.nan
    pn = rng.standard_normal((P, 3))
    pn /= np.linalg.norm(pn, axis=1, keepdims=True)
    # error = pn . (live - pv): a quarter of max_error at most for a vote, 2 to 4 times max_error otherwise
    e = np.where(votes, rng.uniform(-0.25, 0.25, P), rng.choice([-1.0, 1.0], P) * rng.uniform(2, 4, P)) * CENTER_MAX_ERROR
    pv = live - pn * e[:, None]
    label = np.where(lab_ok, CENTER_OBJ, 7).astype(np.int32)
    live, canon, pv, pn = live.astype(F), canon.astype(F), pv.astype(F), pn.astype(F)
    model_x = canon[:, 0].astype(D) - idx                        # cx - roundf(cx) for |vx| <= 0.4, on the rounded input
    if P == 1:      # the single pixel is a voting pair
        lab_ok[:], depth_ok[:], canon_ok[:], votes[:] = True, True, True, True
        label[:] = CENTER_OBJ
        live[0], canon[0], pv[0], pn[0] = (0.1, -0.2, 1.0), (2.25, 0.01, 0.02), (0.1, -0.2, 1.0), (0, 0, 1)
        model_x[0] = 0.25
    else:
        for i, (_, lok, dz, can, mvx, nz, off, valid, vote) in enumerate(CENTER_PLANTS):
            label[i] = CENTER_OBJ if lok else 7
            live[i] = (0.125, -0.25, dz)
            canon[i] = can
            pn[i] = (0.0, 0.0, nz)
            pv[i] = (0.125, -0.25, F(dz) - F(off))
            model_x[i] = mvx
            lab_ok[i], depth_ok[i], canon_ok[i], votes[i] = True, True, bool(valid), bool(vote)     # (`valid` carries all three)
    mask = lab_ok & depth_ok & canon_ok
    vote = mask & votes
    m = np.stack([model_x, canon[:, 1].astype(D), canon[:, 2].astype(D)], -1)
    sums = np.where(vote[:, None], live.astype(D) - m, 0.0).sum(0)
    return dict(id="center/P%d" % P, H=H, W=W, label=label.reshape(H, W), live=live.reshape(H, W, 3), canon=canon.reshape(H, W, 3),
                pv=pv.reshape(H, W, 3), pn=pn.reshape(H, W, 3), mask=mask.reshape(H, W).astype(np.uint8), pairs=int(mask.sum()),
                votes=int(vote.sum()), sums=sums, nblocks=nblocks(H, W))


# =====================================================================================================================
# 6. score
SCORE_H, SCORE_W = 48, 64
SCORE_K = intrinsics(1000.0, 1000.0, 32.0, 24.0)


class ScoreScene:
    """A frame for pcnn_icp_score_fwd built point by point. A masked pixel is both a depth point (its live vertex) and a
    model point (its canonical vertex, moved by the hypothesis): a depth-only pixel carries a NaN canonical vertex (the model
    point is skipped), a model-only pixel the live vertex (0, 0, 0) — 0.7 m from every query, never a candidate."""

    def __init__(self, H=SCORE_H, W=SCORE_W, K=SCORE_K):
        self.H, self.W, self.K = H, W, K
        self.live = np.zeros((H, W, 3), F)
        self.canon = np.full((H, W, 3), np.nan, F)
        self.mask = np.zeros((H, W), np.uint8)

    def ray(self, x, y, z):
        """the point at depth z on the ray of pixel (x, y) (fractional pixels allowed), float32"""
        K = self.K
        return np.array([(x - K[0, 2]) / K[0, 0] * z, (y - K[1, 2]) / K[1, 1] * z, z], D).astype(F)

    def depth(self, y, x, point=None, z=0.7):
        assert not self.mask[y, x]
        self.mask[y, x] = 1
        self.live[y, x] = self.ray(x, y, z) if point is None else point
        return self.live[y, x].copy()

    def model(self, y, x, q):
        assert not self.mask[y, x] and abs(q[0]) < 0.5
        self.mask[y, x] = 1
        self.canon[y, x] = q

    def both(self, y, x, z=0.7):
        p = self.depth(y, x, z=z)
        self.canon[y, x] = p
        return p


IDENTITY12 = IDENTITY34.reshape(12).astype(F)


def _hyp(t=(0, 0, 0)):
    T = IDENTITY34.copy()
    T[:, 3] = t
    return T.reshape(12).astype(F)


def _score_corners():
    """model points projecting near the four corners and just outside each edge; one depth point within reach of each"""
    s = ScoreScene()
    hosts = iter([(24, x) for x in range(24, 40)])
    plan = [((0.3, 0.3), (1, 2)), ((62.6, 0.4), (2, 61)), ((0.4, 46.7), (45, 1)), ((62.8, 46.6), (46, 62)),      # corners
            ((-3.0, 24.2), (24, 0)), ((66.0, 23.3), (23, 63)), ((30.2, -2.5), (0, 30)), ((29.7, 50.0), (47, 30))]    # outside
    for (qx, qy), (dy, dx) in plan:
        s.depth(dy, dx)
        s.model(*next(hosts), s.ray(qx, qy, 0.7))
    return dict(id="corners", scene=s, hyps=[IDENTITY12], radius=0.01, hits=[8],
                why="8 queries, each 1 to 3 px (0.7 to 2.1 mm) from a depth point of its own; every other depth point is more than 9 px away")


def _score_probe_trap():
    """5 x 5 probe empty; A at +5 px, 9 mm behind (inside the 13 x 13 probe, 9.7 mm away); the true nearest B at +9 px in the
    query's depth plane (6.3 mm away, outside the probe). A second query sits on A: hits = 2 if the first took B, else 1"""
    s = ScoreScene()
    q = s.ray(20, 24, 0.7)
    a = s.depth(24, 25, z=0.709)
    s.depth(24, 29, z=0.7)
    s.model(40, 5, q)
    s.model(40, 6, a)
    return dict(id="probe-trap", scene=s, hyps=[IDENTITY12], radius=0.01, hits=[2], trap=dict(q=(24, 20), a=(24, 25), b=(24, 29)),
                why="query 1 -> B (6.3 mm < A's 9.7 mm), query 2 -> A (0 mm): two distinct points")


def _score_tie():
    """two depth points at exactly the same float32 distance (dyadic offsets -+2^-10 along x): the lower pixel index wins.
    A second query 9 mm beyond the higher one can only reach that one: hits = 2 if the lower index won the tie, else 1"""
    s = ScoreScene()
    q = np.array([-2.0 ** -9, 0.0, 0.75], F)              # projects to (29.4, 24)
    lo = s.depth(24, 28, point=q + np.array([-2.0 ** -10, 0, 0], F))
    hi = s.depth(24, 31, point=q + np.array([2.0 ** -10, 0, 0], F))
    s.model(40, 5, q)
    s.model(40, 6, hi + np.array([0.009, 0, 0], F))
    return dict(id="tie", scene=s, hyps=[IDENTITY12], radius=0.01, hits=[2], tie=dict(lo=(24, 28), hi=(24, 31)),
                why="query 1 ties -> pixel (24, 28); query 2 is 9 mm from (24, 31) and 10.95 mm from (24, 28): two distinct points")


def _score_on_radius(inside):
    """a depth point exactly `radius` = 2^-6 behind the query, nothing else: d^2 == r^2 is not a hit. With the radius one ulp
    larger the same point is one ulp inside"""
    s = ScoreScene()
    q = s.ray(30, 20, 0.75)
    s.depth(20, 30, point=q + np.array([0, 0, 2.0 ** -6], F))
    s.model(40, 5, q)
    r = float(up(2.0 ** -6)) if inside else 2.0 ** -6
    return dict(id="on-radius-ulp-inside" if inside else "on-radius", scene=s, hyps=[IDENTITY12], radius=r, hits=[1 if inside else 0],
                why="|dz| = 2^-6 exactly (0.765625 - 0.75 is exact in float32)")


def _score_hypotheses():
    """a 6 x 6 patch of pairs at z = 0.75 (each model point sits on its own depth point), a copy of the depth points at
    z = 2 r = 2^-5 and one at z = -0.25, and nine hypotheses"""
    s = ScoreScene()
    r = 2.0 ** -6
    for y in range(6):
        for x in range(6):
            p = s.both(20 + y, 28 + x, z=0.75)
            s.depth(2 + y, 3 + x, point=np.array([p[0], p[1], 2 * r], F))        # reached by the full scan only (qz <= 2 r)
            s.depth(40 + y, 50 + x, point=np.array([p[0], p[1], -0.25], F))      # qz < 0
    step = 0.00075                                            # one pixel at 0.75 m
    nan_t, nan_r = IDENTITY12.copy(), IDENTITY12.copy()
    nan_t[3], nan_r[5] = np.nan, np.nan
    hyps = [IDENTITY12,                     # every model point finds its own depth point: 36
            _hyp((0, 0, 2 * r - 0.75)),     # qz = 2 r exactly: `qz > 2 r` fails, full scan, the copy at 2 r: 36
            _hyp((0, 0, -1.0)),             # qz = -0.25: full scan, the copy at -0.25: 36
            nan_t,                          # NaN translation: every moved point is NaN: 0
            nan_r,                          # NaN in the rotation: qy NaN: 0
            _hyp((np.inf, 0, 0)),           # nowhere near the image: 0
            _hyp((step, 0, 0)),             # one pixel to the right: columns 1..5 marked, the last model column shares column 5: 30
            _hyp((0, 0, 0.01)),             # 10 mm behind, within r = 15.6 mm: own depth point still nearest: 36
            _hyp((0, 0, 0.02))]             # 20 mm behind: out of reach: 0
    return dict(id="hypotheses", scene=s, hyps=hyps, radius=r, hits=[36, 36, 36, 0, 0, 0, 30, 36, 0],
                why="see the list of hypotheses")


def _score_last_pixel():
    """9 x 13 = 117 pixels, 4 flag words, the last one partial: the only hit is pixel 116 (word 3, bit 20)"""
    K = intrinsics(1000.0, 1000.0, 6.0, 4.0)
    s = ScoreScene(9, 13, K)
    p = s.depth(8, 12)
    s.model(0, 0, p)
    return dict(id="last-pixel", scene=s, hyps=[IDENTITY12], radius=0.01, hits=[1], why="one query on the last pixel's depth point")


@functools.lru_cache(maxsize=None)
def score_cases():
    return [_score_corners(), _score_probe_trap(), _score_tie(), _score_on_radius(False), _score_on_radius(True),
            _score_hypotheses(), _score_last_pixel()]


def score_f64(case):
    """exhaustive float64 search over the float32 data: hits per hypothesis (strictly inside the radius, ties to the lower
    pixel index) and the list of (model pixel, nearest pixel or -1) of each"""
    s = case["scene"]
    live = s.live.reshape(-1, 3).astype(D)
    canon = s.canon.reshape(-1, 3).astype(D)
    pts = np.flatnonzero(s.mask.reshape(-1))
    r2 = D(F(case["radius"])) ** 2
    hits, pairs = [], []
    for T in case["hyps"]:
        T = np.asarray(T, D).reshape(3, 4)
        marked, pr = set(), []
        with np.errstate(all="ignore"):
            for p in pts:
                q = T[:, :3] @ canon[p] + T[:, 3]
                if not np.all(q == q):
                    continue
                d2 = np.sum((live[pts] - q) ** 2, axis=1)
                k = int(np.argmin(np.where(d2 < r2, d2, np.inf))) if np.any(d2 < r2) else -1
                pr.append((int(p), int(pts[k]) if k >= 0 else -1))
                if k >= 0:
                    marked.add(int(pts[k]))
        hits.append(len(marked))
        pairs.append(pr)
    return hits, pairs


def score_window(q, rad, K, H, W):
    """the clipped search window of a query (icp_window restated, float32): (x0, x1, y0, y1) and the unclipped one"""
    qx, qy, qz, rad = F(q[0]), F(q[1]), F(q[2]), F(rad)
    fx, fy, px, py = F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])
    uc, vc = qx / qz * fx + px, qy / qz * fy + py
    hw = np.abs(fx) * rad * (F(1) + np.abs(qx / qz)) / (qz - rad) + F(2)
    hh = np.abs(fy) * rad * (F(1) + np.abs(qy / qz)) / (qz - rad) + F(2)
    raw = (int(np.floor(uc - hw)), int(np.ceil(uc + hw)), int(np.floor(vc - hh)), int(np.ceil(vc + hh)))
    return (max(0, raw[0]), min(W - 1, raw[1]), max(0, raw[2]), min(H - 1, raw[3])), raw


# =====================================================================================================================
# 7. polish
POLISH_H, POLISH_W = 3, 1100
POLISH_K = intrinsics(1000.0, 1000.0, 549.5, 1.0)
POLISH_OBJ = 2
POLISH_RANGE = (0.25, 6.0)
POLISH_BUDGETS = (8, 50)
# id -> how the label is laid out; (dq, dr) = (NM_LANES // bw, NM_LANES % bw) of the per-thread walk
POLISH_CASES = [
    dict(id="polish/w1023", box=(0, 3, 10, 1033), bw=1023, walk=(1, 1)),
    dict(id="polish/w1024", box=(0, 3, 10, 1034), bw=1024, walk=(1, 0)),
    dict(id="polish/w1025", box=(0, 3, 10, 1035), bw=1025, walk=(0, 1024)),
    dict(id="polish/one-pixel-first", box=(0, 1, 0, 1), bw=1, walk=(1024, 0)),
    dict(id="polish/one-pixel-last", box=(2, 3, 1099, 1100), bw=1, walk=(1024, 0)),
    dict(id="polish/no-valid", box=(0, 3, 100, 200), bw=100, walk=(10, 24), no_depth=True),
    dict(id="polish/nan-background", box=(0, 3, 400, 700), bw=300, walk=(3, 124), holes=True),
]
POLISH = {c["id"]: c for c in POLISH_CASES}


@functools.lru_cache(maxsize=None)
def polish_inputs(case_id):
    """-> label int32 [3,1100], live [3,1100,3], pred_v [3,1100,3]: a wavy surface at 0.7 m, the prediction a few millimetres off"""
    c = POLISH[case_id]
    H, W, K = POLISH_H, POLISH_W, POLISH_K
    rng = np.random.default_rng(len(case_id) * 131 + c["bw"])
    s = ((np.arange(W, dtype=D) - K[0, 2]) / K[0, 0])[None, :] + np.zeros((H, 1))
    t = ((np.arange(H, dtype=D) - K[1, 2]) / K[1, 1])[:, None] + np.zeros((1, W))
    z = 0.7 + 0.01 * np.sin(np.arange(W) / 50.0)[None, :] + 0.002 * np.arange(H)[:, None]
    live = np.stack([s * z, t * z, z], -1)
    pred = live + np.array([0.002, -0.001, 0.003]) + rng.uniform(-0.0005, 0.0005, (H, W, 3))
    label = np.zeros((H, W), np.int32)
    y0, y1, x0, x1 = c["box"]
    label[y0:y1, x0:x1] = POLISH_OBJ
    if c.get("no_depth"):
        live[y0:y1, x0:x1, 2] = 0.0             # every labelled pixel fails `vz > z_near`
    if c.get("holes"):
        kind = rng.random((H, W))
        kind[y0, x0] = kind[y1 - 1, x1 - 1] = kind[y0, x1 - 1] = kind[y1 - 1, x0] = 0.5     # the box keeps its corners
        pred[kind < 0.3] = np.nan               # the render's background inside the box
        label[(kind > 0.9) & (label == POLISH_OBJ)] = 0
    return label, live.astype(F), pred.astype(F)


def polish_simplex():
    """the eight initial vertices: x0 = (1, 0, 0, 0, 0, 0, 0) and x0 + (ub - lb) / 4 along each axis"""
    x0 = np.array([1, 0, 0, 0, 0, 0, 0], D)
    step = np.array([0.1, 0.1, 0.1, 0.1, 0.01, 0.01, 0.1], D) * 2 * 0.25
    return [x0] + [x0 + step[i] * np.eye(7)[i] for i in range(7)]


def polish_energy_f64(label, live, pred, x, depth_range=POLISH_RANGE):
    """optEnergy in float64 over the float32 data -> (mean distance or 0, pixels counted)"""
    q = np.asarray(x[:4], D) / np.linalg.norm(x[:4])
    w, a, b, c = q
    R = np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                  [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                  [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]], D)
    sel = label == POLISH_OBJ
    p = pred[..., :3][sel].astype(D) @ R.T + np.asarray(x[4:7], D)
    v = live[sel].astype(D)
    zn, zf = D(F(depth_range[0])), D(F(depth_range[1]))
    with np.errstate(all="ignore"):
        ok = np.all(p == p, axis=1) & (v[:, 2] > zn) & (v[:, 2] < zf) & (p[:, 2] > zn) & (p[:, 2] < zf)
    n = int(ok.sum())
    return (float(np.linalg.norm(p[ok] - v[ok], axis=1).sum() / n) if n else 0.0), n


@functools.lru_cache(maxsize=None)
def polish_expected(case_id):
    """-> (min over the initial simplex of the float64 energy, pixels counted at x0)"""
    label, live, pred = polish_inputs(case_id)
    es = [polish_energy_f64(label, live, pred, x) for x in polish_simplex()]
    return min(e for e, _ in es), es[0][1]


# =====================================================================================================================
def measure():
    """the BOUNDS table from the oracle on the CPU (run `python tests/icp_cases.py`)"""
    import oracle
    out = {}
    for H, W in REDUCTION_SHAPES:
        live, pv, pn = reduction_inputs(H, W)
        upd, st = oracle.icp_refine(live, pv, pn, reduction_K(H, W), REDUCTION_RANGE, REDUCTION_MAX_ERROR, iterations=1)
        ex = reduction_expected(H, W)
        out[reduction_id(H, W)] = {"sum_r2": max(abs(float(st[k, 0, 1]) - ex[k]["sum_r2"]) / ex[k]["sum_r2"] for k in range(REDUCTION_N)),
                                   "update": max(float(np.abs(upd[k] - ex[k]["update"]).max()) for k in range(REDUCTION_N))}
    live, pv, pn = degenerate_single_inputs()
    upd, _ = oracle.icp_refine(live, pv, pn, GATE_K, GATE_RANGE, GATE_MAX_ERROR, iterations=1)
    out["degenerate/single-inlier"] = {"update": float(np.abs(upd[0] - degenerate_single_expected()).max())}
    live, pv, pn = degenerate_plane_inputs()
    upd, _ = oracle.icp_refine(live, pv, pn, GATE_K, GATE_RANGE, GATE_MAX_ERROR, iterations=1)
    out["degenerate/plane"] = {"update": max(float(np.abs(upd[k] - e["update"]).max()) for k, e in enumerate(degenerate_plane_expected()))}
    for P in CENTER_SHAPES:
        c = center_case(P)
        sums, _ = oracle.icp_center(c["label"], c["live"], c["canon"], c["pv"], c["pn"], CENTER_OBJ, CENTER_MAX_ERROR)
        out[c["id"]] = {"sums": float(np.abs(sums[:3] - c["sums"]).max())}
    for c in POLISH_CASES:
        label, live, pred = polish_inputs(c["id"])
        _, e, _ = oracle.icp_polish(label, live, pred, POLISH_OBJ, POLISH_RANGE, 8)
        out[c["id"]] = {"energy": abs(e - polish_expected(c["id"])[0])}
    return out


if __name__ == "__main__":
    for cid, row in measure().items():
        print('    "%s": {%s},' % (cid, ", ".join('"%s": (%.2g, %.3g)' % (k, float("%.2g" % v), 4 * float("%.2g" % v)) for k, v in row.items())))
