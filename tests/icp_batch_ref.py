"""The batched pose refinement restated on the CPU checker (TEST INFRASTRUCTURE): what `posecnn_amd.icp.refine_batch` must
return bit for bit. The stages run through tests/oracle.py (render_mesh, icp_backproject, icp_center, icp_polish, icp_refine,
icp_score); the arithmetic between them is written out as scalar float64 expressions in ONE order — the order of the glue
kernels of posecnn_amd/csrc/icp_batch.hip: 3-term sums are (a + b) + c. No `@`, no norm, no trace: numpy's small matrix
product and norm go through BLAS, whose summation order and FMA use are not fixed."""
import math

import numpy as np

HYPOTHESIS_DZ = (0.0, -0.02, -0.01, 0.01, 0.02, 0.03, 0.04, 0.05)    # synthesize.cpp:2252-2270
INFO_COLUMNS = 12
DEAD, REFINED, BACKGROUND, FEW_PIXELS, NO_MODEL, CAPACITY = range(6)
F32, F64 = np.float32, np.float64


def pose34(x):
    """(quaternion wxyz, translation) -> 3x4 as a list of 12 floats (pose_error.quat2mat's expressions)"""
    w, a, b, c = (float(v) for v in x[:4])
    n = ((w * w + a * a) + b * b) + c * c
    if n < 1e-16:
        R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    else:
        s = 2.0 / n
        R = [1.0 - s * (b * b + c * c), s * (a * b - c * w), s * (a * c + b * w),
             s * (a * b + c * w), 1.0 - s * (a * a + c * c), s * (b * c - a * w),
             s * (a * c - b * w), s * (b * c + a * w), 1.0 - s * (a * a + b * b)]
    return [R[0], R[1], R[2], float(x[4]), R[3], R[4], R[5], float(x[5]), R[6], R[7], R[8], float(x[6])]


def compose(U, T):
    """U o T for 3x4 transforms as flat lists of 12"""
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (U[4 * i] * T[j] + U[4 * i + 1] * T[4 + j]) + U[4 * i + 2] * T[8 + j]
        out[4 * i + 3] = ((U[4 * i] * T[3] + U[4 * i + 1] * T[7]) + U[4 * i + 2] * T[11]) + U[4 * i + 3]
    return out


def pose_row(T):
    """3x4 -> the f32 output row (unit quaternion wxyz with w >= 0, translation): icp.mat2quat's algorithm"""
    R = [[T[0], T[1], T[2]], [T[4], T[5], T[6]], [T[8], T[9], T[10]]]
    q = [0.0] * 4
    tr = (R[0][0] + R[1][1]) + R[2][2]
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0
        q[0] = 0.25 * s
        q[1] = (R[2][1] - R[1][2]) / s
        q[2] = (R[0][2] - R[2][0]) / s
        q[3] = (R[1][0] - R[0][1]) / s
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0) * 2.0
        q[1 + i] = 0.25 * s
        q[0] = (R[k][j] - R[j][k]) / s
        q[1 + j] = (R[j][i] + R[i][j]) / s
        q[1 + k] = (R[k][i] + R[i][k]) / s
    nrm = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [v / nrm for v in q]
    if not q[0] >= 0.0:
        q = [-v for v in q]
    return np.array(q + [T[3], T[7], T[11]], F64).astype(F32)


def _K(intr):
    fx, fy, px, py = (float(v) for v in intr)
    return np.array([[fx, 0, px], [0, fy, py], [0, 0, 1]], F64)


def decode(roi, B, C):
    """status of a live row before the pixel count, frame, class id (the class id is read by truncation, as icp_python's int())"""
    f, c = F32(roi[0]), F32(roi[1])
    if not c >= 1:
        return BACKGROUND, 0, 0
    if not c < C + 1:
        return NO_MODEL, 0, 0
    if not f >= 0 or not f < B:
        return BACKGROUND, 0, 0
    return REFINED, int(f), int(c)


def refine_one(label, depth, intr, factor, cls, pose_row7, mesh, max_error, iterations, polish_evaluations, radius, depth_range):
    """One job. Returns (poses_new row, poses_icp row, info[1:] = agree, pairs, choose, hits[8], extras for the tests)."""
    import oracle
    v, n, f = mesh
    H, W = label.shape
    K = _K(intr)
    T = pose34([float(F32(x)) for x in pose_row7])
    as34 = lambda t: np.array(t, F64).reshape(3, 4)
    maps = oracle.render_mesh(v, n, f, as34(T)[None], K, H, W, depth_range, model_index=cls - 1)
    live = oracle.icp_backproject(depth, label, cls, K, factor)
    sums, mask = oracle.icp_center(label, live, maps["canonical"][0], maps["vertices"][0], maps["normals"][0], cls, max_error)
    agree, pairs = int(sums[3]), int(sums[4])
    Tz = T[11]
    if agree > 0:
        Tz = float(F32(sums[2]) / F32(agree))
        tx, ty, tz = (float(F32(x)) for x in pose_row7[4:7])
        rx = tx / tz if tz != 0.0 else 0.0
        ry = ty / tz if tz != 0.0 else 0.0
        T[3], T[7], T[11] = rx * Tz, ry * Tz, Tz
        if polish_evaluations:
            pv = oracle.render_mesh(v, n, f, as34(T)[None], K, H, W, depth_range, want=("vertices",))["vertices"][0]
            x, _, _ = oracle.icp_polish(label, live, pv, cls, depth_range, polish_evaluations)
            T = compose(pose34(x), T)
            Tz = T[11]
    new_row = pose_row(T)
    hyps = []
    for dz in HYPOTHESIS_DZ:
        h = list(T)
        h[11] = Tz + dz
        hyps.append(h)
    H8 = np.array(hyps, F64).reshape(8, 3, 4)
    pm = oracle.render_mesh(v, n, f, H8, K, H, W, depth_range, want=("vertices", "normals"))
    upd, _ = oracle.icp_refine(np.repeat(live[None], 8, 0), pm["vertices"], pm["normals"], K, depth_range, max_error, iterations)
    hyps = [compose([float(u) for u in U.reshape(12)], h) for U, h in zip(upd, hyps)]
    choose, hits = 0, [-1] * 8
    if pairs > 0:
        hits = [int(h) for h in oracle.icp_score(live, maps["canonical"][0], mask, np.array(hyps, F64).reshape(8, 3, 4), radius)]
        for h in range(1, 8):
            if hits[h] > hits[choose]:
                choose = h
    return new_row, pose_row(hyps[choose]), [agree, pairs, choose] + hits, {"T_new": as34(T), "T_icp": as34(hyps[choose])}


def refine_batch(labels, depth, intrinsics, factor_depth, rois, poses, count, meshes, max_error=0.01, iterations=8,
                 polish_evaluations=50, min_pixels=400, radius=0.01, depth_range=(0.25, 6.0), max_jobs=None):
    """numpy in, (poses_new f32 [R,7], poses_icp f32 [R,7], info int32 [R,12], extras {row: {...}}) out"""
    labels, depth = np.asarray(labels, np.int32), np.asarray(depth, np.uint16)
    rois, poses = np.asarray(rois, F32), np.asarray(poses, F32)
    B, R, C = labels.shape[0], rois.shape[0], len(meshes)
    live_rows = R if count is None else min(max(int(count), 0), R)
    J = R if max_jobs is None else int(max_jobs)
    poses_new, poses_icp = np.zeros((R, 7), F32), np.zeros((R, 7), F32)
    info = np.zeros((R, INFO_COLUMNS), np.int32)
    extras, jobs = {}, 0
    for r in range(live_rows):
        st, frame, cls = decode(rois[r], B, C)
        if st == REFINED and int((labels[frame] == cls).sum()) < min_pixels:
            st = FEW_PIXELS
        if st == REFINED:
            if jobs >= J:
                st = CAPACITY
            jobs += 1
        info[r, 0] = st
        if st != REFINED:
            continue
        poses_new[r], poses_icp[r], info[r, 1:], extras[r] = refine_one(
            labels[frame], depth[frame], intrinsics[frame], factor_depth, cls, poses[r], meshes[cls - 1], max_error, iterations,
            polish_evaluations, radius, depth_range)
    return poses_new, poses_icp, info, extras
