"""numpy restatement of include/posecnn_hip_pose2d.h (TEST INFRASTRUCTURE, the statement of record of the RGB-only 3-D vertex
route's pose stage): prepare, sample (closed-form P3P), one preemptive round with its Gauss-Newton refit, the whole loop.
Every step is the header's f32 / f64 operation in the header's order (numpy's elementwise +, -, *, /, sqrt round once and
never fuse), so the GPU results are compared bit for bit. What the route shares with the depth route (Horn's fit, the
projected box, the index rules, the lane fold, the Philox block) is taken from tests/pose3d_ref.py.

`defect=` plants one of four seeded mistakes (tests/test_pose2d_cpu.py shows that each is caught):
  "le"      reprojection distance <= threshold counts as an inlier
  "fourth"  the P3P solution is the first valid root: the fourth pair is ignored
  "fold"    the 64 lane sums of the refit are added in lane order instead of by the xor butterfly
  "half"    the retraction uses omega instead of omega / 2
"""
import numpy as np

import pose3d_ref as R3
from augment_ref import philox4x64

F, D = np.float32, np.float64
RECORD = 6
GN_STEPS = 2
CUBIC_STEPS = 80
POLISH_STEPS = 4
DEFAULTS = dict(hypotheses=256, pixel_batch=1000, max_pixels=1000, ref_it=8, min_area=400, inlier_threshold=10.0,
                min_dist2d=10.0, min_dist3d=0.01, max_attempts=1024)
TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))

stride_index, philox_index, halving_schedule, fit, box_ok, dist = (R3.stride_index, R3.philox_index, R3.halving_schedule, R3.fit,
                                                                    R3.box_ok, R3.dist)


# ---- prepare ------------------------------------------------------------------------------------------------------------
def prepare(label, vertex_pred, extents):
    """One frame: label int [H,W], vertex_pred f32 [H,W,3C], extents f32 [C,3]
    -> records f32 [total,6] rows (x, y, 0, obj xyz), counts int32 [C], offsets int32 [C]"""
    H, W = label.shape
    depth = np.ones((H, W), np.uint16)
    rec, counts, offsets = R3.prepare(label, depth, vertex_pred, extents, (1.0, 1.0, 0.0, 0.0), 1.0)
    p = np.concatenate([np.nonzero(np.asarray(label).reshape(-1) == c)[0] for c in range(1, extents.shape[0])] + [np.zeros(0, np.int64)])
    rec = rec.copy()
    rec[:, 0], rec[:, 1], rec[:, 2] = (p % W).astype(F), (p // W).astype(F), F(0)
    return rec, counts, offsets


# ---- the quartic ----------------------------------------------------------------------------------------------------------
def quartic_roots(A4, A3, A2, A1, A0):
    """f64 [S] each -> [4,S]: the real roots Ferrari's factorisation finds, in the header's slot order, NaN where a slot has
    none. Not a general solver (see the header): the caller gates every root."""
    with np.errstate(all="ignore"):
        B, C, Dd, E = A3 / A4, A2 / A4, A1 / A4, A0 / A4
        B2 = B * B
        p = C - 0.375 * B2
        q = (Dd - 0.5 * B * C) + 0.125 * B2 * B
        r = ((E - 0.25 * B * Dd) + 0.0625 * B2 * C) - 0.01171875 * B2 * B2
        c2, c1, c0 = p, 0.25 * p * p - r, -0.125 * q * q
        mx = np.abs(c2)
        mx = np.where(np.abs(c1) > mx, np.abs(c1), mx)
        mx = np.where(np.abs(c0) > mx, np.abs(c0), mx)
        m = 1.0 + mx
        for _ in range(CUBIC_STEPS):
            g = ((m + c2) * m + c1) * m + c0
            dg = (3.0 * m + 2.0 * c2) * m + c1
            m = m - g / dg
        s = np.sqrt(2.0 * m)
        h = 0.5 * p + m
        t = q / (2.0 * s)
        sd1 = np.sqrt(s * s - 4.0 * (h + t))
        sd2 = np.sqrt(s * s - 4.0 * (h - t))
        ya = [0.5 * (s + sd1), 0.5 * (s - sd1), 0.5 * (sd2 - s), 0.5 * ((-s) - sd2)]
        sd = np.sqrt(p * p - 4.0 * r)
        z1, z2 = np.sqrt(0.5 * (sd - p)), np.sqrt(0.5 * ((-p) - sd))
        yb = [z1, -z1, z2, -z2]
        main = m > 0.0
        out = []
        for i in range(4):
            v = np.where(main, ya[i], yb[i]) - 0.25 * B
            for _ in range(POLISH_STEPS):
                f = (((v + B) * v + C) * v + Dd) * v + E
                df = ((4.0 * v + 3.0 * B) * v + 2.0 * C) * v + Dd
                v = v - f / df
            out.append(v)
    return np.stack(out)


def grunert_coefficients(px2, obj, K):
    """px2 f32 [S,3,2] pixels, obj f32 [S,3,3], K -> dict of the header's P3P quantities (f64 [S] each; f: [3][3])"""
    fx, fy, px, py = (D(F(v)) for v in K)
    with np.errstate(all="ignore"):
        f = []
        for i in range(3):
            bx, by = (px2[:, i, 0].astype(D) - px) / fx, (px2[:, i, 1].astype(D) - py) / fy
            nrm = np.sqrt((bx * bx + by * by) + 1.0)
            f.append((bx / nrm, by / nrm, 1.0 / nrm))
        o = obj.astype(D)

        def d2(i, j):
            dx, dy, dz = o[:, i, 0] - o[:, j, 0], o[:, i, 1] - o[:, j, 1], o[:, i, 2] - o[:, j, 2]
            return (dx * dx + dy * dy) + dz * dz

        def dot(i, j):
            return (f[i][0] * f[j][0] + f[i][1] * f[j][1]) + f[i][2] * f[j][2]

        a2, b2, c2 = d2(1, 2), d2(0, 2), d2(0, 1)
        ca, cb, cg = dot(1, 2), dot(0, 2), dot(0, 1)
        q, r, cob, aob = (a2 - c2) / b2, (a2 + c2) / b2, c2 / b2, a2 / b2
        qm, ca2, cb2, cg2 = q - 1.0, ca * ca, cb * cb, cg * cg
        A4 = qm * qm - 4.0 * cob * ca2
        A3 = 4.0 * ((q * (1.0 - q) * cb - (1.0 - r) * ca * cg) + 2.0 * cob * ca2 * cb)
        A2 = 2.0 * (((((q * q - 1.0) + 2.0 * q * q * cb2) + 2.0 * ((b2 - c2) / b2) * ca2) - 4.0 * r * ca * cb * cg)
                    + 2.0 * ((b2 - a2) / b2) * cg2)
        A1 = 4.0 * ((-q * (1.0 + q) * cb + 2.0 * aob * cg2 * cb) - (1.0 - r) * ca * cg)
        A0 = (1.0 + q) * (1.0 + q) - 4.0 * aob * cg2
    return dict(f=f, b=np.sqrt(b2), q=q, qm=qm, ca=ca, cb=cb, cg=cg, A=(A4, A3, A2, A1, A0))


def project(P, o):
    """P [...,12] f64, o = (ox, oy, oz) f64 broadcastable, K later: -> (qx, qy, qz)"""
    return [((P[..., 4 * i] * o[0] + P[..., 4 * i + 1] * o[1]) + P[..., 4 * i + 2] * o[2]) + P[..., 4 * i + 3] for i in range(3)]


def reproj(P, rec, K):
    """REPROJ of the header: P [S,12] f64, rec [m,6] f32 -> (distance [S,m] f64, in front [S,m] bool)"""
    fx, fy, px, py = (D(F(v)) for v in K)
    r = rec.astype(D)
    with np.errstate(all="ignore"):
        qx, qy, qz = project(P[:, None, :], (r[None, :, 3], r[None, :, 4], r[None, :, 5]))
        du = (fx * qx / qz + px) - r[None, :, 0]
        dv = (fy * qy / qz + py) - r[None, :, 1]
        return np.sqrt(du * du + dv * dv), qz > 0.0


def reproj_own(P, rec, K):
    """each pose on its own record: P [S,12], rec [S,6] -> (distance [S], in front [S])"""
    fx, fy, px, py = (D(F(v)) for v in K)
    r = rec.astype(D)
    with np.errstate(all="ignore"):
        qx, qy, qz = project(P, (r[:, 3], r[:, 4], r[:, 5]))
        du = (fx * qx / qz + px) - r[:, 0]
        dv = (fy * qy / qz + py) - r[:, 1]
        return np.sqrt(du * du + dv * dv), qz > 0.0


def p3p(r4, K, defect=None, roots=quartic_roots, trace=None):
    """r4 f32 [S,4,6] the attempt's four records -> (P [S,12] the chosen solution (NaN without one), found [S]).
    `roots` replaces the quartic solver (tests); `trace` (a dict) receives the coefficients and, per attempt, the chosen root"""
    S = r4.shape[0]
    g = grunert_coefficients(r4[:, :3, :2], r4[:, :3, 3:], K)
    v4 = roots(*g["A"])
    best = np.full(S, np.inf)
    Pbest = np.full((S, 12), np.nan)
    vbest = np.full(S, np.nan)
    found = np.zeros(S, bool)
    o = r4[:, :3, 3:].astype(D)
    with np.errstate(all="ignore"):
        eyes, oks = [], []
        for v in v4:
            u = (((g["qm"] * v * v - 2.0 * g["q"] * g["cb"] * v) + 1.0) + g["q"]) / (2.0 * (g["cg"] - v * g["ca"]))
            s1 = g["b"] / np.sqrt((1.0 + v * v) - 2.0 * v * g["cb"])
            s2, s3 = u * s1, v * s1
            oks.append((s1 > 0.0) & (s2 > 0.0) & (s3 > 0.0))
            eyes.append(np.stack([np.stack([s * g["f"][i][k] for k in range(3)], axis=1) for i, s in enumerate((s1, s2, s3))], axis=1))
        e = np.concatenate(eyes)                                                    # [4S,3,3] f64, root-major
        o4 = np.concatenate([o] * 4)
        Sa, Sb, Sab = np.zeros((4 * S, 3)), np.zeros((4 * S, 3)), np.zeros((4 * S, 3, 3))
        for i in range(3):
            Sa = Sa + o4[:, i]
            Sb = Sb + e[:, i]
            Sab = Sab + o4[:, i, :, None] * e[:, i, None, :]
        P4 = fit(Sa, Sb, Sab, 3).reshape(4, S, 12)
        for k in range(4):
            ok = oks[k].copy()
            for i in range(4):
                ok &= project(P4[k], (r4[:, i, 3].astype(D), r4[:, i, 4].astype(D), r4[:, i, 5].astype(D)))[2] > 0.0
            d4 = reproj_own(P4[k], r4[:, 3], K)[0]
            take = ok & ((d4 < best) if defect != "fourth" else ~found & (d4 < np.inf))
            best = np.where(take, d4, best)
            Pbest = np.where(take[:, None], P4[k], Pbest)
            vbest = np.where(take, v4[k], vbest)
            found |= take
    if trace is not None:
        trace.setdefault("A", []).append(np.stack(g["A"], axis=1))
        trace.setdefault("v", []).append(vbest)
    return Pbest, found


def point_line(p1, p2, p3):
    """pointLineDistance: f32 differences, widened; |(p2 - p1) x (p3 - p1)| / |p2 - p1| in f64"""
    a, b = (p2.astype(F) - p1.astype(F)).astype(D), (p3.astype(F) - p1.astype(F)).astype(D)
    cx, cy, cz = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    with np.errstate(all="ignore"):
        return np.sqrt((cx * cx + cy * cy) + cz * cz) / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def dist2(a, b):
    """f32 pixel differences, widened: [S,2] x [S,2] -> [S] f64"""
    dd = (a.astype(F) - b.astype(F)).astype(D)
    return np.sqrt(dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1])


# ---- sample -------------------------------------------------------------------------------------------------------------
def sample(records, counts, offsets, extents, K, H, W, stream=0, seed=0, hypotheses=256, max_attempts=1024, min_area=400,
           inlier_threshold=10.0, min_dist2d=10.0, min_dist3d=0.01, defect=None, roots=quartic_roots, trace=None, **_):
    """One frame -> hyp_pose f64 [hyp,12], hyp_class, hyp_attempt int32 [hyp], hyp_rec int32 [hyp,4]"""
    C = len(counts)
    thr, md2, md3 = D(F(inlier_threshold)), D(F(min_dist2d)), D(F(min_dist3d))
    ext = np.asarray(extents, dtype=F)
    live = np.array([c for c in range(1, C) if counts[c] > min_area], dtype=np.int64)
    pose = np.zeros((hypotheses, 12), D)
    cls = np.zeros(hypotheses, np.int32)
    att = np.full(hypotheses, -1, np.int32)
    rec4 = np.full((hypotheses, 4), -1, np.int32)
    pending = np.arange(hypotheses)
    key = (seed & ((1 << 64) - 1), seed >> 64)
    lo32 = np.uint64(0xFFFFFFFF)
    for a in range(max_attempts):
        if len(pending) == 0 or len(live) == 0:
            break
        w = philox4x64((a, int(stream), pending.astype(np.uint64), 0), key)
        c = live[philox_index(w[:, 0], len(live)).astype(np.int64)]
        n = counts[c].astype(np.uint64)
        j = [(((w[:, 1 + i] >> np.uint64(32)) * n) >> np.uint64(32)).astype(np.int64) for i in range(3)]
        j.append((((w[:, 0] & lo32) * n) >> np.uint64(32)).astype(np.int64))
        j = np.stack(j, axis=1)
        r = records[offsets[c].astype(np.int64)[:, None] + j]                       # [S,4,6]
        ok = np.ones(len(pending), bool)
        for i in range(4):
            ok &= ~((r[:, i, 3] == 0) & (r[:, i, 4] == 0) & (r[:, i, 5] == 0))
            for k in range(i):
                ok &= ~(dist2(r[:, k, :2], r[:, i, :2]) < md2) & ~(dist(r[:, k, 3:], r[:, i, 3:]) < md3)
        for t in TRIPLES:
            ok &= ~(point_line(r[:, t[0], 3:], r[:, t[1], 3:], r[:, t[2], 3:]) < md3)
        tr = {} if trace is not None else None
        P, found = p3p(r, K, defect, roots, tr)
        ok &= found
        for i in range(4):
            d, front = reproj_own(P, r[:, i], K)
            ok &= front & (d < thr)
        ok &= box_ok(P, ext[c], K, H, W, min_area)
        ok &= np.isfinite(P).all(axis=1)
        if trace is not None:
            trace.setdefault("A", []).append(tr["A"][0][ok])
            trace.setdefault("v", []).append(tr["v"][0][ok])
        done = pending[ok]
        pose[done], cls[done], att[done], rec4[done] = P[ok], c[ok], a, j[ok]
        pending = pending[~ok]
    return pose, cls, att, rec4


# ---- Gauss-Newton refit -----------------------------------------------------------------------------------------------------
def _fold(vals, defect=None):
    if defect != "fold":
        return R3._fold(vals)
    S, m = vals.shape
    J = (m + 63) // 64
    pad = np.zeros((S, J * 64), D)
    pad[:, :m] = vals
    pad = pad.reshape(S, J, 64)
    acc = np.zeros((S, 64), D)
    for jj in range(J):
        acc = acc + pad[:, jj]
    out = np.zeros(S, D)
    for lane in range(64):
        out = out + acc[:, lane]
    return out


def normal_sums(P, sub, sel, K, defect=None):
    """P [S,12], sub f32 [m,6], sel bool [S,m] -> (Hm [S,6,6] upper triangle filled, g [S,6]): the 21 + 6 sums of the header"""
    fx, fy, px, py = (D(F(v)) for v in K)
    r = sub.astype(D)
    o = (r[None, :, 3], r[None, :, 4], r[None, :, 5])
    Pb = P[:, None, :]
    with np.errstate(all="ignore"):
        y = [(Pb[..., 4 * i] * o[0] + Pb[..., 4 * i + 1] * o[1]) + Pb[..., 4 * i + 2] * o[2] for i in range(3)]
        qx, qy, qz = y[0] + Pb[..., 3], y[1] + Pb[..., 7], y[2] + Pb[..., 11]
        ru = (fx * qx / qz + px) - r[None, :, 0]
        rv = (fy * qy / qz + py) - r[None, :, 1]
        iz = 1.0 / qz
        a, b = fx * iz, fy * iz
        c, d = -(fx * qx * iz * iz), -(fy * qy * iz * iz)
        zero = np.zeros_like(a)
        Ju = [c * y[1], a * y[2] - c * y[0], -(a * y[1]), a, zero, c]
        Jv = [d * y[1] - b * y[2], -(d * y[0]), b * y[0], zero, b, d]
        S = P.shape[0]
        Hm, g = np.zeros((S, 6, 6)), np.zeros((S, 6))
        for i in range(6):
            for jj in range(i, 6):
                Hm[:, i, jj] = _fold(np.where(sel, Ju[i] * Ju[jj] + Jv[i] * Jv[jj], 0.0), defect)
            g[:, i] = _fold(np.where(sel, Ju[i] * ru + Jv[i] * rv, 0.0), defect)
    return Hm, g


def cholesky_solve(Hm, g):
    """Hm [S,6,6] (upper triangle read), g [S,6] -> (x [S,6] with Hm x = -g, ok [S]): the header's written order"""
    S = Hm.shape[0]
    L = np.zeros((S, 6, 6))
    ok = np.ones(S, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = Hm[:, j, j]
            for k in range(j):
                d = d - L[:, j, k] * L[:, j, k]
            ok &= (d > 0.0) & (d - d == 0.0)
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                s = Hm[:, j, i]
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                L[:, i, j] = s / L[:, j, j]
        z = np.zeros((S, 6))
        for i in range(6):
            s = -g[:, i]
            for k in range(i):
                s = s - L[:, i, k] * z[:, k]
            z[:, i] = s / L[:, i, i]
        x = np.zeros((S, 6))
        for i in range(5, -1, -1):
            s = z[:, i]
            for k in range(i + 1, 6):
                s = s - L[:, k, i] * x[:, k]
            x[:, i] = s / L[:, i, i]
    return x, ok


def retract(P, x, defect=None):
    """t <- t + x[3:6]; R <- Q(dq) R with dq = (1, x[0:3] / 2) normalised"""
    with np.errstate(all="ignore"):
        k = 1.0 if defect == "half" else 0.5
        hx, hy, hz = k * x[:, 0], k * x[:, 1], k * x[:, 2]
        nrm = np.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
        w, xq, y, z = 1.0 / nrm, hx / nrm, hy / nrm, hz / nrm
        xx, yy, zz, xy, xz, yz, wx, wy, wz = xq * xq, y * y, z * z, xq * y, xq * z, y * z, w * xq, w * y, w * z
        Q = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
             [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
             [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
        out = np.zeros_like(P)
        for i in range(3):
            for j in range(3):
                out[:, 4 * i + j] = (Q[i][0] * P[:, j] + Q[i][1] * P[:, 4 + j]) + Q[i][2] * P[:, 8 + j]
            out[:, 4 * i + 3] = P[:, 4 * i + 3] + x[:, 3 + i]
    return out


def gauss_newton(P, sub, sel, K, defect=None, steps=GN_STEPS):
    """the refit of the header on a fixed selection; a failed solve or a non-finite pose leaves P as it was"""
    cur, good = P.copy(), np.ones(P.shape[0], bool)
    for _ in range(steps):
        Hm, g = normal_sums(cur, sub, sel, K, defect)
        x, ok = cholesky_solve(Hm, g)
        cur = retract(cur, x, defect)
        good &= ok & np.isfinite(cur).all(axis=1)
    return np.where(good[:, None], cur, P)


# ---- one round ------------------------------------------------------------------------------------------------------------
def class_round(rec, ids, poses, rnd, K, pixel_batch=1000, max_pixels=1000, inlier_threshold=10.0, defect=None, **_):
    """One round for one class (see pose3d_ref.class_round): the inlier test is REPROJ, the refit Gauss-Newton"""
    thr = D(F(inlier_threshold))
    n = rec.shape[0]
    ids, poses = np.asarray(ids, dtype=np.int64), np.asarray(poses, dtype=D).reshape(-1, 12)
    m = min(n, pixel_batch * rnd)
    subset = stride_index(n, m) if m > 0 else np.zeros(0, np.int64)
    sub = rec[subset]
    res, front = reproj(poses, sub, K)
    mask = front & ((res <= thr) if defect == "le" else (res < thr))
    inl = mask.sum(axis=1).astype(np.int64)
    size = len(ids)
    dropped_ids, dropped_inl = np.zeros(0, np.int64), np.zeros(0, np.int64)
    if size > 1:
        order = np.lexsort((ids, -inl))
        keep = size // 2
        dropped_ids, dropped_inl = ids[order[keep:]], inl[order[keep:]]
        order = order[:keep]
        ids, poses, inl, mask = ids[order], poses[order], inl[order], mask[order]
    new = poses.copy()
    refit = np.nonzero(inl >= 4)[0]
    if len(refit):
        sel = np.zeros((len(refit), m), bool)
        for a, s in enumerate(refit):
            where = np.nonzero(mask[s])[0]
            if len(where) >= max_pixels:
                where = where[stride_index(len(where), max_pixels)]
            sel[a, where] = True
        new[refit] = gauss_newton(poses[refit], sub, sel, K, defect)
    return dict(ids=ids, poses=new, inliers=inl, dropped_ids=dropped_ids, dropped_inliers=dropped_inl, masks=mask, subset=subset)


def round_fwd(records, counts, offsets, hyp_pose, hyp_class, rnd, K, **kw):
    """ops.pose2d_round for one frame -> pose_out [n,12], class_out, inliers_out"""
    C = len(counts)
    hyp_pose = np.asarray(hyp_pose, dtype=D).reshape(-1, 12)
    pose_out, class_out, inl_out = hyp_pose.copy(), np.zeros(len(hyp_class), np.int32), np.zeros(len(hyp_class), np.int32)
    for c in range(1, C):
        ids = np.nonzero(np.asarray(hyp_class) == c)[0]
        if len(ids) == 0:
            continue
        rec = records[offsets[c]:offsets[c] + counts[c]]
        r = class_round(rec, ids, hyp_pose[ids], rnd, K, **kw)
        pose_out[r["ids"]], class_out[r["ids"]], inl_out[r["ids"]] = r["poses"], c, r["inliers"]
        inl_out[r["dropped_ids"]] = r["dropped_inliers"]
    return pose_out, class_out, inl_out


# ---- the whole loop -------------------------------------------------------------------------------------------------------
def estimate(label, vertex_pred, extents, K, stream=0, seed=0, defect=None, trace=None, **kw):
    """One frame -> dict(poses64 [C,12], poses32, inliers, ref_steps, num_hyps [C]); `trace` (a dict) receives, per class, the
    last round's result of `class_round` and under "sizes" the halving the loop ran"""
    p = dict(DEFAULTS)
    p.update(kw)
    H, W = label.shape
    C = extents.shape[0]
    records, counts, offsets = prepare(label, vertex_pred, extents)
    pose, cls, _, _ = sample(records, counts, offsets, extents, K, H, W, stream, seed, defect=defect, **p)
    out = dict(poses64=np.zeros((C, 12), D), inliers=np.zeros(C, np.int32), ref_steps=np.zeros(C, np.int32),
               num_hyps=np.zeros(C, np.int32))
    for c in range(1, C):
        ids = np.nonzero(cls == c)[0]
        if len(ids) == 0:
            continue
        rec = records[offsets[c]:offsets[c] + counts[c]]
        poses, inl, rnd, ref_steps, last = pose[ids], np.zeros(1, np.int64), 0, 0, None
        for before, after in halving_schedule(len(ids), p["ref_it"]):
            rnd += 1
            last = class_round(rec, ids, poses, rnd, K, p["pixel_batch"], p["max_pixels"], p["inlier_threshold"], defect)
            ids, poses, inl = last["ids"], last["poses"], last["inliers"]
            ref_steps += 1
            assert len(ids) == after
            if trace is not None:
                trace.setdefault("sizes", {}).setdefault(c, []).append((before, len(ids)))
        out["poses64"][c], out["inliers"][c], out["ref_steps"][c], out["num_hyps"][c] = poses[0], inl[0], ref_steps, (cls == c).sum()
        if trace is not None:
            trace[c] = last
    out["poses32"] = out["poses64"].astype(F)
    return out
