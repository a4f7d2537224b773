"""numpy restatement of include/posecnn_hip_pose3d.h (TEST INFRASTRUCTURE, the statement of record of the 3-D vertex route's
pose stage): prepare, sample, one preemptive round, the whole loop. Every step is the header's f32 / f64 operation in the
header's order (numpy's elementwise +, -, *, /, sqrt round once and never fuse), so the GPU results are compared bit for bit.

`defect=` plants one of five seeded mistakes (tests/test_pose3d_cpu.py shows that each is caught):
  "chan"    object coordinates read from channels 3 (c - 1) instead of 3 c
  "le"      residual <= threshold counts as an inlier
  "ceil"    the halving keeps ceil(size / 2)
  "stride"  the subset / thinning index is floor((k + 1) n / m), clipped, instead of floor(k n / m)
  "eig"     the quaternion is the eigenvector of the largest |eigenvalue| (no handling of the reflection-like solution)
"""
import numpy as np

from augment_ref import philox4x64

F, D = np.float32, np.float64
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
DEFAULTS = dict(hypotheses=256, pixel_batch=1000, max_pixels=1000, ref_it=8, min_area=400, inlier_threshold=0.01,
                min_dist=0.01, max_attempts=1024)


# ---- indices ------------------------------------------------------------------------------------------------------------
def stride_index(count, m, defect=None):
    """floor(k count / m), k = 0 .. m - 1: the round's subset (count = n) and the thinning (count = cnt, m = max_pixels)"""
    k = np.arange(m, dtype=np.int64)
    if defect == "stride":
        return np.minimum((k + 1) * count // m, count - 1)
    return k * count // m


def philox_index(word, n):
    """((word >> 32) n) >> 32 for uint64 words"""
    return ((np.asarray(word, dtype=np.uint64) >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)


def halving_schedule(size, ref_it):
    """[(size before the round's halving, size after)], one entry per round of the loop"""
    out, ref_steps = [], 0
    while size > 1 or ref_steps < ref_it:
        after = size // 2 if size > 1 else size
        out.append((size, after))
        size, ref_steps = after, ref_steps + 1
    return out


# ---- prepare ------------------------------------------------------------------------------------------------------------
def prepare(label, depth, vertex_pred, extents, K, factor, defect=None):
    """One frame: label int [H,W], depth uint16 [H,W], vertex_pred f32 [H,W,3C], extents f32 [C,3], K = (fx, fy, px, py).
    -> records f32 [total,6], counts int32 [C], offsets int32 [C]"""
    H, W = label.shape
    C = extents.shape[0]
    lab = np.asarray(label).reshape(-1).astype(np.int64)
    dep = np.asarray(depth).reshape(-1)
    vp = np.asarray(vertex_pred, dtype=F).reshape(H * W, 3 * C)
    ext = np.asarray(extents, dtype=F)
    fx, fy, px, py = (F(v) for v in K)
    factor = F(factor)
    counts, offsets, recs = np.zeros(C, np.int32), np.zeros(C, np.int32), []
    off = 0
    with np.errstate(all="ignore"):
        for c in range(C):
            offsets[c] = off
            if c == 0:
                continue
            p = np.nonzero(lab == c)[0]
            counts[c] = len(p)
            off += len(p)
            d = dep[p].astype(F)
            x, y = (p % W).astype(F), (p // W).astype(F)
            hole = dep[p] == 0
            ex = np.where(hole, F(0), (x - px) * d / fx / factor).astype(F)
            ey = np.where(hole, F(0), (y - py) * d / fy / factor).astype(F)
            ez = np.where(hole, F(0), d / factor).astype(F)
            ch = 3 * (c - 1) if defect == "chan" else 3 * c
            obj = []
            for i in range(3):
                e = ext[c, i]
                vmin, vmax = F(-e) / F(2), e / F(2)
                span = F(vmax - vmin)
                a = F(D(1.0) / D(span))
                b = F(D(-1.0) * D(vmin) / D(span))
                obj.append(((vp[p, ch + i] - b) / a).astype(F))
            recs.append(np.stack([ex, ey, ez] + obj, axis=1))
    records = np.concatenate(recs, axis=0) if recs else np.zeros((0, 6), F)
    return records.astype(F), counts, offsets


# ---- Kabsch (Horn's quaternion form) ----------------------------------------------------------------------------------------
def fit(Sa, Sb, Sab, n, defect=None):
    """Sa, Sb [S,3], Sab [S,3,3] (a = obj, b = eye) f64, n int or [S] -> P [S,12] (row-major 3 x 4 R|t)"""
    Sa, Sb, Sab = (np.asarray(v, dtype=D) for v in (Sa, Sb, Sab))
    S = Sa.shape[0]
    dn = np.broadcast_to(np.asarray(n, dtype=D), (S,))
    with np.errstate(all="ignore"):
        cA = [Sa[:, i] / dn for i in range(3)]
        cB = [Sb[:, i] / dn for i in range(3)]
        M = [[Sab[:, i, j] - Sa[:, i] * cB[j] for j in range(3)] for i in range(3)]
        (Mxx, Mxy, Mxz), (Myx, Myy, Myz), (Mzx, Mzy, Mzz) = M
        A = [[None] * 4 for _ in range(4)]
        A[0][0] = (Mxx + Myy) + Mzz
        A[1][1] = (Mxx - Myy) - Mzz
        A[2][2] = (Myy - Mxx) - Mzz
        A[3][3] = (Mzz - Mxx) - Myy
        A[0][1] = A[1][0] = Myz - Mzy
        A[0][2] = A[2][0] = Mzx - Mxz
        A[0][3] = A[3][0] = Mxy - Myx
        A[1][2] = A[2][1] = Mxy + Myx
        A[1][3] = A[3][1] = Mzx + Mxz
        A[2][3] = A[3][2] = Myz + Mzy
        V = [[np.full(S, 1.0 if i == j else 0.0) for j in range(4)] for i in range(4)]
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                apq = A[p][q]
                nz = apq != 0.0
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(nz, t, 0.0)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):
                    x, y = A[k][p], A[k][q]
                    A[k][p], A[k][q] = c * x - s * y, s * x + c * y
                for k in range(4):
                    x, y = A[p][k], A[q][k]
                    A[p][k], A[q][k] = c * x - s * y, s * x + c * y
                for k in range(4):
                    x, y = V[k][p], V[k][q]
                    V[k][p], V[k][q] = c * x - s * y, s * x + c * y
        key = (lambda v: np.abs(v)) if defect == "eig" else (lambda v: v)
        best = key(A[0][0])
        q4 = [V[k][0] for k in range(4)]
        for i in range(1, 4):
            better = key(A[i][i]) > best
            best = np.where(better, key(A[i][i]), best)
            q4 = [np.where(better, V[k][i], q4[k]) for k in range(4)]
        qw, qx, qy, qz = q4
        nrm = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
        w, x, y, z = qw / nrm, qx / nrm, qy / nrm, qz / nrm
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        P = np.zeros((S, 12), D)
        P[:, 0], P[:, 1], P[:, 2] = 1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)
        P[:, 4], P[:, 5], P[:, 6] = 2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)
        P[:, 8], P[:, 9], P[:, 10] = 2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)
        for i in range(3):
            P[:, 4 * i + 3] = cB[i] - ((P[:, 4 * i] * cA[0] + P[:, 4 * i + 1] * cA[1]) + P[:, 4 * i + 2] * cA[2])
    return P


def sums_in_order(obj, eye):
    """obj, eye [S,k,3] f32 -> (Sa, Sb, Sab) adding the k pairs in order onto +0 (the sampler's order)"""
    o, e = obj.astype(D), eye.astype(D)
    S, k = o.shape[:2]
    Sa, Sb, Sab = np.zeros((S, 3)), np.zeros((S, 3)), np.zeros((S, 3, 3))
    for i in range(k):
        Sa = Sa + o[:, i]
        Sb = Sb + e[:, i]
        Sab = Sab + o[:, i, :, None] * e[:, i, None, :]
    return Sa, Sb, Sab


def fit_points(obj, eye, defect=None):
    """Kabsch of k pairs in the sampler's sum order: obj, eye [k,3] -> P [12]"""
    return fit(*sums_in_order(np.asarray(obj, F)[None], np.asarray(eye, F)[None]), np.asarray(obj).shape[0], defect)[0]


def residual(P, rec):
    """P [S,12] f64, rec [m,6] f32 -> [S,m] f64"""
    r = rec.astype(D)
    ox, oy, oz = r[None, :, 3], r[None, :, 4], r[None, :, 5]
    d = []
    for i in range(3):
        q = ((P[:, 4 * i, None] * ox + P[:, 4 * i + 1, None] * oy) + P[:, 4 * i + 2, None] * oz) + P[:, 4 * i + 3, None]
        d.append(r[None, :, i] - q)
    with np.errstate(all="ignore"):
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def residual_own(P, rec):
    """P [S,12], rec [S,6]: each pose on its own record -> [S]"""
    r = rec.astype(D)
    d = [r[:, i] - (((P[:, 4 * i] * r[:, 3] + P[:, 4 * i + 1] * r[:, 4]) + P[:, 4 * i + 2] * r[:, 5]) + P[:, 4 * i + 3])
         for i in range(3)]
    with np.errstate(all="ignore"):
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def dist(a, b):
    """f32 differences, widened: [S,3] x [S,3] -> [S] f64"""
    dd = (a.astype(F) - b.astype(F)).astype(D)
    return np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])


def box_ok(P, ext, K, H, W, min_area):
    """P [S,12], ext f32 [S,3] -> bool [S]"""
    S = P.shape[0]
    h = [(ext[:, i].astype(F) * F(0.5)).astype(D) for i in range(3)]
    fx, fy, px, py = (D(F(v)) for v in K)
    ok = np.ones(S, bool)
    mn = [np.full(S, W - 1, np.int64), np.full(S, H - 1, np.int64)]
    mx = [np.zeros(S, np.int64), np.zeros(S, np.int64)]
    with np.errstate(all="ignore"):
        for j in range(8):
            cx, cy, cz = (-h[0] if j & 1 else h[0]), (-h[1] if j & 2 else h[1]), (-h[2] if j & 4 else h[2])
            q = [((P[:, 4 * i] * cx + P[:, 4 * i + 1] * cy) + P[:, 4 * i + 2] * cz) + P[:, 4 * i + 3] for i in range(3)]
            ok &= q[2] > 0.0
            for a, (f, p0, lim) in enumerate(((fx, px, W - 1), (fy, py, H - 1))):
                u = f * q[a] / q[2] + p0
                u = np.where(u >= 0.0, u, 0.0)
                u = np.where(u <= D(lim), u, D(lim))
                iu = u.astype(np.int64)
                mn[a] = np.minimum(mn[a], iu)
                mx[a] = np.maximum(mx[a], iu)
    return ok & ((mx[0] - mn[0] + 1) * (mx[1] - mn[1] + 1) >= min_area)


# ---- sample -------------------------------------------------------------------------------------------------------------
def sample(records, counts, offsets, extents, K, H, W, stream=0, seed=0, hypotheses=256, max_attempts=1024, min_area=400,
           inlier_threshold=0.01, min_dist=0.01, defect=None, **_):
    """One frame -> hyp_pose f64 [hyp,12], hyp_class, hyp_attempt int32 [hyp], hyp_rec int32 [hyp,3]"""
    C = len(counts)
    thr, md = D(F(inlier_threshold)), D(F(min_dist))
    ext = np.asarray(extents, dtype=F)
    live = np.array([c for c in range(1, C) if counts[c] > min_area], dtype=np.int64)
    pose = np.zeros((hypotheses, 12), D)
    cls = np.zeros(hypotheses, np.int32)
    att = np.full(hypotheses, -1, np.int32)
    rec3 = np.full((hypotheses, 3), -1, np.int32)
    pending = np.arange(hypotheses)
    key = (seed & ((1 << 64) - 1), seed >> 64)
    for a in range(max_attempts):
        if len(pending) == 0 or len(live) == 0:
            break
        w = philox4x64((a, int(stream), pending.astype(np.uint64), 0), key)
        c = live[philox_index(w[:, 0], len(live)).astype(np.int64)]
        n = counts[c].astype(np.uint64)
        j = np.stack([(((w[:, 1 + i] >> np.uint64(32)) * n) >> np.uint64(32)).astype(np.int64) for i in range(3)], axis=1)
        r = records[offsets[c].astype(np.int64)[:, None] + j]                       # [S,3,6]
        ok = np.ones(len(pending), bool)
        for i in range(3):
            ok &= (r[:, i, 2] != 0) & ~((r[:, i, 3] == 0) & (r[:, i, 4] == 0) & (r[:, i, 5] == 0))
            for k in range(i):
                ok &= ~(dist(r[:, k, :3], r[:, i, :3]) < md) & ~(dist(r[:, k, 3:], r[:, i, 3:]) < md)
        P = fit(*sums_in_order(r[:, :, 3:], r[:, :, :3]), 3, defect)
        for i in range(3):
            ok &= residual_own(P, r[:, i]) < thr
        ok &= box_ok(P, ext[c], K, H, W, min_area)
        done = pending[ok]
        pose[done], cls[done], att[done], rec3[done] = P[ok], c[ok], a, j[ok]
        pending = pending[~ok]
    return pose, cls, att, rec3


# ---- one round ------------------------------------------------------------------------------------------------------------
def _fold(vals):
    """vals [S,m] f64 -> [S]: lane k mod 64 adds its values in ascending k onto +0, then the xor butterfly 32 .. 1"""
    S, m = vals.shape
    J = (m + 63) // 64
    pad = np.zeros((S, J * 64), D)
    pad[:, :m] = vals
    pad = pad.reshape(S, J, 64)
    acc = np.zeros((S, 64), D)
    for jj in range(J):
        acc = acc + pad[:, jj]
    lanes = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ s]
    return acc[:, 0]


def class_round(rec, ids, poses, rnd, pixel_batch=1000, max_pixels=1000, inlier_threshold=0.01, defect=None, **_):
    """One round for one class: rec f32 [n,6] its records, ids int [S] ascending hypothesis indices, poses f64 [S,12].
    -> dict(ids, poses, inliers: the survivors in rank order; dropped_ids, dropped_inliers; masks: bool [survivors, m] the
    inlier set of each survivor within the subset; subset: the record indices)"""
    thr = D(F(inlier_threshold))
    n = rec.shape[0]
    ids, poses = np.asarray(ids, dtype=np.int64), np.asarray(poses, dtype=D).reshape(-1, 12)
    m = min(n, pixel_batch * rnd)
    subset = stride_index(n, m, defect) if m > 0 else np.zeros(0, np.int64)
    sub = rec[subset]
    res = residual(poses, sub)
    mask = (sub[None, :, 2] != 0) & ((res <= thr) if defect == "le" else (res < thr))
    inl = mask.sum(axis=1).astype(np.int64)
    size = len(ids)
    dropped_ids, dropped_inl = np.zeros(0, np.int64), np.zeros(0, np.int64)
    if size > 1:
        order = np.lexsort((ids, -inl))                                           # inliers descending, then index ascending
        keep = (size + 1) // 2 if defect == "ceil" else size // 2
        dropped_ids, dropped_inl = ids[order[keep:]], inl[order[keep:]]
        order = order[:keep]
        ids, poses, inl, mask = ids[order], poses[order], inl[order], mask[order]
    new = poses.copy()
    refit = np.nonzero(inl >= 4)[0]
    if len(refit):
        sel = np.zeros((len(refit), m), bool)
        nfit = np.zeros(len(refit), np.int64)
        for a, s in enumerate(refit):
            where = np.nonzero(mask[s])[0]
            cnt = len(where)
            if cnt >= max_pixels:
                where = where[stride_index(cnt, max_pixels, defect)]
            sel[a, where] = True
            nfit[a] = min(cnt, max_pixels)
        o, e = sub[:, 3:].astype(D), sub[:, :3].astype(D)
        Sa = np.stack([_fold(np.where(sel, o[None, :, i], 0.0)) for i in range(3)], axis=1)
        Sb = np.stack([_fold(np.where(sel, e[None, :, i], 0.0)) for i in range(3)], axis=1)
        Sab = np.stack([np.stack([_fold(np.where(sel, (o[:, i] * e[:, j])[None], 0.0)) for j in range(3)], axis=1)
                        for i in range(3)], axis=1)
        new[refit] = fit(Sa, Sb, Sab, nfit, defect)
    return dict(ids=ids, poses=new, inliers=inl, dropped_ids=dropped_ids, dropped_inliers=dropped_inl, masks=mask, subset=subset)


def round_fwd(records, counts, offsets, hyp_pose, hyp_class, rnd, **kw):
    """ops.pose3d_round for one frame -> pose_out [n,12], class_out, inliers_out"""
    C = len(counts)
    hyp_pose = np.asarray(hyp_pose, dtype=D).reshape(-1, 12)
    pose_out, class_out, inl_out = hyp_pose.copy(), np.zeros(len(hyp_class), np.int32), np.zeros(len(hyp_class), np.int32)
    for c in range(1, C):
        ids = np.nonzero(np.asarray(hyp_class) == c)[0]
        if len(ids) == 0:
            continue
        rec = records[offsets[c]:offsets[c] + counts[c]]
        r = class_round(rec, ids, hyp_pose[ids], rnd, **kw)
        pose_out[r["ids"]], class_out[r["ids"]], inl_out[r["ids"]] = r["poses"], c, r["inliers"]
        inl_out[r["dropped_ids"]] = r["dropped_inliers"]
    return pose_out, class_out, inl_out


# ---- the whole loop -------------------------------------------------------------------------------------------------------
def estimate(label, depth, vertex_pred, extents, K, factor, stream=0, seed=0, defect=None, trace=None, **kw):
    """One frame -> dict(poses64 [C,12], poses32, inliers, ref_steps, num_hyps [C]); `trace` (a dict) receives, per class, the
    last round's result of `class_round`"""
    p = dict(DEFAULTS)
    p.update(kw)
    H, W = label.shape
    C = extents.shape[0]
    records, counts, offsets = prepare(label, depth, vertex_pred, extents, K, factor, defect)
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
            last = class_round(rec, ids, poses, rnd, p["pixel_batch"], p["max_pixels"], p["inlier_threshold"], defect)
            ids, poses, inl = last["ids"], last["poses"], last["inliers"]
            ref_steps += 1
            if defect != "ceil":
                assert len(ids) == after
            if trace is not None:
                trace.setdefault("sizes", {}).setdefault(c, []).append((before, len(ids)))
        out["poses64"][c], out["inliers"][c], out["ref_steps"][c], out["num_hyps"][c] = poses[0], inl[0], ref_steps, (cls == c).sum()
        if trace is not None:
            trace[c] = last
    out["poses32"] = out["poses64"].astype(F)
    return out
