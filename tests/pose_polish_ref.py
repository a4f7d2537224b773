"""numpy restatement of include/posecnn_hip/pose_polish.h (TEST INFRASTRUCTURE, the statement of record of the Nelder-Mead
polish that ends both pose routes of the 3-D vertex route): the list, the gate, the retraction, the energy and the optimiser.
Every step is the header's f64 operation in the header's order (Python floats and numpy's elementwise +, -, *, /, sqrt round
once and never fuse), so the GPU results are compared bit for bit. RESIDUAL, REPROJ, the retraction, the lane fold and the
thinning index are the routes' own (tests/pose3d_ref.py, tests/pose2d_ref.py), imported.

`defect=` plants one of five seeded mistakes (tests/test_pose_polish_cpu.py shows that each is caught):
  "fold"    the 64 lane sums of the energy are added in lane order instead of by the xor butterfly
  "clamp"   a trial point is not clamped into the box
  "gate"    a class is polished when gate >= min_pixels
  "thin"    the thinning index is floor((j + 1) cnt / max_pixels), clipped, instead of floor(j cnt / max_pixels)
  "gamma"   the expansion coefficient is 1.5 instead of 2
"""
import numpy as np

import pose2d_ref as R2
import pose3d_ref as R3

F, D = np.float32, np.float64
N = 6
BOX = (0.17453292519943295, 0.17453292519943295, 0.17453292519943295, 0.1, 0.1, 0.5)
LB, UB = tuple(-r for r in BOX), BOX
LDS_RECORDS = 1024
MAX_EVALUATIONS = 4096
THRESHOLD = {0: 0.01, 1: 10.0}        # the routes' own defaults
INF = float("inf")


# ---- the list -------------------------------------------------------------------------------------------------------------
def inlier_mask(route, P0, rec, K, inlier_threshold):
    """the route's inlier test of every record under P0 [12]: -> bool [n]"""
    thr = D(F(inlier_threshold))
    P0 = np.asarray(P0, dtype=D).reshape(1, 12)
    if len(rec) == 0:
        return np.zeros(0, bool)
    if route == 0:
        return (rec[:, 2] != 0) & (R3.residual(P0, rec)[0] < thr)
    d, front = R2.reproj(P0, rec, K)
    return front[0] & (d[0] < thr)


def list_indices(route, P0, rec, K, max_pixels, inlier_threshold, defect=None):
    """-> (the record indices of the list in list order, cnt = the inliers before thinning)"""
    where = np.nonzero(inlier_mask(route, P0, rec, K, inlier_threshold))[0]
    cnt = len(where)
    if cnt >= max_pixels:
        where = where[R3.stride_index(cnt, max_pixels, "stride" if defect == "thin" else None)]
    return where, cnt


# ---- the energy -----------------------------------------------------------------------------------------------------------
def pose_of(P0, x):
    """P(x) of the header: [12]"""
    return R2.retract(np.asarray(P0, dtype=D).reshape(1, 12), np.asarray(x, dtype=D).reshape(1, 6))[0]


def distances(route, P, lst, K):
    """-> (d [L] f64, valid [L] bool) of the listed records under P [12]"""
    P = np.asarray(P, dtype=D).reshape(1, 12)
    if route == 0:
        return R3.residual(P, lst)[0], np.ones(len(lst), bool)
    d, front = R2.reproj(P, lst, K)
    return d[0], front[0]


def energy(route, P0, x, lst, K, defect=None):
    """E(x) of the header over the list `lst` f32 [L,6], L > 0: a Python float, +inf for an invalid or non-finite value"""
    with np.errstate(all="ignore"):
        d, valid = distances(route, pose_of(P0, x), lst, K)
        e = R2._fold(d[None, :], "fold" if defect == "fold" else None)[0] / D(len(lst))
    if not valid.all() or not np.isfinite(e):
        return INF
    return float(e)


# ---- the optimiser --------------------------------------------------------------------------------------------------------
def nelder_mead(fn, lb, ub, evaluations, x0=None, defect=None, trace=None):
    """The header's OPTIMISER on any objective `fn(list of n floats) -> float`, n = len(lb), evaluations >= n + 1.
    -> (x of the best vertex, its f, f of x0, evaluations made). `trace` (a list) receives one (kind, x, f) per evaluation,
    kind in init / reflect / expand / outside / inside / shrink, and ("cut", k) when the budget ends a shrink before vertex k."""
    n = len(lb)
    x0 = [0.0] * n if x0 is None else [float(v) for v in x0]
    gamma = 1.5 if defect == "gamma" else 2.0
    V, f, evals = [], [], 0

    def E(x, kind):
        nonlocal evals
        v = fn(x)
        evals += 1
        if trace is not None:
            trace.append((kind, list(x), v))
        return v

    for k in range(n + 1):
        v = list(x0)
        if k > 0:
            v[k - 1] = x0[k - 1] + (ub[k - 1] - lb[k - 1]) * 0.25
        V.append(v)
        f.append(E(v, "init"))
    f_start = f[0]
    while evals < evaluations:
        lo, hi, nh = 0, 0, -1
        for k in range(1, n + 1):
            if f[k] < f[lo]:
                lo = k
            if f[k] >= f[hi]:
                hi = k
        for k in range(n + 1):
            if k != hi and (nh < 0 or f[k] >= f[nh]):
                nh = k
        flo, fhi, fnh = f[lo], f[hi], f[nh]
        c = []
        for i in range(n):
            s = 0.0
            for k in range(n + 1):
                if k != hi:
                    s = s + V[k][i]
            c.append(s / float(n))

        def point(coef):
            out = []
            for i in range(n):
                v = c[i] + coef * (c[i] - V[hi][i])
                if defect != "clamp":
                    if v < lb[i]:
                        v = lb[i]
                    if v > ub[i]:
                        v = ub[i]
                out.append(v)
            return out

        xr = point(1.0)
        fr = E(xr, "reflect")
        if fr < flo:
            if evals < evaluations:
                xe = point(gamma)
                fe = E(xe, "expand")
                V[hi], f[hi] = (xe, fe) if fe < fr else (xr, fr)
            else:
                V[hi], f[hi] = xr, fr
        elif fr < fnh:
            V[hi], f[hi] = xr, fr
        else:
            if evals >= evaluations:
                if fr < fhi:
                    V[hi], f[hi] = xr, fr
                break
            xc = point(0.5 if fr < fhi else -0.5)
            fc = E(xc, "outside" if fr < fhi else "inside")
            fref = fr if fr < fhi else fhi
            if fc < fref:
                V[hi], f[hi] = xc, fc
            else:
                for k in range(n + 1):
                    if k == lo:
                        continue
                    if evals >= evaluations:
                        if trace is not None:
                            trace.append(("cut", k))
                        break
                    V[k] = [V[lo][i] + 0.5 * (V[k][i] - V[lo][i]) for i in range(n)]
                    f[k] = E(V[k], "shrink")
    lo = 0
    for k in range(1, n + 1):
        if f[k] < f[lo]:
            lo = k
    return V[lo], f[lo], f_start, evals


# ---- one class, one frame -------------------------------------------------------------------------------------------------
def polish_class(route, rec, P0, gate, K=None, max_pixels=1000, min_pixels=10, evaluations=100, inlier_threshold=None, defect=None,
                 trace=None):
    """rec f32 [n,6] the class's records, P0 [12] -> dict(pose [12] f64, energy [2] f64, evals, listed); `trace` (a dict)
    receives cnt, the list's record indices and the optimiser's evaluations"""
    thr = THRESHOLD[route] if inlier_threshold is None else inlier_threshold
    P0 = np.asarray(P0, dtype=D).reshape(12)
    out = dict(pose=P0.copy(), energy=np.zeros(2, D), evals=0, listed=0)
    passes = gate >= min_pixels if defect == "gate" else gate > min_pixels
    if evaluations < N + 1 or not passes:
        return out
    where, cnt = list_indices(route, P0, rec, K, max_pixels, thr, defect)
    if len(where) == 0:
        return out
    lst = rec[where]
    steps = [] if trace is not None else None
    xb, fb, f0, evals = nelder_mead(lambda x: energy(route, P0, x, lst, K, defect), LB, UB, evaluations, defect=defect, trace=steps)
    if trace is not None:
        trace.update(cnt=cnt, where=where, steps=steps, x=xb)
    return dict(pose=pose_of(P0, xb), energy=np.array([f0, fb], D), evals=evals, listed=len(lst))


def polish(route, records, counts, offsets, poses, gate, K=None, defect=None, trace=None, **kw):
    """ops.pose_polish for one frame: records f32 [total,6], counts, offsets, gate int [C], poses f64 [C,12] (or [C,3,4])
    -> dict(poses64 [C,12], poses32, energy [C,2], evals, listed [C]); `trace` (a dict) receives one dict per class"""
    C = len(counts)
    poses = np.asarray(poses, dtype=D).reshape(C, 12)
    out = dict(poses64=poses.copy(), energy=np.zeros((C, 2), D), evals=np.zeros(C, np.int32), listed=np.zeros(C, np.int32))
    for c in range(1, C):
        tr = {} if trace is not None else None
        r = polish_class(route, records[offsets[c]:offsets[c] + counts[c]], poses[c], int(gate[c]), K, defect=defect, trace=tr, **kw)
        out["poses64"][c], out["energy"][c], out["evals"][c], out["listed"][c] = r["pose"], r["energy"], r["evals"], r["listed"]
        if trace is not None:
            trace[c] = tr
    out["poses32"] = out["poses64"].astype(F)
    return out
