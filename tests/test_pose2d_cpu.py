"""The numpy restatement of the colour-only pose route (tests/pose2d_ref.py, the statement of record the GPU tests compare
bit for bit against) checked on the CPU: its random indices against numpy's Philox, its quartic roots against np.roots on the
quartics the planted scenes produce, its Gauss-Newton fixed point against scipy's least_squares, the round's rules on ties,
thinning, a small class and three inliers, the frame at the threshold, the planted scenes' recovered poses, and four seeded
defects that the comparisons of tests/test_gpu_pose2d.py would catch. No GPU."""
import functools

import numpy as np
import pytest

import pose2d_cases as CS
import pose2d_ref as R

F, D = np.float32, np.float64
SEED = (0x1234_5678_9ABC_DEF0 << 64) | 0x0FED_CBA9_8765_4321
EPS = np.finfo(D).eps

# Largest displacement of the 8 box corners between the recovered and the planted pose over the posed classes, per scene
# (seed, intrinsics) of scenes(), measured with this file's SEED (metres). Asserted at 10 x the recorded
# value: the slack covers the scene builder's normal() across numpy versions, nothing else — the code under test is held to
# the restatement bit for bit, not to this bound.
CORNER_DISPLACEMENT = {1: 9.319e-09, 2: 4.873e-08, 3: 2.005e-08}


@functools.lru_cache(maxsize=None)
def scenes():
    out = []
    for seed, K in zip((1, 2, 3), CS.INTRINSICS):
        f = CS.make_frame(seed, K)
        trace = {}
        est = R.estimate(f["label"], f["vertex_pred"], f["extents"], f["K"], stream=seed, seed=SEED, trace=trace, **CS.PARAMS)
        out.append((seed, f, est, trace))
    return out


@functools.lru_cache(maxsize=None)
def sampled(hypotheses=64):
    seed, f, _, _ = scenes()[0]
    rec, cnt, off = R.prepare(f["label"], f["vertex_pred"], f["extents"])
    trace = {}
    hyp = R.sample(rec, cnt, off, f["extents"], f["K"], CS.H, CS.W, 11, SEED, hypotheses=hypotheses, trace=trace, **CS.PARAMS)
    return f, rec, cnt, off, hyp, trace


# ---- random indices -------------------------------------------------------------------------------------------------------
def test_philox_indices_against_numpy():
    """the attempt's five indices: the class from the high half of word 0, records 0-2 from the high halves of words 1-3,
    record 3 from the LOW half of word 0"""
    f, rec, cnt, off, (pose, cls, att, rec4), _ = sampled()
    key = np.array([SEED & ((1 << 64) - 1), SEED >> 64], dtype=np.uint64)
    live = [c for c in range(1, CS.C) if cnt[c] > 400]
    checked = 0
    for h in np.nonzero(att > 0)[0][:8]:
        # np.random.Philox increments the counter before it generates: random_raw(4) of counter c is the block of c + 1
        words = np.random.Philox(counter=np.array([int(att[h]) - 1, 11, h, 0], dtype=np.uint64), key=key).random_raw(4)
        c = live[((int(words[0]) >> 32) * len(live)) >> 32]
        n = int(cnt[c])
        want = [((int(words[1 + i]) >> 32) * n) >> 32 for i in range(3)] + [((int(words[0]) & 0xFFFFFFFF) * n) >> 32]
        assert c == cls[h] and rec4[h].tolist() == want and all(0 <= v < n for v in want)
        checked += 1
    assert checked == 8


# ---- the quartic ----------------------------------------------------------------------------------------------------------
# A root's allowed backward error: the quartic's coefficients come from f32 object coordinates and are themselves uncertain by
# about 2^-24 relative; the solver may add a thousandth of that.
ROOT_BACKWARD_ERROR = 2.0 ** -34


def test_quartic_roots_against_numpy():
    """On the quartics of every accepted hypothesis of the three scenes. P3P quartics have clustered roots as a rule (root
    condition numbers of 1e5 and more; pairs that are double within the coefficients' rounding), so "the same root" is stated
    the way that survives ill-conditioning. (1) The chosen root v is an exact root of a quartic within ROOT_BACKWARD_ERROR of
    the given one: |f(v)| <= that x sum |A_i| |v|^i, f evaluated in long double. (2) np.roots has a root where that puts
    one: a polynomial of degree n has a root within n |f / f'| and within sqrt(n (n - 1) |f / f''|) of any point (Laguerre's
    bounds, in the complex plane), with |f| at its allowance; twice that radius, for np.roots' own (much smaller) error."""
    LD = np.longdouble
    worst_be, worst_r, n = 0.0, 0.0, 0
    for seed, f, _, _ in scenes():
        rec, cnt, off = R.prepare(f["label"], f["vertex_pred"], f["extents"])
        trace = {}
        pose, cls, _, _ = R.sample(rec, cnt, off, f["extents"], f["K"], CS.H, CS.W, seed, SEED, trace=trace, **CS.PARAMS)
        assert (cls > 0).all()
        A, v = np.concatenate(trace["A"]), np.concatenate(trace["v"])
        assert len(v) == 256 and np.isfinite(v).all()
        for a, x in zip(A, v):
            al, t = a.astype(LD), LD(x)
            f0 = abs((((al[0] * t + al[1]) * t + al[2]) * t + al[3]) * t + al[4])
            f1 = abs(((4 * al[0] * t + 3 * al[1]) * t + 2 * al[2]) * t + al[3])
            f2 = abs((12 * al[0] * t + 6 * al[1]) * t + 2 * al[2])
            allow = ROOT_BACKWARD_ERROR * sum(abs(al[4 - i]) * abs(t) ** i for i in range(5))
            radius = float(min(4 * allow / f1, np.sqrt(12 * allow / f2)))
            be, d = float(f0 / allow), float(np.abs(np.roots(a) - x).min()) / (2 * radius)
            worst_be, worst_r, n = max(worst_be, be), max(worst_r, d), n + 1
            assert be <= 1.0 and d <= 1.0, (a, x, np.roots(a), be, d)
    print("quartic: %d accepted roots; worst backward error %.3g, worst distance to np.roots %.3g (of the allowances)" % (n, worst_be, worst_r))


def test_quartic_roots_of_known_polynomials():
    """four real roots, two real roots, none, and the biquadratic branch (no cubic term after the shift, q = 0)"""
    cases = [((1.0, -10.0, 35.0, -50.0, 24.0), (1, 2, 3, 4)), ((2.0, -6.0, 6.0, -6.0, 4.0), (1, 2)), ((1.0, 0.0, 5.0, 0.0, 4.0), ()),
             ((1.0, 0.0, -5.0, 0.0, 4.0), (-2, -1, 1, 2)), ((1.0, -4.0, 1.0, 6.0, 0.0), (-1, 0, 2, 3))]
    for a, want in cases:
        v = R.quartic_roots(*(np.array([c]) for c in a))[:, 0]
        got = sorted(v[np.isfinite(v)])
        assert len(got) == len(want) and np.allclose(got, want, atol=1e-9), (a, v)


# ---- the refit ------------------------------------------------------------------------------------------------------------
def test_gauss_newton_fixed_point_against_scipy():
    """class 2's planted inliers with 0.3 pixel of noise on the pixels, from a pose 1 cm and 2 degrees off: the restatement's
    refit iterated to its fixed point against scipy.optimize.least_squares (float64, rotation-vector increments, trust
    region) on the same pairs. Both stop at the same minimiser up to the f64 floor of the normal equations, about
    eps cond(H) ~ 1e-16 x 1e6 in the parameters; the corners may differ by 1e-8 m, a hundred times that floor."""
    from scipy.optimize import least_squares
    seed, f, _, _ = scenes()[0]
    rec, cnt, off = R.prepare(f["label"], f["vertex_pred"], f["extents"])
    r = rec[off[2]:off[2] + cnt[2]][f["inlier"][2]].copy()
    rng = np.random.RandomState(7)
    r[:, :2] += rng.normal(scale=0.3, size=(len(r), 2)).astype(F)
    Rm, t = f["poses"][2]

    def rot(v):
        th = np.linalg.norm(v)
        if th == 0:
            return np.eye(3)
        k = v / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx

    R0 = rot(np.deg2rad(2.0) * np.array([0.6, -0.64, 0.48])) @ Rm
    P0 = np.concatenate([R0, (t + [0.006, -0.006, 0.006])[:, None]], axis=1).reshape(1, 12)
    sel = np.ones((1, len(r)), bool)
    P = P0
    for _ in range(6):
        P = R.gauss_newton(P, r, sel, f["K"], steps=R.GN_STEPS)
    again = R.gauss_newton(P, r, sel, f["K"], steps=R.GN_STEPS)
    assert CS.corner_displacement(again[0], P[0, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(3, 3), P[0, [3, 7, 11]], f["extents"][2]) < 1e-12
    Rg = P[0].reshape(3, 4)[:, :3]
    assert np.abs(Rg @ Rg.T - np.eye(3)).max() < 1e-14                     # the retraction keeps R a rotation

    o, pix, K = r[:, 3:].astype(D), r[:, :2].astype(D), [D(F(v)) for v in f["K"]]

    def resid(x):
        q = o @ (rot(x[:3]) @ R0[:, :3]).T + (P0[0, [3, 7, 11]] + x[3:])
        return np.concatenate([K[0] * q[:, 0] / q[:, 2] + K[2] - pix[:, 0], K[1] * q[:, 1] / q[:, 2] + K[3] - pix[:, 1]])

    sol = least_squares(resid, np.zeros(6), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0)
    d = CS.corner_displacement(P[0], rot(sol.x[:3]) @ R0[:, :3], P0[0, [3, 7, 11]] + sol.x[3:], f["extents"][2])
    moved = CS.corner_displacement(P0[0], Rg, P[0, [3, 7, 11]], f["extents"][2])
    print("gauss-newton against least_squares: corners %.3e m apart (the start was %.3e m off)" % (d, moved))
    assert moved > 5e-3 and d < 1e-8
    # and PCNN_POSE2D_GN_STEPS = 2 steps from a hypothesis-quality start (the sampler's poses are ~1e-6 m off) are converged
    # to the same bound
    near = P.copy()
    near[0, 3] += 1e-5
    one = R.gauss_newton(near, r, sel, f["K"])
    assert CS.corner_displacement(one[0], Rg, P[0, [3, 7, 11]], f["extents"][2]) < 1e-8


def test_cholesky_refuses_what_it_cannot_solve():
    """a singular system (every record the same) and a non-finite one leave the pose as it was"""
    rec = np.zeros((6, 6), F)
    rec[:, :2], rec[:, 3:] = (3.0, 4.0), (0.1, 0.2, 0.0)
    P = CS.THRESHOLD_POSE[None].copy()
    sel = np.ones((1, 6), bool)
    assert (R.gauss_newton(P, rec, sel, (1.0, 1.0, 0.0, 0.0)) == P).all()
    rec2 = np.random.RandomState(0).uniform(-1, 1, size=(6, 6)).astype(F)
    rec2[0, 3] = np.inf
    assert (R.gauss_newton(P, rec2, sel, (1.0, 1.0, 0.0, 0.0)) == P).all()
    x, ok = R.cholesky_solve(np.diag([4.0, 9.0, 1.0, 1.0, 1.0, 16.0])[None], np.array([[4.0, 9.0, 1.0, 2.0, 3.0, 16.0]]))
    assert ok.all() and x[0].tolist() == [-1.0, -1.0, -1.0, -2.0, -3.0, -1.0]


# ---- the round ------------------------------------------------------------------------------------------------------------
def test_round_ties_and_thinning():
    """planted duplicates have equal counts and the lower index outranks the higher; with the whole class in the subset
    (round 3, m = n = 2500) the best hypothesis has more than max_pixels inliers and its refit reads exactly the ranks
    floor(j cnt / max_pixels)"""
    f, rec, cnt, off, (pose, cls, _, _), _ = sampled()
    pose = pose.copy()
    first = np.nonzero(cls == 1)[0]
    pose[first[1]], pose[first[2]] = pose[first[0]], pose[first[0]]
    ids = np.nonzero(cls == 1)[0]
    r1 = rec[off[1]:off[1] + cnt[1]]
    out = R.class_round(r1, ids, pose[ids], 1, f["K"], inlier_threshold=CS.INLIER_THRESHOLD)
    d, front = R.reproj(pose[ids], r1[out["subset"]], f["K"])
    inl = (front & (d < 1.0)).sum(axis=1)
    order = sorted(range(len(ids)), key=lambda i: (-inl[i], ids[i]))
    assert out["ids"].tolist() == [ids[i] for i in order[:len(ids) // 2]] and len(out["subset"]) == 1000
    assert inl[0] == inl[1] == inl[2]
    kept = [h in out["ids"] for h in first[:3]]
    assert kept == sorted(kept, reverse=True)                                # never a later duplicate without the earlier one
    out3 = R.class_round(r1, ids, pose[ids], 3, f["K"], inlier_threshold=CS.INLIER_THRESHOLD)
    assert len(out3["subset"]) == 2500 and out3["inliers"][0] > 1000
    where = np.nonzero(out3["masks"][0])[0]
    thin = where[[j * len(where) // 1000 for j in range(1000)]]
    sel = np.zeros((1, 2500), bool)
    sel[0, thin] = True
    before = pose[out3["ids"][:1]]
    assert (R.gauss_newton(before, r1, sel, f["K"]) == out3["poses"][:1]).all() and (out3["poses"][0] != before[0]).any()


def test_round_small_class_and_three_inliers():
    """a class smaller than one pixel_batch is its own subset from round 1 on; a survivor with 3 inliers is not refitted,
    one with 4 is"""
    f, rec, cnt, off, (pose, cls, _, _), _ = sampled()
    ids = np.nonzero(cls == 3)[0]
    r3 = rec[off[3]:off[3] + cnt[3]]
    out = R.class_round(r3, ids, pose[ids], 1, f["K"], inlier_threshold=CS.INLIER_THRESHOLD)
    assert out["subset"].tolist() == list(range(401))
    small = R.class_round(r3, ids, pose[ids], 2, f["K"], pixel_batch=128, inlier_threshold=CS.INLIER_THRESHOLD)
    assert small["subset"].tolist() == [k * 401 // 256 for k in range(256)]

    import test_gpu_pose2d as G
    records, counts, offsets, p, c, K = G.three_inlier_case()
    wp, wc, wi = R.round_fwd(records[0], counts[0], offsets[0], p[0], c[0], 1, K, inlier_threshold=1.0)
    assert wi.tolist() == [3, 4] and wc.tolist() == [1, 2]
    assert (wp[0] == p[0, 0]).all() and (wp[1] != p[0, 1]).any()
    better = R.reproj(wp[1:2], records[0, 40:90][[1, 9, 20, 41]], K)[0].max() < R.reproj(p[0, 1:2], records[0, 40:90][[1, 9, 20, 41]], K)[0].max()
    assert better


def test_threshold_frame():
    f = CS.threshold_frame()
    rec, cnt, off = R.prepare(f["label"], f["vertex_pred"], f["extents"])
    assert cnt.tolist() == [0, 4] and rec[:, :3].tolist() == [[1, 1, 0], [6, 2, 0], [4, 3, 0], [2, 4, 0]]
    assert rec[:, 3:].tolist() == [[2, 2, 0], [12, 4, 0], [9.5, 8, 0], [4, 8, 0]]
    d, front = R.reproj(CS.THRESHOLD_POSE[None], rec, f["K"])
    assert d[0].tolist() == [0.0, 0.0, 1.25, 0.0] and front.all() and D(F(CS.THRESHOLD)) == 1.25
    one = np.array([1], np.int32)
    ok = R.round_fwd(rec, cnt, off, CS.THRESHOLD_POSE[None], one, 1, f["K"], inlier_threshold=CS.THRESHOLD)
    assert ok[2].tolist() == [3] and ok[1].tolist() == [1] and (ok[0] == CS.THRESHOLD_POSE).all()
    # the three exact pairs alone: the Gauss-Newton increment is exactly zero
    Hm, g = R.normal_sums(CS.THRESHOLD_POSE[None], rec, np.array([[True, True, False, True]]), f["K"])
    assert not g.any()


# ---- the planted scenes ---------------------------------------------------------------------------------------------------
def test_scene_regimes():
    for seed, f, est, trace in scenes():
        rec, cnt, off = R.prepare(f["label"], f["vertex_pred"], f["extents"])
        assert cnt.tolist() == [0, 2500, 900, 401, 400, 448, 0]
        assert [c for c in range(1, CS.C) if cnt[c] > 400] == list(CS.LIVE)
        assert not rec[off[5]:off[5] + cnt[5], 3:].any() and not rec[:, 2].any()                    # class 5: every pixel empty
        k = f["kind"]
        assert (k == 1).sum() > 500 and ((k == 3) & (f["label"] != 5)).sum() > 50
        assert est["num_hyps"].sum() == 256 and (est["num_hyps"][list(CS.POSED)] > 0).all()
        assert not est["num_hyps"][[0, 4, 5, 6]].any() and not est["poses64"][[0, 4, 5, 6]].any()
        assert est["ref_steps"][list(CS.POSED)].tolist() == [8, 8, 8]
        for c in CS.POSED:
            last = trace[c]
            assert len(last["subset"]) == cnt[c]                                                  # the last round sees the class
            assert (last["masks"][0] == f["inlier"][c][last["subset"]]).all()                     # exactly the planted inliers
            assert est["inliers"][c] == f["inlier"][c].sum()
            assert trace["sizes"][c] == R.halving_schedule(int(est["num_hyps"][c]), 8)


def test_recovered_poses():
    for seed, f, est, _ in scenes():
        worst = max(CS.corner_displacement(est["poses64"][c], *f["poses"][c], f["extents"][c]) for c in CS.POSED)
        print("scene %d: corner displacement %.3e m" % (seed, worst))
        assert worst <= 10 * CORNER_DISPLACEMENT[seed]


def test_thirteen_hypotheses_reach_every_posed_class():
    import test_gpu_pose2d as G
    for (seed, f, _, _), gpu_stream in zip(scenes(), G.STREAMS):            # this file's streams and the GPU tests'
        for stream in (seed, gpu_stream):
            est = R.estimate(f["label"], f["vertex_pred"], f["extents"], f["K"], stream=stream, seed=SEED, hypotheses=13, **CS.PARAMS)
            assert est["num_hyps"].sum() == 13 and (est["num_hyps"][list(CS.POSED)] >= 1).all(), (seed, stream, est["num_hyps"])


# ---- seeded defects -------------------------------------------------------------------------------------------------------
def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape != b.shape or (a.view(np.uint8) != b.view(np.uint8)).any()


def test_seeded_defects_are_caught():
    """Each defect changes at least one array that tests/test_gpu_pose2d.py compares bit for bit (named here), on its own
    scenes and parameters."""
    import test_gpu_pose2d as G
    f, rec, cnt, off, (pose, cls, att, rec4), _ = sampled()
    # "le": inliers_out and pose_out of test_round_at_threshold
    t = CS.threshold_frame()
    trec, tcnt, toff = R.prepare(t["label"], t["vertex_pred"], t["extents"])
    one = np.array([1], np.int32)
    ok = R.round_fwd(trec, tcnt, toff, CS.THRESHOLD_POSE[None], one, 1, t["K"], inlier_threshold=CS.THRESHOLD)
    le = R.round_fwd(trec, tcnt, toff, CS.THRESHOLD_POSE[None], one, 1, t["K"], inlier_threshold=CS.THRESHOLD, defect="le")
    assert ok[2].tolist() == [3] and le[2].tolist() == [4] and (ok[0] == CS.THRESHOLD_POSE).all() and (le[0] != ok[0]).any()
    # "fourth": hyp_pose / hyp_attempt of test_sample — a P3P has up to four solutions and the first valid one is often wrong
    bad = R.sample(rec, cnt, off, f["extents"], f["K"], CS.H, CS.W, 11, SEED, hypotheses=64, defect="fourth", **CS.PARAMS)
    assert _bits_differ(bad[0], pose) or _bits_differ(bad[2], att)
    # "fold", "half": pose_out of the rounds of test_round_moved_poses
    # (test_round_moved_poses: on the sampler's own poses the increments are ~1e-9 and a changed sum order rounds away)
    moved = G.moved(pose)
    good = R.round_fwd(rec, cnt, off, moved, cls, 3, f["K"], inlier_threshold=CS.INLIER_THRESHOLD)
    for defect in ("fold", "half"):
        other = R.round_fwd(rec, cnt, off, moved, cls, 3, f["K"], inlier_threshold=CS.INLIER_THRESHOLD, defect=defect)
        assert (other[1] == good[1]).all() and (other[2] == good[2]).all() and _bits_differ(other[0], good[0]), defect
    # and the driver's poses64 (test_driver) differ for the two that change more than the last bits of a sum ("fold" is
    # caught by the rounds alone: on the planted scenes the loop's late increments are below the rounding of the pose)
    seed, fr, est, _ = scenes()[0]
    for defect in ("fourth", "half"):
        other = R.estimate(fr["label"], fr["vertex_pred"], fr["extents"], fr["K"], stream=seed, seed=SEED, defect=defect, **CS.PARAMS)
        assert _bits_differ(other["poses64"], est["poses64"]), defect


# ---- the host wrappers refuse what the header refuses, without a GPU ---------------------------------------------------------
def test_header_constants_are_the_restatements():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "posecnn_hip_pose2d.h")).read()
    for name, value in (("RECORD", R.RECORD), ("GN_STEPS", R.GN_STEPS), ("CUBIC_STEPS", R.CUBIC_STEPS), ("POLISH_STEPS", R.POLISH_STEPS)):
        assert int(re.search(r"#define PCNN_POSE2D_%s (\d+)" % name, header).group(1)) == value


def test_host_validation_needs_no_gpu():
    """argument errors are refused on the host before any launch: the C entries return EINVAL / ENULL with NULL pointers"""
    import ctypes
    from posecnn_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t()
    assert L.pcnn_pose2d_workspace_bytes(16, 480, 640, 22, 256, ctypes.byref(n)) == _lib.PCNN_OK
    assert n.value >= 16 * 480 * 640 * 24 + 2 * 16 * 256 * 96
    assert L.pcnn_pose2d_workspace_bytes(16, 480, 640, 22, 256, None) == _lib.PCNN_ENULL
    for bad in ((0, 480, 640, 22, 256), (1, 0, 640, 22, 256), (1, 480, 640, 1, 256), (1, 480, 640, 65, 256), (1, 480, 640, 22, 0),
                (1, 480, 640, 22, 1025), (1, 8192, 8192, 22, 256)):
        assert L.pcnn_pose2d_workspace_bytes(*bad, ctypes.byref(n)) == _lib.PCNN_EINVAL, bad
    assert L.pcnn_pose2d_prepare_fwd(None, None, None, 1, 8, 8, 4, None, None, None, None) == _lib.PCNN_ENULL
    assert L.pcnn_pose2d_prepare_fwd(None, None, None, 1, 8, 8, 1, None, None, None, None) == _lib.PCNN_EINVAL
    assert L.pcnn_pose2d_sample_fwd(None, None, None, None, None, None, 0, 0, 1, 8, 8, 4, 16, 0, 400, 10.0, 10.0, 0.01, None, None, None,
                                    None, None) == _lib.PCNN_EINVAL
    assert L.pcnn_pose2d_sample_fwd(None, None, None, None, None, None, 0, 0, 1, 8, 8, 4, 16, 4, 400, 10.0, 10.0, 0.01, None, None, None,
                                    None, None) == _lib.PCNN_ENULL
    assert L.pcnn_pose2d_round_fwd(None, None, None, None, None, None, 1, 8, 8, 4, 16, 0, 1000, 1000, 10.0, None, None, None, None) == _lib.PCNN_EINVAL
    assert L.pcnn_pose2d_round_fwd(None, None, None, None, None, None, 1, 8, 8, 4, 16, 1, 1000, 1000, 10.0, None, None, None, None) == _lib.PCNN_ENULL
    assert L.pcnn_pose2d_estimate_fwd(None, None, None, None, None, 0, 0, 1, 8, 8, 4, 16, 1000, 1000, -1, 400, 10.0, 10.0, 0.01, 1024,
                                      None, None, None, None, None, None, 0, None) == _lib.PCNN_EINVAL
