"""The numpy restatement of the 3-D pose route (tests/pose3d_ref.py, the statement of record the GPU tests compare bit for
bit against) checked on the CPU: its Kabsch against two independent float64 references, its random indices against numpy's
Philox, its schedules and index rules in closed form, the planted scenes' regimes and recovered poses, and five seeded
defects that the comparisons of tests/test_gpu_pose3d.py would catch. No GPU."""
import functools

import numpy as np
import pytest

import pose3d_cases as CS
import pose3d_ref as R

F, D = np.float32, np.float64
SEED = (0x1234_5678_9ABC_DEF0 << 64) | 0x0FED_CBA9_8765_4321

# Measured on the cases of kabsch_cases() (max |P - P'| over the 12 entries of R|t, largest over the cases):
#   np.linalg.svd Kabsch against Horn by np.linalg.eigh: 3.531e-14 (the planar 4-point case; 2e-15 typical)
#   the restatement against the farther of the two:       7.494e-14
# The bound is the project's rule: 4 x the references' own distance, re-measured on every run.
KABSCH_REFERENCES_DISTANCE = 3.531e-14
KABSCH_RESTATEMENT_DISTANCE = 7.494e-14

# Largest displacement of the 8 box corners between the recovered and the planted pose, per scene (seed, intrinsics) of
# scenes(), measured with this file's SEED (metres). Asserted at 4 x the recorded value, and below 1 mm — a tenth of the
# inlier threshold; that cap is a condition, not a measurement.
CORNER_DISPLACEMENT = {1: 1.242e-09, 2: 6.803e-09, 3: 5.076e-09}
CORNER_CAP = 1e-3


# ---- Kabsch ---------------------------------------------------------------------------------------------------------------
def kabsch_svd(A, B):
    cA, cB = A.mean(0), B.mean(0)
    U, _, Vt = np.linalg.svd((A - cA).T @ (B - cB))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    Rm = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return np.concatenate([Rm, (cB - Rm @ cA)[:, None]], axis=1)


def horn_eigh(A, B):
    cA, cB = A.mean(0), B.mean(0)
    M = (A - cA).T @ (B - cB)
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([Rm, (cB - Rm @ cA)[:, None]], axis=1)


def kabsch_cases():
    """n in {3 (rank 2), 4, 10, 100, 1000} x {exact, exact, 2 mm noise, 2 mm noise, planar object + noise, 5 cm noise}: f32
    values (what the records hold), widened"""
    rng = np.random.RandomState(42)
    out = []
    for n in (3, 4, 10, 100, 1000):
        for rep in range(6):
            A = rng.uniform(-0.15, 0.15, size=(n, 3))
            if rep == 4:
                A[:, 2] = 0.01 * A[:, 0]
            Rm, t = CS._rotation(rng), rng.uniform(-0.3, 0.3, 3) + [0, 0, 0.9]
            B = A @ Rm.T + t
            if rep >= 2:
                B = B + rng.normal(scale=0.002, size=B.shape)
            if rep == 5 and n > 3:
                B = B + rng.normal(scale=0.05, size=B.shape)
            out.append((A.astype(F), B.astype(F)))
    return out


def test_kabsch_against_two_references():
    between, mine = 0.0, 0.0
    for A, B in kabsch_cases():
        P1, P2 = kabsch_svd(A.astype(D), B.astype(D)), horn_eigh(A.astype(D), B.astype(D))
        P = R.fit_points(A, B).reshape(3, 4)
        assert abs(np.linalg.det(P[:, :3]) - 1) < 1e-12 and np.abs(P[:, :3] @ P[:, :3].T - np.eye(3)).max() < 1e-12
        between = max(between, np.abs(P1 - P2).max())
        mine = max(mine, np.abs(P - P1).max(), np.abs(P - P2).max())
    print("references' distance %.3e, restatement %.3e" % (between, mine))
    assert mine <= 4 * between


def test_kabsch_rank_two_and_reflection():
    """three points (rank-2 covariance) and a mirrored target: a proper rotation comes out, never a reflection"""
    rng = np.random.RandomState(3)
    A = rng.uniform(-0.1, 0.1, size=(3, 3)).astype(F)
    Rm = CS._rotation(rng)
    B = (A.astype(D) @ Rm.T + [0.1, 0.2, 0.8]).astype(F)
    P = R.fit_points(A, B).reshape(3, 4)
    assert np.abs(P[:, :3] - Rm).max() < 1e-5 and np.abs(A.astype(D) @ P[:, :3].T + P[:, 3] - B).max() < 1e-6
    A = rng.uniform(-0.1, 0.1, size=(50, 3)).astype(F)
    B = (A * np.array([1, 1, -1], dtype=F)).astype(F)                      # the best orthogonal map is a reflection
    P = R.fit_points(A, B).reshape(3, 4)
    assert abs(np.linalg.det(P[:, :3]) - 1) < 1e-12
    assert np.abs(P - kabsch_svd(A.astype(D), B.astype(D))).max() < 1e-9


# ---- random indices -------------------------------------------------------------------------------------------------------
def test_philox_indices_against_numpy():
    key = np.array([SEED & ((1 << 64) - 1), SEED >> 64], dtype=np.uint64)
    for attempt, stream, h in ((1, 0, 0), (7, 11, 255), (1023, 1 << 63, 13)):
        # np.random.Philox increments the counter before it generates: random_raw(4) of counter c is the block of c + 1
        words = np.random.Philox(counter=np.array([attempt - 1, stream, h, 0], dtype=np.uint64), key=key).random_raw(4)
        mine = R.philox4x64((attempt, stream, h, 0), (int(key[0]), int(key[1])))[0]
        assert (mine == words).all()
        for n in (1, 3, 401, 2500, (1 << 31) - 1):
            want = [((int(w) >> 32) * n) >> 32 for w in words]
            assert R.philox_index(words, n).tolist() == want and all(0 <= v < n for v in want)
    u = R.philox_index(R.philox4x64((np.arange(4000, dtype=np.uint64), 0, 0, 0), (1, 2))[:, 0], 5)
    assert np.bincount(u.astype(np.int64), minlength=5).min() > 700       # 800 expected per bin


# ---- schedules and index rules --------------------------------------------------------------------------------------------
def test_halving_schedule():
    assert R.halving_schedule(1, 8) == [(1, 1)] * 8
    assert R.halving_schedule(2, 8) == [(2, 1)] + [(1, 1)] * 7
    assert R.halving_schedule(13, 8) == [(13, 6), (6, 3), (3, 1)] + [(1, 1)] * 5
    assert R.halving_schedule(256, 8) == [(256 >> i, 256 >> (i + 1)) for i in range(8)]
    assert R.halving_schedule(256, 0) == [(256 >> i, 256 >> (i + 1)) for i in range(8)]
    assert R.halving_schedule(1024, 3)[-1] == (2, 1) and len(R.halving_schedule(1024, 3)) == 10
    assert R.halving_schedule(1, 0) == []
    for hyp, ref_it in ((1, 8), (2, 8), (13, 8), (256, 8), (1024, 0)):
        assert len(R.halving_schedule(hyp, ref_it)) <= int(np.ceil(np.log2(hyp))) + ref_it + 1


@pytest.mark.parametrize("m", [1, 7, 100, 1000])
def test_stride_index_rule(m):
    for n in (m - 1, m, m + 1, 3 * m + 1):
        if n < 1:
            continue
        mm = min(n, m)                                                       # the round's m never exceeds n
        idx = R.stride_index(n, mm)
        assert idx.tolist() == [k * n // mm for k in range(mm)]
        assert idx[0] == 0 and idx[-1] < n and (np.diff(idx) >= 1).all()      # strictly increasing: no record twice
        if n == mm:
            assert idx.tolist() == list(range(n))
    # the thinning's closed form used on the device: rank r is kept iff j = ceil(r m / cnt) < m and floor(j cnt / m) == r
    for cnt in (m, m + 1, 2 * m + 3):
        kept = set(R.stride_index(cnt, m).tolist())
        for r in range(cnt):
            j = (r * m + cnt - 1) // cnt
            assert (j < m and j * cnt // m == r) == (r in kept)


# ---- the planted scenes ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scenes():
    out = []
    for seed, K in zip((1, 2, 3), CS.INTRINSICS):
        f = CS.make_frame(seed, K)
        trace = {}
        est = R.estimate(f["label"], f["depth"], f["vertex_pred"], f["extents"], f["K"], CS.FACTOR, stream=seed, seed=SEED, trace=trace)
        out.append((seed, f, est, trace))
    return out


def test_scene_regimes():
    for seed, f, est, trace in scenes():
        rec, cnt, off = R.prepare(f["label"], f["depth"], f["vertex_pred"], f["extents"], f["K"], CS.FACTOR)
        assert cnt.tolist() == [0, 2500, 900, 401, 400, 448, 0]
        assert [c for c in range(1, CS.C) if cnt[c] > 400] == list(CS.LIVE)
        assert not rec[off[5]:off[5] + cnt[5], :3].any()                                          # class 5: every depth a hole
        k = f["kind"]
        assert (k == 1).sum() > 500 and (k == 3).sum() > 50 and ((k == 2) & (f["label"] != 5)).sum() > 100
        empty = rec[(rec[:, 3] == 0) & (rec[:, 4] == 0) & (rec[:, 5] == 0)]
        assert len(empty) >= (k[(f["label"] > 0) & (f["label"] < CS.C)] == 3).sum() > 0           # 0.5 unscales to exactly 0
        for c in CS.POSED:
            Rm, t = f["poses"][c]
            r = rec[off[c]:off[c] + cnt[c]].astype(D)
            d = np.linalg.norm(r[:, :3] - (r[:, 3:] @ Rm.T + t), axis=1)
            inl = f["inlier"][c]
            assert d[inl].max() < 1e-6 and d[~inl & (r[:, 2] != 0)].min() >= 0.049                  # exact / gross
        assert est["num_hyps"].sum() == 256 and (est["num_hyps"][list(CS.POSED)] > 0).all()
        assert not est["num_hyps"][[0, 4, 5, 6]].any() and not est["poses64"][[0, 4, 5, 6]].any()
        assert est["ref_steps"][list(CS.POSED)].tolist() == [8, 8, 8]
        for c in CS.POSED:
            last = trace[c]
            assert len(last["subset"]) == cnt[c]                                                  # the last round sees the class
            assert (last["masks"][0] == f["inlier"][c][last["subset"]]).all()
            assert est["inliers"][c] == f["inlier"][c].sum()
            assert trace["sizes"][c] == R.halving_schedule(int(est["num_hyps"][c]), 8)                 # the loop ran that schedule


def test_recovered_poses():
    for seed, f, est, _ in scenes():
        worst = max(CS.corner_displacement(est["poses64"][c], *f["poses"][c], f["extents"][c]) for c in CS.POSED)
        print("scene %d: corner displacement %.3e m" % (seed, worst))
        assert worst <= 4 * CORNER_DISPLACEMENT[seed] and worst < CORNER_CAP


# ---- seeded defects -------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return any((np.asarray(a[k]).view(np.uint8) != np.asarray(b[k]).view(np.uint8)).any() if np.asarray(a[k]).shape == np.asarray(b[k]).shape
               else True for k in a)


def test_seeded_defects_are_caught():
    """Each defect changes at least one array that tests/test_gpu_pose3d.py compares bit for bit (named here), on its own
    scenes and parameters."""
    seed, f, est, _ = scenes()[0]
    args = (f["label"], f["depth"], f["vertex_pred"], f["extents"], f["K"], CS.FACTOR)
    rec, cnt, off = R.prepare(*args)
    # "chan": the records of test_prepare
    assert (R.prepare(*args, defect="chan")[0].view(np.uint32) != rec.view(np.uint32)).any()
    pose, cls, _, _ = R.sample(rec, cnt, off, f["extents"], f["K"], CS.H, CS.W, 11, SEED, hypotheses=64)
    good = R.round_fwd(rec, cnt, off, pose, cls, 3)
    # "ceil": class_out of a round (an odd number of hypotheses in some class)
    sizes = [(cls == c).sum() for c in CS.POSED]
    assert any(s % 2 for s in sizes)
    assert (R.round_fwd(rec, cnt, off, pose, cls, 3, defect="ceil")[1] != good[1]).any()
    # "stride": inliers_out / pose_out of the small-batch rounds (m < n)
    small = R.round_fwd(rec, cnt, off, pose, cls, 1, pixel_batch=128, max_pixels=100)
    bad = R.round_fwd(rec, cnt, off, pose, cls, 1, pixel_batch=128, max_pixels=100, defect="stride")
    assert (small[2] != bad[2]).any() or (small[0].view(np.uint64) != bad[0].view(np.uint64)).any()
    # "le": the frame whose fourth record sits exactly at the threshold (test_round_at_threshold, test_driver_at_threshold)
    t = CS.threshold_frame()
    targs = (t["label"], t["depth"], t["vertex_pred"], t["extents"], t["K"], t["factor"])
    trec, tcnt, toff = R.prepare(*targs)
    assert R.residual(CS.THRESHOLD_POSE[None], trec)[0, 0] == D(F(CS.THRESHOLD["inlier_threshold"]))
    one = np.array([1], np.int32)
    ok = R.round_fwd(trec, tcnt, toff, CS.THRESHOLD_POSE[None], one, 1, inlier_threshold=0.25)
    le = R.round_fwd(trec, tcnt, toff, CS.THRESHOLD_POSE[None], one, 1, inlier_threshold=0.25, defect="le")
    assert ok[2].tolist() == [3] and le[2].tolist() == [4] and (ok[0] == CS.THRESHOLD_POSE).all() and (le[0] != ok[0]).any()
    ok = R.estimate(*targs, stream=3, seed=SEED, **CS.THRESHOLD)
    le = R.estimate(*targs, stream=3, seed=SEED, defect="le", **CS.THRESHOLD)
    assert ok["inliers"][1] == 3 and le["inliers"][1] == 4 and ok["ref_steps"][1] == le["ref_steps"][1] == 8
    assert (ok["poses64"][1] == CS.THRESHOLD_POSE).all() and (le["poses64"][1] != ok["poses64"][1]).any()
    # "eig": the sampler's poses (hyp_pose of test_sample) — a three-point fit has a negative eigenvalue of the largest modulus
    # whenever the rotation angle is large
    bad = R.sample(rec, cnt, off, f["extents"], f["K"], CS.H, CS.W, 11, SEED, hypotheses=64, defect="eig")
    assert (bad[0].view(np.uint64) != pose.view(np.uint64)).any() or (bad[2] != R.sample(rec, cnt, off, f["extents"], f["K"], CS.H,
                                                                                       CS.W, 11, SEED, hypotheses=64)[2]).any()
    # and the driver's outputs differ for the two that change which pose wins on the planted scene
    for defect in ("chan", "eig"):
        other = R.estimate(*args, stream=seed, seed=SEED, defect=defect)
        assert _differs({k: est[k] for k in ("poses64", "inliers", "num_hyps")}, other), defect


# ---- the host wrappers refuse what the header refuses, without a GPU ---------------------------------------------------------
def test_host_validation_needs_no_gpu():
    """argument errors are refused on the host before any launch: the C entries return EINVAL / ENULL with NULL pointers"""
    from posecnn_amd import _lib
    L = _lib.lib()
    import ctypes
    n = ctypes.c_size_t()
    assert L.pcnn_pose3d_workspace_bytes(16, 480, 640, 22, 256, ctypes.byref(n)) == _lib.PCNN_OK
    assert n.value >= 16 * 480 * 640 * 24 + 2 * 16 * 256 * 96
    assert L.pcnn_pose3d_workspace_bytes(16, 480, 640, 22, 256, None) == _lib.PCNN_ENULL
    for bad in ((0, 480, 640, 22, 256), (1, 0, 640, 22, 256), (1, 480, 640, 1, 256), (1, 480, 640, 65, 256), (1, 480, 640, 22, 0),
                (1, 480, 640, 22, 1025), (1, 8192, 8192, 22, 256)):
        assert L.pcnn_pose3d_workspace_bytes(*bad, ctypes.byref(n)) == _lib.PCNN_EINVAL, bad
    assert L.pcnn_pose3d_prepare_fwd(None, None, None, None, None, 1000.0, 1, 8, 8, 4, None, None, None, None) == _lib.PCNN_ENULL
    assert L.pcnn_pose3d_prepare_fwd(None, None, None, None, None, 0.0, 1, 8, 8, 4, None, None, None, None) == _lib.PCNN_EINVAL
    assert L.pcnn_pose3d_sample_fwd(None, None, None, None, None, None, 0, 0, 1, 8, 8, 4, 16, 0, 400, 0.01, 0.01, None, None, None, None,
                                    None) == _lib.PCNN_EINVAL
    assert L.pcnn_pose3d_round_fwd(None, None, None, None, None, 1, 8, 8, 4, 16, 0, 1000, 1000, 0.01, None, None, None, None) == _lib.PCNN_EINVAL
    assert L.pcnn_pose3d_round_fwd(None, None, None, None, None, 1, 8, 8, 4, 16, 1, 1000, 1000, 0.01, None, None, None, None) == _lib.PCNN_ENULL
    assert L.pcnn_pose3d_estimate_fwd(None, None, None, None, None, None, 1000.0, 0, 0, 1, 8, 8, 4, 16, 1000, 1000, -1, 400, 0.01, 0.01,
                                      1024, None, None, None, None, None, None, 0, None) == _lib.PCNN_EINVAL
