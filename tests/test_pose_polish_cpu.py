"""The numpy restatement of the pose polish (tests/pose_polish_ref.py, the statement of record the GPU tests compare bit for
bit against) checked on the CPU: its energy against two independent float64 formulas, the optimiser's properties, its
simplex rules against the C oracle's N = 7 polish on a shared objective, the planted scenes, what every case of
tests/pose_polish_cases.py exercises, five seeded defects, and the host validation of the new entries. No GPU."""
import ctypes
import math

import numpy as np
import pytest

import pose2d_cases as C2
import pose3d_cases as C3
import pose_polish_cases as PC
import pose_polish_ref as PR

F, D = np.float32, np.float64
INF = float("inf")

# Budget of the planted-scene test, reasoned before any run: the initial simplex has edges of 5 degrees, 5 cm and 25 cm (a
# quarter of the box), the planted pose sits 2 degrees and 5 mm from the start, and "recovered" means a tenth of that, 0.5 mm.
# The longest edge must shrink from 0.25 m by 0.25 / 0.0005 = 500 = 2^9; a contraction halves ONE vertex's distance and costs
# two evaluations, so halving the whole simplex once costs about 2 (N + 1) = 14 and nine halvings 7 + 9 x 14 = 133
# evaluations when every step contracts. Reflections that do not shrink come on top: the test runs 3 x that, 400.
# At the reference's own budget of 100 < 133 the simplex cannot have converged; what it does there is printed and recorded
# in DESIGN.md 3.7b / 3.7c, and only the property that holds at every budget — the energy does not rise — is asserted.
PLANTED_EVALUATIONS = 400
# Largest corner displacement (metres) against the planted pose over classes 1, 2, 3 of the three scenes, before the polish
# and after PLANTED_EVALUATIONS evaluations, measured with this file's cases; asserted at 10 x the recorded value (the
# convention of DESIGN.md 3.7c) and below the displacement before.
CORNER_BEFORE = {0: 1.399e-02, 1: 1.399e-02}
CORNER_AFTER = {0: 2.086e-05, 1: 2.392e-03}
# At the reference's 100 evaluations (printed by test_planted_scenes): depth 1.399e-02 -> 9.827e-03 at worst, every class
# closer than before; colour 1.399e-02 -> 2.714e-02 at worst, five of nine classes FARTHER than before although every energy
# fell about tenfold — the reprojection energy barely sees a move along the viewing ray, and the simplex starts 25 cm wide there.


# ---- the energy -----------------------------------------------------------------------------------------------------------
def rotation_quaternion(w3):
    """Q of the retraction by the textbook quaternion-to-matrix product, float64"""
    q = np.concatenate([[1.0], 0.5 * np.asarray(w3)])
    q = q / np.linalg.norm(q)
    w, v = q[0], q[1:]
    S = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + 2 * w * S + 2 * S @ S


def rotation_rodrigues(w3):
    """the same rotation from its axis and angle (2 atan(|w| / 2)) by Rodrigues' formula"""
    n = np.linalg.norm(w3)
    if n == 0:
        return np.eye(3)
    a, k = 2 * math.atan(n / 2), np.asarray(w3) / n
    S = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(a) * S + (1 - math.cos(a)) * S @ S


def energy_independent(route, P0, x, lst, K, variant):
    """variant 0: quaternion product, R = Q R0 first, u = fx (x / z) + px, numpy's pairwise sum;
    variant 1: Rodrigues, the object points through R0 and then through Q, u = (fx x + px z) / z, math.fsum —
    the same mathematics in another order of float64 operations, so that their distance shows the formula's conditioning"""
    P0 = np.asarray(P0, D).reshape(3, 4)
    t = P0[:, 3] + x[3:]
    o = lst[:, 3:].astype(D)
    if variant == 0:
        q = o @ (rotation_quaternion(x[:3]) @ P0[:, :3]).T + t
    else:
        q = (o @ P0[:, :3].T) @ rotation_rodrigues(x[:3]).T + t
    if route == 0:
        d = np.linalg.norm(lst[:, :3].astype(D) - q, axis=1) if variant == 0 else np.sqrt(((q - lst[:, :3].astype(D)) ** 2).sum(axis=1))
    else:
        fx, fy, px, py = (D(F(v)) for v in K)
        if variant == 0:
            d = np.hypot(fx * (q[:, 0] / q[:, 2]) + px - lst[:, 0], fy * (q[:, 1] / q[:, 2]) + py - lst[:, 1])
        else:
            d = np.sqrt(((fx * q[:, 0] + px * q[:, 2]) / q[:, 2] - lst[:, 0]) ** 2 + ((fy * q[:, 1] + py * q[:, 2]) / q[:, 2] - lst[:, 1]) ** 2)
    return (np.sum(d) if variant == 0 else math.fsum(d)) / len(d)


@pytest.mark.parametrize("route", [0, 1])
def test_energy_against_two_references(route):
    """relative distance, the project's rule: the restatement is within 4 x the distance between two independent references
    (two orders of float64 operations, see energy_independent), re-measured on every run"""
    bt = PC.batch(route)
    rng = np.random.RandomState(5)
    between, mine = 0.0, 0.0
    for b, c, mp in ((0, 1, 1000), (0, 2, 1000), (1, 3, 37), (3, 4, 1000), (3, 6, 1000), (2, 1, 2000)):
        rec = bt["records"][b, bt["offsets"][b, c]:bt["offsets"][b, c] + bt["counts"][b, c]]
        K = tuple(bt["K"][b])
        where, _ = PR.list_indices(route, bt["poses"][b, c], rec, K, mp, PC.THRESHOLD[route])
        lst = rec[where]
        for _ in range(5):
            x = rng.uniform(-1, 1, size=6) * np.array(PR.BOX) * 0.2
            e = PR.energy(route, bt["poses"][b, c], x, lst, K)
            e1 = energy_independent(route, bt["poses"][b, c], x, lst, K, 0)
            e2 = energy_independent(route, bt["poses"][b, c], x, lst, K, 1)
            between = max(between, abs(e1 - e2) / e2)
            mine = max(mine, abs(e - e1) / e1, abs(e - e2) / e2)
    print("route %d: references' relative distance %.3e, restatement %.3e" % (route, between, mine))
    assert between > 0 and mine <= 4 * between


def test_pose_of_zero_is_the_pose():
    P = PC.batch(0)["poses"][0, 1]
    assert (PR.pose_of(P, np.zeros(6)) == P).all()


# ---- the optimiser's properties -----------------------------------------------------------------------------------------------
def bowl(centre, weight):
    return lambda x: float(sum(w * (v - m) * (v - m) for v, m, w in zip(x, centre, weight)))


def test_optimiser_properties():
    """inside the box, never worse, exactly `evaluations` evaluations — on a bowl and on a scene's energy"""
    bt = PC.batch(0)
    rec = bt["records"][0, bt["offsets"][0, 2]:bt["offsets"][0, 2] + bt["counts"][0, 2]]
    where, _ = PR.list_indices(0, bt["poses"][0, 2], rec, None, 1000, PC.THRESHOLD[0])
    scene = lambda x: PR.energy(0, bt["poses"][0, 2], x, rec[where], None)
    for fn in (bowl((0.05, -0.3, 0.01, 0.02, -0.09, 0.45), (1, 2, 3, 50, 5, 0.5)), scene):
        last = INF
        for evaluations in list(range(7, 60)) + [100, 250]:
            steps = []
            xb, fb, f0, evals = PR.nelder_mead(fn, PR.LB, PR.UB, evaluations, trace=steps)
            seen = [s for s in steps if s[0] != "cut"]
            assert evals == evaluations == len(seen)
            assert all(PR.LB[i] <= s[1][i] <= PR.UB[i] for s in seen for i in range(6))
            assert fb == min(s[2] for s in seen) <= f0 == seen[0][2] and fb == fn(xb)
            assert fb <= last                                      # a longer budget continues the shorter one
            last = fb


def test_bound_is_reached_exactly():
    """a separable convex bowl whose minimum lies outside the box in coordinate 1 (centre -0.3 < lb = -0.1745..) and 5
    (0.8 > ub = 0.5): those coordinates end ON the bound, the others near their centre"""
    centre = (0.05, -0.3, 0.01, 0.02, -0.05, 0.8)
    xb, fb, f0, evals = PR.nelder_mead(bowl(centre, (1, 1, 1, 1, 1, 1)), PR.LB, PR.UB, 1500)
    assert xb[1] == PR.LB[1] and xb[5] == PR.UB[5] and evals == 1500
    assert all(abs(xb[i] - centre[i]) < 1e-6 for i in (0, 2, 3, 4))


def test_simplex_rules_against_the_c_oracle():
    """The oracle's solveICP polish (oracle_icp_polish, N = 7, box around (1, 0, .., 0)) and this restatement's simplex rules
    on ONE objective — the oracle's own energy entry — give the same point, value and count, bit for bit."""
    import oracle
    rng = np.random.RandomState(2)
    Hh, Ww = 24, 32
    label = np.zeros((Hh, Ww), np.int32)
    label[4:20, 6:26] = 1
    pred = np.zeros((Hh, Ww, 3), F)
    pred[..., 0], pred[..., 1] = rng.uniform(-0.1, 0.1, size=(2, Hh, Ww))
    pred[..., 2] = rng.uniform(0.9, 1.1, size=(Hh, Ww))
    live = (pred + np.array([0.004, -0.003, 0.02]) + rng.normal(scale=0.002, size=pred.shape)).astype(F)
    x0 = (1.0, 0, 0, 0, 0, 0, 0)
    rng7 = (0.1, 0.1, 0.1, 0.1, 0.01, 0.01, 0.1)
    lb, ub = [a - r for a, r in zip(x0, rng7)], [a + r for a, r in zip(x0, rng7)]
    kinds = set()
    for maxeval in (8, 9, 23, 50, 160):
        x, e, n = oracle.icp_polish(label, live, pred, 1, maxeval=maxeval)
        steps = []
        xb, fb, _, evals = PR.nelder_mead(lambda v: oracle.icp_energy(label, live, pred, 1, np.array(v)), lb, ub, maxeval, x0=x0, trace=steps)
        assert evals == n == maxeval and fb == e
        assert (np.array(xb).view(np.uint64) == x.view(np.uint64)).all(), maxeval
        kinds |= {s[0] for s in steps}
    assert {"init", "reflect", "expand", "inside", "outside"} <= kinds


# ---- the planted scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 1])
def test_planted_scenes(route):
    bt, CS = PC.batch(route), PC.CASES[route]
    rows = {}
    for evaluations in (100, PLANTED_EVALUATIONS):
        ref = PC.reference(route, 1000, evaluations)
        for b in range(3):
            for c in PC.POSED:
                before = CS.corner_displacement(bt["poses"][b, c], *bt["planted"][(b, c)], bt["extents"][c])
                after = CS.corner_displacement(ref[b]["poses64"][c], *bt["planted"][(b, c)], bt["extents"][c])
                e0, e1 = ref[b]["energy"][c]
                rows[(evaluations, b, c)] = (before, after)
                print("route %d, %3d evaluations, frame %d class %d: energy %.3e -> %.3e, corners %.3e -> %.3e m, listed %d" % (
                    route, evaluations, b, c, e0, e1, before, after, ref[b]["listed"][c]))
                assert e1 < e0 and ref[b]["evals"][c] == evaluations
                # the list keeps most planted pixels (and, thinned to 1000, nothing else)
                n_planted = int(PC.frames(route)[b][0]["inlier"][c].sum())
                assert ref[b]["listed"][c] >= min(1000, 0.9 * n_planted)
    before = max(v[0] for k, v in rows.items() if k[0] == PLANTED_EVALUATIONS)
    after = max(v[1] for k, v in rows.items() if k[0] == PLANTED_EVALUATIONS)
    print("route %d: largest corner displacement %.3e -> %.3e m at %d evaluations" % (route, before, after, PLANTED_EVALUATIONS))
    assert all(v[1] < v[0] for k, v in rows.items() if k[0] == PLANTED_EVALUATIONS)
    assert before <= 10 * CORNER_BEFORE[route] and after <= 10 * CORNER_AFTER[route]


# ---- what the GPU cases exercise ----------------------------------------------------------------------------------------------
def kinds_of(trace):
    return [s[0] for s in trace["steps"]]


@pytest.mark.parametrize("route", [0, 1])
def test_case_claims(route):
    bt = PC.batch(route)
    out, tr = PC.reference(route, 1000, 100, trace=True)
    # gate and empty lists
    for b in range(4):
        assert out[b]["evals"][0] == 0 and (out[b]["poses64"][0] == bt["poses"][b, 0]).all()             # class 0: copied
        assert out[b]["listed"][6 if b < 3 else 5] == 0 and bt["counts"][b, 6 if b < 3 else 5] == 0      # no record
    assert [int(out[b]["evals"][4]) for b in range(3)] == [0, 100, 0]                                   # gate == / + 1 / 0
    assert bt["gate"][0, 4] == PC.MIN_PIXELS and bt["gate"][1, 4] == PC.MIN_PIXELS + 1
    assert (out[0]["poses64"][4] == bt["poses"][0, 4]).all() and (out[1]["poses64"][4] != bt["poses"][1, 4]).any()
    if route == 0:                                                                                        # all holes: open gate, empty list
        assert all(out[b]["listed"][5] == 0 and out[b]["evals"][5] == 0 and bt["counts"][b, 5] == 448 for b in range(3))
    else:
        assert all(0 < out[b]["listed"][5] < 448 for b in range(3))
    # list lengths around the 64 lanes, and 5 records
    assert out[3]["listed"].tolist() == list(PC.LENGTHS) and out[3]["evals"].tolist() == [0, 100, 100, 100, 100, 0, 100]
    lengths = sorted(int(v) for b in range(4) for v in out[b]["listed"] if v)
    assert any(v < 64 for v in lengths) and any(v % 64 for v in lengths) and 64 in lengths and 1000 in lengths
    # thinning: class 1 of every scene has more than 1000 inliers at max_pixels = 1000; at 37 every polished scene class thins
    assert all(tr[b][1]["cnt"] > 1000 and out[b]["listed"][1] == 1000 for b in range(3))
    assert all(tr[b][c]["cnt"] < 1000 for b in range(3) for c in (2, 3))
    small, trs = PC.reference(route, 37, 100, trace=True)
    assert all(small[b]["listed"][c] == 37 and trs[b][c]["cnt"] >= 37 for b in range(3) for c in PC.POSED)
    assert small[3]["listed"].tolist() == [0, 37, 37, 37, 5, 0, 37]
    # the workspace runs: 1025 thins class 1 to 1025 records (> the LDS bound), 2000 lists all its inliers unthinned
    assert PR.LDS_RECORDS == 1024
    big = PC.reference(route, 1025, 100)
    assert all(big[b]["listed"][1] == 1025 for b in range(3))
    all_of_them, tra = PC.reference(route, 2000, 100, trace=True)
    assert all(all_of_them[b]["listed"][1] == tra[b][1]["cnt"] > 1024 for b in range(3))
    # the optimiser's branches over the batch
    kinds = [k for b in range(4) for c in range(1, PC.C) if tr[b][c].get("steps") for k in kinds_of(tr[b][c])]
    assert {"init", "reflect", "expand", "inside", "outside"} <= set(kinds)
    # 7 evaluations: the initial simplex alone; 8: one reflection
    seven, tr7 = PC.reference(route, 1000, 7, trace=True)
    eight, tr8 = PC.reference(route, 1000, 8, trace=True)
    assert kinds_of(tr7[0][1]) == ["init"] * 7 and kinds_of(tr8[0][1]) == ["init"] * 7 + ["reflect"]
    assert seven[0]["evals"][1] == 7 and eight[0]["evals"][1] == 8
    # 0 evaluations: nothing is polished
    zero = PC.reference(route, 1000, 0)
    assert all((zero[b]["poses64"] == bt["poses"][b]).all() and not zero[b]["evals"].any() for b in range(4))


def test_colour_case_meets_infinity():
    out, tr = PC.near_reference(100, trace=True)
    steps = tr[1]["steps"]
    inf_at = [i for i, s in enumerate(steps) if s[2] == INF]
    assert out["listed"].tolist() == [0, 40] and out["evals"][1] == 100
    assert any(i < 7 for i in inf_at) and any(steps[i][0] == "reflect" for i in inf_at)      # initial vertices and reflections
    assert np.isfinite(out["energy"][1]).all() and out["energy"][1, 1] <= out["energy"][1, 0]
    # a +inf point is never the result, and the pose it stands for does put a listed point behind the camera
    n = PC.near()
    x = steps[inf_at[0]][1]
    _, front = PR.distances(1, PR.pose_of(n["poses"][0, 1], x), n["records"][0, :40], PC.NEAR_K)
    assert not front.all()


@pytest.mark.parametrize("route", [0, 1])
def test_edge_case_is_clamped(route):
    out, tr = PC.edge_reference(route, trace=True)
    on_bound = [s for s in tr[2]["steps"] if s[1][3] == PR.UB[3]]
    assert len(on_bound) >= 3 and out["evals"][2] == 100 and out["listed"][2] > 500
    assert out["energy"][2, 1] < 0.5 * out["energy"][2, 0]


def test_shrink_case():
    """the one simplex of these cases that shrinks: a budget of 292 ends inside the shrink, 300 goes through it"""
    cut, trc = PC.shrink_reference(292, trace=True)
    full, trf = PC.shrink_reference(300, trace=True)
    kc, kf = kinds_of(trc[5]), kinds_of(trf[5])
    assert kc[289:292] == ["shrink"] * 3 and kc[292] == "cut" and cut["evals"][5] == 292
    assert kf[289:295] == ["shrink"] * 6 and kf[295] != "shrink" and full["evals"][5] == 300
    assert cut["listed"][5] == full["listed"][5] == 112
    assert not cut["evals"][[0, 1, 2, 3, 4, 6]].any()


# ---- seeded defects -------------------------------------------------------------------------------------------------------
def differs(a, b):
    return any((np.asarray(a[k]).view(np.uint8) != np.asarray(b[k]).view(np.uint8)).any() for k in ("poses64", "energy", "evals", "listed"))


def run_batch(route, max_pixels, evaluations, defect):
    bt = PC.batch(route)
    return [PR.polish(route, bt["records"][b], bt["counts"][b], bt["offsets"][b], bt["poses"][b], bt["gate"][b], K=tuple(bt["K"][b]),
                      max_pixels=max_pixels, min_pixels=PC.MIN_PIXELS, evaluations=evaluations, inlier_threshold=PC.THRESHOLD[route],
                      defect=defect) for b in range(4)]


@pytest.mark.parametrize("route", [0, 1])
def test_seeded_defects_are_caught(route):
    """each defect changes an array tests/test_gpu_pose_polish.py compares bit for bit, in the named run of the batch"""
    good = PC.reference(route, 1000, 100)
    # "fold": the energies of every polished class
    bad = run_batch(route, 1000, 100, "fold")
    assert any((bad[b]["energy"] != good[b]["energy"]).any() for b in range(4))
    # "gate": class 4 of frame 0, gate == min_pixels
    bad = run_batch(route, 1000, 100, "gate")
    assert bad[0]["evals"][4] == 100 and good[0]["evals"][4] == 0 and differs(bad[0], good[0])
    # "gamma": any class that expands
    bad = run_batch(route, 1000, 100, "gamma")
    assert any(differs(bad[b], good[b]) for b in range(4))
    # "thin": the thinned lists (class 1 at 1000; everything at 37)
    bad = run_batch(route, 1000, 100, "thin")
    assert all((bad[b]["energy"][1] != good[b]["energy"][1]).any() for b in range(3))
    assert all((bad[b]["energy"][c] == good[b]["energy"][c]).all() for b in range(3) for c in (2, 3))      # not thinned: untouched
    # "clamp": the EDGE case, whose trial points are clamped
    assert differs(PC.edge_reference(route, defect="clamp"), PC.edge_reference(route))


# ---- the host wrappers refuse what the header refuses, without a GPU ---------------------------------------------------------
def test_host_validation_needs_no_gpu():
    from posecnn_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t()
    ok, einval, enull, ews = _lib.PCNN_OK, _lib.PCNN_EINVAL, _lib.PCNN_ENULL, _lib.PCNN_EWORKSPACE
    assert L.pcnn_pose_polish_workspace_bytes(16, 22, 1000, ctypes.byref(n)) == ok and n.value == 16
    assert L.pcnn_pose_polish_workspace_bytes(16, 22, 1024, ctypes.byref(n)) == ok and n.value == 16
    assert L.pcnn_pose_polish_workspace_bytes(16, 22, 1025, ctypes.byref(n)) == ok and n.value == 16 * 22 * 1025 * 24
    assert L.pcnn_pose_polish_workspace_bytes(1, 2, 1 << 30, ctypes.byref(n)) == ok and n.value == 2 * (1 << 24) * 24
    assert L.pcnn_pose_polish_workspace_bytes(16, 22, 1000, None) == enull
    for bad in ((0, 22, 1000), (16, 1, 1000), (16, 65, 1000), (16, 22, 0)):
        assert L.pcnn_pose_polish_workspace_bytes(*bad, ctypes.byref(n)) == einval, bad

    def polish(route=0, B=1, H=8, W=8, C=4, max_pixels=1000, min_pixels=10, evaluations=100, thr=0.01):
        return L.pcnn_pose_polish_fwd(route, None, None, None, None, None, None, B, H, W, C, max_pixels, min_pixels, evaluations, thr,
                                      None, None, None, None, None, None, 0, None)
    assert polish() == enull
    for kw in (dict(route=2), dict(route=-1), dict(evaluations=6), dict(evaluations=1), dict(evaluations=-1), dict(evaluations=4097),
               dict(max_pixels=0), dict(min_pixels=-1), dict(thr=float("nan")), dict(thr=float("inf")), dict(B=0), dict(C=1), dict(H=0)):
        assert polish(**kw) == einval, kw
    for kw in (dict(evaluations=0), dict(evaluations=7), dict(evaluations=4096), dict(min_pixels=0), dict(route=1)):
        assert polish(**kw) == enull, kw                               # past the value checks, stopped by the NULL pointers
    # a short workspace: real (host) addresses stand in for the pointers, nothing is launched
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.pcnn_pose_polish_fwd(0, p, p, p, None, p, p, 1, 8, 8, 4, 2000, 10, 100, 0.01, p, p, p, p, p, p, 16, None) == ews
    assert L.pcnn_pose_polish_fwd(0, p, p, p, None, p, p, 1, 8, 8, 4, 1000, 10, 100, 0.01, p, p, p, p, p, None, 0, None) == ews
    assert L.pcnn_pose_polish_fwd(1, p, p, p, None, p, p, 1, 8, 8, 4, 1000, 10, 100, 0.01, p, p, p, p, p, p, 16, None) == enull

    for route, pts in (("pose3d", 3), ("pose2d", 4)):
        base, full = ctypes.c_size_t(), ctypes.c_size_t()
        assert getattr(L, "pcnn_%s_workspace_bytes" % route)(16, 480, 640, 22, 256, ctypes.byref(base)) == ok
        q = getattr(L, "pcnn_%s_estimate_polished_workspace_bytes" % route)
        assert q(16, 480, 640, 22, 256, 1000, ctypes.byref(full)) == ok and full.value == base.value + 16
        assert q(16, 480, 640, 22, 256, 2000, ctypes.byref(full)) == ok and full.value == base.value + 16 * 22 * 2000 * 24
        assert q(16, 480, 640, 22, 256, 1000, None) == enull
        for bad in ((0, 480, 640, 22, 256, 1000), (16, 480, 640, 22, 0, 1000), (16, 480, 640, 22, 256, 0), (16, 480, 640, 65, 256, 1000)):
            assert q(*bad, ctypes.byref(full)) == einval, bad
    nul = [None] * 6

    def est3(evaluations=100, min_pixels=10, ref_it=8, ws=None, ws_bytes=0):
        return L.pcnn_pose3d_estimate_polished_fwd(*nul, 1000.0, 0, 0, 1, 8, 8, 4, 16, 1000, 1000, ref_it, 400, 0.01, 0.01, 1024, min_pixels,
                                                   evaluations, *([None] * 8), ws, ws_bytes, None)

    def est2(evaluations=100, min_pixels=10, ref_it=8, ws=None, ws_bytes=0):
        return L.pcnn_pose2d_estimate_polished_fwd(*nul[:5], 0, 0, 1, 8, 8, 4, 16, 1000, 1000, ref_it, 400, 10.0, 10.0, 0.01, 1024, min_pixels,
                                                   evaluations, *([None] * 8), ws, ws_bytes, None)
    for est in (est3, est2):
        assert est(evaluations=6) == einval and est(evaluations=4097) == einval and est(min_pixels=-1) == einval
        assert est() == enull                                          # the polish outputs
        assert est(evaluations=0) == ews                               # no polish output needed: stopped at the workspace
        assert est(evaluations=0, ws=p, ws_bytes=64) == ews
