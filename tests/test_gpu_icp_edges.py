"""GPU tests of the pose-refinement kernels (posecnn_amd/csrc/icp.hip) on the cases of tests/icp_cases.py: every gate side,
degenerate systems, block counts around the segmented sum's boundaries, clipped and trapped score windows, the polish walk at
box widths around NM_LANES. Every case is held to (a) the oracle bit for bit and (b) the expectation the case carries by
construction (integer counts, masks, float64 sums / normal equations / energies within the CPU-measured bounds of
icp_cases.BOUNDS). tests/test_icp_edges_cpu.py proves the cases and the oracle without a GPU.

Evidence that the tests bite — five value-only mutants of icp.hip (one comparison operator, one loop start or one
rounding function each; no address, barrier or widened bound), built in a scratch copy, each run once against this file
(36 tests) and the two older ICP files (16 tests):

  mutant                                                  fails in this file                                            fails in test_gpu_icp.py / test_gpu_icp_render.py
  ------------------------------------------------------  ------------------------------------------------------------  -------------------------------------------------
  terms: border test `(float)u <= border` -> `<`          gates, reduction (all 8 shapes), plane: 10                    real depth frame: 1
  scan: strict `d2 < best` -> `<=`                        score[tie]: 1                                                 none
  segmented sum: tail loop drops its last row             gates, reduction (6 shapes), single inlier, plane, centre     box scenes (3), centre/score[100-131], icp_python
                                                          (all 5 sizes): 14. Not 128x128 (L = 8: no tail) nor 126x128   flow: 5
                                                          (its one tail row is the last block: border rows, all zero)
  centre: strict `fabsf(error) < max_error` -> `<=`       centre[255, 256, 257, 2049]: 4                                none
  centre: `roundf(cx)` -> `rintf(cx)`                     centre[255, 256, 257, 2049]: 4                                none

Wall time of the whole `-m gpu` run on an MI355X: 226 s with this file (717 tests), of which this file takes 2.9 s (its
slowest test 0.3 s, plus 1.8 s of fixture set-up when it runs first) — 223 s before it.
"""
import functools

import numpy as np
import pytest

import icp_cases as C
import oracle
from test_gpu_ops import N, T, same

pytestmark = pytest.mark.gpu
F = np.float32


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _u16(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16)).to(gpu)


# ---- 1. backproject ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.BACKPROJECT_CASES, ids=[c["id"] for c in C.BACKPROJECT_CASES])
def test_backproject_second_trip_and_single_pixel(gpu, case):
    from posecnn_amd import icp
    depth, label = C.backproject_inputs(case)
    got = N(icp.backproject(_u16(gpu, depth), None if label is None else T(gpu, label), C.BACKPROJECT_OBJ, C.BACKPROJECT_K, C.BACKPROJECT_FACTOR))
    same(got, oracle.icp_backproject(depth, label, C.BACKPROJECT_OBJ, C.BACKPROJECT_K, C.BACKPROJECT_FACTOR), "oracle")
    same(got, C.backproject_expected(case), "numpy float32")


# ---- 2. the gates ------------------------------------------------------------------------------------------------------------
def test_refine_gates_one_planted_pixel_per_side(gpu):
    """23 objects in one call (grid.y), live and empty ones mixed: the inlier count of each is the 0 or 1 its row of
    icp_cases.GATE_ROWS states, and an object without inliers keeps the identity bit for bit"""
    from posecnn_amd import icp
    live, pv, pn = C.gate_inputs()
    want_u, want_s = oracle.icp_refine(live, pv, pn, C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=1)
    for pad in (False, True):
        a, b = (C.pad4(pv), C.pad4(pn)) if pad else (pv, pn)
        upd, stats = icp.icp(T(gpu, live), T(gpu, a), T(gpu, b), C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=1, want_stats=True)
        upd, stats = N(upd), N(stats)
        got = stats[:, 0, 0].astype(np.int64)
        assert np.array_equal(got, C.GATE_EXPECT), [(i, g, w) for i, g, w in zip(C.GATE_IDS, got, C.GATE_EXPECT) if g != w]
        for n in np.flatnonzero(C.GATE_EXPECT == 0):
            assert np.array_equal(bits64(upd[n]), bits64(C.IDENTITY34)), C.GATE_IDS[n]
        assert np.array_equal(bits64(upd), bits64(want_u))
        same(stats, want_s, "stats")


# ---- 3. the reduction ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reduction_oracle(H, W, iterations):
    live, pv, pn = C.reduction_inputs(H, W)
    return oracle.icp_refine(live, pv, pn, C.reduction_K(H, W), C.REDUCTION_RANGE, C.REDUCTION_MAX_ERROR, iterations=iterations)


@pytest.mark.parametrize("H,W", C.REDUCTION_SHAPES)
def test_refine_reduction_block_counts(gpu, H, W):
    """nblocks in {1, 2, 7, 8, 9, 63, 64, 65}: empty segments, L = 8 without a tail, L = 9 with a tail of one row; three
    objects, two iterations, 3- and 4-channel maps. First iteration: inlier count = the float64 count (no pixel is near a
    gate), sum r^2 and the update within the CPU-measured bounds of the float64 normal equations"""
    from posecnn_amd import icp
    live, pv, pn = C.reduction_inputs(H, W)
    K = C.reduction_K(H, W)
    ex = C.reduction_expected(H, W)
    cid = C.reduction_id(H, W)
    live_g = T(gpu, live)
    for pad in (False, True):
        a, b = (T(gpu, C.pad4(pv)), T(gpu, C.pad4(pn))) if pad else (T(gpu, pv), T(gpu, pn))
        for iterations in (1, 2):
            upd, stats = icp.icp(live_g, a, b, K, C.REDUCTION_RANGE, C.REDUCTION_MAX_ERROR, iterations=iterations, want_stats=True)
            upd, stats = N(upd), N(stats)
            want_u, want_s = _reduction_oracle(H, W, iterations)
            assert np.array_equal(bits64(upd), bits64(want_u)), (pad, iterations, np.abs(upd - want_u).max())
            same(stats, want_s, "stats")
            if iterations == 1:
                for k in range(C.REDUCTION_N):
                    assert int(stats[k, 0, 0]) == ex[k]["count"], (k, stats[k, 0, 0], ex[k]["count"])
                    d_r2 = abs(float(stats[k, 0, 1]) - ex[k]["sum_r2"]) / ex[k]["sum_r2"]
                    d_up = float(np.abs(upd[k] - ex[k]["update"]).max())
                    print("%s object %d: sum r^2 rel %.3g (bound %.3g), update abs %.3g (bound %.3g)" %
                          (cid, k, d_r2, C.bound(cid, "sum_r2"), d_up, C.bound(cid, "update")))
                    assert d_r2 <= C.bound(cid, "sum_r2") and d_up <= C.bound(cid, "update")


# ---- 4. degenerate systems -------------------------------------------------------------------------------------------------------
def _refine(gpu, inputs, iterations):
    from posecnn_amd import icp
    live, pv, pn = inputs
    upd, stats = icp.icp(T(gpu, live), T(gpu, pv), T(gpu, pn), C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=iterations, want_stats=True)
    want_u, want_s = oracle.icp_refine(live, pv, pn, C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=iterations)
    upd, stats = N(upd), N(stats)
    assert np.isfinite(upd).all()
    assert np.array_equal(bits64(upd), bits64(want_u)), np.abs(upd - want_u).max()
    same(stats, want_s, "stats")
    return upd, stats


def test_refine_all_objects_empty_for_all_iterations(gpu):
    upd, stats = _refine(gpu, C.degenerate_empty_inputs(), 3)
    assert not stats.any()
    for n in range(3):
        assert np.array_equal(bits64(upd[n]), bits64(C.IDENTITY34))


def test_refine_single_inlier(gpu):
    upd, stats = _refine(gpu, C.degenerate_single_inputs(), 1)
    assert stats[0, 0, 0] == 1
    assert float(np.abs(upd[0] - C.degenerate_single_expected()).max()) <= C.bound("degenerate/single-inlier", "update")
    upd, stats = _refine(gpu, C.degenerate_single_inputs(), 3)
    assert (stats[0, :, 0] == 1).all()


def test_refine_fronto_parallel_plane_rank_3(gpu):
    """every normal (0, 0, -1): t_x, t_y and the roll have zero pivots and are dropped; t_z and the two tilts match the
    float64 solve of the reduced system"""
    ex = C.degenerate_plane_expected()
    upd, stats = _refine(gpu, C.degenerate_plane_inputs(), 1)
    for k, e in enumerate(ex):
        assert int(stats[k, 0, 0]) == e["count"]
        d = float(np.abs(upd[k] - e["update"]).max())
        print("plane object %d: update abs %.3g (bound %.3g)" % (k, d, C.bound("degenerate/plane", "update")))
        assert d <= C.bound("degenerate/plane", "update")
    _refine(gpu, C.degenerate_plane_inputs(), 3)


# ---- 5. centre -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", sorted(C.CENTER_SHAPES))
def test_center_plants_and_block_counts(gpu, P):
    from posecnn_amd import icp
    c = C.center_case(P)
    args = [T(gpu, c[k]) for k in ("label", "live", "canon")]
    for pad in (False, True):
        pv, pn = (C.pad4(c["pv"]), C.pad4(c["pn"])) if pad else (c["pv"], c["pn"])
        want_s, want_m = oracle.icp_center(c["label"], c["live"], c["canon"], pv, pn, C.CENTER_OBJ, C.CENTER_MAX_ERROR)
        sums, mask = icp.center(*args, T(gpu, pv), T(gpu, pn), C.CENTER_OBJ, C.CENTER_MAX_ERROR)
        sums, mask = N(sums), N(mask)
        assert np.array_equal(bits64(sums), bits64(want_s)), (sums, want_s)
        same(mask, want_m, "mask vs oracle")
        same(mask, c["mask"], "mask by construction")
        assert sums[3] == c["votes"] and sums[4] == c["pairs"], (sums, c["votes"], c["pairs"])
        d = float(np.abs(sums[:3] - c["sums"]).max())
        print("%s: sums abs %.3g (bound %.3g)" % (c["id"], d, C.bound(c["id"], "sums")))
        assert d <= C.bound(c["id"], "sums")
    sums, mask = icp.center(*args, T(gpu, c["pv"]), T(gpu, c["pn"]), 99, C.CENTER_MAX_ERROR)        # an object with no valid pixel at all
    assert np.array_equal(bits64(N(sums)), bits64(np.zeros(5))) and not N(mask).any()


# ---- 6. score --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.score_cases(), ids=[c["id"] for c in C.score_cases()])
def test_score_windows_probes_ties_and_radius(gpu, case):
    from posecnn_amd import icp
    s = case["scene"]
    hyps = np.stack(case["hyps"])
    got = N(icp.score(T(gpu, s.live), T(gpu, s.canon), T(gpu, s.mask), hyps, s.K, case["radius"]))
    same(got, oracle.icp_score(s.live, s.canon, s.mask, hyps, case["radius"]), "hits vs the exhaustive oracle")
    assert got.tolist() == case["hits"], (got.tolist(), case["hits"], case["why"])


# ---- 7. polish -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.POLISH_CASES, ids=[c["id"] for c in C.POLISH_CASES])
def test_polish_box_widths_and_empty_boxes(gpu, case):
    from posecnn_amd import icp
    label, live, pred = C.polish_inputs(case["id"])
    e64, _ = C.polish_expected(case["id"])
    label_g, live_g = T(gpu, label), T(gpu, live)
    for pc in (3, 4):
        pv = pred if pc == 3 else C.pad4(pred)
        pv_g = T(gpu, pv)
        for budget in C.POLISH_BUDGETS:
            wx, we, wn = oracle.icp_polish(label, live, pv, C.POLISH_OBJ, C.POLISH_RANGE, budget)
            U, ge, gn, gx = icp.polish(label_g, live_g, pv_g, C.POLISH_OBJ, C.POLISH_RANGE, budget)
            assert gn == wn == budget, (pc, budget, gn, wn)
            assert np.array_equal(bits64(ge), bits64(we)), (pc, budget, ge, we)
            assert np.array_equal(bits64(gx), bits64(wx)), (pc, budget, gx, wx)
            assert np.isfinite(gx).all() and np.isfinite(U).all()
            if budget == 8:
                print("%s pc %d: energy abs %.3g (bound %.3g)" % (case["id"], pc, abs(ge - e64), C.bound(case["id"], "energy")))
                assert abs(ge - e64) <= C.bound(case["id"], "energy")
            if case.get("no_depth"):
                assert ge == 0.0


# ---- 8. the driver ---------------------------------------------------------------------------------------------------------------
def test_refine_poses_with_nothing_to_do(gpu):
    """every ROI skipped (class 0, or under 400 label pixels) and an empty ROI list: all zeros, nothing rendered, no launch error"""
    import torch
    from posecnn_amd import icp
    H, W = 24, 32
    label = np.zeros((H, W), np.int32)
    label[:10, :30] = 5                                  # 300 pixels: under min_pixels
    depth = np.full((H, W), 7000, np.uint16)
    calls = []

    def render(cls, Tco):
        calls.append(cls)
        raise AssertionError("a skipped ROI was rendered")

    rois = np.array([[0, 0, 0, 0, 1, 1, 1], [0, 5, 0, 0, 1, 1, 1], [0, 9, 0, 0, 1, 1, 1]], F)
    poses = np.zeros((3, 7), F)
    poses[:, 0] = 1
    out = icp.refine_poses(label, depth, C.GATE_K, 10000.0, rois, poses, render, device=gpu)
    assert out.shape == (3, 7) and out.dtype == np.float32 and not out.any() and not calls
    out = icp.refine_poses(label, depth, C.GATE_K, 10000.0, np.zeros((0, 7), F), np.zeros((0, 7), F), render, device=gpu)
    assert out.shape == (0, 7) and not calls
    torch.cuda.synchronize()
