"""The audit of tests/icp_cases.py; needs no GPU.

  1. The constants the cases restate (ICP_BLOCK, ICP_NSEG, NM_LANES, ICP_CH and the backproject grid cap) are read out of
     posecnn_amd/csrc/icp.hip: a retune fails here instead of silently moving a boundary away from its cases.
  2. Every case reaches the regime it claims: block counts and segment lengths, the planted pixel exactly on its gate or one
     ulp beside it, empty probes, clipped windows, the walk of the polish through its box.
  3. The oracle meets every by-construction expectation — integers exactly, float64 values within the bound recorded next to
     the measured distance in icp_cases.BOUNDS. tests/test_gpu_icp_edges.py then holds the library to the oracle bit for bit
     and to the same expectations.
"""
import numpy as np
import pytest

import icp_cases as C
import oracle
import thresholds

F = np.float32


# ---- 1. constants ------------------------------------------------------------------------------------------------------
def test_restated_constants_equal_the_kernel_source():
    src = thresholds.parse_constants(C.ICP_HIP)
    for name, value in C.CONSTANTS.items():
        assert name in src, "no `constexpr int %s` in icp.hip" % name
        assert src[name] == value, "icp_cases says %s = %d, icp.hip says %d" % (name, value, src[name])
    assert C.parse_backproject_grid_cap() == C.BACKPROJECT_GRID_CAP
    with open(C.ICP_HIP) as fh:
        text = fh.read()
    assert "__launch_bounds__(256) void icp_backproject_kernel" in text and "i += (long long)gridDim.x * 256" in text


def test_bounds_are_four_times_the_measured_distance():
    for cid, row in C.BOUNDS.items():
        for what, (measured, bound) in row.items():
            assert bound == pytest.approx(4 * measured, rel=1e-9), (cid, what)


# ---- backproject ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.BACKPROJECT_CASES, ids=[c["id"] for c in C.BACKPROJECT_CASES])
def test_backproject_case(case):
    assert C.backproject_trips(case["H"], case["W"]) == case["trips"]
    depth, label = C.backproject_inputs(case)
    assert (label is not None) == case["masked"]
    if case["H"] * case["W"] > 1:
        assert depth.min() == 0 and depth.max() == 65535
        second = depth.reshape(-1)[C.BACKPROJECT_GRID_CAP * 256:]            # pixels only the second trip reaches
        assert second.size == 1024 and second[-1] == 65535 and second[-2] == 0
    assert float(F(C.BACKPROJECT_FACTOR)) == C.BACKPROJECT_FACTOR and np.log2(C.BACKPROJECT_FACTOR) % 1 != 0
    want = C.backproject_expected(case)
    got = oracle.icp_backproject(depth, label, C.BACKPROJECT_OBJ, C.BACKPROJECT_K, C.BACKPROJECT_FACTOR)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if case["masked"] and case["H"] > 1:
        assert (got[..., 2][label != C.BACKPROJECT_OBJ] == 0).all() and (got[..., 2] > 0).sum() > 300000


# ---- the gates -------------------------------------------------------------------------------------------------------------
def test_gate_table_is_complete():
    assert len(C.GATE_ROWS) >= 20 and len(set(C.GATE_IDS)) == len(C.GATE_IDS)
    assert 0 < C.GATE_EXPECT.sum() < len(C.GATE_ROWS)                         # live and empty objects in one call
    assert len({C.gate_pixel(n) // C.ICP_BLOCK for n in range(len(C.GATE_ROWS))}) == C.nblocks(C.GATE_H, C.GATE_W) == 3


@pytest.mark.parametrize("n", range(len(C.GATE_ROWS)), ids=C.GATE_IDS)
def test_gate_pixel_sits_on_its_gate(n):
    """the planted quantity equals the stated value bit for bit, and that value is the threshold or its float32 neighbour;
    every OTHER gate passes with room, so the expected 0 / 1 hangs on the planted comparison alone"""
    cid, _, what, value, threshold, expect, *_ = C.GATE_ROWS[n]
    if what is None:
        return
    q = C.gate_quantities(n)
    if np.isnan(value):
        assert np.isnan(q[what])
    else:
        assert F(q[what]).view(np.uint32) == F(value).view(np.uint32), (cid, q[what], value)
        if cid != "live=0":
            assert value in (threshold, C.up(threshold), C.down(threshold)), cid
    znear, zfar = F(C.GATE_RANGE[0]), F(C.GATE_RANGE[1])
    roomy = dict(pvz=znear * 1.01 < q["pvz"] < zfar * 0.99, projx=2.6 < q["projx"] < 28.4, projy=2.6 < q["projy"] < 20.4,
                 ldepth=znear * 1.01 < q["ldepth"] < zfar * 0.99, negdot=q["negdot"] > 0.15, abserr=q["abserr"] < 0.9 * C.GATE_MAX_ERROR)
    for other, ok in roomy.items():
        if other == what or (what == "pvz" and np.isnan(value)):
            continue
        if what in ("pvz", "ldepth") and other in ("pvz", "ldepth") and cid != "live=0":
            continue      # the two depths sit together at the range's end; the partner is on the passing side (checked below)
        assert ok, (cid, other, q[other])
    if what in ("pvz", "ldepth") and not np.isnan(value) and cid != "live=0":
        partner = q["ldepth" if what == "pvz" else "pvz"]
        assert znear <= partner <= zfar, (cid, partner)


def test_gates_oracle_counts_and_identity():
    live, pv, pn = C.gate_inputs()
    upd, stats = oracle.icp_refine(live, pv, pn, C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=1)
    got = stats[:, 0, 0].astype(np.int64)
    assert np.array_equal(got, C.GATE_EXPECT), [(i, g, w) for i, g, w in zip(C.GATE_IDS, got, C.GATE_EXPECT) if g != w]
    for n in np.flatnonzero(C.GATE_EXPECT == 0):
        assert np.array_equal(upd[n].view(np.uint64), C.IDENTITY34.view(np.uint64)), C.GATE_IDS[n]
    assert np.isfinite(upd).all()
    # the per-pixel exit reason the oracle reports agrees with the gate each row names
    reason = {":60": 1, ":81": 2, ":60/:81": 2, ":92": 3, ":104": 4, ":115": 5}
    q, t = oracle.icp_se3f(C.IDENTITY34)
    for n, row in enumerate(C.GATE_ROWS):
        if row[2] is None:
            continue
        _, _, why = oracle.icp_terms(live[n], pv[n], pn[n], q, t, C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR)
        assert why.reshape(-1)[C.gate_pixel(n)] == (0 if row[5] else reason[row[1]]), row[0]


# ---- the reduction ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", C.REDUCTION_SHAPES)
def test_reduction_case(H, W):
    nb, L = C.REDUCTION_CLAIMS[(H, W)]
    assert C.nblocks(H, W) == nb and C.segment_length(nb) == L
    live, pv, pn = C.reduction_inputs(H, W)
    K = C.reduction_K(H, W)
    ex = C.reduction_expected(H, W)
    upd, st = oracle.icp_refine(live, pv, pn, K, C.REDUCTION_RANGE, C.REDUCTION_MAX_ERROR, iterations=1)
    cid = C.reduction_id(H, W)
    for k in range(C.REDUCTION_N):
        # no pixel within 1e-4 (relative; of a pixel for the projection) of any gate: the float64 count is the only possible count
        assert min(ex[k]["margins"].values()) > 1e-4, (k, ex[k]["margins"])
        interior = (H - 6) * (W - 6)
        assert 0.9 * interior < ex[k]["count"] < interior, (k, ex[k]["count"], interior)           # most pixels, not all
        assert int(st[k, 0, 0]) == ex[k]["count"]
        d_r2 = abs(float(st[k, 0, 1]) - ex[k]["sum_r2"]) / ex[k]["sum_r2"]
        d_up = float(np.abs(upd[k] - ex[k]["update"]).max())
        print("%s object %d: inliers %d, sum r^2 rel %.3g, update abs %.3g" % (cid, k, ex[k]["count"], d_r2, d_up))
        assert d_r2 <= C.bound(cid, "sum_r2") and d_up <= C.bound(cid, "update")
        assert np.abs(ex[k]["x"]).max() > 1e-3                                                        # a real step, not the identity
    if nb >= C.ICP_NSEG * 8:        # rows reach the unrolled body; every block has inliers, so a dropped row changes the count
        q, t = oracle.icp_se3f(C.IDENTITY34)
        _, _, why = oracle.icp_terms(live[0], pv[0], pn[0], q, t, K, C.REDUCTION_RANGE, C.REDUCTION_MAX_ERROR)
        per_block = np.add.reduceat((why.reshape(-1) == 0).astype(np.int64), np.arange(0, H * W, C.ICP_BLOCK))
        assert (per_block[2:-2] > 0).all()
        assert np.array_equal(why == 0, ex[0]["inliers"])


# ---- degenerate systems ------------------------------------------------------------------------------------------------------
def test_degenerate_all_empty():
    live, pv, pn = C.degenerate_empty_inputs()
    upd, st = oracle.icp_refine(live, pv, pn, C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=3)
    assert not st.any()
    for n in range(3):
        assert np.array_equal(upd[n].view(np.uint64), C.IDENTITY34.view(np.uint64))


def test_degenerate_single_inlier():
    live, pv, pn = C.degenerate_single_inputs()
    upd, st = oracle.icp_refine(live, pv, pn, C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=1)
    assert st[0, 0, 0] == 1 and np.isfinite(upd).all()
    d = float(np.abs(upd[0] - C.degenerate_single_expected()).max())
    print("single inlier: update abs %.3g" % d)
    assert d <= C.bound("degenerate/single-inlier", "update")
    upd3, st3 = oracle.icp_refine(live, pv, pn, C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=3)
    assert np.isfinite(upd3).all() and (st3[0, :, 0] == 1).all()


def test_degenerate_plane():
    live, pv, pn = C.degenerate_plane_inputs()
    ex = C.degenerate_plane_expected()
    upd, st = oracle.icp_refine(live, pv, pn, C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=1)
    for k, e in enumerate(ex):
        assert min(e["margins"].values()) > 1e-4 and int(st[k, 0, 0]) == e["count"] == (C.GATE_H - 6) * (C.GATE_W - 6)
        assert np.abs(e["x"][list(C.PLANE_COLUMNS)]).min() > 1e-4          # t_z and both tilts are really exercised
        d = float(np.abs(upd[k] - e["update"]).max())
        print("plane object %d: update abs %.3g" % (k, d))
        assert d <= C.bound("degenerate/plane", "update")
        # rank 3: the full float64 Jacobian has exactly three non-zero columns
        full = C.refine_f64(live[k], pv[k], pn[k], C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR)
        assert np.allclose(full["x"][[0, 1, 5]], 0, atol=1e-12)
    upd3, _ = oracle.icp_refine(live, pv, pn, C.GATE_K, C.GATE_RANGE, C.GATE_MAX_ERROR, iterations=3)
    assert np.isfinite(upd3).all()


# ---- centre --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", sorted(C.CENTER_SHAPES))
def test_center_case(P):
    c = C.center_case(P)
    assert c["H"] * c["W"] == P and c["nblocks"] == -(-P // C.ICP_BLOCK)
    if P > 1:
        flat = c["mask"].reshape(-1)
        for i, plant in enumerate(C.CENTER_PLANTS):
            assert flat[i] == plant[7], plant[0]
        assert 0.5 * P < c["votes"] < c["pairs"] < P
        assert np.float32(1e-45) > 0 and np.float32(1e-45) == np.nextafter(F(0), F(1))
        # no unplanted pixel near the strict error test: |error| <= max / 4 (+ rounding) or >= 2 max
        d = c["live"].astype(np.float64) - c["pv"].astype(np.float64)
        err = np.abs(np.sum(c["pn"].astype(np.float64) * d, axis=-1)).reshape(-1)[len(C.CENTER_PLANTS):] / C.CENTER_MAX_ERROR
        assert ((err < 0.26) | (err > 1.9)).all()
    sums, mask = oracle.icp_center(c["label"], c["live"], c["canon"], c["pv"], c["pn"], C.CENTER_OBJ, C.CENTER_MAX_ERROR)
    assert np.array_equal(mask, c["mask"])
    assert sums[3] == c["votes"] and sums[4] == c["pairs"]
    d = float(np.abs(sums[:3] - c["sums"]).max())
    print("%s: pairs %d votes %d, sums abs %.3g" % (c["id"], c["pairs"], c["votes"], d))
    assert d <= C.bound(c["id"], "sums")
    sums, mask = oracle.icp_center(c["label"], c["live"], c["canon"], c["pv"], c["pn"], 99, C.CENTER_MAX_ERROR)    # an object with no pixel
    assert not sums.any() and not mask.any()


# ---- score ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.score_cases(), ids=[c["id"] for c in C.score_cases()])
def test_score_case(case):
    s = case["scene"]
    hits64, pairs = C.score_f64(case)
    assert hits64 == case["hits"], (hits64, case["why"])
    got = oracle.icp_score(s.live, s.canon, s.mask, np.stack(case["hyps"]), case["radius"])
    assert got.tolist() == case["hits"]
    live = s.live.astype(np.float64)
    if case["id"] == "corners":
        clipped = set()
        for y, x in zip(*np.nonzero(s.mask & np.isfinite(s.canon[..., 0]))):
            (x0, x1, y0, y1), raw = C.score_window(s.canon[y, x], case["radius"], s.K, s.H, s.W)
            clipped.add((raw[0] < 0, raw[1] > s.W - 1, raw[2] < 0, raw[3] > s.H - 1))
        for want in ((True, False, True, False), (False, True, True, False), (True, False, False, True), (False, True, False, True),
                     (True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)):
            assert want in clipped, want      # each corner and each single edge clips some query's window
    if case["id"] == "probe-trap":
        t = case["trap"]
        qy, qx = t["q"]
        assert not s.mask[qy - 2:qy + 3, qx - 2:qx + 3].any()                                # 5 x 5 probe empty
        assert abs(t["a"][1] - qx) <= 6 < abs(t["b"][1] - qx)                                  # A inside the 13 x 13 probe, B outside
        q = s.ray(qx, qy, 0.7).astype(np.float64)
        da, db = np.linalg.norm(live[t["a"]] - q), np.linalg.norm(live[t["b"]] - q)
        assert db < 0.9 * da and da < 0.99 * case["radius"] and abs(live[t["a"]][2] - q[2]) < 0.95 * case["radius"]
        assert pairs[0][0][1] == t["b"][0] * s.W + t["b"][1] and pairs[0][1][1] == t["a"][0] * s.W + t["a"][1]
    if case["id"] == "tie":
        q = s.canon[40, 5]
        d2 = [((s.live[p][0] - q[0]) * (s.live[p][0] - q[0]) + (s.live[p][1] - q[1]) * (s.live[p][1] - q[1])) +
              (s.live[p][2] - q[2]) * (s.live[p][2] - q[2]) for p in (case["tie"]["lo"], case["tie"]["hi"])]
        assert F(d2[0]).view(np.uint32) == F(d2[1]).view(np.uint32) and d2[0] < F(case["radius"]) * F(case["radius"])
        q2 = s.canon[40, 6].astype(np.float64)
        assert np.linalg.norm(live[case["tie"]["hi"]] - q2) < 0.95 * case["radius"] and np.linalg.norm(live[case["tie"]["lo"]] - q2) > 1.05 * case["radius"]
    if case["id"].startswith("on-radius"):
        ez = s.live[20, 30, 2] - s.canon[40, 5, 2]
        assert ez == F(2.0 ** -6) and (F(case["radius"]) == ez or F(case["radius"]) == C.up(ez))
    if case["id"] == "hypotheses":
        assert len(case["hyps"]) == 9
        mz = s.canon[20, 28, 2]
        assert mz + case["hyps"][1][11] == F(2 * case["radius"]) and mz + case["hyps"][2][11] < 0
        shared = [k for _, k in pairs[6]]
        assert len(shared) == 36 and len(set(shared)) == 30                                  # two model points, one depth point
    if case["id"] == "last-pixel":
        P = s.H * s.W
        assert P % 32 != 0 and pairs[0] == [(0, P - 1)]


# ---- polish --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.POLISH_CASES, ids=[c["id"] for c in C.POLISH_CASES])
def test_polish_case(case):
    label, live, pred = C.polish_inputs(case["id"])
    ys, xs = np.nonzero(label == C.POLISH_OBJ)
    bw = xs.max() - xs.min() + 1
    y0, y1, x0, x1 = case["box"]
    assert (ys.min(), ys.max() + 1, xs.min(), xs.max() + 1) == (y0, y1, x0, x1) and bw == case["bw"]
    assert (C.NM_LANES // bw, C.NM_LANES % bw) == case["walk"]
    if case["id"] == "polish/one-pixel-first":
        assert label.reshape(-1)[0] == C.POLISH_OBJ
    if case["id"] == "polish/one-pixel-last":
        assert label.reshape(-1)[-1] == C.POLISH_OBJ
    e64, n0 = C.polish_expected(case["id"])
    if case.get("no_depth"):
        assert n0 == 0 and e64 == 0.0
    else:
        assert n0 > 0 and e64 > 1e-3
    if case.get("holes"):
        box = (slice(y0, y1), slice(x0, x1))
        assert np.isnan(pred[box][label[box] == C.POLISH_OBJ]).any() and (label[box] != C.POLISH_OBJ).any()
    for pc in (3, 4):
        pv = pred if pc == 3 else C.pad4(pred)
        x, e, evals = oracle.icp_polish(label, live, pv, C.POLISH_OBJ, C.POLISH_RANGE, 8)
        assert evals == 8 and np.isfinite(x).all()
        d = abs(e - e64)
        print("%s pc %d: energy %.9g, float64 %.9g, abs %.3g" % (case["id"], pc, e, e64, d))
        assert d <= C.bound(case["id"], "energy")
        x, e, evals = oracle.icp_polish(label, live, pv, C.POLISH_OBJ, C.POLISH_RANGE, 50)
        assert evals == 50 and np.isfinite(x).all() and e <= e64 + C.bound(case["id"], "energy")
        if case.get("no_depth"):
            assert e == 0.0
