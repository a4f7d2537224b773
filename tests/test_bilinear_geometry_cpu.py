"""The preconditions of tests/test_gpu_bilinear_geometry.py; needs no GPU.

  1. The host mirror of make_taps (tests/bilinear_geometry.py) against dense arithmetic the kernels never saw:
     torch.nn.functional.conv_transpose2d in float64 on the make_deconv_filter weights; and the C oracle's deconv, the
     reference of the GPU tests, against that mirror and against exact.deconv_reference at every geometry of the table.
  2. Every row of the table reaches the branch it is there for: tap counts, staged columns within the tile, a second trip
     of the staging loop, odd first pixels.
  3. The dynamic LDS the label head and label_head_loss ask for, over every (kernel, stride, classes) their argument
     checks admit; the tile ladder of vertex_head_loss and the bounds of its static LDS arrays.
  4. The numpy references of the two fused losses against float64 autograd at the new geometries, and the conditions
     the inputs must meet (hard-label pixels on both sides of the threshold, both smooth-L1 branches, Hough detections
     from pixels with more than two taps)."""
import os

import numpy as np
import pytest

import bilinear_geometry as G
import exact
import grad_ref
import label_loss_ref as LR
import oracle
import thresholds
import vertex_head_ref as VR

F = np.float32
CASE_IDS = [G.case_id(c) for c in G.cases()]


def test_restated_constants_equal_the_kernel_sources():
    src = {f: thresholds.parse_constants(os.path.join(thresholds.CSRC, f)) for f in ("label_head_device.h", "vertex_head_loss.hip")}
    assert src["label_head_device.h"]["LH_SEG"] == G.UP_SEG          # the one segment length of upscore.hip and label_loss.hip
    for f in ("upscore.hip", "label_loss.hip"):
        text = open(os.path.join(thresholds.CSRC, f)).read()
        assert '#include "label_head_device.h"' in text and "label_head_plan(B, H, W, C, k, s)" in text
        assert "constexpr int UP_SEG" not in text and "constexpr int LL_SEG" not in text
    assert src["vertex_head_loss.hip"]["VH_FOOTPRINT"] == G.VH_FOOTPRINT and src["vertex_head_loss.hip"]["VH_THREADS"] == 256
    text = open(os.path.join(thresholds.CSRC, "vertex_head_loss.hip")).read()
    assert "{{4, 8}, {4, 4}, {2, 4}, {2, 2}, {1, 2}, {1, 1}}" in text and "s_row[3 * 64]" in text and "s_tap[64]" in text
    assert "sh <= 160 * 1024" in open(os.path.join(thresholds.CSRC, "upscore.hip")).read()
    assert "p->sh_all + 4096 <= 160 * 1024" in open(os.path.join(thresholds.CSRC, "label_loss.hip")).read()
    assert VR.tile_shape(20, 10) == (4, 4) and [VR.GEOMETRY_CASES[G.vertex_name(*ks)][3:5] for ks, _ in G.VERTEX_LADDER] == [ks for ks, _ in G.VERTEX_LADDER]


# ---- 1. make_taps and the oracle against dense arithmetic -------------------------------------------------------------
@pytest.mark.parametrize("ks", G.KS, ids=["k%ds%d" % ks for ks in G.KS])
def test_host_make_taps_equals_conv_transpose_in_float64(ks):
    """The matrix of the mirror's taps against conv_transpose2d applied to the identity: the filter is make_deconv_filter's
    1-D profile rounded to float32 as the network stores it, every output is one product by 1.0, so equality is exact."""
    import torch
    from posecnn_amd.networks import make_deconv_filter_1d
    k, s = ks
    f32 = make_deconv_filter_1d(k).astype(F)
    assert np.array_equal(f32, G.tap_table(k)) and np.array_equal(f32, VR.taps_table(k))
    assert G.is_dyadic(k) == bool(np.array_equal(f32.astype(np.float64), make_deconv_filter_1d(k)))
    for n_in in (G.H_LOW,) + G.WIDTHS[s]:
        eye = torch.eye(n_in, dtype=torch.float64).reshape(n_in, 1, n_in, 1)            # n_in images of n_in x 1, one channel
        w = torch.from_numpy(f32.astype(np.float64)).reshape(1, 1, k, 1)
        dense = torch.nn.functional.conv_transpose2d(eye, w, None, stride=(s, 1), padding=((k - s) // 2, 0))
        assert tuple(dense.shape) == (n_in, 1, n_in * s, 1)
        assert np.array_equal(dense[:, 0, :, 0].numpy().T, G.dense_matrix(k, s, n_in)), (ks, n_in)


def _int_input(c, C=3):
    k, s, w = c
    rng = np.random.default_rng([k, s, w])
    shape = (G.B, G.H_LOW, w, C)
    out = (G.B, G.H_LOW * s, w * s, C)
    return [rng.integers(-64, 65, sh).astype(F) for sh in (shape, out, out, (C,))]


@pytest.mark.parametrize("c", G.cases(), ids=CASE_IDS)
def test_oracle_deconv_is_pinned_at_every_geometry(c):
    """oracle.deconv_bilinear on integers in [-64, 64] against (a) the mirror's matrices applied in float64 and (b)
    exact.deconv_reference, plain and with both addends, the bias and the ReLU.

    Dyadic taps (f a power of two: multiples of 1/(2f), at most 4 x 4 products of at most 2^-0 x 64 each in units of
    1/(4 f^2) <= 1/4096: below 2^24 units): every float32 operation is exact, the comparison is equality. The three
    geometries with f = 3 or 7 have taps that float32 rounds; there each term carries the two taps' roundings, the
    product's and the multiplication's (4 x 2^-24 relative), and the <= 16 additions at most 16 x 2^-24 of the sum of
    magnitudes: |oracle - float64| <= 20 x 2^-24 x deconv_reference(absolute=True). Against the mirror, whose taps are
    the float32 ones, the two tap roundings drop out; the same bound is kept."""
    import torch
    k, s, w = c
    x, a1, a2, b = _int_input(c)
    uy, ux = G.dense_matrix(k, s, G.H_LOW), G.dense_matrix(k, s, w)
    t = torch.from_numpy
    for extras in (False, True):
        kw = dict(add1=a1, add2=a2, bias=b, relu=True) if extras else {}
        got = oracle.deconv_bilinear(x, k, s, **kw).astype(np.float64)
        mirror = np.einsum("oh,bhwc,pw->bopc", uy, x.astype(np.float64), ux)
        if extras:
            mirror = np.maximum(mirror + a1 + a2 + b, 0)
        ref = exact.deconv_reference(t(x), k, s, **{n: t(v) if isinstance(v, np.ndarray) else v for n, v in kw.items()}).numpy()
        if G.is_dyadic(k):
            assert np.array_equal(got, mirror) and np.array_equal(got, ref), c
        else:
            mag = exact.deconv_reference(t(x), k, s, absolute=True, **{n: t(v) for n, v in kw.items() if n != "relu"}).numpy()
            tol = 20 * 2.0 ** -24 * mag
            assert (np.abs(got - mirror) <= tol).all() and (np.abs(got - ref) <= tol).all(), c
            assert not np.array_equal(got, ref)                # (the rounding of the taps is real: equality would be an accident)


@pytest.mark.parametrize("c", G.cases(), ids=CASE_IDS)
def test_oracle_deconv_backward_is_the_transpose(c):
    """oracle.deconv_bilinear_bwd against the transposed mirror matrices in float64, on integers small enough that a cell's
    k x k gather is exact for dyadic taps: at most (sum of the 1-D taps)^2 |g| in units of 1/(4 f^2)."""
    k, s, w = c
    gmax = G.exact_gradient_range(k)
    assert gmax == (2 if k == 64 else 8)
    rng = np.random.default_rng([k, s, w, 1])
    g = rng.integers(-gmax, gmax + 1, (G.B, G.H_LOW * s, w * s, 3)).astype(F)
    got = oracle.deconv_bilinear_bwd(g, k, s).astype(np.float64)
    uy, ux = G.dense_matrix(k, s, G.H_LOW), G.dense_matrix(k, s, w)
    ref = np.einsum("oh,bopc,pw->bhwc", uy, g.astype(np.float64), ux)
    if G.is_dyadic(k):
        assert np.array_equal(got, ref), c
    else:                                                      # one product's and one multiplication's rounding per term, k^2 additions
        mag = np.einsum("oh,bopc,pw->bhwc", uy, np.abs(g).astype(np.float64), ux)
        assert (np.abs(got - ref) <= (2 + k * k) * 2.0 ** -24 * mag).all(), c


# ---- 2. every row reaches its branch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.TABLE, ids=["k%ds%d" % r[0] for r in G.TABLE])
def test_row_shows_the_tap_counts_it_claims(row):
    (k, s), claim, _ = row
    assert G.accepted(k, s) and k <= G.MAX_KERNEL
    for w in G.WIDTHS[s]:
        counts = set(G.tap_counts(k, s, w)) | set(G.tap_counts(k, s, G.H_LOW))
        assert counts == claim, (k, s, w, counts)
        assert max(G.tap_counts(k, s, w)) == max(claim)        # the full count occurs along the row, where the unrolled jx loop runs
    if k in (7, 5):                                            # mixed rows: both counts inside one segment, away from the borders
        inner = set(G.tap_counts(k, s, G.WIDTHS[s][0])[2 * s:3 * s + 3])
        assert len(inner) == 2, inner


def test_the_table_holds_every_tap_count_and_every_parity():
    ks = set(G.KS)
    assert {(1, 1), (2, 2), (13, 13), (4, 2), (16, 8), (64, 32), (3, 1), (6, 2), (8, 2), (64, 16), (7, 3), (5, 3)} == ks
    assert {max(r[1]) for r in G.TABLE} == {1, 2, 3, 4}
    assert any(k % 2 and s % 2 for k, s in ks) and any(k == 64 and 4 in claim for (k, s), claim, _ in G.TABLE)
    assert len(G.tap_table(64)) == 64
    for k, s, w in G.cases():
        segs = G.segments(w, k, s)
        if (s, w) == (1, 127):                                 # the other odd Wo: one segment, one pixel short of full
            assert segs[0][:2] == (0, 127) and len(segs) == 1
            continue
        assert len(segs) == 2 and segs[0][1] == G.UP_SEG and 0 < segs[1][1] <= 32, (k, s, w, segs)   # one boundary, a short last segment
    assert sorted(w * 1 % 2 for w in G.WIDTHS[1]) == [1, 1] and {w for w in G.WIDTHS[1]} == {129, 127}


@pytest.mark.parametrize("c", G.cases(), ids=CASE_IDS)
def test_staged_columns_fit_the_tile(c):
    k, s, w = c
    p = G.label_head_plan(w, 1, k, s)
    assert max(G.tap_counts(k, s, G.H_LOW)) <= p["rows"]
    for ox0, npx, cx0, ncx in G.segments(w, k, s):
        assert 1 <= ncx <= p["ncx_max"] and cx0 + ncx <= w, (c, ox0, ncx, p)
        for ox in range(ox0, ox0 + npx):                       # every pixel's taps lie inside the staged columns
            lo, n, _ = G.make_taps(ox, k, s, w)
            assert cx0 <= lo and lo + n <= cx0 + ncx
    if (k, s) == (3, 1) and w == 129:
        assert max(seg[3] for seg in G.segments(w, k, s)) == 129 and p["ncx_max"] == 131     # 128 pixels + 1, the row ends there


def test_the_staging_loop_takes_a_second_trip_in_each_kernel():
    per_trip = 4 * G.UP_SEG
    fixed = {c: G.staging_elements(G.H_LOW, c[2], 22, c[0], c[1], True) for c in G.cases()}
    gen24 = {c: G.staging_elements(G.H_LOW, c[2], 5, c[0], c[1], False) for c in G.cases()}
    gen64 = {c: G.staging_elements(G.H_LOW, c[2], 25, c[0], c[1], False) for c in G.cases()}
    for name, tot in (("fixed", fixed), ("generic<24>", gen24), ("generic<64>", gen64)):
        assert max(tot.values()) > per_trip and min(tot.values()) <= per_trip, (name, tot)     # one trip and more than one both occur
    assert fixed[(3, 1, 129)] > 2 * per_trip                   # 3 rows x 129 cells x 11 pairs: the clamped tail loads of a third trip


def test_odd_first_pixels_occur_where_the_stride_is_odd():
    """up_copy_out picks wide or single stores per segment from (npx C | 128 C) & 3 and the address of pix0 C floats."""
    for k, s, w in G.cases():
        odd = [p for p in G.first_pixels(G.B, G.H_LOW, w, k, s) if p % 2]
        if s in (1, 3):
            assert (w * s) % 2 == 1 and odd, (k, s, w)
            for C in (22, 5, 25, 64):
                sides = {(p * C * 4) % 16 == 0 and (min(G.UP_SEG, w * s - p % (w * s)) * C) % 4 == 0
                         for p in G.first_pixels(G.B, G.H_LOW, w, k, s)}
                if C in (22, 25) and w != 127:
                    assert sides == {True, False}, (k, s, w, C)     # both sides of the test inside one launch
                if C == 22 and w == 127:
                    assert sides == {False}                         # 127 x 22 floats: never a multiple of four
        else:
            assert not odd


# ---- 3. LDS bytes and the vertex ladder --------------------------------------------------------------------------------
def test_label_head_lds_bytes():
    for (k, s), C, nbytes in G.LDS_CASES:
        assert G.label_head_plan(G.WIDTHS[s][0], C, k, s)["lds_bytes"] == nbytes
        assert G.label_loss_plan(G.WIDTHS[s][0], C, k, s)["sh_bwd"] == nbytes
    assert 66560 > 64 * 1024 and G.label_head_plan(65, 63, 4, 2)["lds_bytes"] <= 64 * 1024
    worst = (0, None)
    for s in range(1, G.MAX_KERNEL + 1):
        for k in range(s, min(4 * s, G.MAX_KERNEL) + 1):
            if not G.accepted(k, s):
                continue
            for C in range(1, G.MAX_CLASSES + 1):
                p = G.label_loss_plan(1, C, k, s)
                assert p["lds_bytes"] <= G.LDS_LIMIT and p["fits"], (k, s, C, p)
                worst = max(worst, (p["lds_bytes"], (k, s, C)))
    assert worst == (133376, (3, 1, 64))                       # the refusal "tile does not fit LDS" is unreachable for C <= 64


@pytest.mark.parametrize("ks,rung", G.VERTEX_LADDER, ids=[G.vertex_name(*ks) for ks, _ in G.VERTEX_LADDER])
def test_vertex_head_ladder(ks, rung):
    k, s = ks
    assert G.accepted(k, s, limit=2) and k <= G.MAX_KERNEL
    B, H, W = VR.GEOMETRY_CASES[G.vertex_name(k, s)][:3]
    p = G.vertex_plan(k, s, H, W)
    assert p["rung"] == rung and (p["th"], p["tw"]) == VR.tile_shape(k, s) == (G.VH_LADDER[rung] if rung is not None else (1, 1))
    if rung is None:
        assert p["footprint"] == k * k > G.VH_FOOTPRINT and p["footprint"] in (4096, 3136)
    else:
        assert p["footprint"] <= G.VH_FOOTPRINT
        if rung > 0:                                           # the rung above does not fit: the choice is forced
            a, b = G.VH_LADDER[rung - 1]
            assert (a * s + k - s) * (b * s + k - s) > G.VH_FOOTPRINT
    assert p["nth"] * s <= 64 and 3 * p["nth"] * s <= 256      # s_row[3 * 64]; one thread per (channel, row) of the dbias sums
    assert p["th"] * s <= 64 and k <= 64                       # s_tap[64]
    assert p["shmem"] == (13 * p["footprint"] + 15) // 16 * 16 <= 64 * 1024
    assert p["clipped_y"] == (p["th"] > 1) and p["clipped_x"] == (p["tw"] > 1)      # 5 x 9 cells: every multi-cell tile is ragged
    assert p["tiles_y"] * p["tiles_x"] > 1


def test_vertex_head_ladder_over_every_accepted_geometry():
    for s in range(1, 65):
        for k in range(s, min(2 * s, 64) + 1):
            if G.accepted(k, s, limit=2):
                p = G.vertex_plan(k, s)
                assert p["th"] * s <= 64 and 3 * p["th"] * s <= 256 and p["footprint"] <= 4096 and p["shmem"] <= 53248, (k, s, p)


# ---- 4. the references at the new geometries ---------------------------------------------------------------------------
def head_cases():
    """Every (k, s, w, C) the label-head tests of the GPU file launch."""
    out = [c + (C,) for c in G.cases() for C in G.HEAD_CLASSES]
    out += [(k, s, G.WIDTHS[s][0], C) for (k, s) in G.DISPATCH_KS for C in G.DISPATCH_CLASSES]
    out += [(k, s, G.WIDTHS[s][0], C) for (k, s), C, _ in G.LDS_CASES]
    out += [(k, s, w, C) for (k, s, w) in G.cases(((1, 1), (3, 1))) for C in (22, 25)]
    return sorted(set(out))


def test_label_head_inputs_put_ground_truth_zero_on_both_sides_of_the_threshold():
    for k, s, w, C in head_cases():
        d = G.head_case(k, s, w, C)                            # (asserts the threshold condition and a gated ReLU itself)
        gt, hard = d["gt"], d["hard"]
        zero = gt == 0
        assert hard[zero][:, 0].any() and not hard[zero][:, 0].all(), (k, s, w, C)
        assert ((gt < 0) | (gt >= C)).any() and not hard[(gt < 0) | (gt >= C)].any()
        assert G.label_head_kernel(C) == ("fixed<%d>" % C if C in (22, 14, 16) else "generic<24>" if C <= 24 else "generic<64>")
    assert {G.label_head_kernel(C) for C in G.DISPATCH_CLASSES} == {"fixed<14>", "fixed<16>", "fixed<22>", "generic<24>", "generic<64>"}
    assert G.label_head_kernel(22, al8=False) == "generic<24>"


LOSS_IDS = [LR.case_id(c) for c in G.label_loss_cases()]
UPSTREAM = 0.37
BOUND = grad_ref.bound(0.0)                                    # as tests/test_label_loss_cpu.py


@pytest.mark.parametrize("c", G.label_loss_cases(), ids=LOSS_IDS)
def test_label_loss_reference_at_the_new_geometries(c):
    import torch
    shape, C, (k, s) = c
    z, bias, gt = LR.case(shape, C, (k, s))
    r = LR.reference(shape, C, (k, s), upstream=UPSTREAM)
    p0 = r["prob"][..., 0][gt == 0]
    assert (p0 < LR.THRESHOLD - 1e-3).any() and (p0 > LR.THRESHOLD + 1e-3).any()     # ground truth 0 on both sides of the threshold
    assert (gt == -1).any() and (gt >= C).any() and ((gt > 0) & (gt < C)).any()
    assert (r["score"] == 0).any() and (r["score"] > 0).any() and 0 < r["count"] < gt.size and r["loss"] > 0
    assert not r["hot"][-1].any() and not r["dscore"][-1].any()
    e = LR.reference(shape, C, (k, s), "ignored")
    assert e["count"] == 0 and e["loss"] == 0 and not e["dscore"].any() and np.array_equal(e["label"], r["label"])
    loss64, dz64, db64 = LR.loss64(z, bias, gt, LR.THRESHOLD, k, s)
    t = torch.from_numpy
    err = {"loss": abs(float(r["loss"]) - loss64) / abs(loss64),
           "dz": grad_ref.rel_err(t(r["dz"].copy()), t(dz64 * UPSTREAM)),
           "dbias": grad_ref.rel_err(t(r["dbias64"].copy()), t(db64 * UPSTREAM))}
    assert all(v <= BOUND for v in err.values()), err


VERTEX_IDS = [(G.vertex_name(*ks), kind) for ks, _ in G.VERTEX_LADDER for kind in G.VERTEX_KINDS]


@pytest.mark.parametrize("nk", VERTEX_IDS, ids=["%s-%s" % nk for nk in VERTEX_IDS])
def test_vertex_head_reference_at_the_ladder_geometries(nk):
    """What tests/test_vertex_head_cpu.py asserts of cases A to D: restatement = dense composition bit for bit, and the
    composition within the criterion of float64 autograd. Both smooth-L1 branches occur in either kind."""
    import torch
    from test_vertex_head_cpu import _autograd
    c = VR.case(*nk)
    r, q = VR.reference(c), VR.restate(c)
    assert VR.same_bits(q["out"], r["out"]) and VR.same_bits(q["dz"], r["dz"])
    tol = 2.0 ** -24 * np.abs(r["dbias64"]) + 2.0 ** -30 * r["dbias_abs"]
    assert (np.abs(q["dbias"].astype(np.float64) - r["dbias64"]) <= tol).all()
    assert q["n_matched"] > 0 and r["out"][0] > 0 and r["dz"].any() and r["n_quadratic"] > 0 and r["n_linear"] > 0
    assert (r["weights"] == 10).any() and (r["weights"] == 1).any()
    l64, dz64, db64 = _autograd(c, torch.float64)
    l32, dz32, db32 = _autograd(c, torch.float32)
    t = lambda a: torch.from_numpy(np.array(a))
    floor = {"loss": abs(l32 - l64) / abs(l64), "dz": grad_ref.rel_err(dz32, dz64), "dbias": grad_ref.rel_err(db32, db64)}
    err = {"loss": abs(float(r["out"][0]) - l64) / abs(l64), "dz": grad_ref.rel_err(t(r["dz"]), dz64),
           "dbias": grad_ref.rel_err(t(r["dbias64"]), db64)}
    for key in err:
        assert floor[key] <= grad_ref.FLOOR_CAP and err[key] <= grad_ref.bound(floor[key]), (key, err[key], floor[key])


@pytest.mark.parametrize("ks", G.HOUGH_KS, ids=["k%ds%d" % ks for ks in G.HOUGH_KS])
def test_hough_cases_detect_something_from_pixels_with_more_than_two_taps(ks):
    from posecnn_amd import config
    from test_gpu_hough import lowres_case
    k, s = ks
    B, H, W, C, n_obj = G.HOUGH_SHAPE[s]
    assert H % s == 0 and W % s == 0 and k > 2 * s and G.accepted(k, s)
    label, z, bias, meta = lowres_case(500 + H, B, H, W, C, n_obj, s)
    assert z.shape == (B, H // s, W // s, 3 * C)
    full = oracle.deconv_bilinear(z, k, s, None, None, bias, False)
    want = oracle.hough_voting(label, full, config.LOV_EXTENTS[:C], meta, None, 0, -1.0, 0.02, G.HOUGH_SKIP,
                               label_thr=G.HOUGH_LABEL_THRESHOLD, padded=True)
    assert int(want[5][1]) >= 1
    # the sampled pixels: rank % skip == 0 within a class of more than label_threshold pixels, in raster order
    wide = 0
    ny, nx = np.array(G.tap_counts(k, s, H // s)), np.array(G.tap_counts(k, s, W // s))
    for cls in range(1, C):
        ys, xs = np.nonzero(label[0] == cls)
        if len(ys) > G.HOUGH_LABEL_THRESHOLD:
            wide += int(((ny[ys[::G.HOUGH_SKIP]] > 2) | (nx[xs[::G.HOUGH_SKIP]] > 2)).sum())
    assert wide > 0
