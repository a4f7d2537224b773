"""Exact-arithmetic GPU tests: the dense MFMA / FMA kernels against float64, element for element, with `==`.

Every kernel here uses only fp32 multiply-adds (v_mfma_f32_16x16x4_f32, FMAs, adds) and multiplications by small dyadic
constants. On the integer (or fixed dyadic) inputs of tests/exact.py, whose per-output sums of absolute terms stay below
2^24 units of the output's last place, every partial sum in every association order is exact, so the fp32 result must
equal the float64 reference whatever K order, split, fold or block map the kernel uses. The reference is independent of
the project's own kernels (plain torch float64 matrix products), it survives any legitimate reordering of a sum, and a
failure names the first wrong elements and the workgroup coordinates they belong to (`exact.first_mismatch`).

Every test asserts `abs_bound < 2^24` on its own inputs BEFORE it looks at the kernel's output; tests/test_exact_cpu.py
proves the references against float64 conv2d and checks the same bounds and the dispatch coverage of the case lists
without a GPU. All calls go through posecnn_amd.ops (one through the C entry itself, to withhold the workspace).

What stays outside: depth frames of the raw first-layer entries. Their blob clip(d / 2000, 0, 1) * 255 - mean moves in
steps of 31.875 for the depths at which d / 2000 is dyadic; that costs 8 of the 24 bits and the per-output bound then
exceeds 2^24. The depth half of the raw path stays on its bit-identity with the blob path (tests/test_gpu_round3.py,
tests/test_gpu_round4.py); the two-filter-set logic is covered exactly by the groups = 2 blob cases here. The tanh outputs
of fc_rows_cols / fc_skinny are transcendental: their LINEAR output is exact, tanh is held to the existing tests'
tolerance against float64 tanh of it. These tests complement the Gaussian-data tolerance tests, which bound rounding
behaviour — something exact data cannot see.

Evidence that these tests bite: three single-line, value-only mutants of the library (built on a scratch copy, never
committed; no address, bound or synchronisation touched, each well under 1 % of the output elements), the whole `-m gpu`
suite run against each. "new" = this file, "old" = every other GPU test.

  mutant                                                           new tests failing                      old tests failing
  1 wino43_splitk_reduce_kernel adds the bias twice for channels   16: every trunk case with S > 1 (14),   15: test_winograd43_mfma_conv_kernel
    20..23 at output column 3                                          chain cases 0, 1                        (11 split cases), memory contract (4)
  2 fc_skinny: wave 2 of column group 1, K slice 0, accumulates    2: test_fc_skinny_equals_float64        3: test_fc_skinny_matches_float64_and_
    its clamped (past-the-slice) step                                  [2064-200], [25088-256]                 is_deterministic (2), memory contract (1)
  3 wino43_mfma_kernel's pooled store leaves the window's fourth   9: pooled trunk cases (7), the          25: trunk kernel (5), fused-vs-unfused
    element out of the max for tile 5, channel 7 of a block            no-workspace case, chain case 2         pair (5), memory contract (4), 11 network /
                                                                                                               pipeline end-to-end tests
  Mutant 2 passed the issue's nine (K, N) pairs of fc_skinny untouched (only the old tests caught it): in those a clamped
  step only runs in column group 0 or in a last, shorter slice. exact.FC_SKINNY_KN_EXTRA closes that; the figure above is
  with it. Mutant 3 is invisible to the fused conv1_1 -> conv1_2 tests here, rightly: that kernel has its own pool; the
  old fused tests fail only because their yardstick (the unfused pair) is the mutated kernel.
  Every failure names the element: e.g. mutant 3, case (1, 10, 6, 64) -> 256: "1 of 3840 elements differ ... (b=0, y=4,
  x=2, c=71) got 1395.0 want 2486.0  tile 5 (ty 2, tx 1) tile block 0, channel block 1, wave 0".

Wall time on one MI355X: `pytest -m gpu tests/test_gpu_exact.py` 7 s (91 tests, 5.6 s inside pytest); the whole `-m gpu` run 196 s at the
parent commit (397 tests) and 203 s with this file. The count sweeps are therefore not thinned.
"""
import ctypes

import pytest
import torch

import exact
from exact import LIMIT, check, zero_bits

pytestmark = pytest.mark.gpu


def require_exact(bound, what):
    assert bound < LIMIT, "input not exact (%s): per-output sum of absolute terms %.0f >= 2^24" % (what, bound)


def count_tensor(gpu, n):
    return torch.tensor([n], dtype=torch.int32, device=gpu)


def outputs(out):
    return out if isinstance(out, tuple) else (out,)


# ---- trunk: ops.winograd43_conv (wino43_mfma_kernel, wino43_splitk_reduce_kernel) ----------------------------------------
def _check_wino(got, ref, case, relu, what):
    (B, H, W, cin), cout, pool, groups = case
    got, ref = outputs(got), outputs(ref)
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        pooled = pool == 1 or i == 1
        check(g, r, {"name": "%s %s relu=%s %s" % (what, case, relu, "pooled" if pooled else "full"), "wino": (B, H, W, groups, pooled)})


@pytest.mark.parametrize("case", exact.wino_cases())
def test_winograd43_conv_equals_float64_on_raw_integer_planes(gpu, case):
    """Raw integer V and U^T fed straight to the kernel (its contract is in the transform domain): 36 independent
    random planes, |V|, |U| <= 8, |bias| <= 1024. Every Cin split, pool mode, block map and ragged tile count of the case
    list (see tests/test_exact_cpu.py), ReLU on and off. Both block maps are reached by shape alone."""
    from posecnn_amd import ops
    (B, H, W, cin), cout, pool, groups = case
    v, ut, bias = exact.wino_inputs(case, gpu)
    require_exact(exact.abs_bound("wino43", v, ut, bias, B, H, W, True, pool, groups), case)
    for relu in (True, False):
        ref = exact.wino43_reference(v, ut, bias, B, H, W, relu, pool, groups)
        got = ops.winograd43_conv(v, ut, bias, B, H, W, relu, pool, groups)
        _check_wino(got, ref, case, relu, "winograd43_conv")
        del ref, got


def test_winograd43_conv_without_workspace_falls_back_to_one_pass(gpu):
    """A split-sized launch whose caller hands no workspace to the C entry: S = 1 is taken, same exact answer."""
    from posecnn_amd import _lib
    case = exact.WINO_NO_WORKSPACE_CASE
    (B, H, W, cin), cout, pool, groups = case
    assert exact.wino43_regime((B, H, W, cin), cout, groups)["S"] > 1 and pool == 2
    v, ut, bias = exact.wino_inputs(case, gpu)
    require_exact(exact.abs_bound("wino43", v, ut, bias, B, H, W, True, pool, groups), case)
    y = torch.empty((B, H, W, cout), dtype=torch.float32, device=gpu)
    yp = torch.empty((B, H // 2, W // 2, cout), dtype=torch.float32, device=gpu)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    _lib.check("pcnn_winograd43_conv_fwd",
               _lib.lib().pcnn_winograd43_conv_fwd(P(v), P(ut), P(bias), B, H, W, cin, cout, groups, 1, pool, P(y), P(yp), ctypes.c_void_p(0), 0, stream))
    _check_wino((y, yp), exact.wino43_reference(v, ut, bias, B, H, W, True, pool, groups), case, True, "winograd43_conv, no workspace")


@pytest.mark.parametrize("case", exact.CHAIN_CASES)
def test_winograd_input_then_conv_equals_float64_on_integer_activations(gpu, case):
    """The chain family: integer activations in [0, 3] (half zeros) through ops.winograd_input and then the trunk kernel,
    |U| <= 2 — V now has the structure B^T d B gives it (correlated planes, values up to ~300)."""
    from posecnn_amd import ops
    (B, H, W, cin), cout, pool, groups = case
    x, ut, bias = exact.chain_inputs(case, gpu)
    require_exact(exact.abs_bound("wino43_input", x), "input transform of %s" % (case,))
    vref = exact.wino43_input_reference(x)
    require_exact(exact.abs_bound("wino43", vref, ut, bias, B, H, W, True, pool, groups), case)
    v = ops.winograd_input(x, 4)
    check(v, vref, {"name": "winograd_input %s" % (case,)})
    for relu in (True, False):
        _check_wino(ops.winograd43_conv(v, ut, bias, B, H, W, relu, pool, groups),
                    exact.wino43_reference(vref, ut, bias, B, H, W, relu, pool, groups), case, relu, "winograd_input + winograd43_conv")


# ---- first layers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,cout,groups", exact.CONV1_CASES)
def test_first_conv_and_its_winograd_form_equal_float64(gpu, shape, cout, groups):
    """ops.conv3x3_c3 against a float64 direct convolution and ops.conv3x3_c3_winograd43 against B^T d B of it, on the
    shapes of the existing tests (W = 131, 300 and 1 x 1 among them), one and two filter sets."""
    from posecnn_amd import ops
    B, H, W = shape
    x, w, b = exact.conv1_inputs(shape, cout, groups, gpu)
    a_abs = exact.conv3x3_c3_reference(x, w, b, True, groups, absolute=True)
    require_exact(float(a_abs.max()), "conv3x3_c3 %s" % (shape,))
    for relu in (True, False):
        a = exact.conv3x3_c3_reference(x, w, b, relu, groups)
        require_exact(exact.abs_bound("wino43_input", a), "B^T d B of conv1_1 %s" % (shape,))
        check(ops.conv3x3_c3_winograd43(x, w, b, relu, groups=groups), exact.wino43_input_reference(a),
              {"name": "conv3x3_c3_winograd43 %s groups %d relu=%s" % (shape, groups, relu)})
        per = B // groups
        for g in range(groups):   # the plain kernel has one filter set: each set on its own images
            check(ops.conv3x3_c3(x[g * per:(g + 1) * per].contiguous(), w[g].contiguous(), b[g].contiguous(), relu), a[g * per:(g + 1) * per],
                  {"name": "conv3x3_c3 %s set %d relu=%s" % (shape, g, relu)})


@pytest.mark.parametrize("B,H,W,groups", exact.CONV12_CASES)
def test_conv1_1_conv1_2_fused_equals_float64(gpu, B, H, W, groups):
    """ops.conv1_1_conv1_2_fused: x in [-2, 2], w1 in {-1, 0, 1}, b1 in [-3, 3], |U2| <= 2. Both ut2 layouts, (relu1, relu2)
    in {(1,1), (0,1), (1,0)}, one and two filter sets, a full 480 x 640 pair of frames."""
    from posecnn_amd import ops
    x, w1, b1, ut2, b2 = exact.conv12_inputs(B, H, W, groups, device=gpu)
    utf = ops.conv12_fragment_major(ut2)
    for relu1, relu2 in exact.CONV12_RELUS:
        require_exact(exact.abs_bound("conv12", x, w1, b1, ut2, b2, relu1, relu2, groups), "conv12 %s" % ((B, H, W, groups),))
        ref = exact.conv12_reference(x, w1, b1, ut2, b2, relu1, relu2, groups)
        for layout, u in ((0, ut2), (1, utf)):
            got = ops.conv1_1_conv1_2_fused(x, w1, b1, u, b2, bool(relu1), bool(relu2), groups=groups, ut2_layout=layout)
            check(got, ref, {"name": "conv1_1_conv1_2_fused %s relu (%d, %d) layout %d" % ((B, H, W, groups), relu1, relu2, layout),
                             "wino": (B, H, W, groups, True)})


@pytest.mark.parametrize("B,H,W", exact.CONV12_RAW_CASES)
def test_raw_colour_frames_through_the_first_layers_equal_float64(gpu, B, H, W):
    """The raw entry points on COLOUR frames (depth=None): integer pixel means, uint8 pixels within +-4 of them, so the
    blob the kernel forms from the bytes is an integer in [-4, 4]; |U2| <= 1. The first float64 anchor of the
    uint8 -> blob conversion inside conv1_1_conv1_2_fused_raw and conv3x3_c3_winograd43_raw. Depth frames cannot be made
    exact at a useful amplitude (module docstring): they stay on their bit-identity with the blob path."""
    from posecnn_amd import ops
    x, w1, b1, ut2, b2 = exact.conv12_inputs(B, H, W, 1, exact.CONV12_RAW_X, exact.CONV12_RAW_U, device=gpu)
    frames = exact.raw_frames(x)
    assert frames.dtype == torch.uint8 and torch.equal(frames.float() - torch.tensor(exact.RAW_MEANS, device=gpu), x)
    utf = ops.conv12_fragment_major(ut2)
    for relu1, relu2 in exact.CONV12_RELUS:
        require_exact(exact.abs_bound("conv12", x, w1, b1, ut2, b2, relu1, relu2, 1), "raw conv12 %s" % ((B, H, W),))
        ref = exact.conv12_reference(x, w1, b1, ut2, b2, relu1, relu2, 1)
        for layout, u in ((0, ut2), (1, utf)):
            got = ops.conv1_1_conv1_2_fused_raw(frames, None, w1, b1, u, b2, bool(relu1), bool(relu2), pixel_means=exact.RAW_MEANS, ut2_layout=layout)
            check(got, ref, {"name": "conv1_1_conv1_2_fused_raw %s relu (%d, %d) layout %d" % ((B, H, W), relu1, relu2, layout),
                             "wino": (B, H, W, 1, True)})
    for relu in (True, False):
        a = exact.conv3x3_c3_reference(x, w1, b1, relu, 1)
        require_exact(exact.abs_bound("wino43_input", a), "raw B^T d B %s" % ((B, H, W),))
        check(ops.conv3x3_c3_winograd43_raw(frames, None, w1, b1, relu, pixel_means=exact.RAW_MEANS), exact.wino43_input_reference(a),
              {"name": "conv3x3_c3_winograd43_raw %s relu=%s" % ((B, H, W), relu)})


# ---- FC family ------------------------------------------------------------------------------------------------------
def _fc_operands(gpu, cap, K, N, addend, scale=1.0):
    s = exact.seed_of("fc", cap, K, N)
    x = exact.ints_dev(s, (cap, K), -exact.FC_A, exact.FC_A, gpu)
    wt = exact.ints_dev(s + 1, (N, K), -exact.FC_A, exact.FC_A, gpu) * scale
    bias = exact.ints_dev(s + 2, (N,), -exact.FC_BIAS, exact.FC_BIAS, gpu) * scale
    ad = exact.ints_dev(s + 3, (cap, N), -exact.FC_BIAS, exact.FC_BIAS, gpu) * scale if addend else None
    require_exact(exact.fc_closed_bound(K, exact.FC_A, exact.FC_A, exact.FC_BIAS, exact.FC_BIAS if addend else 0), "fc closed form K=%d" % K)
    require_exact(exact.abs_bound("fc", x, wt, bias, ad) / scale, "fc %s" % ((cap, K, N),))
    return x, wt, bias, ad


def _act(ref, relu):
    return torch.relu(ref) if relu else ref


@pytest.mark.parametrize("cap,K,N,counted,uncounted,addend", exact.FC_ROWS_CASES)
def test_fc_rows_equals_float64_at_every_row_count(gpu, cap, K, N, counted, uncounted, addend):
    """ops.fc_rows over the device-side row count: {0, 1, 2} + {64 k - 1, 64 k, 64 k + 1} + {capacity}, every
    block boundary up to the capacity. The float64 product is computed once; for each count the rows at or past it are
    NaN in x (and in the addend), rows below it must equal the reference and rows at or past it must be all-zero bits.
    The data being exact, the answer may not depend on the split-K factor the device picks (fc_split: five exits and the
    workspace-fit clause), the partial-output stride, or the reduction kernel's grid: this holds them to the reference
    at every 64-row boundary — and settles, for exact data, the note that fc6's bits change with the live-row count."""
    from posecnn_amd import ops
    x, wt, bias, ad = _fc_operands(gpu, cap, K, N, addend)
    ref = exact.fc_reference(x, wt, bias, ad)
    meta = lambda n, relu: {"name": "fc_rows %s count %s relu=%s" % ((cap, K, N), n, relu), "fc": True}
    for i, n in enumerate(exact.fc_counts(cap)):
        xp = exact.poison_rows(x, n)
        adp = exact.poison_rows(ad, n) if ad is not None else None
        for relu in ((False, True) if n in (cap, 65, 1) else (bool(i & 1),)):
            y = ops.fc_rows(xp, wt, bias, relu, num_rows=count_tensor(gpu, n), addend=adp)
            check(y[:n], _act(ref[:n], relu), meta(n, relu))
            assert zero_bits(y[n:]), "fc_rows %s: rows at or past the count %d are not all-zero bits" % ((cap, K, N), n)
    if uncounted:
        for relu in (False, True):
            check(ops.fc_rows(x, wt, bias, relu, num_rows=None, addend=ad), _act(ref, relu), meta(None, relu))


@pytest.mark.parametrize("cap,K,N", exact.FC_TALL_CASES)
def test_fc_rows_tall_map_equals_float64(gpu, cap, K, N):
    """The tall block map of the 1x1 head convolutions (rows > columns), num_rows=None, with and without an addend."""
    from posecnn_amd import ops
    x, wt, bias, ad = _fc_operands(gpu, cap, K, N, True)
    for addend in (None, ad):
        ref = exact.fc_reference(x, wt, bias, addend)
        for relu in (False, True):
            check(ops.fc_rows(x, wt, bias, relu, num_rows=None, addend=addend), _act(ref, relu),
                  {"name": "fc_rows tall %s addend=%s relu=%s" % ((cap, K, N), addend is not None, relu), "fc": True})


def test_fc_rows_split_equals_float64_at_every_row_count(gpu):
    from posecnn_amd import ops
    cap, K, out_a, out_b = exact.FC_SPLIT_CASE
    x, wt, bias, _ = _fc_operands(gpu, cap, K, out_a + out_b, False)
    ref = exact.fc_reference(x, wt, bias)
    for n in exact.fc_counts(cap):
        ya, yb = ops.fc_rows_split(exact.poison_rows(x, n), wt, bias, out_a, relu_a=True, relu_b=False, num_rows=count_tensor(gpu, n))
        check(ya[:n], torch.relu(ref[:n, :out_a]), {"name": "fc_rows_split a, count %d" % n, "fc": True})
        check(yb[:n], ref[:n, out_a:], {"name": "fc_rows_split b, count %d" % n, "fc": True})
        assert zero_bits(ya[n:]) and zero_bits(yb[n:]), "fc_rows_split: rows at or past the count %d are not all-zero bits" % n


FC_TANH_SCALE = 2.0 ** -14    # weights and bias as integers / 2^14: still exact, and the linear output lands where tanh is not saturated


def test_fc_rows_cols_equals_float64_at_every_row_count(gpu):
    """fc8's shape: 88 real columns of a filter padded to 128. The linear output is exact at every count; y_tanh is held to
    the existing test's 1e-6 against float64 tanh of it (test_fc_rows_cols_is_fc8_and_tanh_in_one_launch)."""
    from posecnn_amd import ops
    cap, K, N, npad = exact.FC_COLS_CASE
    x, wt, bias, _ = _fc_operands(gpu, cap, K, N, False, FC_TANH_SCALE)
    wp = torch.zeros((npad, K), device=gpu); wp[:N] = wt
    bp = torch.zeros((npad,), device=gpu); bp[:N] = bias
    ref = exact.fc_reference(x, wt, bias)
    assert 0.05 < float((ref.abs() < 1).double().mean())      # tanh sees its unsaturated range
    for n in exact.fc_counts(cap):
        xp, cnt = exact.poison_rows(x, n), count_tensor(gpu, n)
        y, t = ops.fc_rows_cols(xp, wp, bp, N, "tanh", num_rows=cnt)
        assert tuple(y.shape) == (cap, N) and tuple(t.shape) == (cap, N)
        check(y[:n], ref[:n], {"name": "fc_rows_cols linear, count %d" % n, "fc": True})
        if n:
            assert float((t[:n].double() - torch.tanh(ref[:n])).abs().max()) < 1e-6
        assert zero_bits(y[n:]) and zero_bits(t[n:]), "fc_rows_cols: rows at or past the count %d are not all-zero bits" % n
        if n in (cap, 65, 1, 0):
            check(ops.fc_rows_cols(xp, wp, bp, N, "relu", num_rows=cnt)[:n], torch.relu(ref[:n]), {"name": "fc_rows_cols relu, count %d" % n, "fc": True})
            check(ops.fc_rows_cols(xp, wp, bp, N, "none", num_rows=cnt)[:n], ref[:n], {"name": "fc_rows_cols none, count %d" % n, "fc": True})


@pytest.mark.parametrize("K,N", exact.fc_skinny_kn())
def test_fc_skinny_equals_float64(gpu, K, N):
    """ops.fc_skinny: M in {1, 5, 16, 17, 21, 32} with device counts on both sides of 16 (the second row block is skipped at
    <= 16), K = 2512 = 16 * 157 among the K (slices that end in clamped steps; exact.FC_SKINNY_KN_EXTRA adds odd slices in a second
    column group), all three activations (linear output exact,
    tanh to the existing test's 3e-7 against float64 tanh of it), NaN rows past the count, tickets back at zero."""
    from posecnn_amd import ops
    x32, wt, bias, _ = _fc_operands(gpu, 32, K, N, False, FC_TANH_SCALE)
    ref32 = exact.fc_reference(x32, wt, bias)
    for M in exact.FC_SKINNY_M:
        for c in exact.skinny_counts(M):
            n = M if c is None else c
            xp = exact.poison_rows(x32[:M], n)
            cnt = None if c is None else count_tensor(gpu, c)
            ref = ref32[:n]
            for act in ("none", "relu", "tanh"):
                out = ops.fc_skinny(xp, wt, bias, act, num_rows=cnt)
                y, t = out if act == "tanh" else (out, None)
                name = "fc_skinny M=%d K=%d N=%d count=%s %s" % (M, K, N, c, act)
                assert tuple(y.shape) == (M, N)
                check(y[:n], torch.relu(ref) if act == "relu" else ref, {"name": name, "fc": True})
                assert zero_bits(y[n:]), name + ": rows at or past the count are not all-zero bits"
                if act == "tanh":
                    if n:
                        assert float((t[:n].double() - torch.tanh(ref)).abs().max()) < 3e-7, name
                    assert zero_bits(t[n:]), name
    assert all(int(v.abs().max()) == 0 for v in ops._tickets.values())


# ---- heads ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", exact.HEAD_CASES)
def test_head_lowres_kernels_equal_float64(gpu, case):
    """ops.head_lowres_mfma, and ops.head_lowres wherever the head fits its documented LDS limit (32 x U + U x Cout floats
    in 60 KB; the network falls back to the matrix-core kernel otherwise: test_small_head_falls_back_...): integer scores,
    planted term and weights; `add` (units of 1/16: the k = 4 deconv's taps) and `z` both exact. Pixel counts that are no
    multiple of the 32- / 64-pixel workgroups, B > 1 so a workgroup straddles two images."""
    from posecnn_amd import ops
    B, h, w, U, cout, plant = case
    s4, s5, wt, pl = exact.head_inputs(case, gpu)
    require_exact(exact.abs_bound("head", s4, s5, wt, pl), "head %s" % (case,))
    add_ref, z_ref = exact.head_reference(s4, s5, wt, pl)
    z_ref = z_ref.reshape(B, h, w, cout)
    add, z = ops.head_lowres_mfma(s4, s5, ops.head_lowres_mfma_filter(wt), cout, planted=pl)
    check(add, add_ref, {"name": "head_lowres_mfma add %s" % (case,)})
    check(z, z_ref, {"name": "head_lowres_mfma z %s" % (case,)})
    if exact.head_lowres_fits(U, cout):
        add, z = ops.head_lowres(s4, s5, wt, planted=pl)
        check(add, add_ref, {"name": "head_lowres add %s" % (case,)})
        check(z, z_ref, {"name": "head_lowres z %s" % (case,)})


@pytest.mark.parametrize("shape", exact.DECONV_SHAPES)
@pytest.mark.parametrize("k,s", exact.DECONV_KS)
def test_deconv_bilinear_equals_float64(gpu, shape, k, s):
    """ops.deconv_bilinear at the network's (4, 2) and (16, 8) on the shapes of test_deconv_bilinear, plain and with both
    addends, bias and ReLU: taps are multiples of 1/16 resp. 1/256 (network.py's make_deconv_filter in float64)."""
    from posecnn_amd import ops
    x, a1, a2, b = exact.deconv_inputs(shape, s, gpu)
    require_exact(exact.abs_bound("deconv%d" % k, x, k, s, a1, a2, b), "deconv %s" % (shape,))
    check(ops.deconv_bilinear(x, k, s), exact.deconv_reference(x, k, s), {"name": "deconv_bilinear %s k=%d s=%d" % (shape, k, s)})
    for relu in (True, False):
        check(ops.deconv_bilinear(x, k, s, add1=a1, add2=a2, bias=b, relu=relu), exact.deconv_reference(x, k, s, a1, a2, b, relu),
              {"name": "deconv_bilinear + adds + bias %s k=%d s=%d relu=%s" % (shape, k, s, relu)})
