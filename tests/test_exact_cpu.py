"""CPU half of the exact-arithmetic tests (tests/exact.py, tests/test_gpu_exact.py); needs no GPU.

  1. The float64 references are right: on real-valued random data, with U = G g G^T in float64, `wino43_reference`
     and `conv12_reference` equal torch's float64 conv2d to 1e-10 — ragged H / W, two filter sets, pool on and off.
     This proves the tile geometry and the A^T / B^T / G constants independently of np_wino43_* (tests/test_gpu_ops.py).
     The bilinear deconv reference is held to the CPU oracle, bit for bit on integers.
  2. Every case the GPU file runs satisfies `abs_bound < 2^24`: the closed forms for all of them, the per-output bound
     on the data itself for all but the largest, a sub-block for those.
  3. The trunk case list reaches the host-side dispatch it claims, answered by the library's own
     pcnn_winograd43_conv_workspace_bytes (libposecnn_hip.so loads without a GPU).
"""
import pytest
import torch

import exact
from exact import LIMIT

torch.set_num_threads(min(8, torch.get_num_threads()))


def _rand(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---- 1. the references ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,cin,cout,groups,relu,pool", [
    (2, 9, 14, 8, 6, 2, True, 0), (1, 8, 12, 5, 7, 1, True, 1), (4, 6, 10, 4, 3, 2, False, 2), (1, 1, 1, 3, 2, 1, True, 0),
    (3, 5, 7, 6, 4, 3, False, 0), (2, 16, 4, 2, 9, 1, True, 2)])
def test_wino43_reference_is_a_convolution(B, H, W, cin, cout, groups, relu, pool):
    x = _rand(1, B, H, W, cin)
    w = _rand(2, groups, cout, cin, 3, 3)
    b = _rand(3, groups, cout)
    ut = torch.stack([exact.wino43_filter64(w[g]) for g in range(groups)])
    got = exact.wino43_reference(exact.wino43_input_reference(x), ut, b, B, H, W, relu, pool, groups)
    per = B // groups
    ref = torch.cat([torch.nn.functional.conv2d(x[g * per:(g + 1) * per].permute(0, 3, 1, 2), w[g], b[g], padding=1) for g in range(groups)])
    if relu:
        ref = torch.relu(ref)
    full = ref.permute(0, 2, 3, 1)
    pooled = torch.nn.functional.max_pool2d(ref, 2, 2).permute(0, 2, 3, 1) if pool else None
    want = {0: (full,), 1: (pooled,), 2: (full, pooled)}[pool]
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(want)
    for g_, w_ in zip(got, want):
        assert g_.shape == w_.shape and float((g_ - w_).abs().max()) < 1e-10


@pytest.mark.parametrize("B,H,W,groups,relu1,relu2", [(2, 16, 32, 2, True, True), (1, 16, 16, 1, False, True), (3, 32, 16, 1, True, False),
                                                     (2, 12, 10, 2, True, True)])   # (the reference itself takes any even H, W)
def test_conv12_reference_is_two_convolutions_and_a_pool(B, H, W, groups, relu1, relu2):
    x = _rand(4, B, H, W, 3)
    w1 = _rand(5, groups, 3, 3, 3, 8) * 0.3                 # (ky, kx, ci, co)
    b1 = _rand(6, groups, 8)
    w2 = _rand(7, groups, 5, 8, 3, 3) * 0.2
    b2 = _rand(8, groups, 5)
    ut2 = torch.stack([exact.wino43_filter64(w2[g]) for g in range(groups)])
    got = exact.conv12_reference(x, w1, b1, ut2, b2, relu1, relu2, groups)
    per = B // groups
    outs = []
    for g in range(groups):
        a = torch.nn.functional.conv2d(x[g * per:(g + 1) * per].permute(0, 3, 1, 2), w1[g].permute(3, 2, 0, 1), b1[g], padding=1)
        c = torch.nn.functional.conv2d(torch.relu(a) if relu1 else a, w2[g], b2[g], padding=1)
        outs.append(torch.nn.functional.max_pool2d(torch.relu(c) if relu2 else c, 2, 2))
    want = torch.cat(outs).permute(0, 2, 3, 1)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-10


def test_wino43_input_reference_inverts_through_the_filter_identity():
    """B^T d B against the definition once more, from the other side: with the centre-tap identity filter the whole
    chain returns the input, so the input transform's tile order is the output transform's."""
    B, H, W, C = 2, 7, 10, 3
    x = _rand(9, B, H, W, C)
    w = torch.zeros((C, C, 3, 3), dtype=torch.float64)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1
    y = exact.wino43_reference(exact.wino43_input_reference(x), exact.wino43_filter64(w)[None], torch.zeros((1, C), dtype=torch.float64),
                               B, H, W, False, 0, 1)
    assert float((y - x).abs().max()) < 1e-12


@pytest.mark.parametrize("k,s", exact.DECONV_KS + [(2, 2), (8, 4)])   # dyadic taps only (k = 6 has thirds)
def test_deconv_reference_equals_the_cpu_oracle_on_integers(k, s):
    import oracle
    x = exact.ints(3, (2, 5, 7, 6), -100, 100)
    a1 = exact.ints(4, (2, 5 * s, 7 * s, 6), -100, 100)
    b = exact.ints(5, (6,), -100, 100)
    for relu in (False, True):
        want = torch.from_numpy(oracle.deconv_bilinear(x.numpy(), k, s, a1.numpy(), None, b.numpy(), relu))
        exact.check(want, exact.deconv_reference(x, k, s, add1=a1, bias=b, relu=relu), {"name": "oracle deconv k=%d s=%d" % (k, s)})
    taps = torch.tensor(exact.deconv_filter_1d(k), dtype=torch.float64)
    if (k, s) in exact.DECONV_KS:
        step = 4.0 if k == 4 else 16.0
        assert torch.equal(taps * step, (taps * step).round())          # 1-D taps are multiples of 1/4 resp. 1/16
        assert all(float(taps[r::s].sum()) == 1.0 for r in range(s))    # every output phase interpolates: |taps| sum to 1


def test_first_mismatch_reports_where():
    ref = torch.zeros((2, 8, 8, 128), dtype=torch.float64)
    got = ref.float().clone()
    got[0, 0, 0, 0] = -0.0
    assert exact.first_mismatch(got, ref) is None                       # by value: -0.0 == 0.0
    got[1, 5, 6, 81] = 3.0
    got[1, 7, 7, 127] = float("nan")
    msg = exact.first_mismatch(got, ref, {"name": "y", "wino": (2, 8, 8, 1, False)})
    assert "2 of" in msg and "b=1, y=5, x=6, c=81" in msg and "got 3.0 want 0.0" in msg
    assert "tile 7 (ty 1, tx 1) tile block 0, channel block 1, wave 1" in msg and "nan" in msg
    rows = torch.zeros((130, 70), dtype=torch.float64)
    g2 = rows.float().clone()
    g2[129, 65] = 1.0
    assert "block (rows 128.., cols 64..)" in exact.first_mismatch(g2, rows, {"fc": True})
    assert exact.zero_bits(torch.zeros(5)) and not exact.zero_bits(-torch.zeros(5)) and not exact.zero_bits(torch.tensor([float("nan")]))


# ---- 2. every GPU case is exact ---------------------------------------------------------------------------------------
PER_OUTPUT_ELEMS = 6_000_000     # V elements up to which the CPU evaluates the per-output bound on the full data


@pytest.mark.parametrize("case", exact.wino_cases())
def test_trunk_cases_are_exact(case):
    (B, H, W, cin), cout, pool, groups = case
    closed = exact.wino43_closed_bound(cin, exact.WINO_VMAX, exact.WINO_UMAX, exact.WINO_BMAX)
    assert closed < LIMIT, closed
    T = B * ((H + 3) // 4) * ((W + 3) // 4)
    if 36 * T * cin <= PER_OUTPUT_ELEMS:
        v, ut, bias = exact.wino_inputs(case)
        b = exact.abs_bound("wino43", v, ut, bias, B, H, W, True, pool, groups)
        assert 0 < b <= closed and b < LIMIT, (b, closed)


def test_trunk_closed_form_is_attained():
    """361 Cin vmax umax + bmax is the bound, not a guess: all-maximal inputs reach it at an interior (3, 3) output."""
    v = torch.full((36, 1, 64), 8.0)
    ut = torch.full((1, 36, 64, 64), 8.0)
    bias = torch.full((1, 64), 1024.0)
    assert exact.abs_bound("wino43", v, ut, bias, 1, 4, 4, True, 0, 1) == exact.wino43_closed_bound(64, 8, 8, 1024)
    assert exact.wino43_closed_bound(512, 8, 8, 1024) == 11_830_272


@pytest.mark.parametrize("case", exact.CHAIN_CASES)
def test_chain_cases_are_exact(case):
    (B, H, W, cin), cout, pool, groups = case
    x, ut, bias = exact.chain_inputs(case)
    v = exact.wino43_input_reference(x, absolute=True)
    b = exact.abs_bound("wino43", v, ut, bias, B, H, W, True, pool, groups)
    print("chain", case, "per-output bound", b)
    assert float(v.max()) < LIMIT and b < LIMIT, b


@pytest.mark.parametrize("B,H,W,groups", exact.CONV12_CASES)
def test_fused_first_layers_cases_are_exact(B, H, W, groups):
    x, w1, b1, ut2, b2 = exact.conv12_inputs(B, H, W, groups)
    if H * W > 128 * 128:    # the full-frame case: a sub-block with the image's top-left borders, every filter set
        x = x[:, :64, :96].contiguous()
    for relu1, relu2 in exact.CONV12_RELUS:
        b = exact.abs_bound("conv12", x, w1, b1, ut2, b2, relu1, relu2, groups)
        print("conv12", (B, H, W, groups), (relu1, relu2), "per-output bound", b)
        assert b < LIMIT, b


@pytest.mark.parametrize("B,H,W", exact.CONV12_RAW_CASES)
def test_fused_first_layers_raw_cases_are_exact(B, H, W):
    x, w1, b1, ut2, b2 = exact.conv12_inputs(B, H, W, 1, exact.CONV12_RAW_X, exact.CONV12_RAW_U)
    frames = exact.raw_frames(x)
    assert frames.dtype == torch.uint8 and torch.equal(frames.float() - torch.tensor(exact.RAW_MEANS), x)
    for relu1, relu2 in exact.CONV12_RELUS:
        b = exact.abs_bound("conv12", x, w1, b1, ut2, b2, relu1, relu2, 1)
        print("conv12 raw", (B, H, W), (relu1, relu2), "per-output bound", b)
        assert b < LIMIT, b
    assert exact.abs_bound("wino43_input", exact.conv3x3_c3_reference(x, w1, b1, True, absolute=True)) < LIMIT


@pytest.mark.parametrize("shape,cout,groups", exact.CONV1_CASES)
def test_first_layer_cases_are_exact(shape, cout, groups):
    closed = (27 * exact.CONV1_X * exact.CONV1_W + exact.CONV1_B) * 100      # 10 = the largest row sum of |B^T|, squared
    assert closed < LIMIT
    if shape[1] * shape[2] <= 64 * 64:
        x, w, b = exact.conv1_inputs(shape, cout, groups)
        a = exact.conv3x3_c3_reference(x, w, b, True, groups, absolute=True)
        assert float(a.max()) <= closed // 100
        assert exact.abs_bound("wino43_input", a) <= closed


def test_fc_cases_are_exact():
    ks = {c[1] for c in exact.FC_ROWS_CASES} | {c[1] for c in exact.FC_TALL_CASES} | {exact.FC_SPLIT_CASE[1], exact.FC_COLS_CASE[1]} | {K for K, _ in exact.fc_skinny_kn()}
    for K in ks:
        assert exact.fc_closed_bound(K, exact.FC_A, exact.FC_A, exact.FC_BIAS, exact.FC_BIAS) < LIMIT, K
    assert exact.fc_closed_bound(25088, 24, 24, 1 << 16, 1 << 16) == 14_581_760
    # the per-output bound on data never exceeds the closed form
    x = exact.ints(1, (70, 2512), -exact.FC_A, exact.FC_A)
    wt = exact.ints(2, (88, 2512), -exact.FC_A, exact.FC_A)
    b = exact.ints(3, (88,), -exact.FC_BIAS, exact.FC_BIAS)
    ad = exact.ints(4, (70, 88), -exact.FC_BIAS, exact.FC_BIAS)
    assert 0 < exact.abs_bound("fc", x, wt, b, ad) <= exact.fc_closed_bound(2512, exact.FC_A, exact.FC_A, exact.FC_BIAS, exact.FC_BIAS)


def test_fc_skinny_cases_put_clamped_steps_in_every_position():
    """csrc/fc_skinny.hip splits K into S = min(max(1, 256 / groups), max(1, K / 256), 64) slices of ceil(K / 16 / S) steps,
    taken two at a time: a slice of an odd number of steps ends in a clamped (loaded, not accumulated) step. The case list
    must have odd full slices in a launch of several column groups, not only a last, shorter slice that happens to be odd."""
    def slices(K, N):
        ks, groups = K // 16, (N + 127) // 128
        S = min(max(1, 256 // groups), max(1, ks // 16), 64)
        per = (ks + S - 1) // S
        return groups, [min(per, ks - i * per) for i in range(S) if ks - i * per > 0]
    kn = exact.fc_skinny_kn()
    assert all((K, N) in kn for K in (25088, 4096, 2512) for N in (4096, 88, 128))
    assert any(g > 1 and sl[0] % 2 and len(sl) > 2 for g, sl in (slices(K, N) for K, N in kn))   # every full slice odd, several groups
    assert any(g > 1 and sl[0] % 2 == 0 and sl[-1] % 2 for g, sl in (slices(K, N) for K, N in kn))   # odd in the last slice only
    assert any(all(n % 2 == 0 for n in sl) for g, sl in (slices(K, N) for K, N in kn))           # no clamped step at all
    assert any(N % 128 for _, N in kn)


def test_fc_count_sweeps_cover_every_block_boundary():
    for cap, K, N, *_ in exact.FC_ROWS_CASES:
        counts = exact.fc_counts(cap)
        assert counts[0] == 0 and counts[-1] == cap and {1, 2} <= set(counts) | {cap}
        for k in range(1, cap // 64 + 1):
            assert {64 * k - 1, 64 * k} <= set(counts) and (64 * k + 1 in counts or 64 * k + 1 > cap)
        assert all(0 <= c <= cap for c in counts)
    for M in exact.FC_SKINNY_M:
        cs = [c for c in exact.skinny_counts(M) if c is not None]
        assert M in cs and 0 in cs and (M <= 16 or {16, 17} <= set(cs))


@pytest.mark.parametrize("case", exact.HEAD_CASES)
def test_head_cases_are_exact(case):
    B, h, w, U, cout, plant = case
    closed = 3 * exact.HEAD_X * U * exact.HEAD_W * 16        # |add| <= 3 x 64 (the deconv's taps sum to 1), units of 1/16
    assert closed < LIMIT
    assert cout <= 96 and U % 16 == 0 and h % 2 == 0 and w % 2 == 0
    if B * h * w <= 1024:
        s4, s5, wt, pl = exact.head_inputs(case)
        assert exact.abs_bound("head", s4, s5, wt, pl) <= closed


def test_head_cases_reach_both_kernels():
    fits = [exact.head_lowres_fits(c[3], c[4]) for c in exact.HEAD_CASES]
    assert sum(fits) >= 3 and not all(fits)
    assert {c[3] for c in exact.HEAD_CASES} == {64, 128} and {c[4] for c in exact.HEAD_CASES} == {22, 66, 96}
    assert any((c[0] * c[1] * c[2]) % 32 and c[0] > 1 for c in exact.HEAD_CASES)


@pytest.mark.parametrize("shape", exact.DECONV_SHAPES)
@pytest.mark.parametrize("k,s", exact.DECONV_KS)
def test_deconv_cases_are_exact(shape, k, s):
    units = 16 if k == 4 else 256
    closed = 4 * exact.DECONV_X * units                      # x (taps sum to 1) + add1 + add2 + bias
    assert closed < LIMIT
    B, H, W, C = shape
    if B * H * W * C * s * s <= 2_000_000:
        x, a1, a2, b = exact.deconv_inputs(shape, s)
        assert exact.abs_bound("deconv%d" % k, x, k, s, a1, a2, b) <= closed


# ---- 3. the trunk list reaches the dispatch it claims ---------------------------------------------------------------------
def test_trunk_cases_reach_every_host_side_regime():
    from posecnn_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    regimes = [(c, exact.wino43_regime(c[0], c[1], c[3])) for c in exact.wino_cases()]
    seen = {(r["S"], c[2]) for c, r in regimes}
    missing = [(S, pool) for S in (1, 2, 4, 8) for pool in (0, 1, 2) if (S, pool) not in seen]
    assert not missing, "no trunk case with (Cin split, pool) = %s" % missing
    assert {r["S"] for _, r in regimes} == {1, 2, 4, 8}
    # eight channel blocks on both sides of the launcher's `u_bytes > v_bytes` rule (channel-block-major / tile-block-major)
    assert any(r["ncb"] == 8 and r["u_heavier"] for _, r in regimes)
    assert any(r["ncb"] == 8 and not r["u_heavier"] for _, r in regimes)
    assert any(r["ncb"] == 8 and r["u_heavier"] and r["S"] == 1 for _, r in regimes)   # ... and that map without a split
    assert any(r["nbt"] % 8 != 0 for _, r in regimes)        # a ragged last round of the 8-XCD block map
    assert any(r["tpg"] % 32 != 0 for _, r in regimes)       # a ragged last tile block per group
    assert any(r["tpg"] % 32 != 0 and c[3] > 1 for c, r in regimes)
    # the base list of test_winograd43_mfma_conv_kernel is a subset, unchanged
    from test_gpu_ops import WINO43_MFMA_CASES
    assert exact.wino_cases()[:len(WINO43_MFMA_CASES)] == list(WINO43_MFMA_CASES) and len(WINO43_MFMA_CASES) == 22
    # the workspace-less fallback case of the GPU file is a split-sized shape
    assert exact.wino43_regime(*exact.WINO_NO_WORKSPACE_CASE[:2], exact.WINO_NO_WORKSPACE_CASE[3])["S"] > 1
