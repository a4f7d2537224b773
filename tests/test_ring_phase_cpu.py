"""The cases of tests/test_gpu_ring_phase.py, checked without a GPU: every one is exact-integer data (per-output sum of
absolute terms below 2^24, so fp32 must equal float64 in any summation order), the library reports the Cin split each
trunk case claims, and the lists hold the stage counts they were written for — per plane (trunk) a multiple of the
ring's three buffers and odd counts above 1, per launch (fc) odd counts and, through the device-side split-K, odd
slices from odd first stages."""
import pytest

import exact
import ring_phase
from exact import LIMIT


@pytest.mark.parametrize("case,S,stages", ring_phase.TRUNK_CASES)
def test_trunk_ring_cases_are_exact(case, S, stages):
    (B, H, W, cin), cout, pool, groups = case
    v, ut, bias = ring_phase.trunk_inputs(case)
    assert exact.abs_bound("wino43", v, ut, bias, B, H, W, True, pool, groups) < LIMIT
    assert exact.wino43_closed_bound(cin, exact.WINO_VMAX, exact.WINO_UMAX, exact.WINO_BMAX) < LIMIT


@pytest.mark.parametrize("cap,K,N", ring_phase.fc_shapes())
def test_fc_ring_cases_are_exact(cap, K, N):
    x, wt, bias = ring_phase.fc_inputs(cap, K, N)
    assert exact.abs_bound("fc", x, wt, bias) < LIMIT
    assert exact.fc_closed_bound(K, exact.FC_A, exact.FC_A, exact.FC_BIAS) < LIMIT


@pytest.mark.parametrize("case,S,stages", ring_phase.TRUNK_CASES)
def test_trunk_ring_cases_take_the_split_they_claim(case, S, stages):
    shape, cout, pool, groups = case
    regime = exact.wino43_regime(shape, cout, groups)
    assert regime["S"] == S, regime
    assert shape[3] % (64 * S) == 0 and shape[3] // 64 // S == stages


def test_ring_cases_hold_the_stage_counts_the_base_lists_lack():
    trunk = {stages for _, _, stages in ring_phase.TRUNK_CASES}
    assert any(n % 3 == 0 for n in trunk), "no plane of a whole number of turns of the three-buffer ring"
    assert {n % 3 for n in trunk} == {0, 1, 2}
    assert sum(1 for n in trunk if n % 2 == 1 and n > 1) >= 3
    assert any(S > 1 and stages % 3 == 0 for _, S, stages in ring_phase.TRUNK_CASES), "no split case with 3 stages per slice"
    one_block = [c for (c, _, _) in ring_phase.TRUNK_CASES if c[3] == 1]
    assert all(B * ((H + 3) // 4) * ((W + 3) // 4) < 32 for ((B, H, W, _), _, _, _) in one_block), "a partially filled workgroup"
    # the base lists, for the record: powers of two only
    assert all((c[0][3] // 64) & (c[0][3] // 64 - 1) == 0 for c in exact.wino_cases())
    assert all(K % 128 == 0 for (_, K, *_) in exact.FC_ROWS_CASES)
    fc = [K // 64 for _, K, _ in ring_phase.fc_shapes()]
    assert all(n % 2 == 1 and n > 1 for n in fc)
    # fc_split (csrc/fc_mfma.hip) for one live 64-row block of one column block: S = min(8, stages // 8); slice ks covers
    # stages [stages ks / S, stages (ks + 1) / S)
    slices = {}
    for cap, K, N in ring_phase.FC_CASES:
        n = K // 64
        S = max(1, min(8, n // 8)) if (cap <= N and K >= 1024 and cap <= 64 and N == 64) else 1
        slices[K] = [(n * ks // S, n * (ks + 1) // S) for ks in range(S)]
    assert slices[1088] == [(0, 8), (8, 17)] and slices[1728] == [(0, 9), (9, 18), (18, 27)]
    assert any(a % 2 == 1 and (b - a) % 2 == 1 for a, b in slices[1728]), "an odd slice from an odd first stage"
