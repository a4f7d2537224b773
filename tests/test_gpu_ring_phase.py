"""Ring-position tests of the two dense MFMA kernels (csrc/wino_mfma.hip, csrc/fc_mfma.hip) on exact-integer data.

Both kernels carry the position in their LDS ring of stage buffers in the `offset:` field of the ds_read_b128
instructions: the trunk kernel picks one of three copies of its reads by the ring position, the fc kernel one of two (every
split-K slice starts in buffer 0, whatever its first stage). Which buffer a read must address depends on
the stage count per plane (trunk) or per split-K slice (fc) modulo the ring length; tests/ring_phase.py lists the counts
the other test files lack (3, 5, 7 and 3 under the Cin split; 3, 5, 17 = 8 + 9 and 27 = 9 + 9 + 9). The kernel's fp32
output must EQUAL the float64 reference of tests/exact.py: an operand taken from the wrong buffer is another stage's
(or a stale one's) data and changes whole 16 x 16 blocks of integers.

Each case is a few tiles or rows: one partially filled workgroup (6 tiles, 26 clamped rows) for the single-set trunk
cases, four workgroups for the grouped ones, one to six for fc. Milliseconds each.
"""
import pytest
import torch

import exact
import ring_phase
from exact import LIMIT, check, zero_bits

pytestmark = pytest.mark.gpu


def _count(gpu, n):
    return torch.tensor([n], dtype=torch.int32, device=gpu)


@pytest.mark.parametrize("case,S,stages", ring_phase.TRUNK_CASES)
def test_trunk_equals_float64_at_every_ring_phase(gpu, case, S, stages):
    from posecnn_amd import ops
    (B, H, W, cin), cout, pool, groups = case
    v, ut, bias = ring_phase.trunk_inputs(case, gpu)
    assert exact.abs_bound("wino43", v, ut, bias, B, H, W, True, pool, groups) < LIMIT
    assert exact.wino43_regime((B, H, W, cin), cout, groups)["S"] == S
    for relu in (True, False):
        ref = exact.wino43_reference(v, ut, bias, B, H, W, relu, pool, groups)
        got = ops.winograd43_conv(v, ut, bias, B, H, W, relu, pool, groups)   # (hands the workspace of a Cin split over)
        got, ref = (got if isinstance(got, tuple) else (got,)), (ref if isinstance(ref, tuple) else (ref,))
        assert len(got) == len(ref)
        for i, (g, r) in enumerate(zip(got, ref)):
            pooled = pool == 1 or i == 1
            check(g, r, {"name": "winograd43_conv %s (%d stages per plane, S = %d) relu=%s %s" % (case, stages, S, relu, "pooled" if pooled else "full"),
                         "wino": (B, H, W, groups, pooled)})


@pytest.mark.parametrize("cap,K,N", ring_phase.FC_CASES)
def test_fc_rows_equals_float64_at_every_ring_phase_and_row_count(gpu, cap, K, N):
    from posecnn_amd import ops
    x, wt, bias = ring_phase.fc_inputs(cap, K, N, gpu)
    assert exact.abs_bound("fc", x, wt, bias) < LIMIT
    ref = exact.fc_reference(x, wt, bias)
    for i, n in enumerate(exact.fc_counts(cap)):
        xp = exact.poison_rows(x, n)
        for relu in ((False, True) if n in (cap, 65, 1) else (bool(i & 1),)):
            y = ops.fc_rows(xp, wt, bias, relu, num_rows=_count(gpu, n))
            check(y[:n], torch.relu(ref[:n]) if relu else ref[:n], {"name": "fc_rows %s count %d relu=%s" % ((cap, K, N), n, relu), "fc": True})
            assert zero_bits(y[n:]), "fc_rows %s: rows at or past the count %d are not all-zero bits" % ((cap, K, N), n)
    for relu in (False, True):
        check(ops.fc_rows(x, wt, bias, relu, num_rows=None), torch.relu(ref) if relu else ref, {"name": "fc_rows %s uncounted relu=%s" % ((cap, K, N), relu), "fc": True})


def test_fc_rows_cols_equals_float64_at_three_stages(gpu):
    from posecnn_amd import ops
    cap, K, N, npad = ring_phase.FC_COLS_CASE
    x, wt, bias = ring_phase.fc_inputs(cap, K, N, gpu)
    assert exact.abs_bound("fc", x, wt, bias) < LIMIT
    wp = torch.zeros((npad, K), device=gpu); wp[:N] = wt
    bp = torch.zeros((npad,), device=gpu); bp[:N] = bias
    ref = exact.fc_reference(x, wt, bias)
    for n in exact.fc_counts(cap):
        y = ops.fc_rows_cols(exact.poison_rows(x, n), wp, bp, N, "none", num_rows=_count(gpu, n))
        assert tuple(y.shape) == (cap, N)
        check(y[:n], ref[:n], {"name": "fc_rows_cols, count %d" % n, "fc": True})
        assert zero_bits(y[n:]), "fc_rows_cols: rows at or past the count %d are not all-zero bits" % n


def test_fc_rows_split_equals_float64_at_three_stages(gpu):
    from posecnn_amd import ops
    cap, K, out_a, out_b = ring_phase.FC_SPLIT_CASE
    x, wt, bias = ring_phase.fc_inputs(cap, K, out_a + out_b, gpu)
    assert exact.abs_bound("fc", x, wt, bias) < LIMIT
    ref = exact.fc_reference(x, wt, bias)
    for n in exact.fc_counts(cap):
        ya, yb = ops.fc_rows_split(exact.poison_rows(x, n), wt, bias, out_a, relu_a=True, relu_b=False, num_rows=_count(gpu, n))
        check(ya[:n], torch.relu(ref[:n, :out_a]), {"name": "fc_rows_split a, count %d" % n, "fc": True})
        check(yb[:n], ref[:n, out_a:], {"name": "fc_rows_split b, count %d" % n, "fc": True})
        assert zero_bits(ya[n:]) and zero_bits(yb[n:]), "fc_rows_split: rows at or past the count %d are not all-zero bits" % n
