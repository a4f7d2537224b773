"""The packed-filter route of the Winograd trunk kernel (include/posecnn_hip_wino_packed.h, csrc/wino_mfma.hip with BSRC = 1):
the filter operand goes straight from global memory into registers, from the fragment-major bank of
ops.winograd43_pack_filters, instead of through the kernel's LDS ring.

Products, K order and fold are those of the old route, so every case is held BIT FOR BIT — no tolerance — to two references:
the old entry on the row-major bank (ops.winograd43_conv(packed=False)) and the float64 evaluation of tests/exact.py. The
inputs are small integers (the method of tests/test_gpu_ring_phase.py): every f32 sum is exact, so float64 is reachable bit
for bit and a wrong operand — another stage's, another wave's, a stale register's — changes whole 16 x 16 blocks of integers.
Two references, so that a bug the two kernels share cannot hide.

Shapes are the smallest at which each path of the kernel and the launcher is taken (see CONV_CASES); milliseconds each.
"""
import numpy as np
import pytest
import torch

import exact
import memguard
from exact import LIMIT, check
from test_gpu_memory_contract import Case, execute

pytestmark = pytest.mark.gpu

PACK_CASES = [(64, 64, 1), (192, 128, 2), (128, 512, 1)]   # (Cin, Cout, groups)

# (B, H, W, Cin, Cout, groups, pool), relu, what it exercises
CONV_CASES = [
    ((2, 8, 12, 64, 64, 1, 0), True, "12 tiles: one partial block; one stage per plane (odd: the planes alternate register parity)"),
    ((2, 10, 18, 192, 128, 2, 1), True, "ragged tile rows and columns; 3 stages per plane; two channel blocks; two filter sets; pooled only"),
    ((2, 10, 18, 192, 128, 2, 2), True, "... both outputs"),
    ((1, 12, 44, 128, 64, 1, 0), False, "33 tiles: a second block with one live tile; 2 stages per plane (even); no ReLU"),
    ((1, 8, 8, 512, 64, 1, 0), True, "Cin split, S > 1, on the workspace the op hands over: every slice starts at its own first K stage"),
    ((1, 8, 8, 64, 512, 1, 0), True, "the channel-block-major workgroup map"),
]


def _case(c):
    B, H, W, cin, cout, groups, pool = c
    return ((B, H, W, cin), cout, pool, groups)


def np_pack(ut):
    """The permutation of the header, in numpy: utp[g][k][n16][kc][j][16 lk + lr][e] = ut[g][k][16 n16 + lr][64 kc + 16 j + 4 lk + e]."""
    G, K36, cout, cin = ut.shape
    a = ut.reshape(G, K36, cout // 16, 16, cin // 64, 4, 4, 4)   # g, k, n16, lr, kc, j, lk, e
    return np.ascontiguousarray(a.transpose(0, 1, 2, 4, 5, 6, 3, 7)).reshape(ut.shape)   # g, k, n16, kc, j, lk, lr, e


@pytest.mark.parametrize("cin,cout,groups", PACK_CASES)
def test_pack_kernel_is_the_numpy_permutation(gpu, cin, cout, groups):
    from posecnn_amd import ops
    n = groups * 36 * cout * cin
    ut = torch.arange(n, dtype=torch.float32, device=gpu).reshape(groups, 36, cout, cin)   # every element its own index (< 2^24)
    assert n < LIMIT
    got = ops.winograd43_pack_filters(ut)
    assert got.shape == ut.shape and got.data_ptr() != ut.data_ptr()
    assert np.array_equal(got.cpu().numpy(), np_pack(ut.cpu().numpy()))
    if groups == 1:   # [36, Cout, Cin] is taken as one group
        assert torch.equal(ops.winograd43_pack_filters(ut[0]), got[0])


@pytest.mark.parametrize("c,relu,what", CONV_CASES, ids=["x".join(map(str, c[0])) for c in CONV_CASES])
def test_packed_route_equals_old_route_and_float64(gpu, c, relu, what):
    from posecnn_amd import ops
    B, H, W, cin, cout, groups, pool = c
    case = _case(c)
    v, ut, bias = exact.wino_inputs(case, gpu)
    assert exact.abs_bound("wino43", v, ut, bias, B, H, W, True, pool, groups) < LIMIT
    regime = exact.wino43_regime((B, H, W, cin), cout, groups)
    if c == (1, 8, 8, 512, 64, 1, 0):
        assert regime["S"] > 1, regime
    if c == (1, 8, 8, 64, 512, 1, 0):
        assert regime["ncb"] == 8 and regime["u_heavier"] and regime["S"] == 1, regime
    utp = ops.winograd43_pack_filters(ut)
    ref = exact.wino43_reference(v, ut, bias, B, H, W, relu, pool, groups)
    old = ops.winograd43_conv(v, ut, bias, B, H, W, relu, pool, groups)
    got = ops.winograd43_conv(v, utp, bias, B, H, W, relu, pool, groups, packed=True)
    tup = lambda t: t if isinstance(t, tuple) else (t,)
    got, old, ref = tup(got), tup(old), tup(ref)
    assert len(got) == len(old) == len(ref) == (2 if pool == 2 else 1)
    for i, (g, o, r) in enumerate(zip(got, old, ref)):
        pooled = pool == 1 or i == 1
        assert torch.equal(g.view(torch.int32), o.view(torch.int32)), "packed route differs from the old route: %s (%s)" % (c, what)
        check(g, r, {"name": "winograd43_conv packed %s (%s) %s" % (c, what, "pooled" if pooled else "full"), "wino": (B, H, W, groups, pooled)})


def _contract_case(name, c, packed):
    """Poisoned outputs and workspace, guard bands intact afterwards (tests/memguard.py), both poison patterns agreeing bit for bit."""
    B, H, W, cin, cout, groups, pool = c

    def make():
        v, ut, bias = exact.wino_inputs(_case(c))
        return dict(v=v, ut=ut, b=bias)

    def run(ctx):
        from posecnn_amd import ops
        utp = ops.winograd43_pack_filters(ctx.e("ut"))
        if not packed:
            return dict(utp=utp)
        out = ops.winograd43_conv(ctx.e("v"), utp, ctx.e("b"), B, H, W, True, pool, groups, packed=True)
        return dict(y=out[0], y_pool=out[1]) if pool == 2 else dict(y=out)

    def chk(d, o):
        if not packed:
            assert np.array_equal(o["utp"], np_pack(memguard.to_numpy(d["ut"])))
            return
        ref = exact.wino43_reference(d["v"], d["ut"], d["b"], B, H, W, True, pool, groups)
        ref = ref if isinstance(ref, tuple) else (ref,)
        for k, r in zip(("y", "y_pool"), ref):
            assert np.array_equal(o[k].astype(np.float64), r.numpy()), k

    covers = ("pcnn_winograd43_pack_filters_fwd",) + (("pcnn_winograd43_conv_packed_fwd",) if packed else ())
    return Case(name, covers, make, run, chk)


CONTRACT = [_contract_case("pack_192x128x2", (2, 10, 18, 192, 128, 2, 2), False),
            _contract_case("conv_packed_both_outputs", (2, 10, 18, 192, 128, 2, 2), True),
            _contract_case("conv_packed_cin_split_workspace", (1, 8, 8, 512, 64, 1, 0), True)]


@pytest.mark.parametrize("case", CONTRACT, ids=[k.name for k in CONTRACT])
def test_memory_contract_of_the_packed_entries(gpu, case):
    execute(case)


def _trunk(net, d, dp, grouped):
    net.layers = {"data": d, "data_p": dp}
    net.inputs = []
    net.grouped_towers = grouped
    if grouped:
        assert net._can_group_towers()
        net._trunk_grouped()
    else:
        net._tower("data", "")
        net._tower("data_p", "_p")
    torch.cuda.synchronize()
    return {k: net.get_output(k).clone() for k in ("conv5_3", "conv4_3", "conv5_3_p", "conv4_3_p")}


@pytest.mark.parametrize("grouped", [True, False], ids=["one_launch_per_layer", "tower_by_tower"])
def test_network_packed_route_equals_unpacked_and_follows_weight_updates(gpu, grouped):
    """A 2-frame RGB-D net at 32 x 48: conv5_3 and conv4_3 of both towers bit for bit the same on either bank, before and after
    an in-place weight update (which must rebuild the packed bank: `Network._derived` keys it on the variable's version)."""
    from posecnn_amd.networks import vgg16_convs
    rng = np.random.default_rng(11)
    d = torch.from_numpy(rng.standard_normal((2, 32, 48, 3)).astype(np.float32) * 50).to(gpu)
    dp = torch.from_numpy(rng.standard_normal((2, 32, 48, 3)).astype(np.float32) * 50).to(gpu)
    net = vgg16_convs("RGBD", 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=False, is_train=False,
                      seed=3, init="he", with_losses=False, device=gpu)
    assert net.winograd_packed   # the default route
    with torch.no_grad():
        runs = []
        for step in range(2):
            net.winograd_packed = True
            a = _trunk(net, d, dp, grouped)
            banks = {k: v[3] for k, v in net._cache.items() if isinstance(k, tuple) and k[0] == "wino_packed"}
            assert len(banks) >= 11, sorted(map(str, banks))   # conv2_1 .. conv5_3 (conv1_2 too without the fused first layers)
            net.winograd_packed = False
            b = _trunk(net, d, dp, grouped)
            for k in a:
                assert a[k].abs().max() > 0, k
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "%s differs between the banks (step %d)" % (k, step)
            runs.append((a, banks))
            if step == 0:
                net._trunk_vars("")[-1][0].mul_(2.0)   # conv5_3/weights of the colour tower, in place
        (a0, banks0), (a1, banks1) = runs
        assert torch.equal(a0["conv4_3"], a1["conv4_3"]) and torch.equal(a0["conv5_3_p"], a1["conv5_3_p"])
        assert not torch.equal(a0["conv5_3"], a1["conv5_3"]), "the packed bank of conv5_3 was not rebuilt after the weight update"
        rebuilt = [k for k in banks0 if banks0[k] is not banks1[k]]
        assert len(rebuilt) == 1, rebuilt   # conv5_3's bank alone
