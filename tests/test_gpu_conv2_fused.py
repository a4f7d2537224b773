"""The one-kernel conv2_1 / conv2_2 route (include/posecnn_hip/trunk/conv2_fused.h, csrc/conv2_fused.hip): Winograd F(4x4,3x3)
input transform, contractions and output transform of a 3x3 convolution with 64 | 128 input and 128 output channels in one
launch, the transformed input kept on the CU.

The claim is equality BIT FOR BIT (torch.equal, no tolerance) with the unfused pair on the same tensors —
ops.winograd_input(x, 4) followed by the packed MFMA kernel's one K chain per accumulator: the same expression trees in the
input transform, the same K order into every accumulator, the same fold. (`_unfused` says where ops.winograd43_conv itself
runs another chain, and why the network never takes the route there.) Shapes are the smallest at which each mechanism can fail (SHAPES);
milliseconds each. The reference of a (shape, Cin) pair is computed once per (relu, pool) and shared.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_memory_contract import Case, execute

pytestmark = pytest.mark.gpu

# (B, H, W, groups), what it exercises
SHAPES = [
    ((1, 16, 16, 1), "one block, all four borders padded"),
    ((2, 16, 32, 2), "two blocks sharing a halo column, two filter sets"),
    ((1, 32, 16, 1), "a shared halo row"),
    ((3, 48, 48, 1), "one fully interior block, odd batch"),
]
CIN_POOL = [(64, 0), (64, 1), (128, 0), (128, 1)]


@functools.lru_cache(maxsize=None)
def _inputs(shape, cin):
    """x with negative values and a band of exact zeros, filters, biases of both signs (CPU tensors, seeded)."""
    B, H, W, groups = shape
    rng = np.random.default_rng(1000 * cin + 17 * H + W + B)
    x = rng.standard_normal((B, H, W, cin)).astype(np.float32) * 3
    x[:, H // 2 - 2:H // 2 + 1] = 0.0           # a band of rows (it crosses tile and block borders)
    x[:, :, 5:7, : cin // 2] = 0.0              # ... and of columns, in half of the channels
    w = rng.standard_normal((groups, 128, cin, 3, 3)).astype(np.float32) * 0.05
    bias = rng.standard_normal((groups, 128)).astype(np.float32)
    assert (bias > 0).any() and (bias < 0).any() and (x < 0).any()
    return torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(bias)


def _bank(w, dev):
    """[groups,128,Cin,3,3] -> (U^T [groups,36,128,Cin], its fragment-major bank) on the device."""
    from posecnn_amd import ops
    ut = torch.stack([ops.winograd_filter(wg.to(dev), 4).transpose(1, 2) for wg in w]).contiguous()
    return ut, ops.winograd43_pack_filters(ut)


def _unfused(x, utp, bias, relu, pool, groups):
    """ops.winograd_input(x, 4) + the packed MFMA entry on the same tensors, WITHOUT a workspace. ops.winograd43_conv hands
    the entry a workspace, and a launch this small with Cin = 128 then splits Cin in two (wino43_cin_split): two partial
    outputs, each folded on its own and summed afterwards — another rounding order than the kernel's one chain per
    accumulator, which is what the fused kernel reproduces and what runs at every size the network takes the route at
    (>= 128 blocks: never split; test_at_the_floor_the_op_itself_is_the_reference). Without the workspace the entry runs that one chain at any size. With
    Cin = 64 there is nothing to split and the op itself is held to as well."""
    from posecnn_amd import _lib, ops
    B, H, W, cin = x.shape
    v = ops.winograd_input(x, 4)
    y = torch.empty((B, H // 2, W // 2, 128) if pool else (B, H, W, 128), dtype=torch.float32, device=x.device)
    st = _lib.lib().pcnn_winograd43_conv_packed_fwd(ops._ptr(v), ops._ptr(utp), ops._ptr(bias), B, H, W, cin, 128, groups,
                                                    1 if relu else 0, pool, ops._ptr(y), ops._ptr(None), ops._ptr(None), 0, ops._stream(x))
    assert st == _lib.PCNN_OK
    if cin == 64:
        assert torch.equal(y, ops.winograd43_conv(v, utp, bias, B, H, W, relu, pool, groups, packed=True))
    return y


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("cin,pool", CIN_POOL, ids=["%d_pool%d" % cp for cp in CIN_POOL])
@pytest.mark.parametrize("shape,what", SHAPES, ids=["x".join(map(str, s[0])) for s in SHAPES])
def test_fused_equals_the_unfused_pair(gpu, shape, what, cin, pool, relu):
    from posecnn_amd import ops
    B, H, W, groups = shape
    x, w, bias = (t.to(gpu) for t in _inputs(shape, cin))
    _, utp = _bank(w, gpu)
    ref = _unfused(x, utp, bias, relu, pool, groups)
    got = ops.winograd43_conv_fused(x, utp, bias, relu, pool, groups)
    assert got.shape == ref.shape == ((B, H // 2, W // 2, 128) if pool else (B, H, W, 128))
    assert ref.abs().max() > 0 and (relu or (ref < 0).any())
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), "%s Cin %d pool %d: %s" % (shape, cin, pool, what)


@pytest.mark.parametrize("cin,pool", CIN_POOL, ids=["%d_pool%d" % cp for cp in CIN_POOL])
def test_block_order_and_image_index(gpu, cin, pool):
    """Four images that differ by a constant, two filter sets, 2 x 3 blocks each: a block that reads another image, another
    block's patch or the other filter set is wrong in every pixel."""
    from posecnn_amd import ops
    shape = (4, 32, 48, 2)
    x, w, bias = (t.to(gpu) for t in _inputs(shape, cin))
    x = (x[:1] + torch.arange(4, device=gpu, dtype=torch.float32).reshape(4, 1, 1, 1) * 0.5).contiguous()
    _, utp = _bank(w, gpu)
    ref = _unfused(x, utp, bias, True, pool, 2)
    got = ops.winograd43_conv_fused(x, utp, bias, True, pool, 2)
    assert not torch.equal(ref[0], ref[1]) and not torch.equal(ref[1], ref[2])
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


REFUSED = [((1, 24, 16, 64, 128, 1), "H = 24"), ((1, 16, 16, 192, 128, 1), "Cin = 192"), ((1, 16, 16, 64, 64, 1), "Cout = 64"),
           ((3, 16, 16, 64, 128, 2), "batch 3 with groups 2")]


@pytest.mark.parametrize("c,what", REFUSED, ids=[r[1].replace(" ", "_") for r in REFUSED])
def test_refusals_leave_the_output_untouched(gpu, c, what):
    from posecnn_amd import _lib, ops
    B, H, W, cin, cout, groups = c
    x = torch.ones((B, H, W, cin), device=gpu)
    utp = torch.ones((groups, 36, cout, cin), device=gpu)
    bias = torch.ones((groups, cout), device=gpu)
    for pool in (0, 1):
        y = torch.full((B, H // (2 if pool else 1), W // (2 if pool else 1), cout), -7.25, device=gpu)
        st = _lib.lib().pcnn_winograd43_conv_fused_fwd(ops._ptr(x), ops._ptr(utp), ops._ptr(bias), B, H, W, cin, cout, groups, 1, pool,
                                                       ops._ptr(y), ops._stream(x))
        torch.cuda.synchronize()
        assert st == _lib.PCNN_EINVAL, what
        assert bool((y == -7.25).all()), what
    with pytest.raises(ValueError):
        ops.winograd43_conv_fused(x, utp, bias, True, 0, groups)


def _contract_case(cin, pool):
    shape = (2, 16, 32, 2)

    def make():
        x, w, bias = _inputs(shape, cin)
        return dict(x=x, utp=_bank(w, torch.device("cuda"))[1].cpu(), b=bias)

    def run(ctx):
        from posecnn_amd import ops
        return dict(y=ops.winograd43_conv_fused(ctx.e("x"), ctx.e("utp"), ctx.e("b"), True, pool, 2))

    def chk(d, o):
        dev = torch.device("cuda")
        ref = _unfused(d["x"].to(dev), d["utp"].to(dev), d["b"].to(dev), True, pool, 2)
        assert np.array_equal(o["y"].view(np.uint32), ref.cpu().numpy().view(np.uint32))

    return Case("conv2_fused_%d_pool%d" % (cin, pool), ("pcnn_winograd43_conv_fused_fwd",), make, run, chk)


CONTRACT = [_contract_case(64, 0), _contract_case(128, 1)]


@pytest.mark.parametrize("case", CONTRACT, ids=[k.name for k in CONTRACT])
def test_memory_contract(gpu, case):
    """Both poison patterns, guard bands around every buffer: inputs unchanged, every output element written by the library."""
    execute(case)


def _run_net(net, d, dp, fused):
    from posecnn_amd import _lib
    net.fused_conv2 = fused
    net.layers = {"data": d, "data_p": dp} if dp is not None else {"data": d}
    net.inputs = []
    _lib.profile_enable(True)
    _lib.profile_report()
    if dp is not None:
        assert net._can_group_towers()
        net._trunk_grouped()
        keys = ("conv4_3", "pool4", "conv5_3", "conv4_3_p", "pool4_p", "conv5_3_p")
    else:
        net._tower("data", "")
        keys = ("conv4_3", "pool4", "conv5_3")
    out = {k: net.get_output(k).clone() for k in keys}
    torch.cuda.synchronize()
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    count = lambda name: sum(v["calls"] for k, v in rep.items() if k.split("<")[0] == name)
    return out, {n: count(n) for n in ("conv2_wino43_fused_kernel", "wino43_input_kernel", "wino43_mfma_kernel")}


@pytest.mark.parametrize("cin,pool", [(128, 0), (128, 1), (64, 1)], ids=["128_pool0", "128_pool1", "64_pool1"])
def test_at_the_floor_the_op_itself_is_the_reference(gpu, cin, pool):
    """128 blocks, the smallest launch the network takes the route at: here ops.winograd43_conv, workspace and all, does not
    split Cin, and the fused kernel equals it bit for bit."""
    from posecnn_amd import ops
    from posecnn_amd.networks import Network
    shape = (2, 128, 128, 2)
    assert shape[0] * (shape[1] // 16) * (shape[2] // 16) == Network.FUSED_CONV2_FLOOR
    x, w, bias = (t.to(gpu) for t in _inputs(shape, cin))
    _, utp = _bank(w, gpu)
    ref = ops.winograd43_conv(ops.winograd_input(x, 4), utp, bias, *shape[:3], True, pool, 2, packed=True)
    got = ops.winograd43_conv_fused(x, utp, bias, True, pool, 2)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


# The smallest frames at which both conv2 launches of a 2-frame network have FUSED_CONV2_FLOOR blocks: the route is never taken
# below (there the unfused conv2_2 splits Cin and a bit-for-bit comparison between the routes would not hold).
NET_CASES = [("RGBD", 128, 256), ("COLOR", 256, 256)]


@pytest.mark.parametrize("fmt,H,W", NET_CASES, ids=["grouped_rgbd", "layer_by_layer_color"])
def test_network_route_is_bit_identical_and_launches_the_kernel_twice(gpu, fmt, H, W):
    from posecnn_amd.networks import vgg16_convs
    rng = np.random.default_rng(5)
    d = torch.from_numpy(rng.standard_normal((2, H, W, 3)).astype(np.float32) * 50).to(gpu)
    dp = torch.from_numpy(rng.standard_normal((2, H, W, 3)).astype(np.float32) * 50).to(gpu) if fmt == "RGBD" else None
    net = vgg16_convs(fmt, 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=False, is_train=False,
                      seed=3, init="he", with_losses=False, device=gpu)
    assert net.fused_conv2 and net.fused_conv2_min_blocks >= 49
    towers = 2 if fmt == "RGBD" else 1
    assert towers * 2 * (H // 32) * (W // 32) == net.FUSED_CONV2_FLOOR
    net.fused_conv2_min_blocks = 1   # counts as the floor
    with torch.no_grad():
        assert not net._conv2_fused_at(towers * 2, 32, 48, 64, 128)      # 64 x 96 frames: below the floor whatever the minimum says
        a, na = _run_net(net, d, dp, True)
        b, nb = _run_net(net, d, dp, False)
    assert na == {"conv2_wino43_fused_kernel": 2, "wino43_input_kernel": 9, "wino43_mfma_kernel": 9}, na
    assert nb == {"conv2_wino43_fused_kernel": 0, "wino43_input_kernel": 11, "wino43_mfma_kernel": 11}, nb
    for k in a:
        assert a[k].abs().max() > 0, k
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
