"""Every pending form of a convolution in `posecnn_amd/networks.py` against every kind of consumer, on a bare `Network`.
The route table (tests/network_routes.py) runs whole `vgg16_convs` graphs, where each deferred conv meets the consumer it was
deferred for; here each form also meets the others: a fetch of the un-pooled tensor, a pool after a fetch, a pool that is not
2x2/2, a plain layer, a following convolution. Per case: (a) every fetched tensor bit for bit the same graph on a network
that defers nothing (`BASELINE`), which `network_routes.CLAIMS` and the op-level tests claim equal; (b) the launches per
library kernel the form implies (0: must not appear) — without them a network that always activated would pass (a)."""
import collections

import pytest
import torch

import network_routes as R
from posecnn_amd.networks import Network
from test_gpu_network_routes import profiled

pytestmark = pytest.mark.gpu

BASELINE = {"defer_act": frozenset(), "dual_pool": frozenset(), "fused_conv12": False, "fuse_first_conv_into_winograd": False}

Form = collections.namedtuple("Form", "name shape raw first defer dual flags pooled fetched")


def _calls(**kw):
    d = {k: 0 for k in R.LIBRARY_TRUNK}
    d.update(kw)
    return d


C3 = _calls(conv3x3_c3_bias_relu_kernel=1)
C12 = _calls(conv12_wino43_fused_kernel=1)
PAIR = _calls(conv3x3_c3_wino43_kernel=1, wino43_mfma_kernel=1)
MFMA = _calls(wino43_input_kernel=1, wino43_mfma_kernel=1)
BMM = _calls(wino43_input_kernel=1, wino43_output_kernel=1)
F23 = _calls(wino_input_kernel=1, wino_output_kernel=1)
NO_WINO = {"winograd_min_channels": 0}
NO_MFMA = {"winograd_mfma": False}
TILE2 = {"winograd_tile": 2, "winograd_min_channels": 64}

# name, input, raw frame?, is "c" the 3-channel first conv (else a 64 -> 64 conv, behind the first conv "c1" on a frame)?, "c" in
# `defer_act`?, in `dual_pool`?, flags, launches when max_pool(2,2,2,2) consumes "c", launches when anything else does (a
# following 1x1 convolution adds its own bias_act_kernel)
FORMS = [
    Form("first_blob", (1, 16, 32, 3), False, True, False, False, {}, C3, C3),
    Form("first_raw", (1, 16, 32, 3), True, True, False, False, {}, C3, C3),
    Form("lazy12_blob", (1, 16, 32, 3), False, False, True, False, {}, C12, PAIR),
    Form("lazy12_raw", (1, 16, 32, 3), True, False, True, False, {}, C12, PAIR),
    Form("gemm", (1, 8, 12, 64), False, False, True, False, {}, MFMA, MFMA),
    Form("both", (1, 8, 12, 64), False, False, False, True, {}, MFMA, MFMA),
    Form("wino43_bmm", (1, 8, 12, 64), False, False, True, False, NO_MFMA, BMM, BMM),
    Form("wino43_bmm_both", (1, 8, 12, 64), False, False, False, True, NO_MFMA, BMM, BMM),
    Form("wino23", (1, 8, 12, 64), False, False, True, False, TILE2, F23, F23),
    Form("y", (1, 8, 12, 64), False, False, True, False, NO_WINO, _calls(bias_relu_pool2_kernel=1), _calls(bias_act_kernel=1)),
    # odd H or W: nothing stays pending, the max_pool is the generic one
    Form("odd_h_defer", (1, 7, 12, 64), False, False, True, False, {}, MFMA, MFMA),
    Form("odd_w_defer", (1, 8, 11, 64), False, False, True, False, {}, MFMA, MFMA),
    Form("odd_h_dual", (1, 7, 12, 64), False, False, False, True, {}, MFMA, MFMA),
    Form("odd_w_dual", (1, 8, 11, 64), False, False, False, True, {}, MFMA, MFMA),
]
CONSUMERS = ("pool", "fetch_pool", "pool_stride1", "relu", "conv1x1")

_SHARED = {}


@pytest.fixture(scope="module", autouse=True)
def _release_what_the_module_shared():
    yield
    _SHARED.clear()


def variables(gpu):
    """One seeded set for the module: c1 3 -> 64 (3x3), c 64 -> 64 (3x3) or 3 -> 64, k 64 -> 64 (1x1); biases of both signs."""
    if "vars" not in _SHARED:
        g = torch.Generator(device="cpu").manual_seed(23)
        v = {}
        for name, shape in (("c1", (64, 3, 3, 3)), ("c", (64, 64, 3, 3)), ("c_first", (64, 3, 3, 3)), ("k", (64, 64, 1, 1))):
            fan_in = shape[1] * shape[2] * shape[3]
            v[name + "/weights"] = (torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5).contiguous(memory_format=torch.channels_last).to(gpu)
            v[name + "/biases"] = (torch.randn((shape[0],), generator=g) * 0.5).to(gpu)
        _SHARED["vars"] = v
    return _SHARED["vars"]


def input_for(gpu, form):
    key = (form.shape, form.raw)
    if key not in _SHARED:
        g = torch.Generator(device="cpu").manual_seed(29)
        if form.raw:
            x = torch.randint(0, 256, form.shape, generator=g, dtype=torch.uint8)
        else:
            x = torch.randn(form.shape, generator=g) * (60.0 if form.shape[-1] == 3 else 1.0)
        _SHARED[key] = x.to(gpu)
    return _SHARED[key]


class _Net(Network):
    pass


def run(gpu, form, consumer, flags):
    """The graph of one case on a fresh network with `flags`: ({layer: cpu tensor}, {kernel: calls})."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    net = _Net(device=gpu, trainable=False)
    v = variables(gpu)
    net.vars = {name + s: v[src + s] for name, src in (("c1", "c1"), ("c", "c_first" if form.first else "c"), ("k", "k"))
                for s in ("/weights", "/biases")}
    net.defer_act = frozenset(["c"]) if form.defer else frozenset()
    net.dual_pool = frozenset(["c"]) if form.dual else frozenset()
    for k, val in flags.items():
        assert hasattr(net, k), k
        setattr(net, k, val)
    net.layers = {"x": input_for(gpu, form)}

    def go():
        with torch.no_grad():
            net.feed("x")
            if form.shape[-1] == 3 and not form.first:
                net.conv(3, 3, 64, 1, 1, name="c1")
            net.conv(3, 3, 64, 1, 1, name="c")
            out = {}
            if consumer == "pool":
                net.max_pool(2, 2, 2, 2, name="p")
                names = ("p",)
            elif consumer == "fetch_pool":
                out["c"] = net.get_output("c").clone()     # (before the pool: a later layer must not have touched it either)
                net.max_pool(2, 2, 2, 2, name="p")
                names = ("c", "p")
            elif consumer == "pool_stride1":
                net.max_pool(2, 2, 1, 1, name="p")
                names = ("p",)
            elif consumer == "relu":
                net.relu(name="r")
                names = ("r",)
            else:
                net.conv(1, 1, 64, 1, 1, name="k")
                names = ("k",)
            got = {n: net.get_output(n).detach().cpu() for n in names}
            if "c" in out:
                assert torch.equal(out["c"].cpu(), got["c"]), "the fetched tensor changed under the max_pool behind it"
            return got
    # the framework's 1x1 convolution behind "c" does not repeat its own bits at 16 x 32 (the same call on the same tensor, twice)
    # unless it is told to: no statement about a pending form could be read off it otherwise
    det, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        return profiled(go)
    finally:
        torch.backends.cudnn.deterministic = det


@pytest.mark.parametrize("consumer", CONSUMERS)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name)
def test_pending_conv_meets_consumer(gpu, form, consumer):
    got, calls = run(gpu, form, consumer, form.flags)
    want, _ = run(gpu, form, consumer, dict(form.flags, **BASELINE))
    print("CALLS %-16s %-12s %s" % (form.name, consumer, sorted(calls.items())))
    assert set(got) == set(want)
    for n in sorted(got):                                                                        # a.
        assert got[n].shape == want[n].shape and torch.isfinite(got[n]).all(), n
        assert torch.equal(got[n], want[n]), "%s differs from the network that defers nothing (max %g)" % (
            n, float((got[n] - want[n]).abs().max()))
    present = dict(form.pooled if consumer == "pool" else form.fetched)                          # b.
    if consumer == "conv1x1":
        present["bias_act_kernel"] += 1
    assert not R.route_errors(calls, present), (R.route_errors(calls, present), sorted(calls.items()))
