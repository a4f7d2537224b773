"""GPU tests of the derived-tensor cache (`Network._derived`): every dense kernel reads a filter that was transformed,
transposed, padded or packed from a variable once and kept — Winograd U^T, the fragment-major conv1_2 bank, the grouped
RGB-D packing, the head and fc transposes, the merged head filters. After the variables change, in place or by `load()`,
a network must compute what a freshly constructed network (empty cache) computes from the same variables, bit for bit:
  * the whole network at 1 x 32 x 48 — the smallest frame at which the fused conv1_1 -> conv1_2 -> pool1 kernel, the MFMA
    trunk, the small-head kernel and the merged head convs all apply — COLOR (the chained path) and RGBD (the grouped one);
  * `fc` and `fc_tanh` on device-counted rows: 8 rows (the skinny kernel) and 40 (the row kernel, the padded fc8 filter).
"""
import numpy as np
import pytest

from posecnn_amd import config, synth
from test_gpu_ops import N, T, same

pytestmark = pytest.mark.gpu

KEEP = ("conv5_3", "score_conv4", "score_conv5", "add_score", "vertex_pred_lowres", "prob_normalized", "label_2d")


def _tf_dict(vars_, scale):
    """The variables as `Network.load` takes them ({layer: {'weights', 'biases'}} in TF layouts, what save_npz writes), scaled."""
    out = {}
    for key, v in vars_.items():
        layer_name, pname = key.rsplit("/", 1)
        t = v.detach().cpu()
        if pname == "weights" and t.dim() == 4:
            t = t.permute(2, 3, 1, 0)   # [cout,cin,kh,kw] -> [kh,kw,cin,cout]
        out.setdefault(layer_name, {})[pname] = np.ascontiguousarray(t.numpy()) * np.float32(scale)
    return out


def _three_steps(net, make, run):
    """`net` holds its variables, `make()` constructs a network like it without any, `run(net)` evaluates one and returns
    {name: array}. Step 1: run. Step 2: every variable times 1.25 in place. Step 3: every variable replaced by a new tensor
    (0.8 x) through load(). After steps 2 and 3 the outputs equal those of a fresh network handed the same variables.
    Returns the outputs of the three steps."""
    import torch
    outs = [run(net)]
    for step in (2, 3):
        if step == 2:
            with torch.no_grad():
                for v in net.vars.values():
                    v.mul_(1.25)
        else:
            old = dict(net.vars)
            net.load(_tf_dict(old, 0.8))
            assert list(net.vars) == list(old) and all(net.vars[k] is not old[k] for k in old)
            del old
        got = run(net)
        fresh = make()
        fresh.vars = dict(net.vars)
        want = run(fresh)
        for name in want:
            same(got[name], want[name], "%s after step %d" % (name, step))
        outs.append(got)
    return outs


def _small_biases(net):
    """init_calibrated's biases are zeros, and 1.25 x 0 tells nothing: small non-zero ones, so that a stale bias (the grouped
    packing, the merged heads and the padded fc8 filter carry biases) shows like a stale filter."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(23)
    for key, v in net.vars.items():
        if key.endswith("/biases"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.05).to(v.device))
    return net


@pytest.mark.parametrize("fmt", ["COLOR", "RGBD"])
def test_whole_network_follows_its_variables(gpu, fmt):
    import torch
    from posecnn_amd import fcn
    from posecnn_amd.networks import vgg16_convs
    C, H, W = 22, 32, 48
    K = config.DEMO_INTRINSICS.copy(); K[:2] *= W / 640.0
    pts = synth.make_model_points(C, 32)
    rng = np.random.default_rng(12)
    data = T(gpu, (rng.integers(0, 256, (1, H, W, 3)).astype(np.float32) - config.PIXEL_MEANS).astype(np.float32))
    data_p = T(gpu, (rng.integers(0, 256, (1, H, W, 3)).astype(np.float32) - config.PIXEL_MEANS).astype(np.float32)) if fmt == "RGBD" else None

    def make():
        return vgg16_convs(fmt, C, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=False, is_train=False,
                           device=gpu)

    def run(net):
        feed = fcn._feed(net, data, data_p, K, config.LOV_EXTENTS, pts, config.LOV_SYMMETRY, C, gpu)
        with torch.no_grad():
            net.run(feed)
        return {n: N(net.get_output(n)) for n in KEEP}

    net = _small_biases(synth.init_calibrated(make()))
    assert net._conv12_fused_at(H, W) and net.small_heads and net.merge_head_convs and net.grouped_towers
    o1, o2, o3 = _three_steps(net, make, run)
    for name in ("conv5_3", "prob_normalized"):
        assert not np.array_equal(o1[name], o2[name]) and not np.array_equal(o2[name], o3[name]), name
        assert np.abs(o1[name]).max() > 0 and np.isfinite(o2[name]).all() and np.isfinite(o3[name]).all(), name


@pytest.mark.parametrize("M", [8, 40])
def test_fc_layers_follow_their_variables(gpu, M):
    """x [M,128] through fc(64) and fc_tanh(88) with a device-side row count of M: the skinny kernel at 8 rows, the row
    kernel (and fc_tanh's zero-padded filter) at 40."""
    import torch
    from posecnn_amd.networks import Network

    class Layers(Network):
        def setup(self):
            pass

    g = torch.Generator(device="cpu").manual_seed(31 + M)
    x = torch.randn((M, 128), generator=g).to(gpu)
    count = torch.tensor([M], dtype=torch.int32, device=gpu)
    want_route = "skinny" if M <= 32 else "rows"

    def make():
        return Layers(device=gpu, trainable=False)

    def run(net):
        assert net._fc_route(True, M, 128, 64, False, True) == want_route
        assert net._fc_route(True, M, 128, 88, False, True, padded_width=True) == want_route
        net.layers = {"x": x}
        net.rows_count = count
        try:
            with torch.no_grad():
                net.feed("x").fc(64, name="f")
                net.feed("x").fc_tanh(88, name="f8", tanh_name="t8")
        finally:
            net.rows_count = None
        return {n: N(net.get_output(n)) for n in ("f", "f8", "t8")}

    net = make()
    net.vars = {"f/weights": (torch.randn((128, 64), generator=g) / 128 ** 0.5).to(gpu), "f/biases": torch.zeros(64, device=gpu),
                "f8/weights": (torch.randn((128, 88), generator=g) / 128 ** 0.5).to(gpu), "f8/biases": torch.zeros(88, device=gpu)}
    o1, o2, o3 = _three_steps(_small_biases(net), make, run)
    assert o1["f"].shape == (M, 64) and o1["f8"].shape == (M, 88) and o1["t8"].shape == (M, 88) and np.abs(o1["f"]).max() > 0.5
    for name in ("f", "f8", "t8"):
        assert not np.array_equal(o1[name], o2[name]) and not np.array_equal(o2[name], o3[name]), name
