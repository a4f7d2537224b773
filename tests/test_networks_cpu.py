"""CPU tests of the `lib/networks` surface: TF1 layer semantics of the dense layers (checked against
direct numpy loops written from the TF definitions), the fixed bilinear deconv filter, and the
`vgg16_convs` graph wiring (run end to end on the CPU restatement with the oracle)."""
import numpy as np
import pytest
import torch

from cpu_reference import run_cpu_pipeline, vgg16_convs_cpu
from posecnn_amd import config, synth
from posecnn_amd.networks import Network, make_deconv_filter_1d

F = np.float32


class Tiny(Network):
    def setup(self):
        pass


def test_make_deconv_filter_values():
    # network.py:141-150: k=4 -> taps .25 .75 .75 .25 ; k=16 -> c = 0.9375
    assert np.allclose(make_deconv_filter_1d(4), [0.25, 0.75, 0.75, 0.25])
    f16 = make_deconv_filter_1d(16)
    assert np.allclose(f16[:3], [1 - 0.9375, 1 - abs(1 / 8 - 0.9375), 1 - abs(2 / 8 - 0.9375)])
    assert np.isclose(f16.sum(), 8.0)  # stride-8 bilinear kernel: taps sum to the stride


def tf_conv_same(x, w, b):
    """tf.nn.conv2d NHWC, stride 1, 'SAME', filter [kh,kw,cin,cout] + bias (direct loops)."""
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    xp = np.pad(x, ((0, 0), (ph, kh - 1 - ph), (pw, kw - 1 - pw), (0, 0)))
    out = np.zeros((B, H, W, Cout), np.float64)
    for i in range(kh):
        for j in range(kw):
            out += np.einsum("bhwc,co->bhwo", xp[:, i:i + H, j:j + W, :].astype(np.float64), w[i, j].astype(np.float64))
    return out + b


def tf_conv2d_transpose_same(x, w, s):
    """tf.nn.conv2d_transpose NHWC 'SAME', output = input * s, filter [k,k,cout,cin]: scatter form.
    out[b, s*h + i - p, s*w + j - p, o] += x[b,h,w,c] * f[i,j,o,c] with p = (k - s) / 2."""
    B, H, W, Cin = x.shape
    k = w.shape[0]
    Cout = w.shape[2]
    p = (k - s) // 2
    out = np.zeros((B, H * s, W * s, Cout), np.float64)
    for h in range(H):
        for ww in range(W):
            for i in range(k):
                for j in range(k):
                    oy, ox = s * h + i - p, s * ww + j - p
                    if 0 <= oy < H * s and 0 <= ox < W * s:
                        out[:, oy, ox, :] += x[:, h, ww, :].astype(np.float64) @ w[i, j].T.astype(np.float64)
    return out


def test_conv_matches_tf_definition():
    rng = np.random.default_rng(0)
    net = vgg16_convs_cpu("COLOR", 22, 64, (1.0,), 1.0, -1.0)
    x = rng.standard_normal((2, 6, 7, 5)).astype(F)
    w = rng.standard_normal((3, 3, 5, 4)).astype(F)
    b = rng.standard_normal(4).astype(F)
    net.load({"c": {"weights": w, "biases": b}})
    net.layers = {"data": torch.from_numpy(x)}
    y = net.feed("data").conv(3, 3, 4, 1, 1, name="c", c_i=5).get_output("c").numpy()
    assert np.allclose(y, np.maximum(tf_conv_same(x, w, b), 0), atol=1e-5)
    y2 = net.feed("data").conv(3, 3, 4, 1, 1, name="c", c_i=5, relu=False).layers["c"].numpy()
    assert np.allclose(y2, tf_conv_same(x, w, b), atol=1e-5)


@pytest.mark.parametrize("k,s", [(4, 2), (16, 8)])
def test_deconv_matches_dense_conv2d_transpose(k, s):
    rng = np.random.default_rng(1)
    C = 3
    net = vgg16_convs_cpu("COLOR", 22, 64, (1.0,), 1.0, -1.0)  # the deconv layer -> oracle restatement
    x = rng.standard_normal((1, 4, 5, C)).astype(F)
    net.layers = {"x": torch.from_numpy(x)}
    y = net.feed("x").deconv(k, k, C, s, s, name="up", trainable=False).get_output("up").numpy()
    f1 = make_deconv_filter_1d(k)
    dense = np.zeros((k, k, C, C))
    for i in range(C):
        dense[:, :, i, i] = np.outer(f1, f1)  # weights[:, :, i, i] = bilinear (network.py:151-153)
    want = tf_conv2d_transpose_same(x, dense, s)
    assert y.shape == (1, 4 * s, 5 * s, C)
    assert np.allclose(y, want, atol=1e-5)


def test_max_pool_and_fc_flatten_order():
    rng = np.random.default_rng(2)
    net = Tiny(device="cpu", trainable=False)
    x = rng.standard_normal((2, 4, 6, 3)).astype(F)
    net.layers = {"x": torch.from_numpy(x)}
    y = net.feed("x").max_pool(2, 2, 2, 2, name="p").get_output("p").numpy()
    assert np.array_equal(y, x.reshape(2, 2, 2, 3, 2, 3).max(axis=(2, 4)))
    w = rng.standard_normal((4 * 6 * 3, 5)).astype(F)
    b = rng.standard_normal(5).astype(F)
    net.load({"fc": {"weights": w, "biases": b}})
    y = net.feed("x").fc(5, height=4, width=6, channel=3, name="fc", relu=False).get_output("fc").numpy()
    assert np.allclose(y, x.reshape(2, -1) @ w + b, atol=1e-4)  # NHWC flatten (network.py:399-408)


def test_vgg16_convs_graph_runs_on_cpu_reference():
    H, W = 96, 128
    K = config.DEMO_INTRINSICS.copy(); K[:2] *= W / 640.0
    net = vgg16_convs_cpu("COLOR", 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True,
                          trainable=False, is_train=False, init="he", with_losses=True)
    synth.init_calibrated(net)
    rng = np.random.default_rng(3)
    data = (rng.integers(0, 256, (1, H, W, 3)).astype(F) - config.PIXEL_MEANS).astype(F)
    # objects at this resolution are < 500 px: the Hough layer returns its dummy row
    planted, scenes = synth.make_planted_batch(0, 1, H=H, W=W, K=K, n_obj=2)
    pts = synth.make_model_points(22, 64)
    out = run_cpu_pipeline(net, data, K, config.LOV_EXTENTS, pts, config.LOV_SYMMETRY, planted=planted)
    assert out["label_2d"].shape == (1, H, W) and out["vertex_pred"].shape == (1, H, W, 66)
    assert net.get_output("conv4_3").shape == (1, H // 8, W // 8, 512)
    assert net.get_output("gt_label_weight").shape == (1, H, W, 22)
    assert out["rois"].shape[1] == 7 and out["poses_tanh"].shape[1] == 88
    # planted labels come through the bilinear deconv + identity head
    lab_lr = scenes[0]["label_lowres"]
    centre = out["label_2d"][0, 4::8, 4::8]
    assert (centre == lab_lr).mean() > 0.95
    # RGBD variant: two towers concatenated for the label head only (vgg16_convs.py:99-126)
    net2 = vgg16_convs_cpu("RGBD", 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True,
                           trainable=False, is_train=False, init="he")
    feed = {"data": torch.from_numpy(data[:, :32, :32]), "data_p": torch.from_numpy(data[:, :32, :32]),
            "gt_label_2d": torch.ones((1, 32, 32), dtype=torch.int32), "keep_prob": 1.0, "poses": torch.zeros((1, 13)),
            "extents": torch.from_numpy(config.LOV_EXTENTS), "meta_data": torch.from_numpy(config.make_meta_data(K)).reshape(1, 1, 1, 48),
            "points": torch.from_numpy(pts), "symmetry": torch.from_numpy(config.LOV_SYMMETRY)}
    with torch.no_grad():
        net2.run(feed)
    assert net2.vars["score_conv5/weights"].shape == (64, 1024, 1, 1)
    assert net2.vars["score_conv5_vertex/weights"].shape == (128, 512, 1, 1)
    assert "conv5_3_p" in net2.layers and net2.get_output("concat_conv5").shape[-1] == 1024


def test_checkpoint_round_trip_npz_and_npy(tmp_path):
    """save_npz writes TF-named / TF-layout variables; load_file reads them back (and the vgg16.npy
    dict format, network.py:71-107) into a second network that then computes the same outputs."""
    rng = np.random.default_rng(7)
    a = vgg16_convs_cpu("COLOR", 22, 64, (1.0,), 1.0, -1.0)
    x = torch.from_numpy(rng.standard_normal((1, 6, 8, 3)).astype(F))
    a.layers = {"x": x}
    a.feed("x").conv(3, 3, 4, 1, 1, name="c1", c_i=3).fc(5, height=6, width=8, channel=4, name="f1", relu=False)
    path = str(tmp_path / "w.npz")
    a.save_npz(path)
    arch = np.load(path)
    assert arch["c1/weights"].shape == (3, 3, 3, 4) and arch["f1/weights"].shape == (6 * 8 * 4, 5)
    b = vgg16_convs_cpu("COLOR", 22, 64, (1.0,), 1.0, -1.0)
    assert b.load_file(path) == ["c1", "f1"]
    b.layers = {"x": x}
    b.feed("x").conv(3, 3, 4, 1, 1, name="c1", c_i=3).fc(5, height=6, width=8, channel=4, name="f1", relu=False)
    assert torch.equal(a.get_output("f1"), b.get_output("f1"))
    npy = str(tmp_path / "vgg.npy")
    np.save(npy, {"c1": {"weights": arch["c1/weights"], "biases": arch["c1/biases"]}}, allow_pickle=True)
    c = vgg16_convs_cpu("COLOR", 22, 64, (1.0,), 1.0, -1.0)
    assert c.load_file(npy) == ["c1"]
    c.layers = {"x": x}
    assert torch.equal(c.feed("x").conv(3, 3, 4, 1, 1, name="c1", c_i=3).get_output("c1"), a.get_output("c1"))


def test_deferred_bias_relu_is_fused_only_into_max_pool():
    """A conv listed in `defer_act` hands its raw output to the next layer: max_pool fuses bias + ReLU,
    every other consumer (and a fetch by name) sees the activated tensor."""
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.standard_normal((1, 6, 8, 5)).astype(F))
    w = rng.standard_normal((3, 3, 5, 4)).astype(F); b = rng.standard_normal(4).astype(F)
    outs = {}
    for defer in (False, True):
        net = vgg16_convs_cpu("COLOR", 22, 64, (1.0,), 1.0, -1.0)
        net.defer_act = frozenset(["c"]) if defer else frozenset()
        net.load({"c": {"weights": w, "biases": b}})
        net.layers = {"x": x}
        with torch.no_grad():
            net.feed("x").conv(3, 3, 4, 1, 1, name="c", c_i=5).max_pool(2, 2, 2, 2, name="p")
            pooled = net.get_output("p").clone()
            net.feed("x").conv(3, 3, 4, 1, 1, name="c", c_i=5).relu(name="r")
            outs[defer] = (pooled, net.get_output("r").clone(), net.get_output("c").clone())
    for a, b_ in zip(outs[False], outs[True]):
        assert torch.equal(a, b_)
    assert float(outs[True][2].min()) >= 0  # fetched by name: activated


def test_deferred_bias_relu_meets_every_kind_of_consumer():
    """The CPU twin of tests/test_gpu_pending_convs.py for the raw-output form: a conv in `defer_act` behind a 2x2/2 max_pool, a
    fetch and then that max_pool, a max_pool with stride 1, a plain layer and a following 1x1 conv gives the tensors of a
    network that defers nothing; only the first of them reaches the fused `_bias_relu_pool2`, and each activates at most once."""
    rng = np.random.default_rng(10)
    x = torch.from_numpy(rng.standard_normal((1, 6, 8, 5)).astype(F))
    data = {"c": {"weights": rng.standard_normal((3, 3, 5, 4)).astype(F), "biases": rng.standard_normal(4).astype(F)},
            "k": {"weights": rng.standard_normal((1, 1, 4, 4)).astype(F), "biases": rng.standard_normal(4).astype(F)}}

    class Counting(vgg16_convs_cpu):
        def _bias_act(self, y, bias, relu):
            self.calls.append("act")
            return vgg16_convs_cpu._bias_act(self, y, bias, relu)

        def _bias_relu_pool2(self, y, bias, relu):
            self.calls.append("pool2")
            return torch.nn.functional.max_pool2d(vgg16_convs_cpu._bias_act(self, y, bias, relu).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()

    consumers = {
        "pool": (lambda n: n.max_pool(2, 2, 2, 2, name="p"), ("p",), ["pool2"]),
        "fetch_pool": (lambda n: (n.get_output("c"), n.max_pool(2, 2, 2, 2, name="p")), ("c", "p"), ["act"]),
        "pool_stride1": (lambda n: n.max_pool(2, 2, 1, 1, name="p"), ("p",), ["act"]),
        "relu": (lambda n: n.relu(name="r"), ("r",), ["act"]),
        "conv1x1": (lambda n: n.conv(1, 1, 4, 1, 1, name="k"), ("k",), ["act", "act"]),
    }
    for tag, (consume, names, calls) in consumers.items():
        outs = {}
        for defer in (False, True):
            net = Counting("COLOR", 22, 64, (1.0,), 1.0, -1.0)
            net.defer_act = frozenset(["c"]) if defer else frozenset()
            net.load(data)
            net.layers, net.calls = {"x": x}, []
            with torch.no_grad():
                net.feed("x").conv(3, 3, 4, 1, 1, name="c", c_i=5)
                consume(net)
                outs[defer] = [net.get_output(n).clone() for n in names]
            if defer:
                assert net.calls == calls, (tag, net.calls)
        for a, b_ in zip(outs[False], outs[True]):
            assert torch.equal(a, b_), tag


def test_load_keeps_depth_tower_weights_and_drops_constant_deconv_filters():
    """(a) a checkpoint that carries '<layer>_p' entries loads each tower from its own
    entry whatever the dict order; vgg16.npy-style dicts (no '_p' keys) still initialise both towers;
    (b) the constant bilinear deconv filters of a checkpoint do not divert `deconv` to the dense path."""
    from posecnn_amd.networks import is_bilinear_deconv_filter
    rng = np.random.default_rng(4)
    wa = rng.standard_normal((3, 3, 3, 64)).astype(F); wb = rng.standard_normal((3, 3, 3, 64)).astype(F)
    ba = rng.standard_normal(64).astype(F); bb = rng.standard_normal(64).astype(F)

    def fresh():
        net = vgg16_convs_cpu("RGBD", 22, 64, (1.0,), 1.0, -1.0, trainable=False, is_train=False)
        for n in ("conv1_1", "conv1_1_p"):   # the variables exist once the graph has been built
            net.vars[n + "/weights"] = torch.zeros((64, 3, 3, 3)); net.vars[n + "/biases"] = torch.zeros(64)
        return net
    for order in (("conv1_1", "conv1_1_p"), ("conv1_1_p", "conv1_1")):
        d = {k: ({"weights": wa, "biases": ba} if k == "conv1_1" else {"weights": wb, "biases": bb}) for k in order}
        net = fresh(); net.load(d)
        assert torch.equal(net.vars["conv1_1/biases"], torch.from_numpy(ba)), order
        assert torch.equal(net.vars["conv1_1_p/biases"], torch.from_numpy(bb)), order
        assert torch.equal(net.vars["conv1_1_p/weights"], torch.from_numpy(wb).permute(3, 2, 0, 1)), order
    net = fresh(); net.load({"conv1_1": {"weights": wa, "biases": ba}})     # vgg16.npy: one entry feeds both towers
    assert torch.equal(net.vars["conv1_1_p/biases"], torch.from_numpy(ba))

    f16 = make_deconv_filter_1d(16)
    tf_filter = np.zeros((16, 16, 64, 64), np.float64)                       # [k, k, c_out, c_in], network.py:151-157
    for i in range(64):
        tf_filter[:, :, i, i] = np.outer(f16, f16)
    tf_filter = tf_filter.astype(F)
    assert is_bilinear_deconv_filter(torch.from_numpy(tf_filter).permute(3, 2, 0, 1))
    assert not is_bilinear_deconv_filter(torch.from_numpy(wa).permute(3, 2, 0, 1))
    net = fresh(); assert net.fused_heads
    net.load({"upscore": {"weights": tf_filter}})
    assert "upscore/weights" not in net.vars and net.fused_heads           # same kernels as an unloaded network
    trained = tf_filter.copy(); trained[3, 3, 0, 1] = 0.01                   # somebody fine-tuned the filter
    net.load({"upscore": {"weights": trained}})
    assert "upscore/weights" in net.vars and not net.fused_heads           # literal op order, dense conv_transpose


# the variables of a lazily initialised network in creation order, as lib/networks/vgg16_convs.py:79-193 creates them
COLOR_TOWER_VARS = [
    "conv1_1/weights", "conv1_1/biases", "conv1_2/weights", "conv1_2/biases",
    "conv2_1/weights", "conv2_1/biases", "conv2_2/weights", "conv2_2/biases",
    "conv3_1/weights", "conv3_1/biases", "conv3_2/weights", "conv3_2/biases",
    "conv3_3/weights", "conv3_3/biases", "conv4_1/weights", "conv4_1/biases",
    "conv4_2/weights", "conv4_2/biases", "conv4_3/weights", "conv4_3/biases",
    "conv5_1/weights", "conv5_1/biases", "conv5_2/weights", "conv5_2/biases",
    "conv5_3/weights", "conv5_3/biases",
]
DEPTH_TOWER_VARS = [
    "conv1_1_p/weights", "conv1_1_p/biases", "conv1_2_p/weights", "conv1_2_p/biases",
    "conv2_1_p/weights", "conv2_1_p/biases", "conv2_2_p/weights", "conv2_2_p/biases",
    "conv3_1_p/weights", "conv3_1_p/biases", "conv3_2_p/weights", "conv3_2_p/biases",
    "conv3_3_p/weights", "conv3_3_p/biases", "conv4_1_p/weights", "conv4_1_p/biases",
    "conv4_2_p/weights", "conv4_2_p/biases", "conv4_3_p/weights", "conv4_3_p/biases",
    "conv5_1_p/weights", "conv5_1_p/biases", "conv5_2_p/weights", "conv5_2_p/biases",
    "conv5_3_p/weights", "conv5_3_p/biases",
]
HEAD_VARS = [
    "score_conv5/weights", "score_conv5/biases", "score_conv4/weights", "score_conv4/biases",
    "score/weights", "score/biases", "score_conv5_vertex/weights", "score_conv5_vertex/biases",
    "score_conv4_vertex/weights", "score_conv4_vertex/biases", "vertex_pred/weights", "vertex_pred/biases",
    "fc6/weights", "fc6/biases", "fc7/weights", "fc7/biases",
    "fc8/weights", "fc8/biases",
]
VARS_IN_ORDER = {"COLOR": COLOR_TOWER_VARS + HEAD_VARS, "RGBD": COLOR_TOWER_VARS + DEPTH_TOWER_VARS + HEAD_VARS}


@pytest.mark.parametrize("fmt", ["COLOR", "RGBD"])
def test_lazily_created_variables_come_in_the_reference_order(fmt):
    """The seeded generator makes creation order part of the behaviour: a lazily initialised network creates its variables
    in the order of lib/networks/vgg16_convs.py:79-193 — the colour tower, the depth tower (RGBD), score_conv5, score_conv4,
    score, the vertex head, fc6-8 (the constant deconv filters are no variables here) — weights before biases in every
    layer (network.py:169-185,409-411)."""
    net = vgg16_convs_cpu(fmt, 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=False, is_train=False)
    K = config.DEMO_INTRINSICS.copy()
    data = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 16, 16, 3)).astype(F))
    feed = {"data": data, "gt_label_2d": torch.ones((1, 16, 16), dtype=torch.int32), "keep_prob": 1.0, "poses": torch.zeros((1, 13)),
            "extents": torch.from_numpy(config.LOV_EXTENTS), "meta_data": torch.from_numpy(config.make_meta_data(K)).reshape(1, 1, 1, 48)}
    if fmt == "RGBD":
        feed["data_p"] = data.clone()
    with torch.no_grad():
        net.run(feed)
    assert list(net.vars) == VARS_IN_ORDER[fmt]


# (rows, dim, num_out, padded_width) -> route, for a CUDA input with a device-side row count and no autograd. The skinny
# kernel takes 1..32 rows of a 2-D input whose width is a multiple of 16; the row kernel takes dim % 64 == 0, dim >= 128 and
# num_out % 64 == 0 — num_out % 4 == 0 when the caller pads the filter (fc_tanh).
FC_ROUTES = {
    (None, 112, 64, False): "addmm", (None, 112, 64, True): "addmm", (None, 112, 88, False): "addmm", (None, 112, 88, True): "addmm",
    (None, 128, 64, False): "rows", (None, 128, 64, True): "rows", (None, 128, 88, False): "addmm", (None, 128, 88, True): "rows",
    (None, 4096, 64, False): "rows", (None, 4096, 64, True): "rows", (None, 4096, 88, False): "addmm", (None, 4096, 88, True): "rows",
    (1, 112, 64, False): "skinny", (1, 112, 64, True): "skinny", (1, 112, 88, False): "skinny", (1, 112, 88, True): "skinny",
    (1, 128, 64, False): "skinny", (1, 128, 64, True): "skinny", (1, 128, 88, False): "skinny", (1, 128, 88, True): "skinny",
    (1, 4096, 64, False): "skinny", (1, 4096, 64, True): "skinny", (1, 4096, 88, False): "skinny", (1, 4096, 88, True): "skinny",
    (32, 112, 64, False): "skinny", (32, 112, 64, True): "skinny", (32, 112, 88, False): "skinny", (32, 112, 88, True): "skinny",
    (32, 128, 64, False): "skinny", (32, 128, 64, True): "skinny", (32, 128, 88, False): "skinny", (32, 128, 88, True): "skinny",
    (32, 4096, 64, False): "skinny", (32, 4096, 64, True): "skinny", (32, 4096, 88, False): "skinny", (32, 4096, 88, True): "skinny",
    (33, 112, 64, False): "addmm", (33, 112, 64, True): "addmm", (33, 112, 88, False): "addmm", (33, 112, 88, True): "addmm",
    (33, 128, 64, False): "rows", (33, 128, 64, True): "rows", (33, 128, 88, False): "addmm", (33, 128, 88, True): "rows",
    (33, 4096, 64, False): "rows", (33, 4096, 64, True): "rows", (33, 4096, 88, False): "addmm", (33, 4096, 88, True): "rows",
}


def test_fc_route_table():
    """`Network._fc_route` is the one routing predicate of `fc`, `fc_tanh` and `fc_masks_dead_rows`: written out as a table."""
    net = Tiny(device="cpu", trainable=False)
    assert len(FC_ROUTES) == 4 * 3 * 2 * 2
    for (rows, dim, num_out, padded), want in FC_ROUTES.items():
        got = net._fc_route(True, rows, dim, num_out, False, True, padded_width=padded)
        assert got == want, (rows, dim, num_out, padded, got)
    # the three causes that send everything to the framework, whatever the shapes
    for padded in (False, True):
        assert net._fc_route(False, 8, 128, 64, False, True, padded_width=padded) == "addmm"    # a CPU tensor
        assert net._fc_route(True, 8, 128, 64, True, True, padded_width=padded) == "addmm"     # recorded for autograd
        assert net._fc_route(True, 8, 128, 64, False, False, padded_width=padded) == "addmm"    # no device-side row count
    net.fc_skinny = False   # the switch: few rows go where many rows go
    assert net._fc_route(True, 8, 128, 64, False, True) == "rows" and net._fc_route(True, 8, 112, 64, False, True) == "addmm"


def test_derived_cache_validity():
    """`Network._derived` — the one place that decides whether a tensor derived from variables is still good: a hit on a
    repeat; a rebuild after an in-place update, after the variable is replaced by another object (even one with equal
    values), and when `extra` changes; and the entry keeps its sources alive, so their addresses cannot be reused under it."""
    import gc
    import weakref
    net = Tiny(device="cpu", trainable=False)
    w, b = torch.arange(6.0).reshape(2, 3), torch.ones(3)
    builds = []

    def build_from(*src):
        def build():
            builds.append(len(builds))
            return src[0].t() + src[1].reshape(-1, 1) if len(src) > 1 else src[0].t().contiguous()
        return build

    first = net._derived("slot", (w, b), build_from(w, b), 4)
    assert builds == [0] and torch.equal(first, w.t() + b.reshape(-1, 1))
    assert net._derived("slot", (w, b), build_from(w, b), 4) is first and builds == [0]              # a repeat: hit
    assert net._derived("other", (w,), build_from(w)) is not first and builds == [0, 1]              # slots are independent
    assert net._derived("slot", (w, b), build_from(w, b), 4) is first and len(builds) == 2
    b.mul_(2.0)                                                                                      # in place: same object, new version
    second = net._derived("slot", (w, b), build_from(w, b), 4)
    assert len(builds) == 3 and torch.equal(second, w.t() + b.reshape(-1, 1)) and not torch.equal(second, first)
    assert net._derived("slot", (w, b), build_from(w, b), 4) is second and len(builds) == 3
    w2 = w.clone()                                                                                   # another object, equal values, version 0 again
    third = net._derived("slot", (w2, b), build_from(w2, b), 4)
    assert len(builds) == 4 and third is not second
    assert net._derived("slot", (w2, b), build_from(w2, b), 4) is third and len(builds) == 4
    fourth = net._derived("slot", (w2, b), build_from(w2, b), 2)                                     # `extra` changed
    assert len(builds) == 5 and fourth is not third
    assert net._derived("slot", (w2, b), build_from(w2, b), 2) is fourth and len(builds) == 5
    assert net._derived("slot", (w2,), build_from(w2), 2) is not fourth and len(builds) == 6         # fewer sources is another entry
    # the entry pins its sources: dropping every outside reference does not free them
    v = torch.full((4,), 3.0)
    ref = weakref.ref(v)
    net._derived("pinned", (v,), lambda: None)
    del v
    gc.collect()
    assert ref() is not None
    net._derived("pinned", (w,), lambda: None)   # replaced entry: the old source goes
    gc.collect()
    assert ref() is None
    # ... and so do the entries of the variables that load() replaces
    net.vars = {"fc/weights": torch.ones((3, 2)), "fc/biases": torch.zeros(2), "other/biases": torch.zeros(1)}
    ref = weakref.ref(net.vars["fc/weights"])
    net._derived("loaded", (net.vars["fc/weights"], net.vars["fc/biases"]), lambda: None)
    kept = net._derived("kept", (net.vars["other/biases"],), lambda: torch.zeros(1))
    net.load({"fc": {"weights": np.ones((3, 2), F)}})
    gc.collect()
    assert ref() is None and net._derived("kept", (net.vars["other/biases"],), lambda: None) is kept
