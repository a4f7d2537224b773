"""The routes `posecnn_amd/networks.py` and `fcn.im_segment_batch` choose between, as a table, and a float64 restatement of
the `vgg16_convs` inference graph to hold each of them against. TEST INFRASTRUCTURE ONLY: nothing here needs a GPU.

  make_vars / make_frames / make_planted   seeded variables (TF names, the network's layouts), sensor frames, planted scene
  reference                                the graph up to `vertex_pred` as plain tensor algebra in a given dtype; reads
                                           nothing of networks.py but the variables
  References                               ref64, ref32 and e32[layer] = max|ref32 - ref64| per (variables, input), cached
  TABLE / Case                             one row per route: constructor arguments, instance flags, input, shapes, the
                                           launches per kernel that `_lib.profile_report()` must show (0: must not appear), the partner route
                                           whose bits it must carry (class E) and the claim that says so
  M                                        the class T margins per route family, from the first GPU run (tests/ROUTES.md)
  kernel_calls / route_errors              profile report -> {kernel: calls}; what a report has against a row
  route_flags / instance_for               the flags the two `__init__` bodies assign and a predicate reads; a bare instance
  pose_tail_cpu                            Hough -> roi_pool x 2 -> add -> fc6-8 -> tanh on the oracle-based CPU network

tests/test_network_routes_cpu.py asserts what can be asserted here; tests/test_gpu_network_routes.py runs the routes;
tests/ROUTES.md records what the GPU run showed."""
import ast
import collections
import os

import numpy as np
import torch
import torch.nn.functional as F

from posecnn_amd import config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

TRUNK_KEEP = ("conv4_3", "pool4", "conv5_3")
HEAD_LAYERS = ("score_conv5", "score_conv4", "score_conv5_vertex", "score_conv4_vertex", "add_score", "add_score_vertex",
               "score", "prob_normalized", "vertex_pred")
# class T margins: max|route - ref64| <= M[family] * e32[layer]. Trunk layers (conv4_3, pool4, conv5_3 [+ _p]) take the row's
# trunk family, every layer behind them "1x1", the quaternion columns of the pose path "fc". Each is twice the largest ratio
# the first GPU run measured in that family, rounded up (tests/ROUTES.md has the ratios); 16 is the ceiling the audit allows.
M = {"direct": 3, "F(2,3)": 3, "F(4,3)": 10, "1x1": 11, "fc": 6}
LABEL_CAP = 0.01     # share of pixels per case whose float64 top-2 margin is too small to pin the argmax


# ---- variables, frames, planted scene -------------------------------------------------------------------------------------
def make_vars(fmt, C, U, with_fc=False, seed=11):
    """The calibrated synthetic network of synth.init_calibrated (He x the frozen per-layer gains, zero biases, identity
    `score` / `vertex_pred` filters on the channels they have in common with their inputs), on the host, from one generator:
    the trunk is the same for every C and U of a format, and leaving the fc layers out (they come last) changes nothing else."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = collections.OrderedDict()
    for name, shape, fan_in, kind in synth.calibrated_layers(fmt, C, U):
        if kind == "fc" and not with_fc:
            continue
        w = torch.randn(shape, generator=g) * (float(np.sqrt(2.0 / fan_in)) * float(synth.CALIBRATED_GAINS.get(name, 1.0)))
        v[name + "/weights"] = w.contiguous(memory_format=torch.channels_last) if kind == "conv" else w
        v[name + "/biases"] = torch.zeros((shape[0] if kind == "conv" else shape[1],))
    for name, co, ci in (("score", C, U), ("vertex_pred", 3 * C, 128)):
        w = torch.zeros((co, ci, 1, 1))
        for c in range(min(co, ci)):
            w[c, c, 0, 0] = 1.0
        v[name + "/weights"] = w.contiguous(memory_format=torch.channels_last)
        v[name + "/biases"] = torch.zeros((co,))
    # biases that are not zero: a swapped or dropped bias row has to move something (seeded apart from the weights)
    gb = torch.Generator(device="cpu").manual_seed(seed + 1)
    for k in v:
        if k.endswith("/biases"):
            v[k] = (torch.randn(v[k].shape, generator=gb) * 0.05).contiguous()
    return v


def make_frames(B, H, W, seed):
    """Sensor frames: uint8 BGR [B,H,W,3] and uint16 depth [B,H,W] below 3000 (what the gains were calibrated on)."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8), rng.integers(0, 3000, (B, H, W)).astype(np.uint16)


def blobs_of(color, depth):
    """lib/fcn/test.py:56-74 in numpy, as fcn._get_image_blob has it: float32 frames minus the pixel means."""
    c = color.astype(np.float32)
    c -= config.PIXEL_MEANS
    d = depth.astype(np.float32)
    d = np.clip(d / 2000.0, 0, 1) * 255
    d = np.tile(d[..., np.newaxis], (1, 1, 1, 3))
    d -= config.PIXEL_MEANS
    return np.ascontiguousarray(c, dtype=F32), np.ascontiguousarray(d, dtype=F32)


def intrinsics(W):
    K = config.DEMO_INTRINSICS.copy()
    K[:2] *= W / 640.0
    return K


def make_planted(B, H, W, C, U, seed=7, n_obj=2):
    planted, scenes = synth.make_planted_batch(seed, B, H=H, W=W, K=intrinsics(W), C=C, num_units=U, n_obj=n_obj)
    return planted, scenes


# ---- the reference ----------------------------------------------------------------------------------------------------
def _conv3x3(x, w, b):
    """3x3 'SAME' as nine shifted products: x [B,H,W,Ci], w [Co,Ci,3,3] -> relu(. + b)."""
    B, H, W, Ci = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    acc = None
    for ky in range(3):
        for kx in range(3):
            t = xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Ci) @ w[:, :, ky, kx].t()
            acc = t if acc is None else acc + t
    return torch.relu(acc + b).view(B, H, W, w.shape[0])


def _pool2(x):
    B, H, W, C = x.shape
    return x.view(B, H // 2, 2, W // 2, 2, C).amax(dim=(2, 4))


def deconv_matrix(k, s, n, dtype):
    """conv2d_transpose 'SAME' along one axis with make_deconv_filter's taps (network.py:141-150): [n s, n]."""
    f = int(np.ceil(k / 2.0))
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    tap = [1 - abs(x / float(f) - c) for x in range(k)]
    pad = (k - s) // 2
    m = torch.zeros((n * s, n), dtype=dtype)
    for o in range(n * s):
        for i in range(n):
            t = o + pad - s * i
            if 0 <= t < k:
                m[o, i] = tap[t]
    return m


def _deconv(x, k, s):
    B, h, w, C = x.shape
    my, mx = deconv_matrix(k, s, h, x.dtype), deconv_matrix(k, s, w, x.dtype)
    return torch.einsum("oh,bhwc->bowc", my, torch.einsum("pw,bhwc->bhpc", mx, x))


def _conv1x1(x, w, b, relu):
    y = x.reshape(-1, x.shape[-1]) @ w.reshape(w.shape[0], -1).t() + b
    y = y.view(*x.shape[:3], w.shape[0])
    return torch.relu(y) if relu else y


VGG = (("conv1_1", None), ("conv1_2", "pool1"), ("conv2_1", None), ("conv2_2", "pool2"), ("conv3_1", None), ("conv3_2", None),
       ("conv3_3", "pool3"), ("conv4_1", None), ("conv4_2", None), ("conv4_3", "pool4"), ("conv5_1", None), ("conv5_2", None),
       ("conv5_3", None))


def reference_trunk(variables, blobs, dtype):
    """One tower per blob ('' then '_p'): {conv4_3, pool4, conv5_3 [+ '_p']} in `dtype`."""
    out = {}
    for sfx, blob in zip(("", "_p"), blobs):
        x = torch.as_tensor(blob).to(dtype)
        for name, pool in VGG:
            x = _conv3x3(x, variables[name + sfx + "/weights"].detach().cpu().to(dtype),
                         variables[name + sfx + "/biases"].detach().cpu().to(dtype))
            if name in TRUNK_KEEP:
                out[name + sfx] = x
            if pool is not None:
                x = _pool2(x)
                if pool in TRUNK_KEEP:
                    out[pool + sfx] = x
    return out


def reference_heads(variables, trunk, planted, dtype):
    """vgg16_convs.py:99-163 behind the towers, in the reference's literal order."""
    V = lambda n: variables[n].detach().cpu().to(dtype)
    towers = ("", "_p") if "conv5_3_p" in trunk else ("",)
    out = dict(trunk)
    cat = lambda n: torch.cat([trunk[n + t] for t in towers], dim=3)
    out["score_conv5"] = _conv1x1(cat("conv5_3"), V("score_conv5/weights"), V("score_conv5/biases"), True)
    out["score_conv4"] = _conv1x1(cat("conv4_3"), V("score_conv4/weights"), V("score_conv4/biases"), True)
    out["score_conv5_vertex"] = _conv1x1(trunk["conv5_3"], V("score_conv5_vertex/weights"), V("score_conv5_vertex/biases"), False)
    out["score_conv4_vertex"] = _conv1x1(trunk["conv4_3"], V("score_conv4_vertex/weights"), V("score_conv4_vertex/biases"), False)
    for sfx, key in (("", "add_score"), ("_vertex", "add_score_vertex")):
        a = out["score_conv4" + sfx] + _deconv(out["score_conv5" + sfx], 4, 2)
        if planted is not None and key in planted:
            a = a + torch.as_tensor(planted[key]).to(dtype)
        out[key] = a
    out["score"] = _conv1x1(_deconv(out["add_score"], 16, 8), V("score/weights"), V("score/biases"), True)
    out["vertex_pred"] = _conv1x1(_deconv(out["add_score_vertex"], 16, 8), V("vertex_pred/weights"), V("vertex_pred/biases"), False)
    out["prob_normalized"] = torch.softmax(out["score"], dim=3)
    out["label_2d"] = torch.argmax(out["score"], dim=3).to(torch.int32)    # first maximum
    top2 = torch.topk(out["score"], 2, dim=3).values
    out["margin"] = top2[..., 0] - top2[..., 1]
    return out


def reference(variables, blobs, planted, dtype):
    return reference_heads(variables, reference_trunk(variables, blobs, dtype), planted, dtype)


class References(object):
    """ref64 / ref32 / e32 per (trunk variables, frames) and per (head variables, planted): computed once, shared, left
    unchanged. Keys are the caller's names for the variable sets and inputs."""

    def __init__(self):
        self._trunk, self._full = {}, {}

    def get(self, vars_key, trunk_key, variables, input_key, blobs, planted_key, planted):
        key = (vars_key, input_key, planted_key)
        if key not in self._full:
            refs = []
            for dtype in (torch.float64, torch.float32):
                tk = (trunk_key, input_key, dtype)
                if tk not in self._trunk:
                    self._trunk[tk] = reference_trunk(variables, blobs, dtype)
                refs.append(reference_heads(variables, self._trunk[tk], planted, dtype))
            r64, r32 = refs
            e32 = {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64 if k not in ("label_2d", "margin")}
            self._full[key] = (r64, r32, e32)
        return self._full[key]


def family_of_layer(layer, trunk_family):
    base = layer[:-2] if layer.endswith("_p") else layer
    return trunk_family if base in TRUNK_KEEP else "1x1"


def label_check(label, r64, e32):
    """3d: (pixels that count, of those how many differ from the float64 argmax, share of pixels left out)."""
    thr = 2.0 * M["1x1"] * e32["score"]
    counted = r64["margin"] > thr
    lab = torch.as_tensor(label).to(torch.int32).cpu()
    wrong = int(((lab != r64["label_2d"]) & counted).sum())
    return int(counted.sum()), wrong, 1.0 - float(counted.double().mean())


# ---- the table ------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name fmt raw B H W C U ctor flags planted grad present family partner e_layers claim expect note")

ALL_WINO = ("wino43_input_kernel", "wino43_mfma_kernel", "wino43_output_kernel", "wino_input_kernel", "wino_output_kernel",
            "conv3x3_c3_wino43_kernel", "conv12_wino43_fused_kernel")
LIBRARY_TRUNK = ALL_WINO + ("conv3x3_c3_bias_relu_kernel", "bias_act_kernel", "bias_relu_pool2_kernel")
LABEL_EPILOGUE = ("upscore_softmax_argmax_fixed_kernel", "upscore_softmax_argmax_kernel")   # either: compile-time C or generic
ALL = "all"      # class E over every layer the two routes both register
HEAD_E = ("conv4_3", "pool4", "conv5_3", "score_conv5", "score_conv4", "score_conv5_vertex", "score_conv4_vertex",
          "add_score", "add_score_vertex")

CLAIMS = {
    "grouped": "networks.py `_trunk_grouped` docstring: 'Identical arithmetic to running the towers one after the other'; "
               "test_gpu_round3.py::test_grouped_trunk_does_not_depend_on_fused_pool",
    "merged": "networks.py `_merged_head_convs` docstring: 'the same kernel, the same bits per column'; "
              "test_gpu_round5.py::test_merged_head_convs_equal_the_separate_products",
    "conv12": "ops.py `conv1_1_conv1_2_fused` docstring: 'Bit-identical to conv3x3_c3_winograd43 + winograd43_conv(pool=1)'; "
              "test_gpu_round4.py::test_conv1_1_conv1_2_fused_equals_the_unfused_pair",
    "first": "ops.py `conv3x3_c3_winograd43` docstring: 'winograd_input(conv3x3_c3(x, ...), tile=4) in one kernel'",
    "raw": "ops.py `conv3x3_c3_winograd43_raw` docstring: 'the blobs ... are formed inside the kernel, bit for bit'; "
           "test_gpu_round3.py::test_network_on_raw_frames_equals_network_on_blobs",
    "small": "ops.py `head_lowres_mfma` docstring: 'the same add (bit-identical `add`)'; test_gpu_round5.py::"
             "test_head_lowres_mfma_equals_the_op_sequence_it_replaces, test_gpu_round3.py::test_head_lowres_equals_the_op_sequence_it_replaces",
    "dual": "networks.py `_trunk_grouped` comment 'the kernel writes both (mode 2) whatever `dual_pool` / `fused_pool` say'; "
            "test_gpu_round3.py::test_grouped_trunk_does_not_depend_on_fused_pool",
    "same-graph": "the same kernels on the same tensors: only an output is added or dropped",
    "pool2": "ops.py `roi_pool_add2`; test_gpu_ops.py::test_roi_pool_add2_equals_two_pools",
}


def _case(name, fmt="COLOR", raw=False, B=1, H=32, W=48, C=22, U=64, ctor=None, flags=None, planted=True, grad=False,
          present=(), family="F(4,3)", partner=None, e_layers=(), claim=None, expect=None, note=""):
    return Case(name, fmt, raw, B, H, W, C, U, dict(ctor or {}), dict(flags or {}), planted, grad, dict(present), family, partner,
                e_layers, claim, dict(expect or {}), note)


def _trunk(conv12=1, c3w=0, c3=0, inp=11, mfma=11):
    """Call counts of the default F(4,3) MFMA trunk and its variants (0 = must not appear)."""
    return {"conv12_wino43_fused_kernel": conv12, "conv3x3_c3_wino43_kernel": c3w, "conv3x3_c3_bias_relu_kernel": c3,
            "wino43_input_kernel": inp, "wino43_mfma_kernel": mfma, "wino43_output_kernel": 0, "wino_input_kernel": 0,
            "wino_output_kernel": 0, "bias_relu_pool2_kernel": 0}


def _heads(rows=2, mfma=2, small=0, deconv=1, literal=False):
    """Head kernels: 1x1 row products, the two small-head kernels, bilinear deconv launches (the fetched vertex_pred is one)."""
    d = {"fc_rows_mfma_kernel": rows, "head_lowres_mfma_kernel": mfma, "head_lowres_kernel": small, "deconv_bilinear_kernel": deconv}
    if literal:
        d.update({"softmax_argmax_kernel": 1, LABEL_EPILOGUE: 0})
    else:
        d.update({"softmax_argmax_kernel": 0, LABEL_EPILOGUE: 1})
    return d


def _both(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


DEFAULT = _both(_trunk(), _heads())
h, w = 32 // 8, 48 // 8

TABLE = [
    # ---- trunk ----------------------------------------------------------------------------------------------------------
    _case("color_default", present=DEFAULT, expect={"conv12": True, "mfma_label": True, "mfma_vertex": True}),
    _case("color_default_b2", B=2, present=DEFAULT),
    _case("color_raw_u8", raw=True, present=DEFAULT, partner="color_default", e_layers=ALL, claim="raw"),
    _case("color_conv12_off", flags={"fused_conv12": False}, present=_both(_trunk(conv12=0, c3w=1, mfma=12), _heads()),
          partner="color_default", e_layers=ALL, claim="conv12", expect={"conv12": False}),
    _case("color_first_into_wino_off", flags={"fuse_first_conv_into_winograd": False},
          present=_both(_trunk(conv12=0, c3=1, inp=12, mfma=12), _heads()), partner="color_conv12_off", e_layers=ALL, claim="first"),
    _case("color_first_conv_off", flags={"fused_first_conv": False},
          present=_both(_trunk(conv12=0, inp=12, mfma=12), _heads(), {"bias_act_kernel": 1}),
          note="conv1_1 is the framework's convolution + bias_act_kernel: not stated in library kernel names beyond that"),
    _case("color_wino_bmm", flags={"winograd_mfma": False},
          present=_both(_trunk(conv12=0, c3w=1, mfma=0), _heads(), {"wino43_output_kernel": 12}), expect={"conv12": False},
          note="all three pool modes: conv1_2 / 2_2 / 3_3 pooled in the output transform, conv4_3 both tensors, the rest plain. The "
               "profile drops template arguments, so the mode is not in the kernel name: the partner row below, which pools in the "
               "framework, has to carry the same bits instead"),
    _case("color_wino_bmm_pool_off", ctor={"fused_pool": False}, flags={"winograd_mfma": False},
          present=_both(_trunk(conv12=0, c3w=1, mfma=0), _heads(), {"wino43_output_kernel": 12}),
          partner="color_wino_bmm", e_layers=ALL, claim="dual"),
    _case("color_f23", flags={"winograd_tile": 2, "winograd_min_channels": 128}, family="F(2,3)",
          present=_both(_trunk(conv12=0, c3=1, inp=0, mfma=0), _heads(),
                        {"wino_input_kernel": 7, "wino_output_kernel": 7, "bias_relu_pool2_kernel": 1,
                         "bias_act_kernel": 4}),
          note="conv1_2 / conv2_1 have 64 < 128 input channels and conv5_x is 2 x 3 (odd width): the framework's convolution there"),
    _case("color_strict", ctor={"strict_numerics": True}, family="direct",
          present=_both(_trunk(conv12=0, c3=1, inp=0, mfma=0), _heads(), {"bias_relu_pool2_kernel": 3, "bias_act_kernel": 9})),
    _case("color_pool_off", ctor={"fused_pool": False}, present=_both(_trunk(conv12=0, c3w=1, mfma=12), _heads()),
          partner="color_default", e_layers=ALL, claim="dual",
          note="without `defer_act` nothing is deferred to a max_pool, so conv1_2 cannot be the lazy one-kernel form either"),
    _case("rgbd_grouped", fmt="RGBD", present=_both(_trunk(), _heads(rows=6)), expect={"conv12": True}),
    _case("rgbd_grouped_b2", fmt="RGBD", B=2, present=_both(_trunk(), _heads(rows=6))),
    _case("rgbd_chained", fmt="RGBD", flags={"grouped_towers": False}, present=_both(_trunk(conv12=2, inp=22, mfma=22), _heads(rows=6)),
          partner="rgbd_grouped", e_layers=ALL, claim="grouped"),
    _case("rgbd_grouped_raw", fmt="RGBD", raw=True, present=_both(_trunk(), _heads(rows=6)), partner="rgbd_grouped", e_layers=ALL, claim="raw"),
    _case("rgbd_chained_raw", fmt="RGBD", raw=True, flags={"grouped_towers": False},
          present=_both(_trunk(conv12=2, inp=22, mfma=22), _heads(rows=6)), partner="rgbd_grouped", e_layers=ALL, claim="raw"),
    _case("rgbd_grouped_conv12_off", fmt="RGBD", flags={"fused_conv12": False}, present=_both(_trunk(conv12=0, c3w=1, mfma=12), _heads(rows=6)),
          partner="rgbd_grouped", e_layers=ALL, claim="conv12"),
    _case("color_trainable_grad", ctor={"trainable": True, "is_train": True, "with_losses": False}, grad=True, family="direct",
          present=_both({k: 0 for k in LIBRARY_TRUNK}, {"fc_rows_mfma_kernel": 0, "head_lowres_mfma_kernel": 0, "head_lowres_kernel": 0,
                                                        LABEL_EPILOGUE: 0, "softmax_argmax_kernel": 1}),
          note="autograd records the graph: every dense layer is the framework's; the deconvs are the differentiable library op"),
    # ---- heads ----------------------------------------------------------------------------------------------------------
    _case("color_merge_off", flags={"merge_head_convs": False}, present=_both(_trunk(), _heads(rows=4)),
          partner="color_default", e_layers=ALL, claim="merged"),
    _case("color_head_gemm_off", flags={"head_gemm": False}, present=_both(_trunk(), _heads(rows=0))),
    _case("color_mfma_heads_off", flags={"mfma_heads": False}, present=_both(_trunk(), _heads(mfma=0, small=2)),
          partner="color_default", e_layers=HEAD_E, claim="small", expect={"mfma_label": False, "mfma_vertex": False}),
    _case("color_small_heads_off", flags={"small_heads": False}, present=_both(_trunk(), _heads(mfma=0, small=0, deconv=3)),
          partner="color_default", e_layers=HEAD_E, claim="small"),
    _case("color_small_at_max_pixels", flags={"mfma_heads": False, "small_heads_max_pixels": 1 * h * w},
          present=_both(_trunk(), _heads(mfma=0, small=2)), partner="color_default", e_layers=HEAD_E, claim="small"),
    _case("color_small_past_max_pixels", flags={"mfma_heads": False, "small_heads_max_pixels": 1 * h * w - 1},
          present=_both(_trunk(), _heads(mfma=0, small=0, deconv=3)), partner="color_default", e_layers=HEAD_E, claim="small"),
    _case("color_small_at_max_pixels_b2", B=2, flags={"mfma_heads": False, "small_heads_max_pixels": 2 * h * w},
          present=_both(_trunk(), _heads(mfma=0, small=2)), partner="color_default_b2", e_layers=HEAD_E, claim="small"),
    _case("color_small_past_max_pixels_b2", B=2, flags={"mfma_heads": False, "small_heads_max_pixels": 2 * h * w - 1},
          present=_both(_trunk(), _heads(mfma=0, small=0, deconv=3)), partner="color_default_b2", e_layers=HEAD_E, claim="small"),
    _case("color_c32", C=32, present=DEFAULT, expect={"mfma_label": True, "mfma_vertex": True}),
    _case("color_c33", C=33, present=_both(_trunk(), _heads(mfma=1, small=0, deconv=2)), expect={"mfma_label": True, "mfma_vertex": False},
          note="3 C = 99 > 96 and 4 (32 x 128 + 128 x 99) > 60 KB: the vertex head fits neither small-head kernel"),
    _case("color_u32", U=32, present=_both(_trunk(), _heads(rows=2, mfma=2)), expect={"mfma_label": True},
          note="`_head_conv1x1` falls back to the framework for the 32-wide score convs; the two vertex convs keep the row kernel"),
    _case("color_u40", U=40, present=_both(_trunk(), _heads(rows=2, mfma=1, small=1)), expect={"mfma_label": False, "mfma_vertex": True}),
    _case("color_literal", ctor={"fused_heads": False}, present=_both(_trunk(), _heads(mfma=0, small=0, deconv=4, literal=True)),
          partner="color_default", e_layers=HEAD_E, claim="small"),
    _case("color_with_losses", ctor={"with_losses": True}, present=_both(DEFAULT, {"hard_label_fwd_kernel": 0}),
          partner="color_default", e_layers=ALL, claim="same-graph"),
    _case("color_no_prob", ctor={"want_prob": False}, present=DEFAULT, partner="color_default", e_layers=ALL, claim="same-graph"),
    _case("color_unplanted", planted=False, present=DEFAULT),
    _case("color_unplanted_small", planted=False, flags={"mfma_heads": False}, present=_both(_trunk(), _heads(mfma=0, small=2)),
          partner="color_unplanted", e_layers=HEAD_E, claim="small"),
    _case("color_unplanted_small_off", planted=False, flags={"small_heads": False}, present=_both(_trunk(), _heads(mfma=0, small=0, deconv=3)),
          partner="color_unplanted", e_layers=HEAD_E, claim="small"),
    _case("rgbd_head_gemm_off", fmt="RGBD", flags={"head_gemm": False}, present=_both(_trunk(), _heads(rows=0))),
]
del h, w

# the lazily initialised COLOR network: first run (the head variables do not exist: four products), second run (two)
LAZY_FIRST = _both(_trunk(), _heads(rows=4))
LAZY_SECOND = _both(_trunk(), _heads(rows=2))

# ---- pose path: 96 x 128, two planted objects, C = 22 -----------------------------------------------------------------------
PoseCase = collections.namedtuple("PoseCase", "name fmt B ctor flags driver kwargs present expect note")
POSE_H, POSE_W, POSE_C = 96, 128, 22
_POSE_COMMON = {"roi_pool_add2_rows": 1, "det_assemble_kernel": 1, "roi_pool_fwd_staged": 0}
POSE_TABLE = [
    PoseCase("pose_b1_skinny", "COLOR", 1, {}, {}, "batch", {},
             _both(_POSE_COMMON, {"fc_skinny_kernel": 3, "pose_l2_normalize_kernel": 0}),
             {"capacity": 21, "fc6": "skinny", "fc8": "skinny", "masks": True}, "21 capacity rows: fc6-8 on the weight-streaming kernel"),
    PoseCase("pose_b2_rows", "COLOR", 2, {}, {}, "batch", {},
             _both(_POSE_COMMON, {"fc_skinny_kernel": 0, "fc_rows_mfma_kernel": 2 + 3}),
             {"capacity": 42, "fc6": "rows", "fc8": "rows", "masks": True}, "42 rows: fc_rows for fc6 / fc7, fc_rows_cols for fc8 (+ 2 merged head products)"),
    PoseCase("pose_b1_skinny_off", "COLOR", 1, {}, {"fc_skinny": False}, "batch", {},
             _both(_POSE_COMMON, {"fc_skinny_kernel": 0, "fc_rows_mfma_kernel": 2 + 3}),
             {"capacity": 21, "fc6": "rows", "fc8": "rows", "masks": True}, ""),
    PoseCase("pose_b2_train_losses", "COLOR", 2, {"is_train": True, "with_losses": False}, {}, "batch", {"with_losses": True, "gt": True},
             _both(_POSE_COMMON, {"fc_skinny_kernel": 0, "pose_l2_normalize_kernel": 1, "hard_label_fwd_kernel": 0}),
             {"capacity": 378, "fc6": "rows", "fc8": "rows", "masks": True}, "row stride 9; both loss layers on the capacity-sized rows"),
    PoseCase("pose_b2_frame_offset", "COLOR", 2, {}, {}, "batch", {"frame_offset": 6},
             _both(_POSE_COMMON, {"fc_skinny_kernel": 0}), {"capacity": 42}, "the packed all-gather block out of the same launch"),
    PoseCase("pose_b1_dsl", "COLOR", 1, {}, {}, "dsl", {},
             {"roi_pool_add2_rows": 0, "roi_pool_fwd_staged": 2, "det_assemble_kernel": 0, "fc_skinny_kernel": 0},
             {}, "net.run with pose_reg: two roi_pool + add, addmm fc6-8 (no device-side row count)"),
]


# ---- profile reports against a row --------------------------------------------------------------------------------------
def kernel_calls(report):
    """{kernel name without template arguments: calls}."""
    out = collections.Counter()
    for k, v in report.items():
        out[k.split("<")[0].strip("() ")] += int(v["calls"])
    return dict(out)


def route_errors(calls, present):
    """What a report has against a row's expectation {kernel | (alternatives): calls, 0 = must not appear}."""
    bad = []
    for k, n in present.items():
        got = sum(calls.get(a, 0) for a in k) if isinstance(k, tuple) else calls.get(k, 0)
        if got != n:
            bad.append("%s: %d launches, the row says %d" % (k, got, n))
    return bad


# ---- flags and predicates ------------------------------------------------------------------------------------------------
NOT_ROUTES = {
    "inputs": "DSL state", "layers": "DSL state", "vars": "the variables themselves (the lazy cases cover their absence)",
    "_cache": "derived-tensor cache (test_gpu_derived_cache.py)", "rows_count": "set by fcn.im_segment_batch around fc6-8: the pose rows",
    "planted": "an argument of run(): the `planted` column of the table", "conv_timing": "a timing aid of bench.py, no arithmetic",
    "init": "which initialiser creates a variable, not where a tensor goes", "reference_trunk": "validation aid (tests/parity_study.py)",
    "keep_prob_queue": "fed per run; < 1 is random dropout, which no reference can follow",
    "lowres_train_heads": "training graph (test_gpu_label_loss.py, test_gpu_gradients.py)",
    "fused_vertex_loss": "training graph (test_gpu_vertex_head.py)", "adaptation": "registers one more output of the Hough layer",
    "vertex_reg_3d": "only ever read or-ed with vertex_reg_2d", "vertex_reg": "true in every PoseCNN configuration: the vertex head is the network",
    "vote_threshold": "an argument of the Hough kernel (test_gpu_hough.py), > 0 only changes the row capacity",
    "fuse_hard_label": "set by fcn.im_segment_batch(with_losses=True): the pose rows with losses",
    "device": "the CPU checker", "_gen": "the initialiser's generator", "scale": "1.0 in every configuration (SCALES_BASE)",
    "skip_pixels": "an argument of the Hough kernel", "vote_percentage": "an argument of the Hough kernel",
    "threshold_label": "an argument of the hard-label kernels (test_gpu_round5.py)",
    "with_losses": None, "trainable": None,     # (None: a route flag after all — listed to say they were looked at)
}


def _init_assignments(cls_name, tree):
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == cls_name:
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef) and fn.name == "__init__":
                    names = set()
                    for n in ast.walk(fn):
                        if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Store) and isinstance(n.value, ast.Name) and n.value.id == "self":
                            names.add(n.attr)
                    return names
    raise AssertionError("no %s.__init__" % cls_name)


def route_flags():
    """Attributes the two `__init__` bodies assign that networks.py or fcn.py read anywhere (as `self.x` / `net.x`: a predicate
    may take them as an argument or through a local), minus NOT_ROUTES."""
    path = os.path.join(ROOT, "posecnn_amd")
    trees = [ast.parse(open(os.path.join(path, f)).read()) for f in ("networks.py", "fcn.py")]
    assigned = _init_assignments("Network", trees[0]) | _init_assignments("vgg16_convs", trees[0])
    read = set()
    for tree in trees:
        for n in ast.walk(tree):
            if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Load) and isinstance(n.value, ast.Name) and n.value.id in ("self", "net"):
                read.add(n.attr)
    return sorted(a for a in assigned & read if NOT_ROUTES.get(a, None) is None), sorted(assigned), sorted(read)


def ctor_args(fmt, C, U, ctor, device):
    kw = dict(vertex_reg_2d=False, vertex_reg_3d=True, pose_reg=False, trainable=False, is_train=False, seed=3, init="he",
              with_losses=False, device=device)
    kw.update(ctor)
    return (fmt, C, U, (1.0,), 1.0, -1.0), kw


def instance_for(case, device="cuda"):
    """A bare network with the row's constructor arguments and flags; creates no tensor on `device`."""
    from posecnn_amd.networks import vgg16_convs
    a, kw = ctor_args(case.fmt, getattr(case, "C", POSE_C), getattr(case, "U", 64), case.ctor, device)
    if isinstance(case, PoseCase):
        kw.update(vertex_reg_2d=True, vertex_reg_3d=False, pose_reg=True)
        kw.update(case.ctor)
    net = vgg16_convs(*a, **kw)
    for k, v in case.flags.items():
        assert hasattr(net, k), k
        setattr(net, k, v)
    return net


# ---- the pose tail on the CPU checker ------------------------------------------------------------------------------------
def pose_tail_cpu(cpu, layers, is_train, rois_per_image, dtype=torch.float32):
    """vgg16_convs.py:165-193 on the oracle-based CPU network from the GPU route's own label_2d / vertex_pred / conv4_3 /
    conv5_3: Hough -> two roi_pool -> add -> fc6 -> fc7 -> fc8 -> tanh. The three fc layers in `dtype` (float64 and float32
    give the yardstick of the quaternion columns)."""
    import oracle
    n = lambda t: np.ascontiguousarray(torch.as_tensor(t).detach().cpu().numpy())
    gt = None if layers.get("poses") is None else n(layers["poses"])
    out = oracle.hough_voting(n(layers["label_2d"]), n(layers["vertex_pred"]), n(layers["extents"]), n(layers["meta_data"]), gt,
                              int(is_train), cpu.vote_threshold, cpu.vote_percentage, cpu.skip_pixels, rois_per_image=rois_per_image, padded=True)
    rows = int(out[5][1])      # the true number of detection rows (num_rois[0] is at least 1)
    rois, poses_init, target, weight = (np.ascontiguousarray(o[:rows]) for o in out[:4])
    p5, _ = oracle.roi_pool(n(layers["conv5_3"]), rois, 7, 7, 1.0 / 16.0, 0)
    p4, _ = oracle.roi_pool(n(layers["conv4_3"]), rois, 7, 7, 1.0 / 8.0, 0)
    pool = torch.from_numpy(p5) + torch.from_numpy(p4)
    res = {"n": rows, "rois": rois, "poses_init": poses_init, "poses_target": target, "poses_weight": weight, "pool_score": pool.numpy()}
    for dt in (torch.float64, torch.float32) if dtype is None else (dtype,):
        V = lambda k: cpu.vars[k].detach().cpu().to(dt)
        x = pool.reshape(pool.shape[0], -1).to(dt)
        x = torch.relu(x @ V("fc6/weights") + V("fc6/biases"))
        x = torch.relu(x @ V("fc7/weights") + V("fc7/biases"))
        x = x @ V("fc8/weights") + V("fc8/biases")
        res["poses_tanh", dt] = torch.tanh(x)
    return res


# ---- a row's inputs and references -----------------------------------------------------------------------------------------
@__import__("functools").lru_cache(maxsize=None)
def frames_for(B, H, W):
    color, depth = make_frames(B, H, W, seed=100 + B)
    return color, depth, blobs_of(color, depth)


@__import__("functools").lru_cache(maxsize=None)
def planted_for(B, H, W, C, U):
    return make_planted(B, H, W, C, U)


@__import__("functools").lru_cache(maxsize=None)
def vars_for(fmt, C, U, with_fc=False):
    return make_vars(fmt, C, U, with_fc)


REFS = References()


def case_reference(case, variables=None, vars_key=None):
    """(ref64, ref32, e32) of a row (TABLE or POSE_TABLE), on the calibrated variables unless others are handed in."""
    C, U = getattr(case, "C", POSE_C), getattr(case, "U", 64)
    H, W = getattr(case, "H", POSE_H), getattr(case, "W", POSE_W)
    color, depth, (bc, bd) = frames_for(case.B, H, W)
    blobs = [bc, bd] if case.fmt == "RGBD" else [bc]
    planted = planted_for(case.B, H, W, C, U)[0] if getattr(case, "planted", True) else None
    if variables is None:
        fc = isinstance(case, PoseCase)     # (the trunk, created first, is the same with and without the fc layers)
        variables, vars_key, trunk_key = vars_for(case.fmt, C, U, fc), (case.fmt, C, U, fc), case.fmt
    else:
        trunk_key = vars_key
    return REFS.get(vars_key, trunk_key, variables, (case.B, H, W), blobs, None if planted is None else (C, U), planted)
