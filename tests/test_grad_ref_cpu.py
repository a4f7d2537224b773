"""Keeps tests/grad_ref.py honest, without a GPU.

  * forward: `training_loss64` against the project's own CPU graph (cpu_reference.vgg16_convs_cpu in training mode +
    train.build_losses) — the only place on the CPU where the restatement meets the project's code; a restatement that
    computes another function fails here;
  * torch.autograd.gradcheck of the four op restatements at tiny float64 shapes, inputs away from their kinks;
  * the comparator's self-test: five seeded defects of the kind the old finite-and-non-zero test let through must each be
    turned down by the comparison tests/test_gpu_gradients.py applies, for a named variable;
  * the float32 floor of that comparison: the same restatement in float32 against float64, per variable, under its cap.
"""
import time

import numpy as np
import pytest
import torch

import cpu_reference
import grad_ref
import oracle
from posecnn_amd import synth, train

F = np.float32


def _tensor_feed(feed_np, keys):
    return {k: (torch.from_numpy(np.ascontiguousarray(feed_np[k])) if isinstance(feed_np[k], np.ndarray) else feed_np[k]) for k in keys}


@pytest.fixture(scope="module")
def graph():
    """The CPU graph in training mode at the shape of the GPU test, its losses, the constants it computes without a
    gradient, and the float64 / float32 gradients of the restatement on the same variables."""
    feed_np = grad_ref.dense_vertex_feed(grad_ref.graph_feed())
    net = cpu_reference.vgg16_convs_cpu("COLOR", grad_ref.NUM_CLASSES, grad_ref.NUM_UNITS, (1.0,), 1.0, -1.0, vertex_reg_2d=True,
                                        pose_reg=True, trainable=True, is_train=True, seed=3, init="he")
    synth.init_calibrated(net)
    feed = _tensor_feed(feed_np, ("data", "gt_label_2d", "keep_prob", "vertex_targets", "vertex_weights", "poses", "extents",
                                  "meta_data", "points", "symmetry"))
    planted = {k: torch.from_numpy(v) for k, v in feed_np["planted"].items()}
    # train.build_losses reaches the vertex loss through the GPU-only op: on the CPU graph the C oracle stands in for it
    # (bit-identical to the kernel, tests/test_gpu_training.py), so VERTEX_W / POSE_W and the sum are build_losses' own
    real = train.smooth_l1_loss_vertex
    train.smooth_l1_loss_vertex = lambda p, t, w, sigma=1.0: torch.tensor(
        oracle.smooth_l1_vertex(p.numpy(), t.numpy(), w.numpy(), sigma, want_grad=False)[0][0])
    try:
        with torch.no_grad():
            net.run(feed, planted=planted)
            losses = {k: float(v) for k, v in train.build_losses(net).items()}
    finally:
        train.smooth_l1_loss_vertex = real
    consts = {k: net.get_output(k).numpy() for k in ("rois", "poses_target", "poses_weight", "gt_label_weight")}
    out = {"feed": feed_np, "net": net, "losses": losses, "consts": consts}
    t0 = time.time()
    out["g64"], out["l64"] = grad_ref.grads_of(grad_ref.vars_from_net(net.vars, torch.float64, True), feed_np, consts, train.TrainConfig)
    out["seconds64"] = time.time() - t0
    out["g32"], out["l32"] = grad_ref.grads_of(grad_ref.vars_from_net(net.vars, torch.float32, True), feed_np, consts, train.TrainConfig)
    out["floor"] = {k: grad_ref.rel_err(out["g32"][k], out["g64"][k]) for k in out["g64"]}
    return out


def test_the_workload_is_not_vacuous(graph):
    """What tests/test_gpu_gradients.py asserts of its run holds for the CPU graph too: two ROI rows with a pose target
    per image, a symmetric class among them, kept and dropped background pixels, three positive loss terms."""
    c, feed = graph["consts"], graph["feed"]
    live = (c["poses_weight"] != 0).any(axis=1)
    for n in range(grad_ref.GRAPH_SHAPE[0]):
        assert int((live & (c["rois"][:, 0] == n)).sum()) >= 2
    classes = {int(np.flatnonzero(r.reshape(-1, 4)[:, 0] > 0)[0]) for r in c["poses_weight"][live]}
    assert any(feed["symmetry"][k] > 0 for k in classes), classes
    bg = c["gt_label_weight"][feed["gt_label_2d"] == 0][:, 0]
    assert 0 < bg.sum() < bg.size
    assert min(graph["losses"][k] for k in ("loss_cls", "loss_vertex", "loss_pose")) > 0


# measured float32-vs-float64 forward error of the three terms on this workload (relative): the CPU graph's float32
# value against the restatement's float64 one
FORWARD_MEASURED = {"loss_cls": 3.4e-8, "loss_vertex": 9.2e-8, "loss_pose": 9.4e-7}


def test_forward_equals_the_cpu_graph(graph, capsys):
    """loss_cls, loss_vertex, loss_pose of `training_loss64` against train.build_losses on the layers of the float32 CPU
    graph, same variables, same feed, `consts` taken from that graph. Bound: 8 x the float32-vs-float64 forward error
    measured here (FORWARD_MEASURED, relative: loss_cls 3.4e-8, loss_vertex 9.2e-8, loss_pose 9.4e-7 — float32 rounding of
    sums over 24 576 pixels x 22 classes, over 66 vertex channels, and over 54 rows x 64 points of a loss of 1e-3), i.e.
    2.7e-7 / 7.4e-7 / 7.5e-6. A wrong head order, a missing ReLU, a wrong ROI scale or a wrong normaliser moves a term by
    percents. The float64 pass of the whole graph at 2 x 96 x 128 is the longest step: 2.6 s on 8 CPU threads."""
    rel = {k: abs(graph["losses"][k] - graph["l64"][k]) / abs(graph["l64"][k]) for k in FORWARD_MEASURED}
    with capsys.disabled():
        print("\nforward, CPU float32 graph vs float64 restatement (relative):", {k: "%.2e" % v for k, v in rel.items()},
              "float64 pass: %.1f s" % graph["seconds64"])
    for k, measured in FORWARD_MEASURED.items():
        assert rel[k] <= 8 * measured, (k, rel[k], graph["losses"][k], graph["l64"][k])
    assert abs(graph["losses"]["loss_regu"] - graph["l64"]["loss_regu"]) <= 1e-6 * graph["l64"]["loss_regu"]


def test_float32_floor_is_under_its_cap(graph, capsys):
    """floor[v] = ||g32 - g64|| / ||g64|| of the restatement itself must not exceed 1e-3 for any variable: a larger one
    means a pool / ReLU / hinge decision flipped between the precisions on this seed — change the seed or the input
    scale (grad_ref.GRAPH_SEED), never the cap. Measured on this seed: at most 5.2e-6 (fc8/weights)."""
    floor = graph["floor"]
    with capsys.disabled():
        print("\nfloat32 floor per variable: max %.2e (%s)" % max((v, k) for k, v in floor.items()))
    assert len(floor) == 44          # 13 trunk + 6 head + 3 fc layers, weights and biases
    for k, v in floor.items():
        assert v <= grad_ref.FLOOR_CAP, (k, v)
        assert float(graph["g64"][k].norm()) > 0, k


class _Sigma3(train.TrainConfig):
    VERTEX_SIGMA = 3.0


# mutation -> the variable that must be turned down
MUTANT_VARIABLE = {"vertex_w_doubled": "vertex_pred/weights", "pose_w_zero": "fc8/weights",
                   "vertex_conv4_detached": "score_conv4_vertex/weights", "roi_pool8_detached": "conv4_3/weights",
                   "sl1_sigma2_once_less": "vertex_pred/weights"}


@pytest.mark.parametrize("mutation", grad_ref.MUTATIONS)
def test_the_comparison_rejects_seeded_defects(graph, mutation, capsys):
    """The float64 gradient recomputed with one defect must fail `err[v] <= 16 max(floor[v], 2^-20)` against the clean
    float64 gradient for the named variable. sigma^2 is 1 in the graph under test, where a dropped factor sigma^2 is
    invisible (and harmless); that mutation is run at sigma = 3, baseline and mutant, to show that the metric sees the
    class of error (the kernels themselves are held to sigma = 3 in tests/test_gpu_gradients.py)."""
    cfg = _Sigma3 if mutation == "sl1_sigma2_once_less" else train.TrainConfig
    v64 = grad_ref.vars_from_net(graph["net"].vars, torch.float64, True)
    base = graph["g64"] if cfg is train.TrainConfig else grad_ref.grads_of(v64, graph["feed"], graph["consts"], cfg)[0]
    mutant, _ = grad_ref.grads_of(v64, graph["feed"], graph["consts"], cfg, mutate=mutation)
    bad = grad_ref.rejected(mutant, base, graph["floor"])
    with capsys.disabled():
        print("\n%s: %d variables rejected, %s" % (mutation, len(bad), {k: "%.1e > %.1e" % bad[k] for k in sorted(bad)[:4]}))
    assert MUTANT_VARIABLE[mutation] in bad, (mutation, sorted(bad))
    assert not grad_ref.rejected(base, base, graph["floor"])


# ---- gradcheck of the op restatements -------------------------------------------------------------------------------
def _r(seed):
    return np.random.default_rng(seed)


@pytest.mark.parametrize("k,s", [(4, 2), (16, 8)])
def test_gradcheck_deconv(k, s):
    rng = _r(1)
    x = torch.from_numpy(rng.standard_normal((1, 3, 2, 2))).requires_grad_(True)
    a1 = torch.from_numpy(rng.standard_normal((1, 3 * s, 2 * s, 2))).requires_grad_(True)
    a2 = torch.from_numpy(rng.standard_normal((1, 3 * s, 2 * s, 2))).requires_grad_(True)
    b = torch.from_numpy(rng.standard_normal(2)).requires_grad_(True)
    y = grad_ref.deconv_bilinear64(x, k, s, a1, a2, b, False)
    assert float(y.detach().abs().min()) > 1e-4                       # no output on the ReLU's kink
    assert torch.autograd.gradcheck(lambda *a: grad_ref.deconv_bilinear64(a[0], k, s, a[1], a[2], a[3], True), (x, a1, a2, b))
    assert torch.autograd.gradcheck(lambda a: grad_ref.deconv_bilinear64(a, k, s), (x,))


@pytest.mark.parametrize("sigma", [1.0, 3.0])
def test_gradcheck_smooth_l1(sigma):
    rng = _r(2)
    n = 60
    w = torch.from_numpy(rng.choice([0.0, 0.5, 1.0, 2.0, 4.0], n))
    t = torch.from_numpy(rng.standard_normal(n))
    p = (t + torch.from_numpy(rng.standard_normal(n)) * (0.6 / sigma ** 2)).requires_grad_(True)
    d = (w * (p - t)).abs().detach()
    assert float((d - 1.0 / sigma ** 2).abs().min()) > 1e-4 and float(d[w > 0].min()) > 1e-4      # away from both kinks
    assert ((d < 1.0 / sigma ** 2) & (w > 0)).any() and (d > 1.0 / sigma ** 2).any()                # both branches
    assert torch.autograd.gradcheck(lambda a: grad_ref.smooth_l1_vertex64(a, t, w, sigma), (p,))


def test_gradcheck_roi_pool():
    rng = _r(3)
    data = torch.from_numpy(rng.permutation(2 * 6 * 7 * 3).reshape(2, 6, 7, 3).astype(np.float64)).requires_grad_(True)   # no ties
    rois = np.array([[0, 1, 2, 3, 20, 17], [1, 2, -6, -4, 30, 40], [1, 0, 9, 9, 3, 3], [5, 0, 0, 0, 9, 9], [0, 0, 40, 2, 60, 9]], F)
    top = grad_ref.roi_pool64(data, rois, 3, 2, 0.25)
    assert top.shape == (5, 3, 2, 3) and not top[3].any() and not top[4].any()       # bad batch index, ROI off the map
    assert torch.autograd.gradcheck(lambda a: grad_ref.roi_pool64(a, rois, 3, 2, 0.25), (data,))


@pytest.mark.parametrize("margin", [0.0, 0.01])
def test_gradcheck_average_distance(margin):
    rng = _r(4)
    C, P, R = 4, 9, 5
    pts = torch.from_numpy(rng.uniform(-0.2, 0.2, (C, P, 3)))
    sym = torch.tensor([0.0, 0.0, 1.0, 0.0])
    pred = torch.zeros((R, 4 * C), dtype=torch.float64)
    tgt = torch.zeros((R, 4 * C), dtype=torch.float64)
    wgt = torch.zeros((R, 4 * C), dtype=torch.float64)
    for n, c in enumerate((1, 2, None, 3, 2)):                 # plain, symmetric, a row without a class, ...
        if c is None:
            continue
        pred[n, 4 * c:4 * c + 4] = torch.from_numpy(np.tanh(rng.standard_normal(4)))
        tgt[n, 4 * c:4 * c + 4] = torch.from_numpy(synth.random_unit_quats(rng, 1)[0].astype(np.float64))
        wgt[n, 4 * c:4 * c + 4] = 1
    pred.requires_grad_(True)
    dist = torch.cat([t[1] for t in grad_ref.average_distance_terms(pred, tgt, wgt, pts, sym) if t is not None]).detach()
    assert float((dist - margin).abs().min()) > 1e-5          # no point on the hinge
    assert torch.autograd.gradcheck(lambda a: grad_ref.average_distance64(a, tgt, wgt, pts, sym, margin), (pred,))
    assert torch.autograd.gradcheck(lambda a: grad_ref.average_distance64(a, tgt, wgt, pts, sym, margin, num_rows=3), (pred,))
