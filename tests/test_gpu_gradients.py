"""Gradients on the GPU against float64 autograd of a plain restatement of the FORWARD (tests/grad_ref.py).

The forwards are pinned elsewhere (C oracle bit for bit, dense kernels against float64). The hand-written backward
kernels were so far only compared with oracle/pcnn_oracle.c's transliteration of the reference's backward code — the
same reading of it the kernels were written from — and the training graph only had to produce finite, non-zero
gradients. Here the question is the other one: is each backward the derivative of its forward, and does
`vgg16_convs(is_train=True)` + `train.build_losses` route every one of them to the right variable with the right weight.

  whole graph   every trainable variable's gradient of one step (no optimiser step) against the float64 gradient of
                grad_ref.training_loss64: err[v] <= 16 max(floor[v], 2^-20), floor[v] the float32 error of the same
                restatement, measured in the same test; with dense vertex targets and with the target-free vertex feed
  deconv        ops.deconv_bilinear_grad and the autograd route, bit for bit on integer upstream gradients; the
                add1 / add2 / bias gradients of the fallback route with ReLU
  smooth L1     both entries, weights in {0, 0.5, 1, 2, 4}, sigma in {1, 3}, elements planted on and next to the branch
                point and on p == t, sum(w) == 0; <= 4 ulp per element
  ROI pooling   tie-free integer data, wide / malformed ROIs, a ROI list longer than the backward's LDS list; bit for bit
  average dist. `bottom_diff` against the derivative of the loss it is returned with

`backproject` is left to its oracle test: its backward is a pixel -> voxel copy in the reference, not the adjoint of
its averaging forward, and the op is not part of this training graph.
"""
import time

import numpy as np
import pytest

import exact
import grad_ref
import np_ref
import vertex_ref
from posecnn_amd import synth
from test_gpu_ops import adl_case, random_rois

pytestmark = pytest.mark.gpu
F = np.float32


def T(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def t64(a, grad=False):
    import torch
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float64)).requires_grad_(grad)


# ---- whole graph ----------------------------------------------------------------------------------------------------
def _graph_step(gpu, target_free):
    """One forward + backward of the trainable graph on the GPU (no optimiser step), then the float64 and float32
    gradients of the restatement on the same variables with the constants of that run."""
    import torch
    from posecnn_amd import train
    from posecnn_amd.networks import vgg16_convs
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    feed_np = grad_ref.dense_vertex_feed(grad_ref.graph_feed())
    net = vgg16_convs("COLOR", grad_ref.NUM_CLASSES, grad_ref.NUM_UNITS, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True,
                      trainable=True, is_train=True, device=gpu, seed=3, init="he")
    synth.init_calibrated(net)      # He x frozen per-layer gains + identity score heads: O(1) activations, the planted scene reaches the Hough layer
    keys = ["data", "gt_label_2d", "poses", "extents", "meta_data", "points", "symmetry"]
    keys += ["vertex_objects"] if target_free else ["vertex_targets", "vertex_weights"]
    feed = {k: T(gpu, feed_np[k]) for k in keys}
    feed["keep_prob"] = 1.0
    planted = {k: T(gpu, v) for k, v in feed_np["planted"].items()}
    with torch.enable_grad():
        net.run(feed, planted=planted)
        losses = train.build_losses(net)
        assert ("vertex_targets" in net.layers) != target_free
        data_loss = losses["loss_cls"] + losses["loss_vertex"] + losses["loss_pose"]
        # the data terms alone for the two variables with structural zeros (the regulariser's gradient is dense)
        sparse = dict(zip(("fc8/weights", "vertex_pred/weights"),
                          torch.autograd.grad(data_loss, [net.vars["fc8/weights"], net.vars["vertex_pred/weights"]], retain_graph=True)))
        losses["loss"].backward()
    torch.cuda.synchronize()
    assert not net.fused_heads and not any(k.startswith("upscore") for k in net.vars)     # the fixed filters are no variables: no gradient
    trainable = sorted(k for k, v in net.vars.items() if v.requires_grad)
    assert trainable == sorted(net.vars) and len(trainable) == 44
    consts = {k: net.get_output(k).detach().cpu().numpy() for k in ("rois", "poses_target", "poses_weight", "gt_label_weight")}
    out = {"feed": feed_np, "consts": consts, "losses": {k: float(v.detach()) for k, v in losses.items()},
           "g": {k: net.vars[k].grad.detach().cpu() for k in trainable}, "sparse": {k: v.detach().cpu() for k, v in sparse.items()},
           "w": {k: net.vars[k].detach().cpu() for k in trainable}}
    t0 = time.time()
    out["g64"], out["l64"] = grad_ref.grads_of(grad_ref.vars_from_net(net.vars, torch.float64), feed_np, consts, train.TrainConfig)
    out["seconds64"] = time.time() - t0
    out["g32"], out["l32"] = grad_ref.grads_of(grad_ref.vars_from_net(net.vars, torch.float32), feed_np, consts, train.TrainConfig)
    out["weight_reg"] = train.TrainConfig.WEIGHT_REG
    return out


def _check_graph(r, capsys, title):
    import torch
    feed, c = r["feed"], r["consts"]
    B = grad_ref.GRAPH_SHAPE[0]
    # --- the run is not vacuous
    live = (c["poses_weight"] != 0).any(axis=1)
    for n in range(B):
        assert int((live & (c["rois"][:, 0] == n)).sum()) >= 2, "image %d has no two ROI rows with a pose target" % n
    roi_classes = sorted({int(np.flatnonzero(row.reshape(-1, 4)[:, 0] > 0)[0]) for row in c["poses_weight"][live]})
    assert any(feed["symmetry"][k] > 0 for k in roi_classes), roi_classes
    assert min(r["losses"][k] for k in ("loss_cls", "loss_vertex", "loss_pose")) > 0, r["losses"]
    bg = c["gt_label_weight"][feed["gt_label_2d"] == 0][:, 0]
    assert 0 < bg.sum() < bg.size, "gt_label_weight keeps %d of %d background pixels" % (bg.sum(), bg.size)
    # --- every variable, every loss term
    floor = {k: grad_ref.rel_err(r["g32"][k], r["g64"][k]) for k in r["g64"]}
    err = {k: grad_ref.rel_err(r["g"][k], r["g64"][k]) for k in r["g64"]}
    lfloor = {k: abs(r["l32"][k] - r["l64"][k]) / abs(r["l64"][k]) for k in r["l64"]}
    lerr = {k: abs(r["losses"][k] - r["l64"][k]) / abs(r["l64"][k]) for k in r["l64"]}
    with capsys.disabled():
        print("\n%s (float64 reference pass: %.1f s)" % (title, r["seconds64"]))
        print("%-28s %10s %10s %10s" % ("variable", "err", "floor", "bound"))
        for k in sorted(err):
            print("%-28s %10.2e %10.2e %10.2e" % (k, err[k], floor[k], grad_ref.bound(floor[k])))
        for k in sorted(lerr):
            print("%-28s %10.2e %10.2e %10.2e   (%.9g)" % (k, lerr[k], lfloor[k], grad_ref.bound(lfloor[k]), r["losses"][k]))
    assert sorted(err) == sorted(r["g"])
    for k in sorted(floor):
        assert floor[k] <= grad_ref.FLOOR_CAP, (k, floor[k])
    bad = {k: (err[k], grad_ref.bound(floor[k])) for k in err if not err[k] <= grad_ref.bound(floor[k])}
    assert not bad, bad
    for k in lerr:
        assert lerr[k] <= grad_ref.bound(lfloor[k]), (k, r["losses"][k], r["l64"][k])
    # --- structural zeros: fc8 columns of classes without a ROI, vertex_pred rows of classes absent from the labels.
    # The float64 gradient there is the regulariser's alone; the GPU's data gradient there is +-0, exactly.
    C = grad_ref.NUM_CLASSES
    fc8_dead = np.array([k for k in range(C) if k not in roi_classes])
    cols = (4 * fc8_dead[:, None] + np.arange(4)).ravel()
    present = set(np.unique(feed["gt_label_2d"]).tolist())
    vp_dead = np.array([k for k in range(C) if k == 0 or k not in present])
    rows = (3 * vp_dead[:, None] + np.arange(3)).ravel()
    assert 0 < len(fc8_dead) < C and 0 < len(vp_dead) < C
    reg = r["weight_reg"]
    w8, wv = r["w"]["fc8/weights"].double(), r["w"]["vertex_pred/weights"].double()
    assert float((r["g64"]["fc8/weights"][:, cols] - reg * w8[:, cols]).abs().max()) <= 1e-15 * float(w8.abs().max())
    assert float((r["g64"]["vertex_pred/weights"][rows] - reg * wv[rows]).abs().max()) <= 1e-15
    assert not r["sparse"]["fc8/weights"][:, cols].any(), "fc8 columns of classes without a ROI receive a data gradient"
    assert not r["sparse"]["vertex_pred/weights"][rows].any(), "vertex_pred rows of absent classes receive a data gradient"
    assert not r["g"]["fc8/biases"][cols].any() and not r["g"]["vertex_pred/biases"][rows].any()      # (biases are zero: no regulariser term)
    # (a class WITH a ROI may still get none: every point of a small or symmetric model can lie under the 0.01 margin)
    live_cols = (4 * np.array(roi_classes)[:, None] + np.arange(4)).ravel()
    assert int((r["sparse"]["fc8/weights"][:, live_cols].abs().sum(dim=0) > 0).sum()) >= 8


def test_training_graph_gradients_equal_float64(gpu, capsys):
    """vgg16_convs(is_train=True) + train.build_losses + loss.backward() at 2 x 96 x 128, dense vertex targets. The
    measured table of the MI355X run is in DESIGN.md ("Gradient parity")."""
    _check_graph(_graph_step(gpu, target_free=False), capsys, "training graph, dense vertex targets")


def test_training_graph_gradients_equal_float64_target_free_vertex_feed(gpu, capsys):
    """The same with `vertex_objects` in place of vertex_targets / vertex_weights (ops.smooth_l1_loss_vertex_gt); the
    reference is unchanged: the dense loss on the targets of the numpy restatement."""
    _check_graph(_graph_step(gpu, target_free=True), capsys, "training graph, target-free vertex feed")


# ---- deconv backward ------------------------------------------------------------------------------------------------
def _deconv_gmax(k, s):
    """Largest integer |g| <= exact.DECONV_X for which the BACKWARD is exact: an input element collects k x k taps whose
    absolute sum is s^2 (4 for k = 4, 64 for k = 16) in units of 1/16 resp. 1/256, so s^2 |g| units must stay below 2^24.
    The forward's bound (four taps per output) allows 4096 for both; the backward of k = 16 allows 512."""
    units = 16 if k == 4 else 256
    gmax = exact.DECONV_X
    while s * s * gmax * units >= exact.LIMIT:
        gmax //= 2
    return gmax


@pytest.mark.parametrize("k,s", exact.DECONV_KS)
@pytest.mark.parametrize("shape", exact.DECONV_SHAPES)
def test_deconv_backward_equals_float64(gpu, shape, k, s):
    import torch
    from posecnn_amd import ops
    B, H, W, C = shape
    gmax = _deconv_gmax(k, s)
    g = exact.ints(exact.seed_of("deconv_bwd", shape, k), (B, H * s, W * s, C), -gmax, gmax)
    x64 = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    y64 = grad_ref.deconv_bilinear64(x64, k, s)
    (ref,) = torch.autograd.grad(y64, x64, g.double(), retain_graph=True)
    (bound,) = torch.autograd.grad(y64, x64, g.double().abs())
    assert float(bound.max()) * (16 if k == 4 else 256) < exact.LIMIT, "input not exact"
    exact.check(ops.deconv_bilinear_grad(g.to(gpu), k, s), ref, {"name": "deconv_bilinear_grad"})
    x = torch.zeros(shape, device=gpu, requires_grad=True)
    ops.deconv_bilinear(x, k, s).backward(g.to(gpu))
    exact.check(x.grad, ref, {"name": "deconv_bilinear autograd"})


@pytest.mark.parametrize("k,s", exact.DECONV_KS)
@pytest.mark.parametrize("shape", exact.DECONV_SHAPES[2:])
def test_deconv_fallback_route_gradients(gpu, shape, k, s):
    """add1, add2, bias ask for a gradient: the op applies them (and the ReLU) as framework ops behind the kernel. On the
    integers of exact.deconv_inputs the forward is exact, so the ReLU mask is the same in both precisions; the gradients
    of x, add1 and add2 are then exact too, the bias gradient is a sum over B Ho Wo masked integers — compared under the
    rule of the graph test, 16 max(floor, 2^-20) with the float32 restatement's own error as floor."""
    import torch
    from posecnn_amd import ops
    B, H, W, C = shape
    x, a1, a2, b = exact.deconv_inputs(shape, s)
    gmax = _deconv_gmax(k, s)
    g = exact.ints(exact.seed_of("deconv_fb", shape, k), (B, H * s, W * s, C), -gmax, gmax)
    leaves = [t.clone().to(gpu).requires_grad_(True) for t in (x, a1, a2, b)]
    y = ops.deconv_bilinear(leaves[0], k, s, add1=leaves[1], add2=leaves[2], bias=leaves[3], relu=True)
    y.backward(g.to(gpu))
    refs = {}
    for dt in (torch.float64, torch.float32):
        lv = [t.clone().to(dt).requires_grad_(True) for t in (x, a1, a2, b)]
        y_ = grad_ref.deconv_bilinear64(lv[0], k, s, lv[1], lv[2], lv[3], True)
        refs[dt] = (y_.detach(), torch.autograd.grad(y_, lv, g.to(dt)))
    y64, g64 = refs[torch.float64]
    assert 0.2 < float((y64 > 0).double().mean()) < 0.8 and torch.equal(refs[torch.float32][0].double(), y64)
    exact.check(y.detach(), y64, {"name": "forward"})
    for name, got, want in zip(("x", "add1", "add2"), leaves, g64):
        exact.check(got.grad, want, {"name": "gradient of " + name})
    floor = grad_ref.rel_err(refs[torch.float32][1][3], g64[3])
    assert grad_ref.rel_err(leaves[3].grad, g64[3]) <= grad_ref.bound(floor), (grad_ref.rel_err(leaves[3].grad, g64[3]), floor)


# ---- smooth L1 ------------------------------------------------------------------------------------------------------
SL1_W = np.array([0.0, 0.5, 1.0, 2.0, 4.0], F)
# |p - t| <= steps 2^-11: 0.59 for sigma = 1 (w |p - t| crosses 1 for w = 2, 4), 0.34 for sigma = 3 (crosses 1/9 for every w)
SL1_STEPS = {1.0: 1200, 3.0: 700}
UPSTREAM = 5.0


def _planted_diffs(sigma):
    """w (p - t) on the branch point 1 / sigma^2 (as the float32 the kernel and TF compare with), one float32 step
    either side of it, both signs, and exactly 0."""
    d = F(1.0) / F(sigma * sigma)
    up, dn = np.nextafter(d, F(2)), np.nextafter(d, F(0))
    return [d, -d, dn, -dn, up, -up, F(0)]


def _branch_candidates(diff, w, sigma, denom):
    """The float32 value of the gradient element under either branch, with the kernel's operation order (one rounding
    per operation; csrc/sl1_device.h): (quadratic, linear). Where the two differ the kernel's bits tell its branch."""
    s2 = F(sigma * sigma)
    quad = ((w * (s2 * diff).astype(F)).astype(F) / denom).astype(F) * F(UPSTREAM)
    lin = ((w * np.sign(diff).astype(F)).astype(F) / denom).astype(F) * F(UPSTREAM)
    return quad.astype(F), lin.astype(F)


def _check_sl1(got_loss, got_grad, p, t, w, sigma, planted):
    """got_* from the GPU; p, t, w float32 arrays chosen so that w (p - t) is EXACTLY representable: the product and the
    difference are then the same number in float32 and float64, and so is the branch."""
    import torch
    p64, t64_, w64 = (a.astype(np.float64).ravel() for a in (p, t, w))
    d32 = (w.ravel() * (p.ravel() - t.ravel()).astype(F)).astype(F)
    assert np.array_equal(d32.astype(np.float64), w64 * (p64 - t64_)), "input not exact"
    pt = torch.from_numpy(p64).requires_grad_(True)
    loss = grad_ref.smooth_l1_vertex64(pt, torch.from_numpy(t64_), torch.from_numpy(w64), sigma)
    (g64,) = torch.autograd.grad(loss * UPSTREAM, pt)
    g64 = g64.numpy()
    got = got_grad.detach().cpu().numpy().ravel()
    ulp = np.spacing(np.abs(g64).astype(F)).astype(np.float64)
    off = np.abs(got.astype(np.float64) - g64) / ulp
    assert np.isfinite(got).all() and off.max() <= 4, "gradient: %g ulp at %d (got %r want %r)" % (off.max(), off.argmax(), got[off.argmax()], g64[off.argmax()])
    assert not got[w.ravel() == 0].any() and not got[d32 == 0].any()
    # the loss: n non-negative terms of a few roundings each, summed in float32 by a tree of depth <= ~24 over at most a few
    # serial adds per thread: relative error <= (4 + 32) 2^-24, far below anything a wrong branch or weight power produces
    lv = float(loss.detach())
    assert abs(float(got_loss) - lv) <= 36 * 2.0 ** -24 * abs(lv), (float(got_loss), lv)
    # the branch at the planted elements
    sw = F(w64.sum())
    denom = F(sw + F(1e-10))
    told = 0
    for i in planted:
        quad, lin = _branch_candidates(d32[i:i + 1], w.ravel()[i:i + 1], sigma, denom)
        want_quad = abs(float(d32[i])) < 1.0 / (sigma * sigma)                 # the float64 side's mask
        want, other = (quad, lin) if want_quad else (lin, quad)
        assert got[i] == want[0], (i, float(d32[i]), got[i], want[0])
        told += int(want[0] != other[0])
    return told


def _sl1_case(n, sigma, seed, zero_weights=False):
    """p, t multiples of 2^-11 below 8, w a power of two or 0: p - t and w (p - t) are exact. Planted elements at the
    front (as many of the seven as fit): t = 0, p = d / w on even ones, p = 0, t = -d / w on odd ones."""
    rng = np.random.default_rng(seed)
    w = SL1_W[rng.integers(0, len(SL1_W), n)]
    t = (rng.integers(-8191, 8192, n) * 2.0 ** -11).astype(F)
    p = (t + rng.integers(-SL1_STEPS[sigma], SL1_STEPS[sigma] + 1, n) * 2.0 ** -11).astype(F)
    planted = []
    if zero_weights:
        w[:] = 0
    else:
        for i, d in enumerate(_planted_diffs(sigma)[:n]):
            w[i] = SL1_W[1 + i % 4]
            if i % 2 == 0:
                t[i], p[i] = 0, d / w[i]
            else:
                p[i], t[i] = 0, -d / w[i]
            planted.append(i)
    return p, t, w, planted


@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("n", [1, 1000, 66 * 40 * 48])
def test_smooth_l1_vertex_gradient_equals_float64(gpu, n, sigma):
    import torch
    from posecnn_amd import ops
    for zero_weights in (False, True):
        p, t, w, planted = _sl1_case(n, sigma, 61 + n % 7, zero_weights)
        pt = T(gpu, p).requires_grad_(True)
        loss = ops.smooth_l1_loss_vertex(pt, T(gpu, t), T(gpu, w), sigma)
        (loss * UPSTREAM).backward()
        told = _check_sl1(loss.detach().cpu(), pt.grad, p, t, w, sigma, planted)
        if zero_weights:
            assert float(loss.detach()) == 0 and not pt.grad.any()
        elif n >= 7:
            live = np.abs(w * (p - t))[w > 0]
            assert (live < 1 / sigma ** 2).any() and (live > 1 / sigma ** 2).any()        # both branches among the random elements too
            assert told >= 2, "no planted element tells the branches apart"


# (B, H, W, C) of the target-free entry: its element count is a multiple of 3 C, so n = 1 and n = 1000 become the nearest
# shapes it takes (6 and 1020 elements); the third is the 66 x 40 x 48 of the dense entry
SL1_GT_SHAPES = [(1, 1, 1, 2), (1, 10, 17, 2), (1, 40, 48, 22)]


def _sl1_gt_case(shape, sigma, seed, zero_weights=False):
    """Label map + object table (cls, mask_id, cx, cy, log_z, w) with w from SL1_W. The targets are the table's
    (tests/vertex_ref.py); pred = target + a multiple of 2^-11 wherever that difference is exact in float32, else
    pred = target. Elements are planted on the log-depth channel of objects with log_z = 0 (target 0: p = d / w is exact)."""
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    label = rng.integers(0, C, (B, H, W)).astype(np.int32)
    obj = np.zeros((B, C - 1, 6), F)
    for b in range(B):
        for j, cls in enumerate(range(1, C)):
            obj[b, j] = (cls, 0, rng.uniform(0, W), rng.uniform(0, H), 0.0 if j % 2 == 0 else F(rng.uniform(-0.5, 0.5)),
                         0.0 if zero_weights else SL1_W[1 + j % 4] if j < 8 else SL1_W[rng.integers(0, 5)])
    t, w = vertex_ref.vertex_targets(label, obj, C)
    step = rng.integers(-SL1_STEPS[sigma], SL1_STEPS[sigma] + 1, t.shape) * 2.0 ** -11
    p = (t + step).astype(F)
    inexact = (p.astype(np.float64) - t.astype(np.float64)) != (p - t).astype(F).astype(np.float64)
    p[inexact] = t[inexact]
    p[w == 0] = (rng.integers(-8191, 8192, t.shape) * 2.0 ** -11).astype(F)[w == 0]       # finite noise where nothing is weighted
    planted = []
    if not zero_weights:
        diffs = _planted_diffs(sigma)
        flat_p, flat_w = p.reshape(-1), w.reshape(-1)
        for cls in range(1, C, 2):                                   # objects with log_z = 0
            ys, xs = np.nonzero(label[0] == cls)
            for y, x_ in zip(ys, xs):
                if not diffs:
                    break
                i = ((0 * H + y) * W + x_) * 3 * C + 3 * cls + 2
                assert t.reshape(-1)[i] == 0 and flat_w[i] > 0
                flat_p[i] = diffs.pop(0) / flat_w[i]
                planted.append(int(i))
    return label, obj, p, t, w, planted


@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("shape", SL1_GT_SHAPES)
def test_smooth_l1_vertex_gt_gradient_equals_float64(gpu, shape, sigma):
    import torch
    from posecnn_amd import ops
    for zero_weights in (False, True):
        label, obj, p, t, w, planted = _sl1_gt_case(shape, sigma, 67, zero_weights)
        pt = T(gpu, p).requires_grad_(True)
        loss = ops.smooth_l1_loss_vertex_gt(pt, T(gpu, label), T(gpu, obj), None, sigma)
        (loss * UPSTREAM).backward()
        told = _check_sl1(loss.detach().cpu(), pt.grad, p, t, w, sigma, planted)
        if zero_weights:
            assert float(loss.detach()) == 0 and not pt.grad.any()
        elif p.size > 1000:
            assert len(planted) == 7 and told >= 2
            assert shape[3] < 9 or set(np.unique(w)) == set(SL1_W.tolist())


# ---- ROI pooling ----------------------------------------------------------------------------------------------------
def _roi_case(name):
    rng = np.random.default_rng(71)
    if name == "small":
        B, H, W, C = 2, 10, 12, 8
        rois = random_rois(rng, 9, B, C, W * 8, H * 8)
        return (B, H, W, C), rois, 3, 3, 0.125
    B, H, W, C = 2, 9, 150, 40
    rois = random_rois(rng, 1200, B, C, W * 4, H * 4)              # the mix of test_roi_pool_ties_wide_rois_and_long_roi_lists
    rois[:40, 2] = 0; rois[:40, 4] = W * 4 - 1                      # full-width ROIs: wider than the LDS window
    rois[40:60, 4] = rois[40:60, 2] - 13                            # x2 < x1
    rois[60:80, 5] = rois[60:80, 3] - 9                             # y2 < y1
    rois[80:700, 0] = 1                                             # more ROIs on one image than the backward's list holds ...
    rois[80:700, 2:6] = [0, 0, W * 4 - 1, H * 4 - 1]                # ... all touching every tile
    return (B, H, W, C), rois, 4, 6, 0.25


@pytest.mark.parametrize("name", ["small", "wide_malformed_long_list"])
def test_roi_pool_backward_equals_float64(gpu, name):
    """data is a permutation of distinct integers (no ties: amax's gradient and the op's first-maximum rule agree), the
    upstream gradients are small integers: every sum is exact in any order, so the kernel must equal autograd of the
    float64 restatement bit for bit. A ROI with x2 < x1 or y2 < y1 pools a strip one cell wide in the forward; its
    gradient belongs to that strip's maxima."""
    import torch
    from posecnn_amd import ops
    shape, rois, ph, pw, scale = _roi_case(name)
    rng = np.random.default_rng(72)
    data = rng.permutation(int(np.prod(shape))).reshape(shape).astype(F)
    d = T(gpu, data).requires_grad_(True)
    top, _ = ops.roi_pool(d, T(gpu, rois), ph, pw, scale, 0)
    g = rng.integers(-3, 4, tuple(top.shape)).astype(F)
    top.backward(T(gpu, g))
    d64 = t64(data, grad=True)
    top64 = grad_ref.roi_pool64(d64, rois, ph, pw, scale)
    exact.check(top.detach(), top64.detach(), {"name": "roi_pool forward"})
    (want,) = torch.autograd.grad(top64, d64, t64(g))
    assert float(want.abs().max()) < exact.LIMIT and bool(want.any())
    exact.check(d.grad, want, {"name": "roi_pool backward"})


# ---- average distance -----------------------------------------------------------------------------------------------
# Measured on the CPU: the float32 numpy restatement (np_ref.average_distance, one rounding per operation in the
# reference's order) against float64 autograd of grad_ref.average_distance64 on the six cases below.
#   largest |bottom_diff - d loss / d pred| relative to its row's gradient norm, per case (R, C, P, margin):
#     (7,22,300,0) 2.1e-7   (7,22,300,.01) 2.5e-7   (12,5,1025,0) 5.3e-7   (12,5,1025,.01) 4.0e-7   (1,22,64,0) 1.1e-7   (1,22,64,.01) 7.3e-8
#   largest relative error of the loss: 2.7e-7 (12,5,1025,0)
ADL_MEASURED = 5.3e-7
ADL_LOSS_MEASURED = 2.7e-7


def _rot_np(q):
    """[K,4] quaternions (s, u, v, w) -> [K,3,3], the formula of np_ref._rot in float64."""
    s_, u, v, w = (q[:, i].astype(np.float64) for i in range(4))
    return np.stack([np.stack([s_ * s_ + u * u - v * v - w * w, 2 * (u * v - s_ * w), 2 * (u * w + s_ * v)], -1),
                     np.stack([2 * (u * v + s_ * w), s_ * s_ - u * u + v * v - w * w, 2 * (v * w - s_ * u)], -1),
                     np.stack([2 * (u * w - s_ * v), 2 * (v * w + s_ * u), s_ * s_ - u * u - v * v + w * w], -1)], 1)


def _adl_inputs(R, C, P, margin, seed=73):
    """adl_case (plain and symmetric classes, every fifth row without a class). With a margin, each row's prediction is
    redrawn (in batches, float64) until no point's squared distance is within 1e-4 of it and some point is above it:
    on the hinge the two precisions may disagree about a point. margin = 0 has no hinge: dist >= 0 always holds."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    pred, tgt, wgt, pts, sym = adl_case(rng, R, C, P, sym_classes=(16, 21) if C == 22 else (2,))
    for n in range(R if margin > 0 else 0):
        live = np.flatnonzero(wgt[n].reshape(C, 4)[:, 0] > 0)
        if len(live) == 0:
            continue
        c = int(live[0])
        pc = pts[c].astype(np.float64)
        x2 = pc @ _rot_np(tgt[n:n + 1, 4 * c:4 * c + 4])[0].T
        tree = cKDTree(x2) if sym[c] > 0 else None
        for _ in range(40):
            cand = np.tanh(rng.standard_normal((256, 4))).astype(F)
            x1 = np.einsum("kij,pj->kpi", _rot_np(cand), pc)
            near = x2[tree.query(x1.reshape(-1, 3))[1]].reshape(x1.shape) if tree is not None else x2
            dist = ((x1 - near) ** 2).sum(-1)
            ok = (np.abs(dist - margin).min(axis=1) > 1.05e-4) & (dist >= margin).any(axis=1)
            if ok.any():
                pred[n, 4 * c:4 * c + 4] = cand[int(np.argmax(ok))]
                break
        else:
            raise AssertionError("no prediction away from the hinge for row %d" % n)
    return pred, tgt, wgt, pts, sym


@pytest.mark.parametrize("margin", [0.0, 0.01])
@pytest.mark.parametrize("R,C,P", [(7, 22, 300), (12, 5, 1025), (1, 22, 64)])
def test_average_distance_bottom_diff_is_the_derivative_of_the_loss(gpu, R, C, P, margin, capsys):
    """`bottom_diff` (what AveragedistanceGrad scales by the upstream gradient) against d loss / d prediction of
    grad_ref.average_distance64 by float64 autograd, on full buffers and through the `num_rows` device count with
    R < capacity. Bound per element, relative to its row's gradient norm: 8 x the error of the float32 numpy
    restatement (np_ref.average_distance) against the same float64 gradient, measured over these six cases
    (ADL_MEASURED above): 8 x 5.3e-7 = 4.2e-6, and 8 x 2.7e-7 = 2.2e-6 for the loss; a wrong factor, a transposed
    rotation derivative or a wrong nearest point is an error of order 1."""
    import torch
    from posecnn_amd import ops
    cap = R + 3
    pred, tgt, wgt, pts, sym = _adl_inputs(cap, C, P, margin)
    p64 = t64(pred[:R], grad=True)
    terms = grad_ref.average_distance_terms(p64, t64(tgt[:R]), t64(wgt[:R]), t64(pts), sym)
    dist = torch.cat([t_[1] for t_ in terms if t_ is not None]).detach()
    assert (margin == 0 or float((dist - margin).abs().min()) > 1e-4) and (dist >= margin).any()
    assert any(t_ is None for t_ in terms) or R == 1
    if R > 1:
        assert {bool(sym[t_[0]] > 0) for t_ in terms if t_ is not None} == {True, False}
    loss64 = grad_ref.average_distance64(p64, t64(tgt[:R]), t64(wgt[:R]), t64(pts), sym, margin)
    (want,) = torch.autograd.grad(loss64, p64)
    loss64 = loss64.detach()
    want = want.numpy()
    norm = np.maximum(np.linalg.norm(want, axis=1, keepdims=True), 1e-300)
    measured = float("nan")
    if P <= 300:      # (the restatement is a Python loop over points: re-measured where that costs a fraction of a second)
        measured = float((np.abs(np_ref.average_distance(pred[:R], tgt[:R], wgt[:R], pts, sym, margin)[1] - want) / norm).max())
    loss, diff = ops.average_distance_loss(T(gpu, pred[:R]), T(gpu, tgt[:R]), T(gpu, wgt[:R]), T(gpu, pts), T(gpu, sym), margin)
    cnt = torch.tensor([R], dtype=torch.int32, device=gpu)
    loss_c, diff_c = ops.average_distance_loss(T(gpu, pred), T(gpu, tgt), T(gpu, wgt), T(gpu, pts), T(gpu, sym), margin, num_rows=cnt)
    errs = []
    for name, l_, d_ in (("full", loss, diff), ("num_rows", loss_c, diff_c[:R])):
        got = d_.cpu().numpy().astype(np.float64)
        errs.append(float((np.abs(got - want) / norm).max()))
        assert not got[np.all(want == 0, axis=1)].any(), name           # rows without a class
        assert abs(float(l_) - float(loss64)) <= 8 * ADL_LOSS_MEASURED * float(loss64), (name, float(l_), float(loss64))
    assert not diff_c[R:].any()
    with capsys.disabled():
        print("\naverage distance R=%d C=%d P=%d margin=%g: kernel %.2e / %.2e, float32 numpy restatement %.2e (relative to the row norm)"
              % (R, C, P, margin, errs[0], errs[1], measured))
    assert max(errs) <= 8 * ADL_MEASURED, errs
