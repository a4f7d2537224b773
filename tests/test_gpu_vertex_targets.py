"""The device-side vertex targets and the target-free vertex loss (include/posecnn_hip_train.h) on the GPU:

  * `ops.vertex_targets` against the numpy restatement (tests/vertex_ref.py, itself pinned to the reference's outputs),
    bit for bit;
  * `pcnn_smooth_l1_vertex_gt_fwd` / `_bwd` against `pcnn_smooth_l1_vertex_fwd` / `_bwd` on the materialised tensors and
    against the C oracle: the three forward outputs bit for bit; the gradient bit for bit wherever the weight is
    non-zero and numerically equal everywhere (a zero-weight element may differ in the sign of zero);
  * autograd and the `train.build_losses` route;
  * the memory contract of the three entries (tests/memguard.py through the harness of test_gpu_memory_contract.py).
"""
import numpy as np
import pytest

import oracle
import vertex_ref
from posecnn_amd import config, synth
from test_gpu_memory_contract import Case, execute
from vertex_ref import same_bits

pytestmark = pytest.mark.gpu
F = np.float32
W_INSIDE = 10.0


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def synth_feed(seed, B, H, W, C=22, n_obj=4, w=W_INSIDE):
    """label int32 [B,H,W] and the object table [B,n_obj,6] of `synth.make_batch` frames (centre, depth per object)."""
    K = config.DEMO_INTRINSICS.copy()
    K[:2] *= W / 640.0
    label, _, frames = synth.make_batch(seed, B, H=H, W=W, C=C, n_obj=n_obj, K=K, min_pixels=1)
    obj = np.zeros((B, n_obj, 6), F)
    for b, fr in enumerate(frames):
        for j, (cls, cx, cy, z) in enumerate(fr["objects"]):
            obj[b, j] = (cls, 0, F(cx), F(cy), F(np.log(z)), w)
    return label.astype(np.int32), obj


def multi_instance_frame(H, W, rows=6):
    """Two instances of class 4 told apart by the instance map, one plain object of class 9, a stale first row of class 4
    that every pixel of it overrides, and class 7 pixels nobody describes."""
    yy, xx = np.mgrid[0:H, 0:W]
    label = np.zeros((H, W), np.int32)
    inst = np.zeros((H, W), np.int32)
    discs = [(4, 0.25 * W, 0.3 * H, 0.12 * H, 1), (4, 0.7 * W, 0.6 * H, 0.15 * H, 2), (9, 0.5 * W, 0.8 * H, 0.1 * H, 3),
             (7, 0.1 * W, 0.9 * H, 0.05 * H, 4)]
    for cls, cx, cy, r, k in discs:
        m = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
        label[m], inst[m] = cls, k
    obj = np.zeros((rows, 6), F)
    obj[0] = (4, 0, 1.0, 2.0, 0.5, 3.0)
    obj[1] = (4, 1, F(0.25 * W + 0.3), F(0.3 * H - 0.2), F(np.log(0.8)), W_INSIDE)
    obj[2] = (9, 0, F(0.5 * W), F(0.8 * H), F(np.log(1.1)), W_INSIDE)
    obj[3] = (4, 2, F(0.7 * W - 0.4), F(0.6 * H + 0.1), F(np.log(1.3)), W_INSIDE)
    return label, inst, obj


def big_batch():
    """B = 4 at 480 x 640, C = 22: two synthetic frames, an empty frame, a multi-instance frame."""
    label, obj = synth_feed(300, 2, 480, 640, n_obj=6)
    ml, mi, mo = multi_instance_frame(480, 640, rows=6)
    label = np.concatenate([label, np.zeros((1, 480, 640), np.int32), ml[None]])
    inst = np.concatenate([np.zeros((3, 480, 640), np.int32), mi[None]])
    obj = np.concatenate([obj, np.zeros((1, 6, 6), F), mo[None]])
    return label, inst, obj


def run_generator(dev, label, obj, C, inst=None):
    import torch
    from posecnn_amd import ops
    t, w = ops.vertex_targets(_t(label, dev), _t(obj, dev), C, None if inst is None else _t(inst, dev))
    torch.cuda.synchronize()
    assert t.shape == w.shape == label.shape + (3 * C,)
    return t.cpu().numpy(), w.cpu().numpy()


# ---- generator parity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vertex_ref.golden_cases(), ids=lambda c: c["name"])
def test_generator_equals_the_reference_outputs(gpu, case):
    inst = None if case["instance"] is None else case["instance"][None]
    t, w = run_generator(gpu, case["label"][None], case["objects"][None], case["num_classes"], inst)
    assert same_bits(t[0], case["targets"]) and same_bits(w[0], case["weights"])


def test_generator_equals_the_restatement_on_a_full_size_batch(gpu):
    label, inst, obj = big_batch()
    want_t, want_w = vertex_ref.vertex_targets(label, obj, 22, inst)
    assert want_w[0].any() and want_w[1].any() and not want_w[2].any() and want_w[3].any()
    assert set(np.unique(want_w[3])) == {0.0, W_INSIDE}          # the stale row (w = 3) is overridden everywhere
    t, w = run_generator(gpu, label, obj, 22, inst)
    assert same_bits(t, want_t) and same_bits(w, want_w)
    # without the instance map the rows with a mask id match nothing: class 4 falls back to the stale row
    want_t, want_w = vertex_ref.vertex_targets(label[3:], obj[3:], 22)
    t, w = run_generator(gpu, label[3:], obj[3:], 22)
    assert same_bits(t, want_t) and same_bits(w, want_w) and (w[0][label[3] == 4][:, 12] == 3).all()


def test_generator_without_objects_and_on_odd_shapes(gpu):
    label, _, obj = big_batch()
    t, w = run_generator(gpu, label[:1], obj[:1, :0], 22)        # M = 0
    assert not t.any() and not w.any() and not np.signbit(t).any()
    # frames whose element count is not a multiple of four: the 128-bit stores start mid-tile
    rng = np.random.default_rng(5)
    for B, H, W, C in ((3, 7, 9, 5), (2, 33, 31, 3), (1, 1, 1, 2), (5, 1, 300, 64)):
        label = rng.integers(-1, C + 1, (B, H, W)).astype(np.int32)
        inst = rng.integers(0, 3, (B, H, W)).astype(np.int32)
        obj = np.zeros((B, 2 * C, 6), F)
        obj[..., 0] = rng.integers(0, C + 1, (B, 2 * C))
        obj[..., 1] = rng.integers(0, 3, (B, 2 * C))
        obj[..., 2] = rng.uniform(-W, 2 * W, (B, 2 * C))
        obj[..., 3] = rng.uniform(-H, 2 * H, (B, 2 * C))
        obj[..., 4:] = rng.uniform(-1, 1, (B, 2 * C, 2))
        want_t, want_w = vertex_ref.vertex_targets(label, obj[:, :64], C, inst)
        t, w = run_generator(gpu, label, obj[:, :64], C, inst)
        assert same_bits(t, want_t) and same_bits(w, want_w), (B, H, W, C)


# ---- loss parity ---------------------------------------------------------------------------------------------------
def loss_inputs(B, H, W, sigma, seed):
    """pred around the targets so that both branches of the smooth L1 are taken under a weight: w |p - t| is below
    1 / sigma^2 for |N(0,1)| < 1 (68 %) and above it for the rest; finite noise where the weight is zero."""
    label, obj = synth_feed(seed, B, H, W)
    targets, weights = vertex_ref.vertex_targets(label, obj, 22)
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal(targets.shape).astype(F)
    pred = np.where(weights != 0, targets + noise * F(0.1 / sigma ** 2), noise * F(2)).astype(F)
    # the split, from the inputs alone
    live = weights != 0
    quad = np.abs(weights * (pred - targets))[live] < F(1.0) / F(sigma * sigma)
    assert live.mean() > 0.001 and 0.01 <= quad.mean() <= 0.99, (live.mean(), quad.mean())
    return label, obj, pred, targets, weights


LOSS_SHAPES = [(16, 60, 80), (2, 480, 640)]


@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_fused_loss_equals_the_unfused_kernels_and_the_oracle(gpu, shape, sigma):
    import torch
    from posecnn_amd import ops
    B, H, W = shape
    label, obj, pred, targets, weights = loss_inputs(B, H, W, sigma, 900 + B)
    want_out, want_grad = oracle.smooth_l1_vertex(pred, targets, weights, sigma)

    d_label, d_obj = _t(label, gpu), _t(obj, gpu)
    p_f = _t(pred, gpu).requires_grad_(True)
    loss_f, sums_f = ops._SmoothL1VertexGtFn.apply(p_f, d_label, None, d_obj, sigma)
    (grad_f,) = torch.autograd.grad(loss_f * 5.0, p_f)
    p_u = _t(pred, gpu).requires_grad_(True)
    loss_u, sums_u = ops._SmoothL1VertexFn.apply(p_u, _t(targets, gpu), _t(weights, gpu), sigma)
    (grad_u,) = torch.autograd.grad(loss_u * 5.0, p_u)
    torch.cuda.synchronize()

    out_f = np.concatenate([loss_f.detach().reshape(1).cpu().numpy(), sums_f.detach().cpu().numpy()])
    out_u = np.concatenate([loss_u.detach().reshape(1).cpu().numpy(), sums_u.detach().cpu().numpy()])
    print("sigma %g %s: fused %r unfused %r oracle %r" % (sigma, shape, out_f, out_u, want_out))
    assert same_bits(out_f, out_u) and same_bits(out_f, want_out)
    assert out_f[2] > 0 and np.isfinite(out_f).all()

    grad_f, grad_u = grad_f.cpu().numpy(), grad_u.cpu().numpy()
    live = weights != 0
    assert np.array_equal(grad_f[live].view(np.uint32), grad_u[live].view(np.uint32)) and grad_f[live].any()
    assert np.array_equal(grad_f, grad_u)                        # -0 == +0: only the sign of zero may differ
    assert not np.signbit(grad_f[~live]).any() and not grad_f[~live].any()
    assert same_bits(grad_u, (want_grad * F(5.0)).astype(F))


def test_autograd_shapes_instance_and_errors(gpu):
    import torch
    from posecnn_amd import ops
    ml, mi, mo = multi_instance_frame(48, 64)
    label, inst, obj = ml[None], mi[None], mo[None]
    targets, weights = vertex_ref.vertex_targets(label, obj, 22, inst)
    rng = np.random.default_rng(3)
    pred = (targets + rng.standard_normal(targets.shape) * 0.05).astype(F)
    p = _t(pred, gpu).requires_grad_(True)
    loss = ops.smooth_l1_loss_vertex_gt(p, _t(label, gpu), _t(obj, gpu), _t(inst, gpu), sigma=2.0)
    assert loss.shape == () and loss.requires_grad
    loss.backward()
    want_out, want_grad = oracle.smooth_l1_vertex(pred, targets, weights, 2.0)
    assert same_bits(loss.detach().reshape(1).cpu().numpy(), want_out[:1])
    assert p.grad.shape == p.shape and np.array_equal(p.grad.cpu().numpy(), want_grad)
    assert np.array_equal(p.detach().cpu().numpy(), pred)        # inputs untouched
    # an infinite prediction under a zero weight has no influence (the documented precondition of the unfused path)
    pred2 = pred.copy()
    pred2[0, 0, 0, 0] = np.inf
    assert weights[0, 0, 0, 0] == 0
    loss2 = ops.smooth_l1_loss_vertex_gt(_t(pred2, gpu), _t(label, gpu), _t(obj, gpu), _t(inst, gpu), sigma=2.0)
    assert same_bits(loss2.reshape(1).cpu().numpy(), want_out[:1])
    d_label, d_obj = _t(label, gpu), _t(obj, gpu)
    with pytest.raises(ValueError):
        ops.smooth_l1_loss_vertex_gt(p[:, :-1], d_label, d_obj)                   # pred / label shapes
    with pytest.raises(ValueError):
        ops.smooth_l1_loss_vertex_gt(p[..., :-1], d_label, d_obj)                 # channels not 3C
    with pytest.raises(ValueError):
        ops.smooth_l1_loss_vertex_gt(p, d_label, d_obj[:, :, :5])                 # table columns
    with pytest.raises(ValueError):
        ops.smooth_l1_loss_vertex_gt(p, d_label, d_obj.repeat(2, 1, 1))           # table batch
    with pytest.raises(ValueError):
        ops.smooth_l1_loss_vertex_gt(p, d_label, d_obj, _t(inst[:, :-1], gpu))    # instance shape
    with pytest.raises(ValueError):
        ops.vertex_targets(d_label, d_obj, 1)                                     # C < 2 (the library's check)
    with pytest.raises(ValueError):
        ops.vertex_targets(d_label, torch.zeros(1, 65, 6, device=gpu), 22)        # M > 64


def test_build_losses_takes_the_fused_route_with_the_same_bits(gpu):
    import torch
    from posecnn_amd import ops, train
    from posecnn_amd.networks import vgg16_convs
    from test_gpu_training import training_feed
    B, H, W, seed = 1, 160, 208, 77
    feed = training_feed(gpu, B, H, W, seed)
    K = config.DEMO_INTRINSICS.copy(); K[:2] *= W / 640.0
    _, _, frames = synth.make_batch(seed, B, H=H, W=W, C=22, n_obj=2, K=K)          # the frames training_feed drew
    obj = np.zeros((B, 2, 6), F)
    for b, fr in enumerate(frames):
        for j, (cls, cx, cy, z) in enumerate(fr["objects"]):
            obj[b, j] = (cls, 0, F(cx), F(cy), F(np.log(z)), W_INSIDE)
    d_obj = _t(obj, gpu)
    targets, weights = ops.vertex_targets(feed["gt_label_2d"], d_obj, 22)
    assert float(weights.sum()) > 0
    torch.manual_seed(0)
    net = vgg16_convs("COLOR", 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=True,
                      is_train=True, device=gpu, seed=3, init="he")
    with torch.enable_grad():
        net.run(dict(feed, vertex_targets=targets, vertex_weights=weights))
        unfused = train.build_losses(net)
        (g_u,) = torch.autograd.grad(unfused["loss_vertex"], net.get_output("vertex_pred"), retain_graph=True)
        del net.layers["vertex_targets"], net.layers["vertex_weights"]
        net.layers["vertex_objects"] = d_obj
        fused = train.build_losses(net)
        (g_f,) = torch.autograd.grad(fused["loss_vertex"], net.get_output("vertex_pred"), retain_graph=True)
    bits = lambda v: v.detach().reshape(1).cpu().numpy()
    assert same_bits(bits(fused["loss_vertex"]), bits(unfused["loss_vertex"])) and float(fused["loss_vertex"]) > 0
    assert same_bits(bits(fused["loss"]), bits(unfused["loss"]))
    assert np.array_equal(g_f.cpu().numpy(), g_u.cpu().numpy()) and g_f.abs().sum() > 0
    # a feed that carries vertex_targets keeps the unfused route even when the table is there too
    net.layers["vertex_targets"], net.layers["vertex_weights"] = targets * 0, weights
    assert not same_bits(bits(train.build_losses(net)["loss_vertex"]), bits(fused["loss_vertex"]))


# ---- memory contract -----------------------------------------------------------------------------------------------
def _contract_inputs(B, H, W, C, M, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    label = np.zeros((B, H, W), np.int32)
    inst = rng.integers(0, 3, (B, H, W)).astype(np.int32)
    obj = np.zeros((B, M, 6), F)
    for b in range(B):
        for j in range(M - 1):                                   # the last row stays empty
            cls = int(rng.integers(1, C))
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            label[b][(xx - cx) ** 2 + (yy - cy) ** 2 <= (0.2 * min(H, W)) ** 2] = cls
            obj[b, j] = (cls, j % 3, F(cx), F(cy), F(rng.uniform(-0.5, 0.5)), W_INSIDE)
    targets, weights = vertex_ref.vertex_targets(label, obj, C, inst)
    pred = (targets + rng.standard_normal(targets.shape) * 0.2).astype(F)
    return dict(label=label, inst=inst, obj=obj, pred=pred, targets=targets, weights=weights)


def _generator_case(name, B, H, W, C, M):
    def run(c):
        from posecnn_amd import ops
        t, w = ops.vertex_targets(c.e("label"), c.e("obj"), C, c.e("inst"))
        return dict(targets=t, weights=w)

    def check(d, o):
        assert d["weights"].any()
        assert same_bits(o["targets"], d["targets"]) and same_bits(o["weights"], d["weights"])
    return Case(name, ("pcnn_vertex_targets_fwd",), lambda: _contract_inputs(B, H, W, C, M, 61), run, check)


def _loss_case(name, B, H, W, C, M, sigma):
    def run(c):
        import torch
        from posecnn_amd import ops
        p = c.e("pred").requires_grad_(True)
        loss = ops.smooth_l1_loss_vertex_gt(p, c.e("label"), c.e("obj"), c.e("inst"), sigma)
        (gp,) = torch.autograd.grad(loss * 5.0, p)
        return dict(loss=loss.detach().reshape(1), grad=gp)

    def check(d, o):
        out, grad = oracle.smooth_l1_vertex(d["pred"], d["targets"], d["weights"], sigma)
        assert out[2] > 0 and same_bits(o["loss"], out[:1])
        assert np.array_equal(o["grad"], (grad * F(5.0)).astype(F)) and not np.signbit(o["grad"][d["weights"] == 0]).any()
    return Case(name, ("pcnn_smooth_l1_vertex_gt_fwd", "pcnn_smooth_l1_vertex_gt_bwd"),
                lambda: _contract_inputs(B, H, W, C, M, 62), run, check)


CONTRACT = [_generator_case("vertex_targets_3x7x9_c5", 3, 7, 9, 5, 4),           # 945 elements per frame: odd tile starts
            _generator_case("vertex_targets_2x37x53_c22", 2, 37, 53, 22, 7),
            _loss_case("smooth_l1_gt_3x7x9_c5", 3, 7, 9, 5, 4, 1.0),
            _loss_case("smooth_l1_gt_2x37x53_c22", 2, 37, 53, 22, 7, 3.0)]


@pytest.mark.parametrize("case", CONTRACT, ids=[c.name for c in CONTRACT])
def test_memory_contract_of_the_training_entries(gpu, case):
    """Guard bands around every output, input and workspace, both poison patterns of uninitialised memory: identical
    results, guards and inputs intact, every entry reached."""
    execute(case)
