"""The training label head on the GPU (include/posecnn_hip_loss.h, ops.label_head_loss, vgg16_convs(lowres_train_heads=True)).

Per-pixel results are compared bit for bit with tests/label_loss_ref.py (the numpy restatement on top of the C oracle, which
is itself within the float64 criterion: tests/test_label_loss_cpu.py); the two reductions with the bounds their f64
accumulation gives:

  loss    S is a float64 sum of at most 2^23 non-negative terms, relative error <= 2^-30 whatever the order; the division and
          the one rounding to float32 add half an ulp: |loss - float32(S64 / (count + 1e-10))| <= 1 ulp
  dbias   a float64 sum of signed float32 values, |error| <= 2^-30 sum |dscore[:, c]|, then one rounding to float32:
          |dbias[c] - S64[c]| <= 2^-24 |S64[c]| + 2^-30 sum |dscore[:, c]|

The cases (label_loss_ref.cases) are the smallest at which each branch can go wrong: a row of two 128-pixel segments with 8
live pixels in the second, tap sets clipped at every border, both (kernel, stride) pairs of the network, the compile-time
class counts 22 and 14 and the generic kernel at C = 5.
"""
import os
import tempfile

import numpy as np
import pytest

import grad_ref
import label_loss_ref as R
import oracle

pytestmark = pytest.mark.gpu
F = np.float32
UPSTREAM = 0.37
KINDS = R.GT_KINDS


def T(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)        # (a copy: the shared cases are read-only arrays)


def bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d differ, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][:3], want[bad][:3])


def check_loss(loss, r):
    want = F(r["S64"] / (r["count"] + 1e-10))
    assert abs(float(loss) - float(want)) <= float(np.spacing(want)), (float(loss), float(want))


def check_dbias(dbias, r):
    got = np.asarray(dbias, np.float64)
    tol = 2.0 ** -24 * np.abs(r["dbias64"]) + 2.0 ** -30 * r["dbias_abs"]
    assert np.isfinite(got).all() and (np.abs(got - r["dbias64"]) <= tol).all(), (got, r["dbias64"], tol)


def _inputs(gpu, c, kind):
    shape, C, ks = c
    z, bias, gt = R.case(shape, C, ks, kind)
    return T(gpu, z), T(gpu, bias), T(gpu, gt)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", R.cases(), ids=R.case_id)
def test_forward_bit_for_bit_and_loss(gpu, c, kind):
    from posecnn_amd import ops
    shape, C, (k, s) = c
    r = R.reference(shape, C, (k, s), kind)
    z, bias, gt = _inputs(gpu, c, kind)
    loss, sums, label, terms = ops._label_head_loss_raw(z, bias, gt, R.THRESHOLD, k, s, want_terms=True)
    assert np.array_equal(label.cpu().numpy(), r["label"])
    bits_equal(terms.cpu().numpy(), r["terms"], "terms")
    S, count = sums.cpu().numpy()
    assert count == r["count"] and (kind == "mixed") == (count > 0)
    assert abs(S - r["S64"]) <= 2.0 ** -30 * r["S64"]
    check_loss(loss.cpu().numpy(), r)
    # the public call: same loss and labels, no terms unless asked for
    out = ops.label_head_loss(z, bias, gt, R.THRESHOLD, k, s)
    assert len(out) == 2 and out[0].shape == () and out[1].dtype == label.dtype
    bits_equal(out[0].cpu().numpy().reshape(1), loss.cpu().numpy().reshape(1), "loss of the public call")
    assert np.array_equal(out[1].cpu().numpy(), r["label"])
    out3 = ops.label_head_loss(z, bias, gt, R.THRESHOLD, k, s, want_terms=True)
    bits_equal(out3[2].cpu().numpy(), r["terms"], "terms of the public call")
    if kind == "ignored":
        assert float(loss) == 0.0


# 2 x 136 rows x 1 segment = 272 workgroups: more than 256 partials per class, so the strided pass of the kernel that folds
# them (channel_partials_final_kernel, 256 threads) takes a second trip; the generic kernel, a few KB of data
MANY_PARTIALS = ((2, 17, 2), 5, (16, 8))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", R.cases() + [MANY_PARTIALS], ids=R.case_id)
def test_backward_kernel(gpu, c, kind):
    from posecnn_amd import ops
    shape, C, (k, s) = c
    r = R.reference(shape, C, (k, s), kind)
    z, bias, gt = _inputs(gpu, c, kind)
    dscore, dbias = ops.label_head_loss_grad(z, bias, gt, R.THRESHOLD, k, s)
    bits_equal(dscore.cpu().numpy(), r["dscore"], "dscore")
    dz = ops.deconv_bilinear_grad(dscore, k, s)
    bits_equal(dz.cpu().numpy(), oracle.deconv_bilinear_bwd(r["dscore"], k, s), "dz")
    check_dbias(dbias.cpu().numpy(), r)
    if kind == "ignored" or shape[0] > 1:
        frame = dscore.cpu().numpy() if kind == "ignored" else dscore[-1].cpu().numpy()
        assert np.isfinite(frame).all() and not frame.any()                  # an all-ignored frame: zeros, no NaN
    if kind == "ignored":
        assert not dz.cpu().numpy().any() and not dbias.cpu().numpy().any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", R.cases(), ids=R.case_id)
def test_autograd_with_a_non_unit_upstream_gradient(gpu, c, kind):
    import torch
    from posecnn_amd import ops
    shape, C, (k, s) = c
    r = R.reference(shape, C, (k, s), kind, upstream=UPSTREAM)
    z, bias, gt = _inputs(gpu, c, kind)
    z.requires_grad_(True)
    bias.requires_grad_(True)
    with torch.enable_grad():
        loss, label = ops.label_head_loss(z, bias, gt, R.THRESHOLD, k, s)
        assert loss.requires_grad and not label.requires_grad
        (loss * UPSTREAM).backward()
    check_loss(loss.detach().cpu().numpy(), r)
    bits_equal(z.grad.cpu().numpy(), r["dz"], "dz through autograd")
    check_dbias(bias.grad.cpu().numpy(), r)
    assert torch.isfinite(z.grad).all() and torch.isfinite(bias.grad).all()


def test_no_relu_and_the_other_compile_time_class_count(gpu):
    """relu=False (no gate, negative scores) and C = 16, the third compile-time instance."""
    from posecnn_amd import ops
    rng = np.random.default_rng(5)
    for C, relu in ((16, True), (16, False), (5, False), (33, True)):
        z = (rng.standard_normal((1, 2, 17, C)) * 1.5).astype(F)
        bias = (rng.standard_normal(C) * 0.5).astype(F)
        gt = rng.integers(-1, C + 1, (1, 16, 136)).astype(np.int32)
        r = R.restate(z, bias, gt, 0.2, 16, 8, relu=relu)
        assert 0 < r["count"] < gt.size and (relu or (r["score"] < 0).any())
        loss, sums, label, terms = ops._label_head_loss_raw(T(gpu, z), T(gpu, bias), T(gpu, gt), 0.2, 16, 8, relu=relu, want_terms=True)
        assert np.array_equal(label.cpu().numpy(), r["label"]) and int(sums[1]) == r["count"]
        bits_equal(terms.cpu().numpy(), r["terms"], "terms C=%d relu=%s" % (C, relu))
        check_loss(loss.cpu().numpy(), r)
        dscore, dbias = ops.label_head_loss_grad(T(gpu, z), T(gpu, bias), T(gpu, gt), 0.2, 16, 8, relu=relu)
        bits_equal(dscore.cpu().numpy(), r["dscore"], "dscore C=%d relu=%s" % (C, relu))
        check_dbias(dbias.cpu().numpy(), r)


# ---- memory contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [((2, 3, 17), 22, (16, 8)), ((1, 1, 3), 5, (4, 2))], ids=R.case_id)
def test_memory_contract(gpu, c):
    """Both poison patterns and guard bands of tests/memguard.py, as tests/test_gpu_memory_contract.py runs every other
    entry: identical outputs, inputs and guards intact, a workspace of exactly the declared size whose prior contents
    (0xFF bytes = NaN partials under P1, zero bytes under P2) do not matter. With want_terms=False the call allocates, and
    so touches, no terms buffer: every buffer the op makes is returned here and compared."""
    from test_gpu_memory_contract import Case, execute
    shape, C, (k, s) = c
    r = R.reference(shape, C, (k, s))

    def make():
        z, bias, gt = R.case(shape, C, (k, s))
        return dict(z=np.array(z), bias=np.array(bias), gt=np.array(gt))       # (copies: the shared cases are read-only)

    def run(ctx):
        from posecnn_amd import ops
        z, bias, gt = ctx.e("z"), ctx.e("bias"), ctx.e("gt")
        n0 = len(ctx.g.arenas)
        loss, label = ops.label_head_loss(z, bias, gt, R.THRESHOLD, k, s)
        made = [a.describe() for a in ctx.g.arenas[n0:]]
        assert len(made) == 4, made            # workspace, loss, sums, label: no terms, nothing of size [B,Ho,Wo,C]
        assert max(a.nbytes for a in ctx.g.arenas[n0:] if a.dtype != ops.torch.uint8) == label.numel() * 4
        loss_t, label_t, terms = ops.label_head_loss(z, bias, gt, R.THRESHOLD, k, s, want_terms=True)
        dscore, dbias = ops.label_head_loss_grad(z, bias, gt, R.THRESHOLD, k, s)
        dz = ops.deconv_bilinear_grad(dscore, k, s)
        return dict(loss=loss.reshape(1), label=label, loss_t=loss_t.reshape(1), label_t=label_t, terms=terms, dscore=dscore,
                    dbias=dbias, dz=dz)

    def check(d, out):
        assert np.array_equal(out["label"], r["label"]) and np.array_equal(out["label_t"], r["label"])
        bits_equal(out["terms"], r["terms"], "terms")
        bits_equal(out["loss"], out["loss_t"], "loss with and without terms")
        check_loss(out["loss"][0], r)
        bits_equal(out["dscore"], r["dscore"], "dscore")
        bits_equal(out["dz"], r["dz"], "dz")
        check_dbias(out["dbias"], r)

    execute(Case("label_head_loss " + R.case_id(c),
                 ("pcnn_label_head_loss_workspace_bytes", "pcnn_label_head_loss_fwd", "pcnn_label_head_loss_bwd",
                  "pcnn_deconv_bilinear_bwd"), make, run, check))


def test_two_streams_give_identical_bits(gpu):
    import torch
    from posecnn_amd import ops
    rng = np.random.default_rng(11)
    C, k, s = 22, 16, 8
    z = T(gpu, (rng.standard_normal((2, 9, 33, C)) * 1.5).astype(F))          # 2 x 72 x 264: 432 workgroups, 2 partials per thread
    bias = T(gpu, (rng.standard_normal(C) * 0.5).astype(F))
    gt = T(gpu, rng.integers(-1, C, (2, 72, 264)).astype(np.int32))
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        stream = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(stream):
            zz = z.clone().requires_grad_(True)
            bb = bias.clone().requires_grad_(True)
            with torch.enable_grad():
                loss, _ = ops.label_head_loss(zz, bb, gt, 0.3, k, s)
                loss.backward()
        stream.synchronize()
        runs.append([t.detach().cpu().numpy().reshape(-1) for t in (loss, bb.grad, zz.grad)])
    for name, a, b in zip(("loss", "dbias", "dz"), *runs):
        bits_equal(a, b, name + " on two streams")
    assert runs[0][0][0] > 0 and runs[0][2].any()


# ---- the training graph ------------------------------------------------------------------------------------------------
def _net(gpu, lowres, variables=None):
    import torch
    from posecnn_amd.networks import vgg16_convs
    net = vgg16_convs("COLOR", grad_ref.NUM_CLASSES, grad_ref.NUM_UNITS, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True,
                      trainable=True, is_train=True, device=gpu, seed=3, init="he", lowres_train_heads=lowres)
    if variables is not None:
        net.vars = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in variables.items()}
    return net


def _feeds(gpu):
    feed_np = grad_ref.dense_vertex_feed(grad_ref.graph_feed())
    keys = ["data", "gt_label_2d", "poses", "extents", "meta_data", "points", "symmetry", "vertex_targets", "vertex_weights"]
    feed = {k: T(gpu, feed_np[k]) for k in keys}
    feed["keep_prob"] = 1.0
    planted = {k: T(gpu, v) for k, v in feed_np["planted"].items()}
    return feed_np, feed, planted


def test_whole_graph_gradients_equal_float64(gpu, capsys):
    """vgg16_convs(lowres_train_heads=True) + train.build_losses + backward at grad_ref.GRAPH_SHAPE against float64 autograd
    of grad_ref.training_loss64 — the restatement of the LITERAL graph — under the criterion of tests/test_gpu_gradients.py:
    err[v] <= 16 max(floor[v], 2^-20), floor[v] the float32 restatement's own error. The constants of the float64 pass
    (ROIs, pose targets, hard-label weights) come from the literal graph on the same variables; the discrete outputs of
    the two graphs must be equal, element for element."""
    import torch
    from posecnn_amd import synth, train
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    feed_np, feed, planted = _feeds(gpu)
    literal = _net(gpu, False)
    synth.init_calibrated(literal)
    with torch.enable_grad():
        literal.run(feed, planted=planted)
        lit_losses = {k: float(v.detach()) for k, v in train.build_losses(literal).items()}
    assert not literal.fused_heads and not literal.lowres_train_heads and "upscore" in literal.layers
    discrete = ("label_2d", "rois", "poses_target", "poses_weight")
    lit = {k: literal.get_output(k).detach().cpu().numpy() for k in discrete + ("gt_label_weight",)}

    net = _net(gpu, True, literal.vars)
    with torch.enable_grad():
        net.run(feed, planted=planted)
        losses = train.build_losses(net)
        losses["loss"].backward()
    torch.cuda.synchronize()
    assert net.lowres_train_heads and not net.fused_heads
    assert sorted(net.vars) == sorted(literal.vars) and all(v.requires_grad for v in net.vars.values()) and len(net.vars) == 44
    for name in ("upscore", "score", "prob", "prob_normalized", "gt_label_weight", "upscore_vertex"):
        assert name not in net.layers
        with pytest.raises(KeyError, match="lowres_train_heads"):
            net.get_output(name)
    # the discrete outputs: flips are counted and reported, and none is accepted
    flips = {k: int((net.get_output(k).detach().cpu().numpy() != lit[k]).sum()) if net.get_output(k).shape == lit[k].shape else -1
             for k in discrete}
    got = {k: float(v.detach()) for k, v in losses.items()}
    consts = {k: lit[k] for k in ("rois", "poses_target", "poses_weight", "gt_label_weight")}
    g64, l64 = grad_ref.grads_of(grad_ref.vars_from_net(net.vars, torch.float64), feed_np, consts, train.TrainConfig)
    g32, l32 = grad_ref.grads_of(grad_ref.vars_from_net(net.vars, torch.float32), feed_np, consts, train.TrainConfig)
    floor = {k: grad_ref.rel_err(g32[k], g64[k]) for k in g64}
    err = {k: grad_ref.rel_err(net.vars[k].grad, g64[k]) for k in g64}
    lfloor = {k: abs(l32[k] - l64[k]) / abs(l64[k]) for k in l64}
    lerr = {k: abs(got[k] - l64[k]) / abs(l64[k]) for k in l64}
    with capsys.disabled():
        print("\ntraining graph, lowres_train_heads=True; elements that differ from the literal graph: %s" % flips)
        print("%-28s %10s %10s %10s" % ("variable", "err", "floor", "bound"))
        for k in sorted(err):
            print("%-28s %10.2e %10.2e %10.2e" % (k, err[k], floor[k], grad_ref.bound(floor[k])))
        for k in sorted(lerr):
            print("%-28s %10.2e %10.2e %10.2e   (%.9g, literal graph %.9g)" % (k, lerr[k], lfloor[k], grad_ref.bound(lfloor[k]), got[k], lit_losses[k]))
    assert flips == {k: 0 for k in discrete}, flips
    assert sorted(err) == sorted(net.vars)
    for k in sorted(floor):
        assert floor[k] <= grad_ref.FLOOR_CAP, (k, floor[k])
    bad = {k: (err[k], grad_ref.bound(floor[k])) for k in err if not err[k] <= grad_ref.bound(floor[k])}
    assert not bad, bad
    assert min(got[k] for k in ("loss_cls", "loss_vertex", "loss_pose")) > 0
    for k in lerr:
        assert lerr[k] <= grad_ref.bound(lfloor[k]), (k, got[k], l64[k])


def test_solver_steps_and_snapshots_cross_the_switch(gpu):
    import torch
    from posecnn_amd import train
    from test_gpu_training import training_feed
    torch.manual_seed(0)
    feed = training_feed(gpu, 1, 96, 128, 77)

    class Cfg(train.TrainConfig):
        LEARNING_RATE = 1e-6

    on, off = _net(gpu, True), _net(gpu, False)
    solver = train.SolverWrapper(on, Cfg)
    for _ in range(3):
        step = solver.train_step(feed)
        assert sorted(step) == ["loss", "loss_cls", "loss_pose", "loss_regu", "loss_vertex"]
        assert all(np.isfinite(v) for v in step.values()) and step["loss_cls"] > 0 and step["loss_vertex"] > 0, step
    for k, v in on.vars.items():
        assert v.requires_grad and v.grad is not None and torch.isfinite(v.grad).all(), k
    assert float(on.vars["score/weights"].grad.abs().max()) > 0 and float(on.vars["vertex_pred/weights"].grad.abs().max()) > 0
    path = os.path.join(tempfile.mkdtemp(), "snap.pt")
    solver.snapshot(path)
    other = train.SolverWrapper(off, Cfg)
    first_off = other.train_step(feed)              # creates the literal graph's variables: the same names
    assert sorted(off.vars) == sorted(on.vars)
    other.restore(path)
    assert other.iter == 3 and all(torch.equal(off.vars[k], on.vars[k]) for k in on.vars)
    assert all(np.isfinite(v) for v in other.train_step(feed).values()) and np.isfinite(first_off["loss"])
    other.snapshot(path)                            # and back: a snapshot of the literal graph into the switched one
    solver.restore(path)
    assert solver.iter == 4 and all(torch.equal(off.vars[k], on.vars[k]) for k in on.vars)
    assert all(np.isfinite(v) for v in solver.train_step(feed).values())


def test_default_graph_is_untouched(gpu):
    import torch
    from posecnn_amd.networks import vgg16_convs
    feed_np, feed, planted = _feeds(gpu)
    train_net = _net(gpu, False)
    assert not train_net.fused_heads and not train_net.lowres_train_heads
    with torch.enable_grad():
        train_net.run(feed, planted=planted)
    for name in ("upscore", "score", "prob", "prob_normalized", "gt_label_weight", "label_2d", "upscore_vertex", "vertex_pred"):
        assert isinstance(train_net.get_output(name), torch.Tensor), name
    assert "loss_cls" not in train_net.layers
    # the switch is inert outside a trainable training graph: inference keeps its fused heads
    for kw in (dict(trainable=False, is_train=False), dict(trainable=False, is_train=True)):
        a, b = (vgg16_convs("COLOR", 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, device=gpu, seed=3, init="he",
                            lowres_train_heads=sw, **kw) for sw in (False, True))
        assert a.fused_heads and b.fused_heads and not a.lowres_train_heads and not b.lowres_train_heads
        with torch.no_grad():
            a.run(feed, planted=planted)
            b.run(feed, planted=planted)
        assert sorted(a.layers) == sorted(b.layers) and "loss_cls" not in b.layers
        assert torch.equal(a.get_output("label_2d"), b.get_output("label_2d")) and torch.equal(a.get_output("rois"), b.get_output("rois"))
