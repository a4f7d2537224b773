"""The training vertex head on the GPU (include/posecnn_hip_vertex_loss.h, ops.vertex_head_loss,
vgg16_convs(lowres_train_heads=True, fused_vertex_loss=True)).

The acceptance criterion is bit equality with entries that exist and are tested already: `out` is what
pcnn_smooth_l1_vertex_gt_fwd returns on deconv(z) + bias, dz what pcnn_deconv_bilinear_bwd makes of pcnn_smooth_l1_vertex_gt_bwd.
tests/vertex_head_ref.py states both sides in numpy — `reference`, the dense composition on the C oracle, and `restate`, the
fused order — and tests/test_vertex_head_cpu.py holds them to each other and to float64. dbias is a float64 sum of float32
values rounded once: |dbias[c] - S64[c]| <= 2^-24 |S64[c]| + 2^-30 sum |g[:, c]| (the label head's bound), and its order is
written down, so it is also compared bit for bit with the restatement.
"""
import functools
import os
import tempfile

import numpy as np
import pytest

import grad_ref
import vertex_head_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
IDS = ["%s-%s" % nk for nk in R.case_ids()]
VERTEX_W = 5.0


def T(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)        # (a copy: the shared cases are read-only arrays)


def bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d differ, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][:3], want[bad][:3])


def check_dbias(dbias, r, scale=1.0, extra=0.0):
    got = np.asarray(dbias, np.float64)
    want = scale * r["dbias64"]
    tol = 2.0 ** -24 * np.abs(want) + (2.0 ** -30 + extra) * scale * r["dbias_abs"]
    assert np.isfinite(got).all() and (np.abs(got - want) <= tol).all(), (got, want, tol)


@functools.lru_cache(maxsize=None)
def _restated(name, kind):
    return R.restate(R.case(name, kind))


def _inputs(gpu, c):
    return (T(gpu, c["z"]), T(gpu, c["bias"]), T(gpu, c["label"]), T(gpu, c["objects"])), T(gpu, c["instance"])


# ---- the kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", R.case_ids(), ids=IDS)
def test_forward_and_backward_bit_for_bit(gpu, nk):
    from posecnn_amd import ops
    c = R.case(*nk)
    r, q = R.reference(c), _restated(*nk)
    k, s, sigma = c["k"], c["s"], c["sigma"]
    args, inst = _inputs(gpu, c)
    out = ops._vertex_head_loss_raw(*args, k, s, inst, sigma)
    bits_equal(out.cpu().numpy(), r["out"], "out")
    loss, sums = ops.vertex_head_loss(*args, k, s, instance=inst, sigma=sigma)
    assert loss.shape == () and sums.shape == (2,)
    bits_equal(np.concatenate([loss.cpu().numpy().reshape(1), sums.cpu().numpy()]), r["out"], "out of the public call")
    dz, dbias = ops.vertex_head_loss_grad(*args, k, s, instance=inst, sigma=sigma)
    bits_equal(dz.cpu().numpy(), r["dz"], "dz")
    check_dbias(dbias.cpu().numpy(), r)
    bits_equal(dbias.cpu().numpy(), q["dbias"], "dbias against the restated order")
    if nk[1] == "empty":
        assert float(loss) == 0.0 and not dz.cpu().numpy().any() and not dbias.cpu().numpy().any()
        assert np.isfinite(out.cpu().numpy()).all()
    else:
        assert float(loss) > 0 and dz.cpu().numpy().any()


@pytest.mark.parametrize("nk", R.case_ids(), ids=IDS)
def test_autograd_equals_the_unfused_composition_on_the_gpu(gpu, nk):
    """Upstream 5.0 (VERTEX_W): loss and z.grad of ops.vertex_head_loss against
    ops.smooth_l1_loss_vertex_gt(ops.deconv_bilinear(z, k, s) + bias, ...) bit for bit, both on the GPU. bias.grad: every
    term is now a rounded product g * 5, 2^-24 relative each, on top of the float64 sum's bound."""
    import torch
    from posecnn_amd import ops
    c = R.case(*nk)
    k, s, sigma = c["k"], c["s"], c["sigma"]
    (z, bias, label, obj), inst = _inputs(gpu, c)
    grads = []
    for fused in (True, False):
        zz, bb = z.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        with torch.enable_grad():
            if fused:
                loss = ops.vertex_head_loss(zz, bb, label, obj, k, s, instance=inst, sigma=sigma)[0]
            else:
                loss = ops.smooth_l1_loss_vertex_gt(ops.deconv_bilinear(zz, k, s) + bb, label, obj, instance=inst, sigma=sigma)
            assert loss.requires_grad
            (loss * VERTEX_W).backward()
        grads.append((loss.detach().cpu().numpy().reshape(1), zz.grad.cpu().numpy(), bb.grad.cpu().numpy()))
    bits_equal(grads[0][0], grads[1][0], "loss")
    bits_equal(grads[0][1], grads[1][1], "z.grad")
    assert np.isfinite(grads[0][2]).all()
    check_dbias(grads[0][2], R.reference(c), scale=VERTEX_W, extra=2.0 ** -24)


# ---- memory contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_memory_contract(gpu, name):
    """Both poison patterns and guard bands of tests/memguard.py, as tests/test_gpu_label_loss.py::test_memory_contract: identical
    outputs, inputs and guards intact, a workspace of exactly the declared size whose prior contents (0xFF bytes = NaN
    partials under P1, zero bytes under P2) do not matter. Nothing of size [B,H s,W s,3C] is allocated."""
    from test_gpu_memory_contract import Case, execute
    c = R.case(name, "mixed")
    r = R.reference(c)
    k, s = c["k"], c["s"]

    def make():
        return {key: np.array(c[key]) for key in ("z", "bias", "label", "objects", "instance")}

    def run(ctx):
        from posecnn_amd import ops
        z, bias, label, obj, inst = (ctx.e(key) for key in ("z", "bias", "label", "objects", "instance"))
        n0 = len(ctx.g.arenas)
        out = ops._vertex_head_loss_raw(z, bias, label, obj, k, s, inst)
        dz, dbias = ops.vertex_head_loss_grad(z, bias, label, obj, k, s, instance=inst, out=out)
        made = ctx.g.arenas[n0:]
        assert len(made) == 4, [a.describe() for a in made]        # workspace, out, dz, dbias
        assert max(a.nbytes for a in made if a.dtype != ops.torch.uint8) == z.numel() * 4
        dz1, dbias1 = ops.vertex_head_loss_grad(z, bias, label, obj, k, s, instance=inst)   # runs its own forward
        return dict(out=out, dz=dz, dbias=dbias, dz1=dz1, dbias1=dbias1)

    def check(d, o):
        bits_equal(o["out"], r["out"], "out")
        bits_equal(o["dz"], r["dz"], "dz")
        bits_equal(o["dz1"], r["dz"], "dz, forward run inside")
        check_dbias(o["dbias"], r)
        bits_equal(o["dbias"], _restated(name, "mixed")["dbias"], "dbias")
        bits_equal(o["dbias1"], o["dbias"], "dbias, forward run inside")

    execute(Case("vertex_head_loss " + name,
                 ("pcnn_vertex_head_loss_workspace_bytes", "pcnn_vertex_head_loss_fwd", "pcnn_vertex_head_loss_bwd"), make, run, check))


def test_two_streams_give_identical_bits(gpu):
    import torch
    from posecnn_amd import ops
    c = R.case("C", "mixed")
    (z, bias, label, obj), inst = _inputs(gpu, c)
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        stream = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(stream):
            zz, bb = z.clone().requires_grad_(True), bias.clone().requires_grad_(True)
            with torch.enable_grad():
                loss = ops.vertex_head_loss(zz, bb, label, obj, c["k"], c["s"], instance=inst)[0]
                loss.backward()
        stream.synchronize()
        runs.append([t.detach().cpu().numpy().reshape(-1) for t in (loss, bb.grad, zz.grad)])
    for what, a, b in zip(("loss", "dbias", "dz"), *runs):
        bits_equal(a, b, what + " on two streams")
    assert runs[0][0][0] > 0 and runs[0][2].any()


# ---- the training graph ------------------------------------------------------------------------------------------------
def _net(gpu, lowres, fused, variables=None, **kw):
    from posecnn_amd.networks import vgg16_convs
    kw = dict(dict(trainable=True, is_train=True), **kw)
    net = vgg16_convs("COLOR", grad_ref.NUM_CLASSES, grad_ref.NUM_UNITS, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True,
                      device=gpu, seed=3, init="he", lowres_train_heads=lowres, fused_vertex_loss=fused, **kw)
    if variables is not None:
        net.vars = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in variables.items()}
    return net


COMMON = ["data", "gt_label_2d", "poses", "extents", "meta_data", "points", "symmetry"]


def _feeds(gpu, seed=grad_ref.GRAPH_SEED):
    """-> (numpy feed with dense targets, dense-target feed, object-table feed, planted)"""
    feed_np = grad_ref.dense_vertex_feed(grad_ref.graph_feed(seed))
    dense = {k: T(gpu, feed_np[k]) for k in COMMON + ["vertex_targets", "vertex_weights"]}
    table = {k: T(gpu, feed_np[k]) for k in COMMON + ["vertex_objects"]}
    dense["keep_prob"] = table["keep_prob"] = 1.0
    planted = {k: T(gpu, v) for k, v in feed_np["planted"].items()}
    return feed_np, dense, table, planted


def test_whole_graph_gradients_equal_float64(gpu, capsys):
    """vgg16_convs(lowres_train_heads=True, fused_vertex_loss=True) fed the object table, + train.build_losses + backward at
    grad_ref.GRAPH_SHAPE, against float64 autograd of grad_ref.training_loss64 — the restatement of the LITERAL graph on the
    dense targets of the same table — under the criterion of tests/test_gpu_gradients.py. The discrete outputs must equal
    the literal graph's element for element, and vertex_pred must not have been built by the step."""
    import torch
    from posecnn_amd import networks, ops, synth, train
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    feed_np, dense, table, planted = _feeds(gpu)
    literal = _net(gpu, False, False)
    synth.init_calibrated(literal)
    with torch.enable_grad():
        literal.run(dense, planted=planted)
        lit_losses = {k: float(v.detach()) for k, v in train.build_losses(literal).items()}
    assert not literal.fused_heads and not literal.lowres_train_heads and not literal.fused_vertex_loss
    discrete = ("label_2d", "rois", "poses_target", "poses_weight")
    lit = {k: literal.get_output(k).detach().cpu().numpy() for k in discrete + ("gt_label_weight",)}

    net = _net(gpu, True, True, literal.vars)
    with torch.enable_grad():
        net.run(table, planted=planted)
        losses = train.build_losses(net)
        losses["loss"].backward()
    torch.cuda.synchronize()
    assert net.lowres_train_heads and net.fused_vertex_loss and "loss_vertex_sl1" in net.layers
    assert isinstance(net.layers["vertex_pred"], networks._Lazy)                     # the step never built it
    assert sorted(net.vars) == sorted(literal.vars) and all(v.requires_grad for v in net.vars.values()) and len(net.vars) == 44
    for k in discrete:
        got = net.get_output(k).detach().cpu().numpy()
        assert got.shape == lit[k].shape and np.array_equal(got, lit[k]), k
    got = {k: float(v.detach()) for k, v in losses.items()}
    consts = {k: lit[k] for k in ("rois", "poses_target", "poses_weight", "gt_label_weight")}
    g64, l64 = grad_ref.grads_of(grad_ref.vars_from_net(net.vars, torch.float64), feed_np, consts, train.TrainConfig)
    g32, l32 = grad_ref.grads_of(grad_ref.vars_from_net(net.vars, torch.float32), feed_np, consts, train.TrainConfig)
    floor = {k: grad_ref.rel_err(g32[k], g64[k]) for k in g64}
    err = {k: grad_ref.rel_err(net.vars[k].grad, g64[k]) for k in g64}
    lfloor = {k: abs(l32[k] - l64[k]) / abs(l64[k]) for k in l64}
    lerr = {k: abs(got[k] - l64[k]) / abs(l64[k]) for k in l64}
    with capsys.disabled():
        print("\ntraining graph, lowres_train_heads=True, fused_vertex_loss=True")
        print("%-28s %10s %10s %10s" % ("variable", "err", "floor", "bound"))
        for k in sorted(err):
            print("%-28s %10.2e %10.2e %10.2e" % (k, err[k], floor[k], grad_ref.bound(floor[k])))
        for k in sorted(lerr):
            print("%-28s %10.2e %10.2e %10.2e   (%.9g, literal graph %.9g)" % (k, lerr[k], lfloor[k], grad_ref.bound(lfloor[k]), got[k], lit_losses[k]))
    assert sorted(err) == sorted(net.vars) and len(err) == 44
    for k in sorted(floor):
        assert floor[k] <= grad_ref.FLOOR_CAP, (k, floor[k])
    bad = {k: (err[k], grad_ref.bound(floor[k])) for k in err if not err[k] <= grad_ref.bound(floor[k])}
    assert not bad, bad
    assert min(got[k] for k in ("loss_cls", "loss_vertex", "loss_pose")) > 0
    for k in lerr:
        assert lerr[k] <= grad_ref.bound(lfloor[k]), (k, got[k], l64[k])
    # fetched afterwards, it is the interpolation of the field the loss saw
    zv, bv = net.get_output("vertex_pred_lowres"), net.get_output("vertex_pred_bias")
    assert not zv.requires_grad and not bv.requires_grad
    vp = net.get_output("vertex_pred")
    assert isinstance(vp, torch.Tensor) and tuple(vp.shape) == (2, 96, 128, 66) and not vp.requires_grad
    assert torch.equal(vp, ops.deconv_bilinear(zv, 16, 8, bias=bv)) and net.layers["vertex_pred"] is vp


def _table_feed(gpu, seed):
    feed_np = grad_ref.graph_feed(seed, shape=(1, 96, 128), n_obj=2)
    feed = {k: T(gpu, feed_np[k]) for k in COMMON + ["vertex_objects"]}
    feed["keep_prob"] = 1.0
    return feed


def test_solver_steps_and_snapshots_cross_the_switch(gpu):
    import torch
    from posecnn_amd import train
    torch.manual_seed(0)
    feed = _table_feed(gpu, 77)

    class Cfg(train.TrainConfig):
        LEARNING_RATE = 1e-6

    on, off = _net(gpu, True, True), _net(gpu, True, False)
    solver = train.SolverWrapper(on, Cfg)
    for _ in range(3):
        step = solver.train_step(feed)
        assert sorted(step) == ["loss", "loss_cls", "loss_pose", "loss_regu", "loss_vertex"]
        assert all(np.isfinite(v) for v in step.values()) and step["loss_vertex"] > 0, step
        assert "loss_vertex_sl1" in on.layers
    for k, v in on.vars.items():
        assert v.requires_grad and v.grad is not None and torch.isfinite(v.grad).all(), k
    assert float(on.vars["vertex_pred/weights"].grad.abs().max()) > 0 and float(on.vars["vertex_pred/biases"].grad.abs().max()) > 0
    path = os.path.join(tempfile.mkdtemp(), "snap.pt")
    solver.snapshot(path)
    other = train.SolverWrapper(off, Cfg)
    first_off = other.train_step(feed)              # creates the unfused graph's variables: the same names
    assert sorted(off.vars) == sorted(on.vars) and "loss_vertex_sl1" not in off.layers
    other.restore(path)
    assert other.iter == 3 and all(torch.equal(off.vars[k], on.vars[k]) for k in on.vars)
    assert all(np.isfinite(v) for v in other.train_step(feed).values()) and np.isfinite(first_off["loss"])
    other.snapshot(path)                            # and back
    solver.restore(path)
    assert solver.iter == 4 and all(torch.equal(off.vars[k], on.vars[k]) for k in on.vars)
    assert all(np.isfinite(v) for v in solver.train_step(feed).values())


def test_the_switch_is_inert_where_it_does_not_apply(gpu):
    """Without lowres_train_heads, with a dense-target feed, and in inference graphs: the layers of today's graph."""
    import torch
    feed_np, dense, table, planted = _feeds(gpu)
    situations = (("without lowres_train_heads", dict(lowres=False), table, torch.enable_grad),
                  ("dense-target feed", dict(lowres=True), dense, torch.enable_grad),
                  ("inference graph", dict(lowres=True, trainable=False, is_train=False), table, torch.no_grad),
                  ("frozen training graph", dict(lowres=True, trainable=False, is_train=True), table, torch.no_grad))
    for what, kw, feed, mode in situations:
        lowres = kw.pop("lowres")
        a, b = _net(gpu, lowres, False, **kw), _net(gpu, lowres, True, **kw)
        with mode():
            a.run(feed, planted=planted)
            b.run(feed, planted=planted)
        assert sorted(a.layers) == sorted(b.layers) and "loss_vertex_sl1" not in b.layers, what
        assert type(a.layers["vertex_pred"]) is type(b.layers["vertex_pred"]), what
        if kw.get("trainable", True):
            assert isinstance(b.layers["vertex_pred"], torch.Tensor) and b.layers["vertex_pred"].requires_grad, what
        assert torch.equal(a.get_output("label_2d"), b.get_output("label_2d")) and torch.equal(a.get_output("rois"), b.get_output("rois")), what
