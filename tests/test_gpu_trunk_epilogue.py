"""The trunk's training epilogues on the GPU (include/posecnn_hip_trunk_train.h, ops.bias_relu_train_,
ops.bias_relu_pool2_train, vgg16_convs(fused_train_epilogue=True)).

The kernels are compared bit for bit with tests/trunk_epilogue_ref.py — pooled, act, sel, dy and, its order being written
down, dbias — which tests/test_trunk_epilogue_cpu.py holds to float64 autograd. The shapes are the smallest at which each
path can go wrong: one window; C = 3 and 5 (scalar loads); C = 64, 68 and 66 (one full chunk of channels, a second partial
one on either load path); 127 / 128 / 129 pixels (one below, at and one above a workgroup's run of the dbias partition);
257 runs (more partials than the finishing workgroup has threads); every one again with all pointers 4 bytes off a 16-byte
boundary. Against the framework composition on the GPU: outputs and dy bit for bit on tie-free inputs, dbias within
2^-24 |S64| + 2^-30 sum |dy| of the float64 sum.
"""
import functools
import os
import tempfile

import numpy as np
import pytest

import grad_ref
import trunk_epilogue_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
# (B, H, W, C); windows = B H W / 4
SHAPES = ((1, 2, 2, 4), (1, 2, 2, 3), (2, 4, 6, 5), (2, 6, 4, 64), (2, 4, 4, 68), (1, 4, 4, 66),
          (1, 2, 254, 4), (1, 2, 256, 4), (1, 2, 258, 4), (1, 258, 510, 4))
ROWS = ((127, 4), (128, 4), (129, 4), (129, 5), (40, 68), (32769, 4), (257 * 128 + 1, 3))


def T(gpu, a, offset=False):
    """-> a device copy of `a`; `offset`: starting 4 bytes past a 16-byte boundary, so that the scalar paths run"""
    import torch
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.from_numpy(a.copy()).to(gpu)
    step = 4 // a.dtype.itemsize
    buf = torch.empty(a.size + step, dtype=torch.from_numpy(a[:0].copy()).dtype, device=gpu)
    view = buf[step:].view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def N(t):
    return t.detach().cpu().numpy()


def bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint32 if got.dtype.itemsize == 4 else np.uint8) != want.view(np.uint32 if want.dtype.itemsize == 4 else np.uint8)
    assert not bad.any(), "%s: %d of %d differ, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][:3], want[bad][:3])


def check_dbias(dbias, dy):
    s, tol = R.dbias_bound(dy)
    got = np.asarray(dbias, np.float64)
    assert np.isfinite(got).all() and (np.abs(got - s) <= tol).all(), (got, s, tol)


@functools.lru_cache(maxsize=None)
def _pool_case(shape, relu):
    y, bias = R.edge_input(shape, 7)
    dpooled, dact = R.grads(shape, 7)
    pooled, sel, act = R.pool_forward(y, bias, relu)
    c = dict(y=y, bias=bias, dpooled=dpooled, dact=dact, pooled=pooled, sel=sel, act=act)
    c["dy"], c["dbias"] = R.pool_backward(dpooled, sel)
    if relu:
        c["dy2"], c["dbias2"] = R.pool_backward(dpooled, sel, dact, act)
    for v in c.values():
        v.setflags(write=False)
    return c


# ---- the kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset4"))
@pytest.mark.parametrize("relu", (1, 0))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_pooled_kernels_bit_for_bit(gpu, shape, relu, offset):
    from posecnn_amd import ops
    c = _pool_case(shape, relu)
    assert c["sel"][0, 0, 0, 0] == 0 and c["pooled"][0, 0, 0, 0] == 1025.0          # the bias-induced tie is in
    y, bias = T(gpu, c["y"], offset), T(gpu, c["bias"], offset)
    act, pooled, sel = ops._bias_relu_pool2_train_raw(y, bias, relu)                 # pooled only: y is left alone
    assert act is None and sel.dtype.itemsize == 1
    bits_equal(N(y), c["y"], "y after the pooled-only forward")
    bits_equal(N(pooled), c["pooled"], "pooled")
    bits_equal(N(sel), c["sel"], "sel")
    bits_equal(N(pooled), N(ops.bias_relu_pool2(y, bias, relu)), "pooled against pcnn_bias_relu_pool2_fwd")
    want_act = N(ops.bias_act_(y.clone(), bias, relu))
    act, pooled2, sel2 = ops._bias_relu_pool2_train_raw(y, bias, relu, want_act=True)   # act aliases y
    assert act.data_ptr() == y.data_ptr()
    bits_equal(N(act), c["act"], "act")
    bits_equal(N(act), want_act, "act against pcnn_bias_act_fwd")
    bits_equal(N(pooled2), c["pooled"], "pooled of the dual form")
    bits_equal(N(sel2), c["sel"], "sel of the dual form")
    # backward
    dpooled, sel_in = T(gpu, c["dpooled"], offset), T(gpu, c["sel"], offset)
    dy, dbias = ops.bias_relu_pool2_train_grad(dpooled, sel_in)
    bits_equal(N(dy), c["dy"], "dy")
    bits_equal(N(dbias), c["dbias"], "dbias")
    check_dbias(N(dbias), c["dy"])
    dy, none = ops.bias_relu_pool2_train_grad(dpooled, sel_in, want_dbias=False)
    assert none is None
    bits_equal(N(dy), c["dy"], "dy without dbias")
    if relu:
        dy, dbias = ops.bias_relu_pool2_train_grad(dpooled, sel_in, T(gpu, c["dact"], offset), act)
        bits_equal(N(dy), c["dy2"], "dy of the dual form")
        bits_equal(N(dbias), c["dbias2"], "dbias of the dual form")
        check_dbias(N(dbias), c["dy2"])


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset4"))
@pytest.mark.parametrize("relu", (1, 0))
@pytest.mark.parametrize("rc", ROWS, ids=str)
def test_unpooled_backward_bit_for_bit(gpu, rc, relu, offset):
    from posecnn_amd import ops
    rows, C = rc
    rng = np.random.default_rng(rows + C)
    y = np.where(rng.random((rows, C)) < 0.5, rng.integers(-8, 9, (rows, C)) / 4.0, rng.standard_normal((rows, C))).astype(F)
    bias = (rng.integers(-4, 5, C) / 4.0).astype(F)
    da = rng.standard_normal((rows, C)).astype(F)
    a_ref = R.bias_act(y, bias, relu)
    assert not relu or (a_ref == 0).sum() > 0
    a = ops.bias_act_(T(gpu, y, offset), T(gpu, bias), relu)
    bits_equal(N(a), a_ref, "a")
    want_dy, want_db = R.backward(da, a_ref, relu)
    dy, dbias = ops.bias_relu_train_grad(T(gpu, da, offset), a if relu else None, relu)
    bits_equal(N(dy), want_dy, "dy")
    bits_equal(N(dbias), want_db, "dbias")
    check_dbias(N(dbias), want_dy)
    dy, none = ops.bias_relu_train_grad(T(gpu, da, offset), a, relu, want_dbias=False)
    assert none is None
    bits_equal(N(dy), want_dy, "dy without dbias")


# ---- autograd against the framework composition --------------------------------------------------------------------------
def _composition(torch, y, bias, relu, dpooled, dact):
    import torch.nn.functional as Fn
    x = y.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True)
    a = x + b
    a = Fn.relu(a) if relu else a
    p = Fn.max_pool2d(a.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    loss = (p * dpooled).sum()
    if dact is not None:
        loss = loss + (a * dact).sum()
    loss.backward()
    return p.detach(), a.detach(), x.grad, b.grad


@pytest.mark.parametrize("layout", ("nhwc", "channels_last"))
@pytest.mark.parametrize("form", ("pooled", "pooled_norelu", "dual", "unpooled", "unpooled_norelu", "frozen_bias"))
@pytest.mark.parametrize("shape", ((2, 6, 4, 64), (2, 4, 6, 5), (1, 2, 258, 4)), ids=str)
def test_autograd_equals_the_framework_composition(gpu, shape, form, layout):
    import torch
    from posecnn_amd import ops
    relu = not form.endswith("norelu")
    y_np, bias_np = R.tie_free(shape, 23)
    dpooled_np, dact_np = R.grads(shape, 23)
    y0, bias0, dpooled, dact = T(gpu, y_np), T(gpu, bias_np), T(gpu, dpooled_np), T(gpu, dact_np)
    if form.startswith("unpooled"):
        dpooled = torch.zeros_like(dpooled)
    elif form != "dual":
        dact = None
    want_p, want_a, want_dy, want_db = _composition(torch, y0, bias0, relu, dpooled, dact)
    leaf = y0.clone().requires_grad_(True)
    bias = bias0.clone().requires_grad_(form != "frozen_bias")
    with torch.enable_grad():
        if layout == "channels_last":
            y = leaf.permute(0, 3, 1, 2) * 1.0             # [B,C,H,W] over NHWC memory, as a framework convolution returns it
            assert ops._channels_first(y) and not y._is_view()
        else:
            y = leaf * 1.0
        back = (lambda t: t.permute(0, 2, 3, 1)) if layout == "channels_last" else (lambda t: t)
        if form.startswith("unpooled"):
            a = ops.bias_relu_train_(y, bias, relu)
            assert a is y or a.data_ptr() == y.data_ptr()
            bits_equal(N(back(a).contiguous()), N(want_a), "act")
            (back(a) * dact).sum().backward()
        elif form == "dual":
            a, p = ops.bias_relu_pool2_train(y, bias, relu, want_act=True)
            assert a.data_ptr() == y.data_ptr()
            bits_equal(N(back(a).contiguous()), N(want_a), "act")
            bits_equal(N(back(p).contiguous()), N(want_p.contiguous()), "pooled")
            ((back(p) * dpooled).sum() + (back(a) * dact).sum()).backward()
        else:
            p = ops.bias_relu_pool2_train(y, bias, relu)
            assert isinstance(p, torch.Tensor)
            bits_equal(N(back(p).contiguous()), N(want_p.contiguous()), "pooled")
            (back(p) * dpooled).sum().backward()
    bits_equal(N(leaf.grad), N(want_dy), "dy")
    if form == "frozen_bias":
        assert bias.grad is None
    else:
        check_dbias(N(bias.grad), N(want_dy))


# ---- memory contract -----------------------------------------------------------------------------------------------------
def test_forward_allocates_pooled_and_sel_and_nothing_else(gpu):
    import torch
    from posecnn_amd import ops
    shape = (2, 8, 16, 64)                                            # y 64 KiB, pooled 16 KiB, sel 4 KiB: multiples of 512 bytes
    y_np, bias_np = R.tie_free(shape, 1)
    leaf, bias = T(gpu, y_np).requires_grad_(True), T(gpu, bias_np).requires_grad_(True)
    with torch.enable_grad():
        y = leaf * 1.0
        ops.bias_relu_pool2_train(y.detach().clone(), bias)            # (anything the first call sets up is behind us)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(gpu)
        p = ops.bias_relu_pool2_train(y, bias)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated(gpu) - before == p.numel() * 4 + p.numel()
        saved = p.grad_fn.saved_tensors
        assert [s.dtype for s in saved] == [torch.uint8] and saved[0].numel() == p.numel()
        assert all(s.numel() < y.numel() for s in saved)              # nothing of full resolution is kept
        before = torch.cuda.memory_allocated(gpu)
        a = ops.bias_relu_train_(y, bias)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated(gpu) == before and a.data_ptr() == y.data_ptr()
        assert [s.data_ptr() for s in a.grad_fn.saved_tensors] == [y.data_ptr()]
        y2 = leaf * 2.0
        before = torch.cuda.memory_allocated(gpu)
        a2, p2 = ops.bias_relu_pool2_train(y2, bias, want_act=True)   # the dual form: act is y's storage
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated(gpu) - before == p2.numel() * 5
        assert sorted(s.data_ptr() for s in p2.grad_fn.saved_tensors if s.dtype == torch.float32) == [y2.data_ptr()]


@pytest.mark.parametrize("shape", ((2, 6, 4, 64), (2, 4, 6, 5), (1, 2, 258, 4), (1, 4, 4, 66)), ids=str)
def test_guard_bands_and_poisoned_outputs(gpu, monkeypatch, shape):
    """tests/memguard.py: every allocation of the ops between two guard bands, outputs and workspace poisoned with two
    patterns. No store outside an output or the workspace, no input written (but y, by contract, in the dual form), and no
    output element that depends on what the memory held."""
    import torch
    import memguard
    from posecnn_amd import ops
    c = _pool_case(shape, 1)
    runs = {}
    for pattern in memguard.PATTERNS:
        g = memguard.GuardedTorch(pattern)
        monkeypatch.setattr(ops, "torch", g)
        monkeypatch.setattr(ops, "_default_ws", {})          # (a workspace of this pattern, between guards)
        y, bias, dpooled, dact = (g.embed(np.array(c[k]), gpu) for k in ("y", "bias", "dpooled", "dact"))   # (copies: the cases are read-only)
        _, pooled, sel = ops._bias_relu_pool2_train_raw(y, bias, 1)
        dy, dbias = ops.bias_relu_pool2_train_grad(dpooled, sel)
        y2 = g.embed(np.array(c["y"]), gpu, mutable=True)
        act, pooled2, sel2 = ops._bias_relu_pool2_train_raw(y2, bias, 1, want_act=True)
        dy2, dbias2 = ops.bias_relu_pool2_train_grad(dpooled, sel2, dact, act)
        dy3, dbias3 = ops.bias_relu_train_grad(dact, act, True)
        torch.cuda.synchronize()
        g.check()
        assert len(g.arenas) >= 5 + 10 + 1                   # the inputs, the outputs, the workspace
        runs[pattern] = {k: memguard.to_numpy(v) for k, v in dict(
            pooled=pooled, sel=sel, dy=dy, dbias=dbias, act=act, pooled2=pooled2, sel2=sel2, dy2=dy2, dbias2=dbias2, dy3=dy3,
            dbias3=dbias3).items()}
    memguard.compare_patterns(runs)
    for k in ("pooled", "sel", "dy", "dbias", "act"):
        bits_equal(runs["P2"][k], c[k], k)
    bits_equal(runs["P2"]["dy2"], c["dy2"], "dy of the dual form")
    bits_equal(runs["P2"]["dbias2"], c["dbias2"], "dbias of the dual form")


# ---- streams -------------------------------------------------------------------------------------------------------------
def test_two_streams_give_identical_bits(gpu):
    import torch
    from posecnn_amd import ops
    shape = (1, 258, 510, 4)
    c = _pool_case(shape, 1)
    y0, bias0, dpooled, dact = (T(gpu, c[k]) for k in ("y", "bias", "dpooled", "dact"))
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        stream = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(stream):
            leaf, bias = y0.clone().requires_grad_(True), bias0.clone().requires_grad_(True)
            with torch.enable_grad():
                a, p = ops.bias_relu_pool2_train(leaf * 1.0, bias, want_act=True)
                q = ops.bias_relu_pool2_train(a, bias)
                ((p * dpooled).sum() + (a * dact).sum() + q.sum()).backward()
        stream.synchronize()
        runs.append([N(t).reshape(-1) for t in (p, a, q, leaf.grad, bias.grad)])
    for what, u, v in zip(("pooled", "act", "pooled of act", "dy", "dbias"), *runs):
        bits_equal(u, v, what + " on two streams")
    bits_equal(runs[0][0], c["pooled"].reshape(-1), "pooled")


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_validation_with_real_buffers(gpu):
    import torch
    from posecnn_amd import ops
    bias = torch.zeros(4, device=gpu)
    for bad in ((1, 3, 4, 4), (1, 4, 3, 4)):
        with pytest.raises(ValueError):
            ops.bias_relu_pool2_train(torch.zeros(bad, device=gpu), bias)
        with pytest.raises(ValueError):
            ops._bias_relu_pool2_train_raw(torch.zeros(bad, device=gpu), bias)
    y = torch.zeros((1, 4, 4, 4), device=gpu)
    for wrong in (torch.zeros(3, device=gpu), torch.zeros(5, device=gpu), torch.zeros((1, 4), device=gpu)):
        with pytest.raises(ValueError):
            ops.bias_relu_pool2_train(y, wrong)
        with pytest.raises(ValueError):
            ops.bias_relu_train_(y, wrong)
    with pytest.raises(ValueError):
        ops.bias_relu_pool2_train(y, bias, relu=False, want_act=True)
    with pytest.raises(ValueError):
        ops.bias_relu_pool2_train_grad(torch.zeros((1, 2, 2, 4), device=gpu), torch.zeros((1, 2, 2, 4), dtype=torch.uint8, device=gpu),
                                       dact=torch.zeros((1, 4, 4, 4), device=gpu))
    with pytest.raises(ValueError):
        ops.bias_relu_train_grad(torch.zeros((4, 4), device=gpu), torch.zeros((4, 5), device=gpu))
    with pytest.raises(RuntimeError):
        ops.bias_relu_pool2_train(torch.zeros((1, 4, 4, 4)), bias)     # a CPU tensor: there is no CPU path
    assert not y.any()
    # the C entries themselves: the workspace rules of the header, nothing launched on a refusal
    import ctypes
    from posecnn_amd import _lib
    L = _lib.lib()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rows, C = 130, 4
    da = torch.ones((rows, C), device=gpu)
    dy, db = torch.full_like(da, 7.0), torch.full((C,), 7.0, device=gpu)
    ws = torch.zeros(512, dtype=torch.uint8, device=gpu)
    need = ctypes.c_size_t(0)
    assert L.pcnn_bias_relu_train_workspace_bytes(rows, C, ctypes.byref(need)) == _lib.PCNN_OK and need.value == 2 * C * 8
    assert L.pcnn_bias_relu_pool2_train_workspace_bytes(1, 2, 2 * rows, C, ctypes.byref(need)) == _lib.PCNN_OK and need.value == 2 * C * 8
    assert L.pcnn_bias_relu_pool2_train_workspace_bytes(1, 3, 4, C, ctypes.byref(need)) == _lib.PCNN_EINVAL
    call = lambda dbias, w, nbytes: L.pcnn_bias_relu_train_bwd(P(da), P(da), rows, C, 1, P(dy), dbias, w, nbytes, None)
    assert call(P(db), P(ws), need.value - 1) == _lib.PCNN_EWORKSPACE
    assert call(P(db), None, need.value) == _lib.PCNN_EWORKSPACE
    assert call(P(db), P(ws, 8), need.value) == _lib.PCNN_EINVAL
    assert L.pcnn_bias_relu_train_bwd(None, P(da), rows, C, 1, P(dy), P(db), P(ws), need.value, None) == _lib.PCNN_ENULL
    assert L.pcnn_bias_relu_train_bwd(P(da), P(da), 0, C, 1, P(dy), P(db), P(ws), need.value, None) == _lib.PCNN_EINVAL
    torch.cuda.synchronize()
    assert bool((dy == 7).all()) and bool((db == 7).all())              # nothing ran
    assert call(None, None, 0) == _lib.PCNN_OK                           # without dbias no workspace is needed
    assert call(P(db), P(ws), need.value) == _lib.PCNN_OK
    torch.cuda.synchronize()
    assert bool((dy == 1).all()) and bool((db == rows).all())


# ---- the training graph ----------------------------------------------------------------------------------------------------
def _net(gpu, lowres, fused, epilogue, variables=None, **kw):
    from posecnn_amd.networks import vgg16_convs
    kw = dict(dict(trainable=True, is_train=True), **kw)
    net = vgg16_convs("COLOR", grad_ref.NUM_CLASSES, grad_ref.NUM_UNITS, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True,
                      device=gpu, seed=3, init="he", lowres_train_heads=lowres, fused_vertex_loss=fused,
                      fused_train_epilogue=epilogue, **kw)
    if variables is not None:
        net.vars = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in variables.items()}
    return net


COMMON = ["data", "gt_label_2d", "poses", "extents", "meta_data", "points", "symmetry"]
DISCRETE = ("label_2d", "rois", "poses_target", "poses_weight")


def _feeds(gpu, seed=grad_ref.GRAPH_SEED):
    feed_np = grad_ref.dense_vertex_feed(grad_ref.graph_feed(seed))
    dense = {k: T(gpu, feed_np[k]) for k in COMMON + ["vertex_targets", "vertex_weights"]}
    table = {k: T(gpu, feed_np[k]) for k in COMMON + ["vertex_objects"]}
    dense["keep_prob"] = table["keep_prob"] = 1.0
    planted = {k: T(gpu, v) for k, v in feed_np["planted"].items()}
    return feed_np, dense, table, planted


_GRAPH = {}


def _graph_reference(gpu):
    """Once for both whole-graph tests: the literal graph with the switch off, its discrete outputs, and the float64 /
    float32 restatements' gradients and losses (tests/grad_ref.py) for its variables."""
    if not _GRAPH:
        import torch
        from posecnn_amd import synth, train
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False
        feed_np, dense, table, planted = _feeds(gpu)
        literal = _net(gpu, False, False, False)
        synth.init_calibrated(literal)
        with torch.enable_grad():
            literal.run(dense, planted=planted)
            train.build_losses(literal)
        assert not literal.fused_train_epilogue
        lit = {k: N(literal.get_output(k)) for k in DISCRETE + ("gt_label_weight",)}
        consts = {k: lit[k] for k in ("rois", "poses_target", "poses_weight", "gt_label_weight")}
        g64, l64 = grad_ref.grads_of(grad_ref.vars_from_net(literal.vars, torch.float64), feed_np, consts, train.TrainConfig)
        g32, l32 = grad_ref.grads_of(grad_ref.vars_from_net(literal.vars, torch.float32), feed_np, consts, train.TrainConfig)
        _GRAPH.update(vars=literal.vars, lit=lit, g64=g64, l64=l64, g32=g32, l32=l32, dense=dense, table=table, planted=planted)
    return _GRAPH


@pytest.mark.parametrize("heads", ("switch_alone", "with_lowres_heads_and_fused_vertex_loss"))
def test_whole_graph_gradients_equal_float64(gpu, capsys, heads, monkeypatch):
    """vgg16_convs(fused_train_epilogue=True) + train.build_losses + backward at grad_ref.GRAPH_SHAPE against float64 autograd
    of grad_ref.training_loss64 under the criterion of tests/test_gpu_gradients.py; the discrete outputs equal those of the
    graph with the switch off; every biased convolution went through the new ops."""
    import torch
    from posecnn_amd import ops, train
    G = _graph_reference(gpu)
    lowres = heads != "switch_alone"
    calls = {"act": 0, "pool": 0, "dual": 0}
    real_act, real_pool = ops.bias_relu_train_, ops.bias_relu_pool2_train

    def count_act(y, bias, relu=True):
        calls["act"] += 1
        return real_act(y, bias, relu)

    def count_pool(y, bias, relu=True, want_act=False):
        calls["dual" if want_act else "pool"] += 1
        return real_pool(y, bias, relu, want_act)

    monkeypatch.setattr(ops, "bias_relu_train_", count_act)
    monkeypatch.setattr(ops, "bias_relu_pool2_train", count_pool)
    net = _net(gpu, lowres, lowres, True, G["vars"])
    assert net.fused_train_epilogue and net.lowres_train_heads == lowres
    with torch.enable_grad():
        net.run(G["table"] if lowres else G["dense"], planted=G["planted"])
        losses = train.build_losses(net)
        losses["loss"].backward()
    torch.cuda.synchronize()
    # 13 trunk layers: 3 conv -> pool pairs, conv4_3 dual, 9 others; + score_conv5 / score_conv4 [+ their vertex twins]
    # [+ the literal heads' full-resolution score and vertex_pred]
    assert calls["pool"] == 3 and calls["dual"] == 1 and calls["act"] == (9 + 4 if lowres else 9 + 6), calls
    assert sorted(net.vars) == sorted(G["vars"]) and all(v.requires_grad for v in net.vars.values()) and len(net.vars) == 44
    for k in DISCRETE:
        got = N(net.get_output(k))
        assert got.shape == G["lit"][k].shape and np.array_equal(got, G["lit"][k]), k
    got = {k: float(v.detach()) for k, v in losses.items()}
    g64, l64, g32, l32 = G["g64"], G["l64"], G["g32"], G["l32"]
    floor = {k: grad_ref.rel_err(g32[k], g64[k]) for k in g64}
    err = {k: grad_ref.rel_err(net.vars[k].grad, g64[k]) for k in g64}
    lfloor = {k: abs(l32[k] - l64[k]) / abs(l64[k]) for k in l64}
    lerr = {k: abs(got[k] - l64[k]) / abs(l64[k]) for k in l64}
    with capsys.disabled():
        print("\ntraining graph, fused_train_epilogue=True, %s" % heads)
        print("%-28s %10s %10s %10s" % ("variable", "err", "floor", "bound"))
        for k in sorted(err):
            print("%-28s %10.2e %10.2e %10.2e" % (k, err[k], floor[k], grad_ref.bound(floor[k])))
        for k in sorted(lerr):
            print("%-28s %10.2e %10.2e %10.2e   (%.9g)" % (k, lerr[k], lfloor[k], grad_ref.bound(lfloor[k]), got[k]))
    assert sorted(err) == sorted(net.vars) and len(err) == 44
    for k in sorted(floor):
        assert floor[k] <= grad_ref.FLOOR_CAP, (k, floor[k])
    bad = {k: (err[k], grad_ref.bound(floor[k])) for k in err if not err[k] <= grad_ref.bound(floor[k])}
    assert not bad, bad
    assert min(got[k] for k in ("loss_cls", "loss_vertex", "loss_pose")) > 0
    for k in lerr:
        assert lerr[k] <= grad_ref.bound(lfloor[k]), (k, got[k], l64[k])


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

    on, off = _net(gpu, True, True, True), _net(gpu, True, True, False)
    solver = train.SolverWrapper(on, Cfg)
    for _ in range(2):
        step = solver.train_step(feed)
        assert sorted(step) == ["loss", "loss_cls", "loss_pose", "loss_regu", "loss_vertex"]
        assert all(np.isfinite(v) for v in step.values()) and step["loss_vertex"] > 0, step
    for k, v in on.vars.items():
        assert v.requires_grad and v.grad is not None and torch.isfinite(v.grad).all(), k
        if k.endswith("/biases"):
            assert float(v.grad.abs().max()) > 0, k
    path = os.path.join(tempfile.mkdtemp(), "snap.pt")
    solver.snapshot(path)
    other = train.SolverWrapper(off, Cfg)
    first_off = other.train_step(feed)              # creates the unfused graph's variables: the same names
    assert sorted(off.vars) == sorted(on.vars) and len(on.vars) == 44
    other.restore(path)
    assert other.iter == 2 and all(torch.equal(off.vars[k], on.vars[k]) for k in on.vars)
    assert all(np.isfinite(v) for v in other.train_step(feed).values()) and np.isfinite(first_off["loss"])
    other.snapshot(path)                            # and back
    solver.restore(path)
    assert solver.iter == 3 and all(torch.equal(off.vars[k], on.vars[k]) for k in on.vars)
    assert all(np.isfinite(v) for v in solver.train_step(feed).values())


def test_the_switch_is_inert_where_it_does_not_apply(gpu, monkeypatch):
    """Inference graphs, frozen graphs, graphs built with the constructor's default, runs without grad and CPU tensors keep
    today's composition: neither op is reached."""
    import torch
    from posecnn_amd import networks, ops

    def never(*a, **k):
        raise AssertionError("the training epilogue ran where the switch does not apply")

    monkeypatch.setattr(ops, "bias_relu_train_", never)
    monkeypatch.setattr(ops, "bias_relu_pool2_train", never)
    feed_np, dense, table, planted = _feeds(gpu)
    situations = (("inference graph", dict(epilogue=True, trainable=False, is_train=False), torch.no_grad, False),
                  ("frozen training graph", dict(epilogue=True, trainable=False, is_train=True), torch.no_grad, False),
                  ("constructor default", dict(epilogue=False), torch.enable_grad, False),
                  ("without grad", dict(epilogue=True), torch.no_grad, True))
    for what, kw, mode, flag in situations:
        epilogue = kw.pop("epilogue")
        if what == "constructor default":
            from posecnn_amd.networks import vgg16_convs
            net = vgg16_convs("COLOR", grad_ref.NUM_CLASSES, grad_ref.NUM_UNITS, (1.0,), 1.0, -1.0, vertex_reg_2d=True,
                              pose_reg=True, device=gpu, seed=3, init="he")
        else:
            net = _net(gpu, False, False, epilogue, **kw)
        ref = _net(gpu, False, False, False, **kw)
        assert net.fused_train_epilogue == flag, what
        feed = dense if mode is torch.enable_grad else table
        with mode():
            net.run(feed, planted=planted)
            ref.run(feed, planted=planted)
        assert sorted(net.layers) == sorted(ref.layers), what
        assert torch.equal(net.get_output("label_2d"), ref.get_output("label_2d")), what
    # CPU tensors, under grad, the switch on: the framework composition
    net = networks.Network(device="cpu", trainable=True).use_fused_train_epilogue()
    assert net.fused_train_epilogue and not networks.Network.fused_train_epilogue
    net.defer_act = frozenset(("c",))
    x = torch.from_numpy(R.tie_free((1, 4, 4, 3), 2)[0])
    with torch.enable_grad():
        net.layers = {"x": x}
        net.feed("x").conv(3, 3, 8, 1, 1, name="c").max_pool(2, 2, 2, 2, name="p").conv(1, 1, 4, 1, 1, name="d")
        out = net.get_output("d")
        assert tuple(out.shape) == (1, 2, 2, 4) and out.requires_grad
        out.sum().backward()
    assert all(v.grad is not None for v in net.vars.values())
