"""The kernels that include posecnn_amd/csrc/bilinear.h at every legal (kernel, stride) geometry of tests/bilinear_geometry.py:
the fixed deconv forward and backward, the label head (plain and hard), the low-resolution Hough source and the two
fused training losses. tests/test_bilinear_geometry_cpu.py holds the table's branch claims and the references; this file
runs the launches. tests/GEOMETRY.md has the table and what the first run showed.

No tolerance is new. What an existing test compares bit for bit is compared bit for bit here (the C oracle, pinned on the
CPU against float64 arithmetic the kernels never saw); the loss scalars and dbias go through the helpers of
tests/test_gpu_label_loss.py and tests/test_gpu_vertex_head.py, whose test functions are called with the new cases.
The deconv backward is also compared with float64 autograd exactly, as test_deconv_backward_equals_float64 does, where
that is possible: for the geometries whose taps are dyadic. The taps of (13, 13), (6, 2) and (5, 3) are thirds and
sevenths, rounded by float32: there is no exact float64 statement of them, and the oracle is the reference."""
import ctypes
import functools

import numpy as np
import pytest

import bilinear_geometry as G
import exact
import grad_ref
import label_loss_ref as LR
import oracle
import test_gpu_label_loss as TL
import test_gpu_vertex_head as TV
from posecnn_amd import config
from test_gpu_hough import compare as hough_compare, lowres_case
from test_gpu_training import same

pytestmark = pytest.mark.gpu
F = np.float32
CASE_IDS = [G.case_id(c) for c in G.cases()]
THRESHOLD = G.HEAD_THRESHOLD


def T(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)


def N(t):
    return t.cpu().numpy()


# ---- deconv --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deconv_case(c, C):
    k, s, w = c
    rng = np.random.default_rng([k, s, w, C])
    shape, out = (G.B, G.H_LOW, w, C), (G.B, G.H_LOW * s, w * s, C)
    arrays = [rng.standard_normal(sh).astype(F) for sh in (shape, out, out, (C,), out)]
    for a in arrays:
        a.setflags(write=False)
    return arrays                                             # x, add1, add2, bias, grad_out


@pytest.mark.parametrize("C", G.DECONV_CLASSES)
@pytest.mark.parametrize("c", G.cases(), ids=CASE_IDS)
def test_deconv_forward(gpu, c, C):
    from posecnn_amd import ops
    k, s, w = c
    x, a1, a2, b, _ = deconv_case(c, C)
    same(N(ops.deconv_bilinear(T(gpu, x), k, s)), oracle.deconv_bilinear(x, k, s), "deconv")
    got = ops.deconv_bilinear(T(gpu, x), k, s, add1=T(gpu, a1), add2=T(gpu, a2), bias=T(gpu, b), relu=True)
    want = oracle.deconv_bilinear(x, k, s, a1, a2, b, True)
    assert (want == 0).any() and (want > 0).any()
    same(N(got), want, "deconv + add1 + add2 + bias, ReLU")


@pytest.mark.parametrize("C", G.DECONV_CLASSES)
@pytest.mark.parametrize("c", G.cases(), ids=CASE_IDS)
def test_deconv_backward(gpu, c, C):
    import torch
    from posecnn_amd import ops
    k, s, w = c
    x, _, _, _, g = deconv_case(c, C)
    want = oracle.deconv_bilinear_bwd(g, k, s)
    same(N(ops.deconv_bilinear_grad(T(gpu, g), k, s)), want, "deconv bwd")
    xt = T(gpu, x).requires_grad_(True)
    y = ops.deconv_bilinear(xt, k, s)
    same(N(y.detach()), oracle.deconv_bilinear(x, k, s), "deconv fwd (autograd route)")
    y.backward(T(gpu, g))
    same(N(xt.grad), want, "deconv autograd")
    if not G.is_dyadic(k):
        return
    # exactly float64 on integers (tests/test_gpu_gradients.py::test_deconv_backward_equals_float64): a cell gathers k x k taps
    # of absolute sum (sum of the 1-D taps)^2, in units of 1 / (4 f^2)
    f = (k + 1) // 2
    gmax = G.exact_gradient_range(k)
    gi = exact.ints(exact.seed_of("geometry_bwd", c, C), g.shape, -gmax, gmax)
    x64 = torch.zeros(x.shape, dtype=torch.float64, requires_grad=True)
    y64 = grad_ref.deconv_bilinear64(x64, k, s)
    (ref,) = torch.autograd.grad(y64, x64, gi.double(), retain_graph=True)
    (bound,) = torch.autograd.grad(y64, x64, gi.double().abs())
    assert gmax >= 1 and float(bound.max()) * 4 * f * f < exact.LIMIT, "input not exact"
    exact.check(ops.deconv_bilinear_grad(gi.to(gpu), k, s), ref, {"name": "deconv_bilinear_grad"})


# ---- label head ----------------------------------------------------------------------------------------------------------
def check_label_head(gpu, k, s, w, C):
    from posecnn_amd import ops
    d = G.head_case(k, s, w, C)
    z, b, gt = T(gpu, d["z"]), T(gpu, d["bias"]), T(gpu, d["gt"])
    s0, p0, l0 = ops.upscore_softmax_argmax(z, b, k, s, relu=True, want_score=True)
    same(N(s0), d["score"], "score"); same(N(p0), d["prob"], "prob"); same(N(l0), d["label"], "label")
    s1, p1, l1 = ops.upscore_softmax_argmax(z, b, k, s, relu=False, want_score=False, want_prob=False)
    assert s1 is None and p1 is None
    same(N(l1), d["label_norelu"], "label of the label-only call (no ReLU)")
    _, _, l2 = ops.upscore_softmax_argmax(z, b, k, s, relu=True, want_score=False, want_prob=False)
    same(N(l2), d["label"], "label of the label-only call")
    s3, p3, l3, h3 = ops.upscore_softmax_argmax(z, b, k, s, relu=True, want_score=True, hard_gt=gt, hard_threshold=THRESHOLD)
    same(N(s3), d["score"], "score (hard launch)"); same(N(p3), d["prob"], "prob (hard launch)")
    same(N(l3), d["label"], "label (hard launch)"); same(N(h3), d["hard"], "hard label")
    _, p4, _, h4 = ops.upscore_softmax_argmax(z, b, k, s, relu=True, want_prob=False, hard_gt=gt, hard_threshold=THRESHOLD)
    assert p4 is None
    same(N(h4), d["hard"], "hard label without prob")


@pytest.mark.parametrize("C", G.HEAD_CLASSES)
@pytest.mark.parametrize("c", G.cases(), ids=CASE_IDS)
def test_label_head(gpu, c, C):
    check_label_head(gpu, *c, C)


@pytest.mark.parametrize("C", G.DISPATCH_CLASSES)
@pytest.mark.parametrize("ks", G.DISPATCH_KS, ids=["k%ds%d" % ks for ks in G.DISPATCH_KS])
def test_label_head_class_dispatch(gpu, ks, C):
    """22 / 14 / 16 -> the compile-time kernels, <= 24 -> <24>, else <64>: both sides of 24 and the limit 64."""
    check_label_head(gpu, ks[0], ks[1], G.WIDTHS[ks[1]][0], C)


@pytest.mark.parametrize("ks,C,nbytes", G.LDS_CASES, ids=["k%ds%d-C%d" % (ks + (C,)) for ks, C, _ in G.LDS_CASES])
def test_label_head_with_more_than_64_kib_of_dynamic_lds(gpu, ks, C, nbytes):
    """66 560 and 133 376 bytes of dynamic LDS, the latter the largest request the argument checks let through."""
    k, s = ks
    w = G.WIDTHS[s][0]
    assert G.label_head_plan(w, C, k, s)["lds_bytes"] == nbytes > 64 * 1024
    check_label_head(gpu, k, s, w, C)


@pytest.mark.parametrize("C,k,s", G.REFUSED, ids=["C%d-k%ds%d" % r for r in G.REFUSED])
def test_label_head_refusals_write_nothing(gpu, C, k, s):
    import torch
    from posecnn_amd import _lib
    L = _lib.lib()
    B, h, w = 1, 2, 3
    z = torch.zeros((B, h, w, C), device=gpu)
    bias = torch.zeros(C, device=gpu)
    n = B * h * s * w * s
    score, prob, hard = (torch.full((n * C,), 7.0, device=gpu) for _ in range(3))
    label = torch.full((n,), 7, dtype=torch.int32, device=gpu)
    gt = torch.zeros(n, dtype=torch.int32, device=gpu)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    rc = L.pcnn_upscore_softmax_argmax_fwd(p(z), p(bias), B, h, w, C, k, s, 1, p(score), p(prob), p(label), stream)
    assert rc == _lib.PCNN_EINVAL, (rc, L.pcnn_last_error_string())
    rc = L.pcnn_upscore_softmax_argmax_hard_fwd(p(z), p(bias), B, h, w, C, k, s, 1, p(score), p(prob), p(label), p(gt), 0.5, p(hard), stream)
    assert rc == _lib.PCNN_EINVAL, (rc, L.pcnn_last_error_string())
    torch.cuda.synchronize()
    for t in (score, prob, hard, label):
        assert bool((t == 7).all())


# ---- input alignment -------------------------------------------------------------------------------------------------------
def shifted(gpu, a, offset):
    """A contiguous view holding `a` that starts `offset` bytes past a 16-byte boundary."""
    import torch
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + 8, dtype=torch.from_numpy(a).dtype, device=gpu)
    assert buf.data_ptr() % 16 == 0 and offset % 4 == 0 and a.itemsize == 4
    v = buf[offset // 4:offset // 4 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == offset
    return v


@pytest.mark.parametrize("offset", [4, 8])
@pytest.mark.parametrize("C", [64, 22])
def test_input_alignment_switches_kernels_not_bits(gpu, C, offset):
    """The launchers pick a vector width (deconv fwd / bwd, bias_act, bias_relu_pool2) or the compile-time label head from
    the alignment of their INPUTS; the ABI asks 16 bytes of outputs and workspaces only. Every result must equal the
    aligned call's bits. The ops wrappers pass a contiguous view through unchanged (asserted: the pointer the library sees
    is the view's); bias_act goes through the C entry with an output of its own, aligned."""
    import torch
    from posecnn_amd import _lib, ops
    k, s, w = 16, 8, 17
    x, a1, a2, b, g = deconv_case((k, s, w), C)
    sh = lambda a: shifted(gpu, a, offset)
    assert ops._dev(sh(x), "x", torch.float32).data_ptr() % 16 == offset
    # deconv forward: each of in, add1, add2 misaligned alone, and all three
    full = lambda xx, aa1, aa2: N(ops.deconv_bilinear(xx, k, s, add1=aa1, add2=aa2, bias=T(gpu, b), relu=True))
    want = full(T(gpu, x), T(gpu, a1), T(gpu, a2))
    same(want, oracle.deconv_bilinear(x, k, s, a1, a2, b, True), "aligned deconv")
    same(full(sh(x), T(gpu, a1), T(gpu, a2)), want, "deconv, in at +%d" % offset)
    same(full(T(gpu, x), sh(a1), T(gpu, a2)), want, "deconv, add1 at +%d" % offset)
    same(full(T(gpu, x), T(gpu, a1), sh(a2)), want, "deconv, add2 at +%d" % offset)
    same(full(sh(x), sh(a1), sh(a2)), want, "deconv, all at +%d" % offset)
    same(N(ops.deconv_bilinear(sh(x), k, s)), N(ops.deconv_bilinear(T(gpu, x), k, s)), "plain deconv, in at +%d" % offset)
    # deconv backward
    want = N(ops.deconv_bilinear_grad(T(gpu, g), k, s))
    same(N(ops.deconv_bilinear_grad(sh(g), k, s)), want, "deconv bwd, grad_out at +%d" % offset)
    # bias_act, out of place through the C entry
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    outs = []
    for xin in (T(gpu, a1), sh(a1)):
        y = torch.empty(a1.shape, device=gpu)
        assert y.data_ptr() % 16 == 0
        assert L.pcnn_bias_act_fwd(p(xin), p(T(gpu, b)), a1.size // C, C, 1, p(y), stream) == _lib.PCNN_OK
        outs.append(N(y))
    same(outs[0], np.maximum(a1 + b, 0).astype(F), "aligned bias_act")
    same(outs[1], outs[0], "bias_act, x at +%d" % offset)
    # bias_relu_pool2 (Ho = 24, Wo = 136: even)
    want = N(ops.bias_relu_pool2(T(gpu, a1), T(gpu, b)))
    same(N(ops.bias_relu_pool2(sh(a1), T(gpu, b))), want, "bias_relu_pool2, x at +%d" % offset)
    # label head: z and bias, alone and together (at +4 the compile-time kernel's float2 loads are not possible)
    d = G.head_case(k, s, w, C)
    head = lambda zz, bb: [N(t) for t in ops.upscore_softmax_argmax(zz, bb, k, s, relu=True, want_score=True, hard_gt=T(gpu, d["gt"]),
                                                                      hard_threshold=THRESHOLD)]
    want = head(T(gpu, d["z"]), T(gpu, d["bias"]))
    for name, got in zip(("score", "prob", "label", "hard"), want):
        same(got, d[name], "aligned label head: " + name)
    for what, zz, bb in (("z", sh(d["z"]), T(gpu, d["bias"])), ("bias", T(gpu, d["z"]), sh(d["bias"])), ("z and bias", sh(d["z"]), sh(d["bias"]))):
        for name, got, ref in zip(("score", "prob", "label", "hard"), head(zz, bb), want):
            same(got, ref, "label head, %s at +%d: %s" % (what, offset, name))


# ---- the low-resolution Hough source -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", G.HOUGH_KS, ids=["k%ds%d" % ks for ks in G.HOUGH_KS])
def test_hough_lowres_source_with_more_than_two_taps(gpu, ks):
    """tests/test_gpu_hough.py::test_lowres_vertex_source_equals_materialised_field at k > 2 s: bilinear_at3's general branch."""
    import torch
    from posecnn_amd import ops
    k, s = ks
    B, H, W, C, n_obj = G.HOUGH_SHAPE[s]
    label, z, bias, meta = lowres_case(500 + H, B, H, W, C, n_obj, s)
    ext = config.LOV_EXTENTS[:C]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    lt = G.HOUGH_LABEL_THRESHOLD
    got = ops.hough_voting_gpu_lowres_padded(t(label), t(z), t(bias), k, s, t(ext), t(meta), None, 0, -1.0, 0.02, G.HOUGH_SKIP,
                                             label_threshold=lt)
    full = ops.deconv_bilinear(t(z), k, s, bias=t(bias))
    ref = ops.hough_voting_gpu_padded(t(label), full, t(ext), t(meta), None, 0, -1.0, 0.02, G.HOUGH_SKIP, label_threshold=lt)
    torch.cuda.synchronize()
    got = [N(o) for o in got]
    hough_compare(got, [N(o) for o in ref])
    want = oracle.hough_voting(label, oracle.deconv_bilinear(z, k, s, None, None, bias, False), ext, meta, None, 0, -1.0, 0.02,
                               G.HOUGH_SKIP, label_thr=lt, padded=True)
    hough_compare(got, want)
    assert int(got[5][1]) >= 1


# ---- label_head_loss: the checks of tests/test_gpu_label_loss.py on the new cases ---------------------------------------------
LOSS_IDS = [LR.case_id(c) for c in G.label_loss_cases()]


@pytest.mark.parametrize("kind", LR.GT_KINDS)
@pytest.mark.parametrize("c", G.label_loss_cases(), ids=LOSS_IDS)
def test_label_head_loss_forward(gpu, c, kind):
    TL.test_forward_bit_for_bit_and_loss(gpu, c, kind)


@pytest.mark.parametrize("kind", LR.GT_KINDS)
@pytest.mark.parametrize("c", G.label_loss_cases(), ids=LOSS_IDS)
def test_label_head_loss_backward(gpu, c, kind):
    TL.test_backward_kernel(gpu, c, kind)


@pytest.mark.parametrize("kind", LR.GT_KINDS)
@pytest.mark.parametrize("c", G.label_loss_cases(), ids=LOSS_IDS)
def test_label_head_loss_autograd(gpu, c, kind):
    TL.test_autograd_with_a_non_unit_upstream_gradient(gpu, c, kind)


# ---- vertex_head_loss: the checks of tests/test_gpu_vertex_head.py on the ladder ------------------------------------------------
VERTEX_IDS = [(G.vertex_name(*ks), kind) for ks, _ in G.VERTEX_LADDER for kind in G.VERTEX_KINDS]


@pytest.mark.parametrize("nk", VERTEX_IDS, ids=["%s-%s" % nk for nk in VERTEX_IDS])
def test_vertex_head_loss_forward_and_backward(gpu, nk):
    TV.test_forward_and_backward_bit_for_bit(gpu, nk)


@pytest.mark.parametrize("nk", VERTEX_IDS, ids=["%s-%s" % nk for nk in VERTEX_IDS])
def test_vertex_head_loss_autograd(gpu, nk):
    TV.test_autograd_equals_the_unfused_composition_on_the_gpu(gpu, nk)


# ---- memory contract -----------------------------------------------------------------------------------------------------
S1_CASES = [(k, s, w, C) for (k, s, w) in G.cases(((1, 1), (3, 1))) for C in (22, 25)]
CONTRACT_HEAD = S1_CASES + [(k, s, G.WIDTHS[s][0], C) for (k, s), C, _ in G.LDS_CASES]


@pytest.mark.parametrize("khwc", CONTRACT_HEAD, ids=["k%ds%d-w%d-C%d" % c for c in CONTRACT_HEAD])
def test_memory_contract_label_head(gpu, khwc):
    """Both poison patterns of tests/memguard.py with guard bands: the s = 1 cases (odd rows of 129 and 127 pixels: a
    segment's run starts on any 4-byte phase) and the two launches above 64 KiB of LDS."""
    from test_gpu_memory_contract import Case, execute
    k, s, w, C = khwc
    d = G.head_case(k, s, w, C)

    def make():
        return dict(z=np.array(d["z"]), bias=np.array(d["bias"]), gt=np.array(d["gt"]))

    def run(ctx):
        from posecnn_amd import ops
        z, b = ctx.e("z"), ctx.e("bias")
        s0, p0, l0 = ops.upscore_softmax_argmax(z, b, k, s, relu=True, want_score=True)
        _, _, l1 = ops.upscore_softmax_argmax(z, b, k, s, relu=False, want_score=False, want_prob=False)
        _, p2, l2, h2 = ops.upscore_softmax_argmax(z, b, k, s, relu=True, want_score=False, hard_gt=ctx.e("gt"), hard_threshold=THRESHOLD)
        return dict(score=s0, prob=p0, label=l0, label_norelu=l1, hard_prob=p2, hard_label=l2, hard=h2)

    def check(_, o):
        for name, ref in (("score", "score"), ("prob", "prob"), ("label", "label"), ("label_norelu", "label_norelu"),
                          ("hard_prob", "prob"), ("hard_label", "label"), ("hard", "hard")):
            same(o[name], d[ref], name)

    execute(Case("label head k%ds%d w%d C%d" % khwc, ("pcnn_upscore_softmax_argmax_fwd", "pcnn_upscore_softmax_argmax_hard_fwd"),
                 make, run, check))


@pytest.mark.parametrize("ks", [ks for ks, rung in G.VERTEX_LADDER if rung != 0], ids=[G.vertex_name(*ks) for ks, rung in G.VERTEX_LADDER if rung != 0])
def test_memory_contract_vertex_head_ladder(gpu, ks):
    """Ladder rungs 1 to 5 and the two geometries no rung fits."""
    TV.test_memory_contract(gpu, G.vertex_name(*ks))
