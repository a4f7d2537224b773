"""numpy restatement of the training label head (include/posecnn_hip_loss.h). TEST INFRASTRUCTURE ONLY.

  log_sum_f32                the kernel's f32 log of the softmax denominator, one IEEE operation per numpy operation
  restate                    per-pixel label / hot / terms / dscore in float32 from oracle.upscore_softmax_argmax (the
                             oracle's score, prob and label are bit-equal to the existing label-head kernel), the f64
                             sums of the bit-exact terms and the expected loss, dbias and dz
  loss64                     the whole loss in float64 — grad_ref.deconv_bilinear64 + torch ops, differentiated by
                             torch.autograd; MUTATIONS are the seeded defects of the comparator self-test
  cases / case               the shapes and inputs shared by tests/test_label_loss_cpu.py and tests/test_gpu_label_loss.py
"""
import functools

import numpy as np

import np_ref
import oracle

F = np.float32
MUTATIONS = ("threshold_ignored", "relu_gate_dropped", "count_is_pixel_count", "one_hot_dropped", "coef_twice")


def log_sum_f32(x):
    """log_sum_f32 of posecnn_amd/csrc/label_loss.hip on an array of float32 in [1, 64] (NaN passes through)."""
    x = np.asarray(x, F)
    bits = x.view(np.int32)
    n = (bits >> 23) - 127
    t = ((bits & 0x007fffff) | 0x3f800000).astype(np.int32).view(F)
    big = t > F(1.41421354)
    t = np.where(big, t * F(0.5), t)
    n = np.where(big, n + 1, n)
    f = t - F(1.0)
    q = f / (F(2.0) + f)
    y = q * q
    p = np.full(x.shape, F(0.222222224), F)
    p = p * y + F(0.285714298)
    p = p * y + F(0.4)
    p = p * y + F(0.666666687)
    p = p * y
    l = (q + q) + q * p
    nf = n.astype(F)
    out = nf * F(0.693145752) + (l + nf * F(1.42860677e-06))
    assert out.dtype == F
    return np.where(x != x, x, out)


def restate(z, bias, gt, threshold, k, s, relu=True, upstream=1.0):
    """Everything the kernels produce, in float32 with their operation order, plus the float64 sums the tests bound the
    reductions with. `upstream` is rounded to float32 as the op receives it."""
    z, bias = np.ascontiguousarray(z, F), np.ascontiguousarray(bias, F)
    gt = np.ascontiguousarray(gt, np.int32)
    C = z.shape[-1]
    score, prob, label = oracle.upscore_softmax_argmax(z, bias, k, s, relu=relu)
    # the softmax once more in numpy, for the denominator the oracle does not return; its probabilities must be the oracle's
    m = np.fmax.reduce(score, axis=-1, keepdims=True)
    d = (score - m).astype(F)
    e = np_ref.exp_softmax_f32(d)
    tot = np.zeros(score.shape[:-1] + (1,), F)
    for c in range(C):
        tot = (tot + e[..., c:c + 1]).astype(F)
    assert np.array_equal((e / tot).astype(F).view(np.uint32), prob.view(np.uint32)), "numpy softmax differs from the oracle"
    hard = np_ref.hard_label(prob, gt, threshold)                        # [B,Ho,Wo,C], one 1 per hot pixel
    hot = hard.sum(-1) > 0
    g = np.where(hot, gt, 0)
    dg = np.take_along_axis(d, g[..., None].astype(np.int64), -1)[..., 0]
    terms = np.where(hot, (log_sum_f32(tot[..., 0]) - dg).astype(F), F(0)).astype(F)
    count = int(hot.sum())
    S64 = float(terms.astype(np.float64).sum())
    loss = F(S64 / (count + 1e-10))
    coef = F(upstream) / (F(count) + F(1e-10)) if count else F(0)      # no hot pixel: coef is never used
    dscore = (coef * (prob - hard).astype(F)).astype(F)
    dscore = np.where(hot[..., None], dscore, F(0))
    if relu:
        dscore = np.where(score > 0, dscore, F(0))
    dscore = np.ascontiguousarray(dscore, F)
    dbias64 = dscore.astype(np.float64).reshape(-1, C).sum(0)
    dbias_abs = np.abs(dscore.astype(np.float64)).reshape(-1, C).sum(0)
    return {"score": score, "prob": prob, "label": label, "hot": hot, "terms": terms, "count": count, "S64": S64, "loss": loss,
            "dscore": dscore, "dbias64": dbias64, "dbias_abs": dbias_abs, "dz": oracle.deconv_bilinear_bwd(dscore, k, s)}


def loss64(z, bias, gt, threshold, k, s, relu=True, dtype=None, mutate=None):
    """(loss, dz, dbias) of the label head as one plain torch function in `dtype` (float64), by autograd. The Hardlabel
    weights are computed without a gradient from the function's own probabilities."""
    import torch

    import grad_ref
    assert mutate is None or mutate in MUTATIONS, mutate
    dtype = dtype or torch.float64
    zt = torch.tensor(np.asarray(z), dtype=dtype, requires_grad=True)
    bt = torch.tensor(np.asarray(bias), dtype=dtype, requires_grad=True)
    g = torch.tensor(np.asarray(gt), dtype=torch.int64)
    C = zt.shape[-1]
    y = grad_ref.deconv_bilinear64(zt, k, s, bias=bt)
    score = torch.relu(y) if relu else y
    if relu and mutate == "relu_gate_dropped":
        score = score.detach() + (y - y.detach())                      # the value of the ReLU, the gradient of the identity
    logp = torch.log_softmax(score, dim=-1)
    with torch.no_grad():
        ok = (g >= 0) & (g < C)
        gi = torch.where(ok, g, torch.zeros_like(g))
        pg = torch.gather(logp.exp(), -1, gi[..., None])[..., 0]
        hot = ok & ((g > 0) | (pg < threshold))
        if mutate == "threshold_ignored":
            hot = ok
        weight = torch.zeros_like(logp)
        weight.scatter_(-1, gi[..., None], hot.to(dtype)[..., None])
    count = weight.sum()
    if mutate == "count_is_pixel_count":
        count = torch.tensor(float(g.numel()), dtype=dtype)
    ce = -(weight * logp).sum()
    if mutate == "one_hot_dropped":
        # d/dscore of sum_hot logsumexp(score) is prob: the gradient without the one-hot subtraction, the value unchanged
        lse = (weight.sum(-1) * torch.logsumexp(score, dim=-1)).sum()
        ce = ce.detach() + (lse - lse.detach())
    loss = ce / (count + 1e-10)
    if mutate == "coef_twice":
        twice = loss / (count + 1e-10)
        loss = loss.detach() + (twice - twice.detach())
    dz, db = torch.autograd.grad(loss, [zt, bt], allow_unused=True)
    dz = torch.zeros_like(zt) if dz is None else dz
    db = torch.zeros_like(bt) if db is None else db
    return float(loss.detach()), dz.numpy(), db.numpy()


# ---- the shared cases -------------------------------------------------------------------------------------------------
THRESHOLD = 0.5
SHAPES = ((2, 3, 17), (1, 2, 1), (1, 1, 3))     # two 128-pixel segments (8 live in the second); every tap set clipped
CLASSES = (22, 14, 5)                           # compile-time path, compile-time path, generic path (odd)
KS = ((16, 8), (4, 2))
GT_KINDS = ("mixed", "ignored")                 # "ignored": -1 everywhere, count = 0


def cases():
    return [(shape, C, ks) for shape in SHAPES for C in CLASSES for ks in KS]


def case_id(c):
    (B, h, w), C, (k, s) = c
    return "z%dx%dx%dx%d-k%ds%d" % (B, h, w, C, k, s)


@functools.lru_cache(maxsize=None)
def case(shape, C, ks, kind="mixed"):
    """(z [B,h,w,C], bias [C], gt [B,h s,w s]) of a case, seeded. Class 0 is planted high in the first low-resolution
    cell of every frame and low in the last, so that ground-truth 0 meets prob[0] on either side of THRESHOLD; the map
    cycles through 0, foreground classes, -1 and a label >= C; the last frame of a batch of two is -1 everywhere."""
    B, h, w = shape
    k, s = ks
    rng = np.random.default_rng(1000 * C + 10 * h + w + k)
    z = (rng.standard_normal((B, h, w, C)) * 1.5).astype(F)
    # (more than 24 classes — the geometry cases of tests/bilinear_geometry.py — share the denominator among more terms and
    #  a corner pixel of a 3-tap kernel takes only 9/16 of its cell: planted higher, so that prob[0] still crosses THRESHOLD)
    plant = F(9.0) if C <= 24 else F(16.0)
    z[:, 0, 0, 0] = plant
    z[:, 0, 0, 1:] -= F(2.0)
    z[:, -1, -1, 0] = -plant
    z[:, -1, -1, 1:] += F(2.0)
    bias = (rng.standard_normal(C) * 0.5).astype(F)
    pattern = np.array([0, 3 % C, -1, 0, C + 2, 1, 0, C - 1, 0, C], np.int32)
    n = B * h * s * w * s
    gt = pattern[np.arange(n) % len(pattern)].reshape(B, h * s, w * s).copy()
    if B > 1:
        gt[-1] = -1
    if kind == "ignored":
        gt[:] = -1
    for a in (z, bias, gt):
        a.setflags(write=False)
    return z, bias, gt


@functools.lru_cache(maxsize=None)
def reference(shape, C, ks, kind="mixed", upstream=1.0):
    """`restate` of a case, computed once and shared (read-only)."""
    z, bias, gt = case(shape, C, ks, kind)
    r = restate(z, bias, gt, THRESHOLD, ks[0], ks[1], upstream=upstream)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r
