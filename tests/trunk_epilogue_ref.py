"""numpy restatement of include/posecnn_hip_trunk_train.h: the trunk's training epilogues, forward and backward, one numpy
operation per operation of the header, and the bias gradient in the header's order (runs of 128 pixels, 16 slots summed
in ascending order, halving trees, 256-way finishing pass). TEST INFRASTRUCTURE ONLY.

`defect` seeds one of three mistakes the tests must reject:
  "last_max"    the last maximum of a window instead of the first
  "relu_ge"     a ReLU gate of >= instead of >
  "raw_argmax"  the argmax taken on the raw values, before the bias is added
"""
import numpy as np

F = np.float32
RUN, SLOTS, FIN = 128, 16, 256
DEFECTS = ("last_max", "relu_ge", "raw_argmax")


def windows(y):
    """[B,H,W,C] -> [B,H/2,W/2,4,C], window order (y,x), (y,x+1), (y+1,x), (y+1,x+1)"""
    B, H, W, C = y.shape
    v = y.reshape(B, H // 2, 2, W // 2, 2, C)
    return np.stack([v[:, :, 0, :, 0], v[:, :, 0, :, 1], v[:, :, 1, :, 0], v[:, :, 1, :, 1]], axis=3)


def unwindows(w):
    B, Ho, Wo, _, C = w.shape
    v = np.empty((B, Ho, 2, Wo, 2, C), w.dtype)
    v[:, :, 0, :, 0], v[:, :, 0, :, 1], v[:, :, 1, :, 0], v[:, :, 1, :, 1] = w[:, :, :, 0], w[:, :, :, 1], w[:, :, :, 2], w[:, :, :, 3]
    return v.reshape(B, 2 * Ho, 2 * Wo, C)


def _gate(v, defect=None):
    return v >= 0 if defect == "relu_ge" else v > 0


def bias_act(y, bias, relu):
    """pcnn_bias_act_fwd"""
    t = (y.astype(F) + bias.astype(F)).astype(F)
    return np.where(t > 0, t, F(0)).astype(F) if relu else t


def pool_forward(y, bias, relu, defect=None):
    """-> (pooled f32 [B,H/2,W/2,C], sel u8 [B,H/2,W/2,C], act f32 [B,H,W,C])"""
    raw = windows(y.astype(F))
    t = (raw + bias.astype(F)).astype(F)
    key = raw if defect == "raw_argmax" else t
    best_key = key[:, :, :, 0].copy()
    s = np.zeros(best_key.shape, np.uint8)
    for k in (1, 2, 3):
        better = key[:, :, :, k] >= best_key if defect == "last_max" else key[:, :, :, k] > best_key
        best_key = np.where(better, key[:, :, :, k], best_key)
        s = np.where(better, np.uint8(k), s)
    best = np.take_along_axis(t, s[:, :, :, None, :].astype(np.int64), axis=3)[:, :, :, 0]
    if not relu:
        return best.astype(F), s, unwindows(t)
    sel = np.where(_gate(best, defect), s, np.uint8(4)).astype(np.uint8)
    pooled = np.where(best > 0, best, F(0)).astype(F)
    return pooled, sel, unwindows(np.where(t > 0, t, F(0)).astype(F))


def existing_pool(y, bias, relu):
    """pcnn_bias_relu_pool2_fwd as csrc/upscore.hip states it: the maximum of the raw values, then one add, then the ReLU"""
    w = windows(y.astype(F))
    a = w[:, :, :, 0]
    for k in (1, 2, 3):
        a = np.where(w[:, :, :, k] > a, w[:, :, :, k], a)
    m = (a + bias.astype(F)).astype(F)
    return np.where(m > 0, m, F(0)).astype(F) if relu else m


def dbias_sum(vals):
    """vals [P, K, C]: pixel p contributes vals[p, 0..K-1] in that order. -> f32 [C], the header's order."""
    P, K, C = vals.shape
    nruns = (P + RUN - 1) // RUN
    v = np.zeros((nruns * RUN, K, C), np.float64)
    v[:P] = vals
    v = v.reshape(nruns, RUN // SLOTS, SLOTS, K, C)
    acc = np.zeros((nruns, SLOTS, C), np.float64)
    for j in range(RUN // SLOTS):
        for k in range(K):
            acc = acc + v[:, j, :, k, :]
    st = SLOTS // 2
    while st >= 1:
        acc[:, :st] = acc[:, :st] + acc[:, st:2 * st]
        st //= 2
    part = acc[:, 0]
    rounds = (nruns + FIN - 1) // FIN
    p = np.zeros((rounds * FIN, C), np.float64)
    p[:nruns] = part
    p = p.reshape(rounds, FIN, C)
    a = np.zeros((FIN, C), np.float64)
    for i in range(rounds):
        a = a + p[i]
    st = FIN // 2
    while st >= 1:
        a[:st] = a[:st] + a[st:2 * st]
        st //= 2
    return a[0].astype(F)


def pool_backward(dpooled, sel, dact=None, act=None, defect=None):
    """-> (dy f32 [B,H,W,C], dbias f32 [C])"""
    B, Ho, Wo, C = dpooled.shape
    g = np.empty((B, Ho, Wo, 4, C), F)
    if dact is not None:
        dw, aw = windows(dact.astype(F)), windows(act.astype(F))
    for k in range(4):
        r = np.where(sel == k, dpooled.astype(F), F(0)).astype(F)
        if dact is not None:
            r = (np.where(_gate(aw[:, :, :, k], defect), dw[:, :, :, k], F(0)).astype(F) + r).astype(F)
        g[:, :, :, k] = r
    return unwindows(g), dbias_sum(g.reshape(B * Ho * Wo, 4, C))


def backward(da, a, relu, defect=None):
    """-> (dy, dbias) of the un-pooled form; da, a [..., C]"""
    da = da.astype(F)
    dy = np.where(_gate(a, defect), da, F(0)).astype(F) if relu else da
    C = da.shape[-1]
    return dy, dbias_sum(dy.reshape(-1, 1, C))


def dbias_bound(dy):
    """-> (float64 sum [C], tolerance [C]): 2^-24 |S| + 2^-30 sum |.|, the bound of the label head's dbias"""
    d = dy.reshape(-1, dy.shape[-1]).astype(np.float64)
    s = d.sum(axis=0)
    return s, 2.0 ** -24 * np.abs(s) + 2.0 ** -30 * np.abs(d).sum(axis=0)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def tie_free(shape, seed):
    """(y, bias): every biased value is exact in f32 and non-zero, and the four of a window differ — so float64 autograd of
    the framework composition routes exactly as the f32 kernels do. About a quarter of the windows are closed."""
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    w = np.argsort(rng.random((B, H // 2, W // 2, 4, C)), axis=3).astype(np.float64)        # a permutation of 0..3 per window
    w = w * rng.integers(1, 4, (B, H // 2, W // 2, 1, C)) / 8.0 + rng.integers(-12, 5, (B, H // 2, W // 2, 1, C)) / 8.0
    bias = (2 * rng.integers(-3, 4, C) + 1) / 16.0                                          # odd multiples of 1/16
    return unwindows(w.astype(F)), bias.astype(F)


def edge_input(shape, seed):
    """(y, bias) with everything the kernels can get wrong: values on a grid of 1/4 (exact ties, exact zeros after the bias),
    rounded normal values, all-negative windows, and in window 0 / channel 0 the bias-induced tie: 1 then 1 + 2^-23 under a
    bias of 2^10 are equal after the add, so position 0 wins, while the raw argmax is position 1."""
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    w = (rng.integers(-8, 9, (B, H // 2, W // 2, 4, C)) / 4.0).astype(F)
    normal = rng.standard_normal(w.shape).astype(F)
    w = np.where(rng.random(w.shape) < 0.4, normal, w)
    closed = rng.random((B, H // 2, W // 2, 1, C)) < 0.2
    w = np.where(closed, -np.abs(w) - F(4), w).astype(F)
    bias = (rng.integers(-4, 5, C) / 4.0).astype(F)
    bias[0] = F(1024.0)
    w[0, 0, 0, :, 0] = (F(1.0), F(1.0) + F(2.0 ** -23), F(0.5), F(-1.0))
    if w.shape[1] * w.shape[2] > 1:
        w[0, -1, -1, :, 0] = (F(-1024.0), F(-1030.0), F(-1024.0), F(-1025.0))     # best exactly 0 under the ReLU: closed
    return unwindows(w), bias


def grads(shape, seed):
    """upstream gradients (dpooled [B,H/2,W/2,C], dact [B,H,W,C]) for `shape`"""
    B, H, W, C = shape
    rng = np.random.default_rng(seed + 1000)
    return rng.standard_normal((B, H // 2, W // 2, C)).astype(F), rng.standard_normal((B, H, W, C)).astype(F)
