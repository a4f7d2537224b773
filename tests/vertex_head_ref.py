"""numpy statements of the training vertex head (include/posecnn_hip_vertex_loss.h). TEST INFRASTRUCTURE ONLY.

  reference(c)   the UNFUSED composition from pieces that are pinned elsewhere: oracle.deconv_bilinear(z, k, s, bias) ->
                 vertex_ref.vertex_targets -> oracle.smooth_l1_vertex -> oracle.deconv_bilinear_bwd. Dense tensors throughout.
  restate(c)     the FUSED form the kernels implement: a pixel's prediction is interpolated only under a matching row, for
                 its three live channels; the loss takes the forward's partial order; dz is the per-cell gather that SKIPS
                 every pixel whose matched class does not own the channel (no +-0 is ever added: the skip is a `where`);
                 dbias takes the order the header gives. `mutate` seeds one of MUTATIONS.

Both return {"out" f32 [3], "dz" f32 [B,H,W,3C]}; the reference adds "grad_pred", "dbias64" (float64 channel sums of it) and
"dbias_abs" (of its magnitudes), the restatement "dbias" f32 [3C].

Cases are low-resolution H x W, each the smallest shape at which its branch can go wrong:
  A  2 x  6 x 11, 16/8, C =  4, M = 3   two tiles of 4 x 8 cells per axis, ragged; taps clipped on all four borders
  B  1 x  5 x  7,  4/2, C = 22, M = 5   the other (kernel, stride) pair
  C  3 x 12 x 16, 16/8, C = 22, M = 5   2 433 024 elements > 8 * 262 144: the forward's strided loop runs a second outer
                                        iteration with a ragged tail
  D  1 x  2 x  3, 16/8, C = 64, M = 5   the class-count limit
"""
import functools

import numpy as np

import oracle
import vertex_ref

F = np.float32
SL1_BLOCKS = 1024
CASES = {"A": (2, 6, 11, 16, 8, 4, 3), "B": (1, 5, 7, 4, 2, 22, 5), "C": (3, 12, 16, 16, 8, 22, 5), "D": (1, 2, 3, 16, 8, 64, 5)}
# The tile ladder of vertex_head_loss.hip (tests/bilinear_geometry.py, tests/GEOMETRY.md): one case per rung and the two
# geometries no rung fits, 2 x 5 x 9 cells each so that the tiles of more than one cell are clipped in both directions.
# Kept out of CASES: case_ids() and the tests parametrised over it stay as they were.
GEOMETRY_CASES = {"G%d_%d" % ks: (2, 5, 9) + ks + (4, 3)
                  for ks in ((16, 8), (20, 10), (14, 14), (32, 16), (28, 28), (40, 40), (64, 32), (56, 56))}
KINDS = ("mixed", "empty", "full", "branches_sigma1", "branches_sigma3")
MUTATIONS = ("bias_dropped", "row_priority_reversed", "taps_swapped")
INSTANCE_ID = 7


def case_ids():
    return [(n, k) for n in sorted(CASES) for k in KINDS]


@functools.lru_cache(maxsize=None)
def case(name, kind="mixed"):
    """-> dict(z, bias, label, instance, objects, k, s, C, M, sigma); the arrays are read-only (shared among tests).

    mixed     palette of labels -1, 0, C, c1, c2 (and c4 when M = 5) in 4 x 4 pixel blocks, so that tiles differ in the
              classes they hold. Rows: 0 = (c1, unmasked, w 1), 1 = (c1, instance 7, w 10) — two rows of one class, the higher
              index wins where the instance matches —, 2 = (c3, ...) whose class never appears; c2 has no row; with M = 5,
              rows 3 and 4 are two unmasked rows of c4 (w 1, w 10): the higher wins everywhere.
    empty     labels from -1, 0, C only;  full: every pixel c1, one live row.
    branches  `mixed` with sigma 1 / 3 and z scaled so that both smooth-L1 branches occur (reference() asserts it)."""
    if name in CASES:
        B, H, W, k, s, C, M = CASES[name]
        rng = np.random.default_rng([sorted(CASES).index(name), KINDS.index(kind), 20])
    else:
        B, H, W, k, s, C, M = GEOMETRY_CASES[name]
        rng = np.random.default_rng([100 + sorted(GEOMETRY_CASES).index(name), KINDS.index(kind), 20])
    Ho, Wo = H * s, W * s
    sigma = 3.0 if kind == "branches_sigma3" else 1.0
    scale = {"branches_sigma1": 1.5, "branches_sigma3": 0.4}.get(kind, 1.0)
    z = (rng.standard_normal((B, H, W, 3 * C)) * scale).astype(F)
    bias = (rng.standard_normal(3 * C) * 0.3).astype(F)
    c1, c2, c3, c4 = (1, 2, 3, None) if C == 4 else (C - 1, 5, 9, 2)
    palette = [-1, 0, C, c1, c1, c2] + ([c4, c4] if M >= 5 else [])
    if kind == "empty":
        palette = [-1, 0, C]
    elif kind == "full":
        palette = [c1]
    blk = 4
    coarse = rng.integers(0, len(palette), (B, (Ho + blk - 1) // blk, (Wo + blk - 1) // blk))
    label = np.asarray(palette, np.int32)[np.kron(coarse, np.ones((blk, blk), np.int64))[:, :Ho, :Wo]]
    instance = np.asarray([0, INSTANCE_ID, 3], np.int32)[rng.integers(0, 3, (B, Ho, Wo))]
    if kind not in ("empty", "full"):                        # the small maps too hold every palette entry, c1 with either instance
        for i, v in enumerate(palette):
            label[:, 1, 1 + i] = v
        instance[:, 1, 1 + palette.index(c1)] = INSTANCE_ID
        instance[:, 1, 2 + palette.index(c1)] = 0
    objects = np.zeros((B, M, 6), F)

    def row(cls, mask_id, w):
        return (cls, mask_id, F(rng.uniform(-4, Wo + 4)), F(rng.uniform(-4, Ho + 4)), F(np.log(rng.uniform(0.5, 2.0))), w)

    for b in range(B):
        if kind == "full":
            objects[b, M - 1] = row(c1, 0, 1.0)
            continue
        objects[b, 0] = row(c1, 0, 1.0)
        objects[b, 1] = row(c1, INSTANCE_ID, 10.0)
        objects[b, 2] = row(c3, 0, 1.0)
        if M >= 5:
            objects[b, 3] = row(c4, 0, 1.0)
            objects[b, 4] = row(c4, 0, 10.0)
    if kind != "full":
        label[:, 0, 0] = -1 if kind == "empty" else c1       # a pixel exactly under a clipped corner tap
    out = dict(z=z, bias=bias, label=np.ascontiguousarray(label), instance=instance, objects=objects, k=k, s=s, C=C, M=M,
               sigma=sigma, name=name, kind=kind)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- the unfused composition ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    c = case(name, kind)
    k, s, C = c["k"], c["s"], c["C"]
    pred = oracle.deconv_bilinear(c["z"], k, s, bias=c["bias"])
    targets, weights = vertex_ref.vertex_targets(c["label"], c["objects"], C, c["instance"])
    out, grad = oracle.smooth_l1_vertex(pred, targets, weights, c["sigma"])
    dz = oracle.deconv_bilinear_bwd(grad, k, s)
    live = weights > 0
    quad = np.abs(weights * (pred - targets)) < F(1.0) / (F(c["sigma"]) * F(c["sigma"]))
    if kind.startswith("branches"):
        assert (quad & live).any() and (~quad & live).any(), (name, kind, (quad & live).sum(), (~quad & live).sum())
    g64 = grad.astype(np.float64).reshape(-1, 3 * C)
    r = dict(out=out, grad_pred=grad, dz=dz, dbias64=g64.sum(axis=0), dbias_abs=np.abs(g64).sum(axis=0), pred=pred, targets=targets,
             weights=weights, n_quadratic=int((quad & live).sum()), n_linear=int((~quad & live).sum()))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def reference(c):
    return _reference(c["name"], c["kind"])


# ---- the fused form ---------------------------------------------------------------------------------------------------
def taps_table(k):
    f = (k + 1) // 2
    cc = (2 * f - 1 - f % 2) / (2.0 * f)
    return np.array([1.0 - abs(t / f - cc) for t in range(k)], np.float64).astype(F)


def _taps(o, k, s, n_in, tab):
    """make_taps of csrc/bilinear.h for an int array o: first index, count, weights [N,2] (k <= 2 s: at most two)."""
    pad = (k - s) // 2
    a = o + pad
    lo = np.maximum(-((k - 1 - a) // s), 0)               # ceil((a - k + 1) / s), clipped
    hi = np.minimum(a // s, n_in - 1)
    n = np.maximum(hi - lo + 1, 0)
    assert o.size == 0 or (n.max() <= 2 and n.min() >= 1)
    w = np.zeros(o.shape + (2,), F)
    for j in range(2):
        ok = j < n
        w[ok, j] = tab[(a - s * (lo + j))[ok]]
    return lo, n, w


def tile_shape(k, s):
    for th, tw in ((4, 8), (4, 4), (2, 4), (2, 2), (1, 2), (1, 1)):
        if (th * s + k - s) * (tw * s + k - s) <= 3072:
            return th, tw
    return 1, 1


def _tree(x):
    """halving tree over axis 0 (length a power of two): x[t] = x[t] + x[t + stride], stride = n/2 .. 1."""
    x = x.copy()
    st = x.shape[0] // 2
    while st >= 1:
        x[:st] = x[:st] + x[st:2 * st]
        st //= 2
    return x[0]


def _sl1(p, t, w, sigma2):
    diff = w * (p - t)
    ad = np.abs(diff)
    quad = ad < F(1.0) / sigma2
    in_loss = np.where(quad, (diff * diff) * (sigma2 / F(2.0)), ad - F(0.5) / sigma2)
    dp = np.where(quad, w * (sigma2 * diff), w * np.sign(diff).astype(F))
    assert in_loss.dtype == F and dp.dtype == F
    return in_loss, dp


def restate(c, upstream=None, mutate=None):
    assert mutate is None or mutate in MUTATIONS
    z, bias, label, instance, objects = c["z"], c["bias"], c["label"], c["instance"], c["objects"]
    k, s, C = c["k"], c["s"], c["C"]
    B, H, W, C3 = z.shape
    Ho, Wo = H * s, W * s
    pad = (k - s) // 2
    tab = taps_table(k)
    sigma2 = F(c["sigma"]) * F(c["sigma"])

    # ---- label -> row: the highest-index matching row
    sel = np.full((B, Ho, Wo), -1, np.int64)
    live = (label > 0) & (label < C)
    order = range(objects.shape[1])
    for j in (reversed(order) if mutate == "row_priority_reversed" else order):
        cls, mid = objects[:, j, 0][:, None, None], objects[:, j, 1][:, None, None]
        hit = live & (label.astype(F) == cls) & ((mid == 0) | (instance.astype(F) == mid))
        sel = np.where(hit, j, sel)
    bi, yi, xi = np.nonzero(sel >= 0)                      # the matched pixels, in pixel order
    rows = objects[bi, sel[bi, yi, xi]]
    li = label[bi, yi, xi].astype(np.int64)
    dx, dy = rows[:, 2].astype(np.float64) - xi, rows[:, 3].astype(np.float64) - yi
    nrm = np.sqrt(dx * dx + dy * dy) + 1e-10
    tgt = np.stack([(dx / nrm).astype(F), (dy / nrm).astype(F), rows[:, 4]], axis=1)
    wgt = rows[:, 5]

    # ---- the three live channels of each matched pixel: rows then columns ascending, acc = acc + (wy * wx) * z; + bias
    y0, ny, wy = _taps(yi, k, s, H, tab)
    x0, nx, wx = _taps(xi, k, s, W, tab)
    if mutate == "taps_swapped":
        wy, wx = wx, wy
    ch = 3 * li[:, None] + np.arange(3)[None, :]
    acc = np.zeros((len(bi), 3), F)
    for jy in range(2):
        for jx in range(2):
            ok = (jy < ny) & (jx < nx)
            w = (wy[:, jy] * wx[:, jx])[:, None]
            v = z[bi[:, None], np.minimum(y0 + jy, H - 1)[:, None], np.minimum(x0 + jx, W - 1)[:, None], ch]
            acc = np.where(ok[:, None], acc + w * v, acc)
    pred = acc if mutate == "bias_dropped" else acc + bias[ch]
    in_loss, dp = _sl1(pred, tgt, wgt[:, None], sigma2)

    # ---- forward: thread (blk, t) takes elements blk 256 + t + m 1024 256, m ascending; a skipped element adds nothing
    n = B * Ho * Wo * C3
    stride = SL1_BLOCKS * 256
    elem = (((bi * Ho + yi) * Wo + xi) * C3)[:, None] + ch
    al, aw = np.zeros(stride, F), np.zeros(stride, F)
    order = np.argsort(elem.reshape(-1), kind="stable")
    e_sorted, il_sorted = elem.reshape(-1)[order], in_loss.reshape(-1)[order]
    w_sorted = np.broadcast_to(wgt[:, None], in_loss.shape).reshape(-1)[order]
    for m in range((n + stride - 1) // stride):            # within one m every virtual thread has at most one element
        lo, hi = np.searchsorted(e_sorted, [m * stride, (m + 1) * stride])
        v = e_sorted[lo:hi] - m * stride
        al[v] = al[v] + il_sorted[lo:hi]
        aw[v] = aw[v] + w_sorted[lo:hi]
    sl = _tree(_tree(al.reshape(SL1_BLOCKS, 256).T.copy()))
    sw = _tree(_tree(aw.reshape(SL1_BLOCKS, 256).T.copy()))
    denom = sw + F(1e-10)
    out = np.array([sl / denom, sl, sw], F)

    # ---- backward: per cell and matched class, output rows ascending, output columns ascending, skipping everything else
    up = F(1.0 if upstream is None else upstream)
    g = (dp / denom) * up
    assert g.dtype == F
    cls_map = np.zeros((B, Ho, Wo), np.int64)
    g_map = np.zeros((B, Ho, Wo, 3), F)
    cls_map[bi, yi, xi] = li
    g_map[bi, yi, xi] = g
    acc = np.zeros((B, H, W, C, 3), F)
    ci, cj = np.arange(H), np.arange(W)
    for ty in range(k):
        oy = s * ci + ty - pad
        iy = ci[(oy >= 0) & (oy < Ho)]
        for tx in range(k):
            ox = s * cj + tx - pad
            jx = cj[(ox >= 0) & (ox < Wo)]
            w = tab[ty] * tab[tx]
            cm = cls_map[:, (s * iy + ty - pad)[:, None], (s * jx + tx - pad)[None, :]]
            bb, ii, jj = np.nonzero(cm > 0)
            gi, gj, gl = iy[ii], jx[jj], cm[bb, ii, jj]
            acc[bb, gi, gj, gl] = acc[bb, gi, gj, gl] + w * g_map[bb, s * gi + ty - pad, s * gj + tx - pad]
    dz = acc.reshape(B, H, W, C3)

    # ---- dbias: per tile the own pixels' rows ascending in x from +0, the row sums ascending in y from +0 (float64); then
    #      per channel thread t of 256 takes tiles t, t + 256, ... from +0 and a halving tree. (Dense here: an absent term is
    #      a float64 +0 added to a sum that is never -0.)
    th, tw = tile_shape(k, s)
    tiles_y, tiles_x = (H + th - 1) // th, (W + tw - 1) // tw
    G = np.zeros((B, tiles_y * th * s, tiles_x * tw * s, C3), np.float64)
    G[bi[:, None], yi[:, None], xi[:, None], ch] = g
    G = G.reshape(B, tiles_y, th * s, tiles_x, tw * s, C3)
    rowsum = np.zeros((B, tiles_y, th * s, tiles_x, C3), np.float64)
    for x in range(tw * s):
        rowsum = rowsum + G[:, :, :, :, x, :]
    part = np.zeros((B, tiles_y, tiles_x, C3), np.float64)
    for y in range(th * s):
        part = part + rowsum[:, :, y]
    part = part.reshape(-1, C3)
    nblk = part.shape[0]
    lanes = np.zeros((256, C3), np.float64)
    for m in range((nblk + 255) // 256):
        chunk = part[m * 256:(m + 1) * 256]
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    dbias = _tree(lanes).astype(F)
    return dict(out=out, dz=dz, dbias=dbias, n_matched=len(bi))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == F and np.array_equal(a.view(np.uint32), b.view(np.uint32))
