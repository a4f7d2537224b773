"""The (kernel, stride) geometries the kernels that include posecnn_amd/csrc/bilinear.h accept, and a host mirror of what
their launchers decide for each. TEST INFRASTRUCTURE ONLY: no GPU; nothing here calls the library.

  bilinear_tap / make_taps    bilinear.h restated: first input index, tap count and the f32 weights of one output index
  dense_matrix                the [n s, n] interpolation matrix those taps make (float64 of the f32 weights)
  label_head_plan             pcnn_upscore_softmax_argmax{,_hard}_fwd (upscore.hip): nseg, rows, ncx_max, s_out_off, LDS bytes
  label_loss_plan             pcnn_label_head_loss_{fwd,bwd} (label_loss.hip): the same tile, the LDS bytes of both directions
  segments / staging_elements what each 128-pixel workgroup of those kernels stages: cx0, ncx, first pixel, loop elements
  vertex_plan                 pcnn_vertex_head_loss_bwd (vertex_head_loss.hip): ladder rung, tile, footprint, LDS bytes
  TABLE / cases()             the geometries of tests/test_gpu_bilinear_geometry.py, each with the branch it is there for

tests/test_bilinear_geometry_cpu.py asserts every claim made here; tests/GEOMETRY.md records what the GPU run showed."""
import functools

import numpy as np

F = np.float32
UP_SEG = 128                  # pixels (= threads) per workgroup of the label head and of label_head_loss
MAX_CLASSES = 64              # PCNN_MAX_CLASSES
MAX_KERNEL = 64               # the s_tab[64] tap tables
LDS_LIMIT = 160 * 1024        # what the launchers compare their dynamic LDS request with
VH_FOOTPRINT = 3072
VH_LADDER = ((4, 8), (4, 4), (2, 4), (2, 2), (1, 2), (1, 1))
FIXED_CLASSES = (22, 14, 16)  # compile-time instances of the label head


# ---- bilinear.h ---------------------------------------------------------------------------------------------------------
def bilinear_tap(t, k):
    f = (k + 1) // 2
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    return F(1.0 - abs(t / float(f) - c))


def tap_table(k):
    return np.array([bilinear_tap(t, k) for t in range(k)], F)


def is_dyadic(k):
    """True when every tap of the kernel is a multiple of 1 / (2 f) with f a power of two: products and short sums of
    integers times taps are then exact in float32 and float64 alike."""
    f = (k + 1) // 2
    return f & (f - 1) == 0


def exact_gradient_range(k):
    """Largest power of two gmax <= 8 such that a cell's k x k gather of integers |g| <= gmax is exact in float32 for dyadic
    taps: the taps' absolute sum is (sum of the 1-D taps)^2, in units of 1 / (4 f^2), and must stay below 2^24 units."""
    f = (k + 1) // 2
    total = float(tap_table(k).astype(np.float64).sum()) ** 2
    gmax = 8
    while gmax >= 1 and total * gmax * 4 * f * f >= (1 << 24):
        gmax //= 2
    return gmax


def make_taps(o, k, s, n_in):
    """make_taps(o, k, s, (k - s) / 2, n_in): (lo, n, [w0, w1, w2, w3]) with C's truncating division."""
    pad = (k - s) // 2
    a = o + pad
    lo = (a - k + 1 + s - 1) // s if a - k + 1 >= 0 else -((k - 1 - a) // s)
    hi = a // s
    lo = max(lo, 0)
    hi = min(hi, n_in - 1)
    n = max(hi - lo + 1, 0)
    assert n <= 4, (o, k, s, n)
    w = [bilinear_tap(a - s * (lo + j), k) if j < n else F(0) for j in range(4)]
    return lo, n, w


def tap_counts(k, s, n_in):
    return [make_taps(o, k, s, n_in)[1] for o in range(n_in * s)]


def dense_matrix(k, s, n_in):
    m = np.zeros((n_in * s, n_in), np.float64)
    for o in range(n_in * s):
        lo, n, w = make_taps(o, k, s, n_in)
        for j in range(n):
            m[o, lo + j] = float(w[j])
    return m


def accepted(k, s, limit=4):
    """The argument check shared by the deconv, the label head, label_head_loss (limit 4, the latter two with k <= 64) and
    vertex_head_loss (limit 2, k <= 64)."""
    return s >= 1 and s <= k <= limit * s and (k - s) % 2 == 0


# ---- upscore.hip / label_loss.hip: the 128-pixel segment ---------------------------------------------------------------
def label_head_plan(W, C, k, s):
    Wo = W * s
    rows = (k + s - 1) // s
    ncx_max = (UP_SEG - 1) // s + rows + 1
    s_out_off = (rows * ncx_max * C + 3) // 4 * 4
    return dict(nseg=(Wo + UP_SEG - 1) // UP_SEG, rows=rows, ncx_max=ncx_max, s_out_off=s_out_off,
                lds_bytes=4 * (s_out_off + UP_SEG * C))


def label_loss_plan(W, C, k, s):
    p = label_head_plan(W, C, k, s)
    return dict(p, sh_fwd=4 * p["s_out_off"], sh_bwd=p["lds_bytes"], fits=p["lds_bytes"] + 4096 <= LDS_LIMIT)


def label_head_kernel(C, al8=True, s_out_off=0):
    """Which instance the label head's launcher picks."""
    if al8 and s_out_off % 2 == 0 and C in FIXED_CLASSES:
        return "fixed<%d>" % C
    return "generic<24>" if C <= 24 else "generic<64>"


def segments(W, k, s):
    """Per workgroup of one output row: (ox0, npx, cx0, ncx)."""
    Wo = W * s
    out = []
    for ox0 in range(0, Wo, UP_SEG):
        npx = min(UP_SEG, Wo - ox0)
        first, last = make_taps(ox0, k, s, W), make_taps(ox0 + npx - 1, k, s, W)
        out.append((ox0, npx, first[0], last[0] + (last[1] if last[1] > 0 else 1) - first[0]))
    return out


def staging_elements(h, W, C, k, s, fixed):
    """Largest element count of the staging loop over the workgroups of a case (the loop advances 4 x 128 elements a
    trip; the compile-time kernel copies float2 pairs, the generic kernels floats)."""
    ny = max(tap_counts(k, s, h))
    ncx = max(seg[3] for seg in segments(W, k, s))
    return ny * (ncx * C // 2 if fixed else ncx * C)


def first_pixels(B, h, W, k, s):
    """pix0 = (b Ho + oy) Wo + ox0 of every workgroup."""
    Ho, Wo = h * s, W * s
    return [(b * Ho + oy) * Wo + ox0 for b in range(B) for oy in range(Ho) for ox0 in range(0, Wo, UP_SEG)]


# ---- vertex_head_loss.hip ----------------------------------------------------------------------------------------------
def vertex_plan(k, s, H=None, W=None):
    rung, (th, tw) = None, (1, 1)
    for i, (a, b) in enumerate(VH_LADDER):
        if (a * s + k - s) * (b * s + k - s) <= VH_FOOTPRINT:
            rung, (th, tw) = i, (a, b)
            break
    fp = (th * s + k - s) * (tw * s + k - s)
    p = dict(rung=rung, th=th, tw=tw, footprint=fp, shmem=(fp * 13 + 15) // 16 * 16)
    if H is not None:
        # a last tile with fewer cells than th (tw): only tiles of more than one cell can be clipped
        p.update(tiles_y=(H + th - 1) // th, tiles_x=(W + tw - 1) // tw, nth=min(th, H), clipped_y=H % th != 0, clipped_x=W % tw != 0)
    return p


# ---- the table ---------------------------------------------------------------------------------------------------------
B, H_LOW = 2, 3
# Wo = w s crosses one 128-pixel segment boundary and leaves a short last segment
WIDTHS = {1: (129, 127), 2: (65,), 3: (43,), 8: (17,), 13: (10,), 16: (9,), 32: (5,)}

# (k, s), the tap counts per axis the row must show, the branch it is there to reach
TABLE = (
    ((1, 1), {1}, "one tap, the identity: k = s = 1, odd Wo; pad 0"),
    ((2, 2), {1}, "one tap, even stride"),
    ((13, 13), {1}, "one tap, odd k and s; f = 7 (taps not dyadic)"),
    ((4, 2), {1, 2}, "anchor: the network's score deconv"),
    ((16, 8), {1, 2}, "anchor: the network's upscore deconv"),
    ((64, 32), {1, 2}, "two taps at k = 64: a full 64-entry tap table; vertex_head_loss without a ladder rung"),
    ((3, 1), {2, 3}, "third tap at s = 1: the widest ncx (129 of ncx_max 131), the largest LDS tile, odd Wo and pix0"),
    ((6, 2), {2, 3}, "third tap, even stride; taps not dyadic (f = 3); bilinear_at3's else branch"),
    ((8, 2), {2, 3, 4}, "fourth tap (interior pixels), clipped to 3 and 2 at the borders"),
    ((64, 16), {2, 3, 4}, "fourth tap from a full 64-entry tap table; h = 3 < 4 rows clips every ty"),
    ((7, 3), {1, 2, 3}, "3 and 2 taps alternate inside one segment; odd k, odd s, odd Wo and pix0"),
    ((5, 3), {1, 2}, "2 and 1 taps alternate inside one segment; odd k, odd s; taps not dyadic (f = 3)"),
)
KS = tuple(row[0] for row in TABLE)


def cases(ks_list=KS):
    """-> [(k, s, w)]: every width of every geometry (s = 1 has two, so that Wo is odd either way round a segment)."""
    return [(k, s, w) for (k, s) in ks_list for w in WIDTHS[s]]


def case_id(c):
    return "k%ds%d-w%d" % c


DECONV_CLASSES = (3, 22, 64)
HEAD_CLASSES = (22, 5, 25)                                   # fixed kernel, generic <24> (odd), generic <64>
DISPATCH_CLASSES = (2, 14, 16, 22, 23, 24, 25, 63, 64)
DISPATCH_KS = ((16, 8), (4, 2))
LDS_CASES = (((4, 2), 64, 66560), ((3, 1), 64, 133376))      # (k, s), C, dynamic LDS bytes of the label head
REFUSED = ((65, 16, 8), (22, 66, 22), (22, 5, 2), (22, 9, 2))  # (C, k, s): C > 64, k > 64, odd difference, k > 4 s

HOUGH_KS = ((6, 2), (8, 2), (3, 1), (7, 3))
HOUGH_SHAPE = {1: (1, 96, 128, 6, 2), 2: (1, 96, 128, 6, 2), 3: (1, 96, 126, 6, 2)}    # B, H, W, C, objects of lowres_case
HOUGH_LABEL_THRESHOLD = 60
HOUGH_SKIP = 10

LOSS_KS = ((2, 2), (3, 1), (6, 2), (8, 2), (7, 3), (64, 16))
LOSS_CLASSES = (22, 5, 25, 64)


def label_loss_cases():
    """-> [((B, h, w), C, (k, s))] in the form of label_loss_ref.cases()."""
    return [((B, H_LOW, w), C, (k, s)) for (k, s, w) in cases(LOSS_KS) for C in LOSS_CLASSES]


# vertex_head_loss: the rung each geometry must take (None: no rung fits, the 1 x 1 tile's footprint exceeds VH_FOOTPRINT)
VERTEX_LADDER = (((16, 8), 0), ((20, 10), 1), ((14, 14), 2), ((32, 16), 3), ((28, 28), 4), ((40, 40), 5), ((64, 32), None),
                 ((56, 56), None))
VERTEX_KINDS = ("mixed", "branches_sigma1")


def vertex_name(k, s):
    return "G%d_%d" % (k, s)


# ---- inputs of the label-head cases (shared by the CPU and the GPU file) -----------------------------------------------
HEAD_THRESHOLD = 0.5


@functools.lru_cache(maxsize=None)
def head_case(k, s, w, C):
    """z [2,3,w,C] with an all-equal pixel and a saturated row, as the memory-contract cases of the label head; gt with 40 %
    zeros (the thresholded class), labels outside [0, C) and -1; one cell where class 0 wins under ground truth 0."""
    rng = np.random.default_rng([k, s, w, C, 7])
    z = (rng.standard_normal((B, H_LOW, w, C)) * 4).astype(F)
    z[0, 0, 0, :] = 0.0
    z[0, -1, :, 1 % C] = 95.0
    bias = rng.standard_normal(C).astype(F)
    gt = rng.integers(-1, C, (B, H_LOW * s, w * s)).astype(np.int32)
    gt[rng.random(gt.shape) < 0.4] = 0
    gt[0, 0, :3] = [C, C + 5, -7]
    z[:, 1, 1, 0] = 30.0                                      # class 0 dominant under ground truth 0 somewhere: cell (1, 1) ...
    gt[:, s:2 * s, s:2 * s] = 0                               # ... and the s x s pixels it is the nearest cell of
    import oracle
    score, prob, label = oracle.upscore_softmax_argmax(z, bias, k, s, True)
    hard = oracle.hard_label(prob, gt, HEAD_THRESHOLD)
    p0 = prob[..., 0][gt == 0]
    assert (p0 < HEAD_THRESHOLD).any() and (p0 >= HEAD_THRESHOLD).any() and (score == 0).any()
    out = dict(z=z, bias=bias, gt=gt, score=score, prob=prob, label=label, hard=hard,
               label_norelu=oracle.upscore_softmax_argmax(z, bias, k, s, False)[2])
    for a in out.values():
        a.setflags(write=False)
    return out
