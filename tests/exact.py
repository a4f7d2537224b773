"""Exact-arithmetic support for tests/test_exact_cpu.py and tests/test_gpu_exact.py.

The dense kernels (Winograd trunk, first layers, FC family, small heads, bilinear deconv) use nothing but fp32
multiply-adds, MFMAs and multiplications by small dyadic constants. On integer-valued inputs (or fixed dyadic
fractions) for which the sum of the ABSOLUTE values of all terms of every output stays below 2^24 units of the
output's last dyadic place, every partial sum in every association order is an integer of fewer than 24 bits: fp32
evaluates it exactly, with or without FMA, through split-K partials, column folds, pools and reductions. The kernel's
fp32 answer must then EQUAL the float64 answer, whatever order the kernel sums in.

This module holds what both test files share:
  * seeded generators of integer-valued fp32 tensors (`ints`, `poison_rows`);
  * float64 references written in torch (they run on either device; the float64 library GEMM is exact on these
    integers, being far below 2^53), each with an `absolute=True` form that runs the same pipeline on absolute values
    with |A^T|, |B^T| and returns the per-output sum of absolute terms;
  * `abs_bound(...)`: the largest such sum in units of the output's least significant dyadic step, to be asserted
    `< LIMIT` BEFORE a test looks at a kernel's output (a bad input choice then fails as "input not exact", never as
    a kernel bug);
  * `first_mismatch(got, ref, meta)`: count + first coordinates + the derived workgroup coordinates of a failure;
  * the case lists of the GPU file, which the CPU file checks for exactness and for the dispatch regimes they claim.
"""
import ctypes

import numpy as np
import torch

LIMIT = 1 << 24

# F(4x4,3x3): V = B^T d B per 6x6 input patch, Y = A^T M A per 6x6 product tile, U = G g G^T per 3x3 filter
BT6 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
AT6 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
G6 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
AT6_ROW_SUM = 19          # largest row sum of |A^T| (1 + 1 + 8 + 8 + 1); squared it bounds one output's weight on |M|


def _mat(rows, like, absolute=False):
    m = torch.tensor(rows, dtype=torch.float64, device=like.device)
    return m.abs() if absolute else m


# ---- generators -----------------------------------------------------------------------------------------------------
def ints(seed, shape, lo, hi, zero_frac=0.0, device=None):
    """Seeded integer-valued fp32 tensor, uniform on [lo, hi]; `zero_frac` of the entries forced to zero."""
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, hi + 1, size=shape).astype(np.float32)
    if zero_frac:
        a[rng.random(size=shape) < zero_frac] = 0
    t = torch.from_numpy(a)
    return t.to(device) if device is not None else t


def ints_dev(seed, shape, lo, hi, device):
    """`ints` for operands of hundreds of megabytes: drawn on `device` by torch's seeded generator."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=device, dtype=torch.int32).to(torch.float32)


def poison_rows(x, count):
    """A copy of x whose rows at or past `count` are NaN: whatever reads them shows in every output it touches."""
    p = x.clone()
    p[count:] = float("nan")
    return p


# ---- F(4x4,3x3) references -----------------------------------------------------------------------------------------
def wino43_filter64(w):
    """torch filter [Cout, Cin, 3, 3] -> U^T float64 [36, Cout, Cin] = (G g G^T)[i][j] at plane 6 i + j."""
    G = _mat(G6, w)
    u = torch.einsum("ir,ocrs,js->ijoc", G, w.double(), G)
    return u.reshape(36, w.shape[0], w.shape[1])


def wino43_input_reference(x, absolute=False):
    """x [B,H,W,C] -> V float64 [36, B*Ht*Wt, C]: B^T d B of the 6x6 patches at stride 4 of the SAME-padded input
    (one zero row / column in front; zeros behind up to the patch grid), tile t = (b Ht + ty) Wt + tx."""
    B, H, W, C = x.shape
    Ht, Wt = (H + 3) // 4, (W + 3) // 4
    x = x.double().abs() if absolute else x.double()
    xp = torch.zeros((B, 4 * Ht + 2, 4 * Wt + 2, C), dtype=torch.float64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    d = torch.stack([torch.stack([xp[:, r:r + 4 * Ht:4, s:s + 4 * Wt:4] for s in range(6)]) for r in range(6)])   # [r, s, B, Ht, Wt, C]
    bt = _mat(BT6, x, absolute)
    v = torch.einsum("ir,rsbyxc,js->ijbyxc", bt, d, bt)
    return v.reshape(36, B * Ht * Wt, C)


def wino43_reference(v, ut, bias, B, H, W, relu, pool, groups, absolute=False):
    """y = [pool][ReLU](A^T (sum_ci V[k] U[k]) A + bias) in float64: v [36,T,Cin], ut [groups,36,Cout,Cin], bias
    [groups,Cout]; image b uses filter set b // (B // groups). Cropped to [:H, :W]. pool: 0 -> y [B,H,W,Cout];
    1 -> its 2x2 max-pool; 2 -> (y, pooled). absolute=True: the same pipeline on |V|, |U|, |A^T|, |bias| (no ReLU
    needed, the pool's max kept): every output's sum of absolute terms."""
    Ht, Wt = (H + 3) // 4, (W + 3) // 4
    T = B * Ht * Wt
    Cout = ut.shape[-2]
    assert v.shape[0] == 36 and v.shape[1] == T and T % groups == 0 and B % groups == 0
    tpg = T // groups
    v, ut, bias = v.double(), ut.double().reshape(groups, 36, Cout, -1), bias.double().reshape(groups, Cout)
    if absolute:
        v, ut, bias = v.abs(), ut.abs(), bias.abs()
    m = torch.cat([torch.bmm(v[:, g * tpg:(g + 1) * tpg], ut[g].transpose(1, 2)) for g in range(groups)], dim=1)   # [36, T, Cout]
    at = _mat(AT6, v, absolute)
    y = torch.einsum("ai,ijbyxc,ej->byaxec", at, m.reshape(6, 6, B, Ht, Wt, Cout), at).reshape(B, 4 * Ht, 4 * Wt, Cout)
    del m
    y = y[:, :H, :W] + bias.repeat_interleave(B // groups, dim=0)[:, None, None, :]
    if relu and not absolute:
        y = torch.relu(y)
    if pool == 0:
        return y
    yp = y.reshape(B, H // 2, 2, W // 2, 2, Cout).amax(dim=(2, 4))
    return yp if pool == 1 else (y, yp)


def conv3x3_c3_reference(x, w, b, relu, groups=1, absolute=False):
    """Direct float64 3x3 / SAME convolution of a 3-channel NHWC input: w [groups,3,3,3,Cout] (ky, kx, ci, co),
    b [groups,Cout]; image i uses set i // (B // groups). -> [B,H,W,Cout]."""
    B = x.shape[0]
    Cout = w.shape[-1]
    x, w, b = x.double(), w.double().reshape(groups, 3, 3, 3, Cout), b.double().reshape(groups, Cout)
    if absolute:
        x, w, b = x.abs(), w.abs(), b.abs()
    B, H, W = x.shape[:3]
    per = B // groups
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.cat([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], dim=-1)      # [B,H,W,27] in (ky, kx, ci) order
    y = torch.cat([cols[g * per:(g + 1) * per] @ w[g].reshape(27, Cout) + b[g] for g in range(groups)])   # (a matrix product: exact on either device)
    return torch.relu(y) if relu and not absolute else y


def conv12_reference(x, w1, b1, ut2, b2, relu1, relu2, groups, absolute=False):
    """max_pool_2x2([ReLU](conv1_2([ReLU](conv1_1(x))))) in float64 with conv1_2 given in the transform domain:
    direct 3 -> 64 conv + bias + ReLU, 6x6 tiles with SAME padding, B^T d B, then `wino43_reference` with pool = 1.
    absolute=True: the bound stage by stage, (sum |x| |w1| + |b1|, |B^T| |a| |B^T|^T, |A^T| (sum |V| |U|) |A^T|^T + |b2|),
    each stage on the TRUE output a resp. V of the one before (propagating the absolute values through all three stages
    at once would bound an evaluation that folds the stages into one sum, which no kernel does: the kernel materialises
    conv1_1's output and V, both exact once their own stage's bound holds, and each is then an input like any other)."""
    B, H, W, _ = x.shape
    a = conv3x3_c3_reference(x, w1, b1, relu1, groups)
    v = wino43_input_reference(a)
    if absolute:
        return (conv3x3_c3_reference(x, w1, b1, relu1, groups, True), wino43_input_reference(a, True),
                wino43_reference(v, ut2, b2, B, H, W, relu2, 1, groups, True))
    return wino43_reference(v, ut2, b2, B, H, W, relu2, 1, groups)


# ---- FC, heads, deconv ----------------------------------------------------------------------------------------------
def fc_reference(x, wt, bias, addend=None, absolute=False):
    """x @ wt.T + bias (+ addend) in float64; activations are applied by the caller."""
    x, wt, bias = x.double(), wt.double(), bias.double()
    if absolute:
        x, wt, bias = x.abs(), wt.abs(), bias.abs()
    y = x @ wt.t() + bias
    if addend is not None:
        y = y + (addend.double().abs() if absolute else addend.double())
    return y


def deconv_filter_1d(k):
    """lib/networks/network.py make_deconv_filter: f = ceil(k / 2), c = (2 f - 1 - f % 2) / (2 f), w[x] = 1 - |x / f - c|."""
    f = (k + 1) // 2
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    return [1 - abs(x / f - c) for x in range(k)]


def deconv_reference(x, k, s, add1=None, add2=None, bias=None, relu=False, absolute=False):
    """The fixed bilinear transposed convolution (per channel; SAME: padding (k - s) / 2, output H s x W s) in float64,
    plus optional addends, bias, ReLU. For k = 4 the 2-D taps are multiples of 1/16, for k = 16 of 1/256."""
    B, H, W, C = x.shape
    f = deconv_filter_1d(k)
    p = (k - s) // 2

    def up(n):   # [n s, n]: output o takes input i with tap f[o + p - i s]
        m = torch.zeros((n * s, n), dtype=torch.float64)
        for o in range(n * s):
            for i in range(n):
                if 0 <= o + p - i * s < k:
                    m[o, i] = f[o + p - i * s]
        return m.to(x.device)
    xd = x.double().abs() if absolute else x.double()
    y = torch.einsum("oh,bhwc,pw->bopc", up(H), xd, up(W))
    for t in (add1, add2, bias):
        if t is not None:
            y = y + (t.double().abs() if absolute else t.double())
    return torch.relu(y) if relu and not absolute else y


def head_reference(score4, score5, weights_t, planted=None, kernel=4, stride=2, absolute=False):
    """add = score4 + deconv(score5) [+ planted]; z = add . weights_t [U, Cout] -> (add, z) in float64."""
    add = deconv_reference(score5, kernel, stride, add1=score4, add2=planted, absolute=absolute)
    w = weights_t.double().abs() if absolute else weights_t.double()
    return add, add @ w


# ---- the exactness condition ----------------------------------------------------------------------------------------
_ABS = {
    "wino43": (wino43_reference, 1),
    "wino43_input": (wino43_input_reference, 1),
    "conv3x3_c3": (conv3x3_c3_reference, 1),
    "conv12": (conv12_reference, 1),
    "fc": (fc_reference, 1),
    "deconv4": (deconv_reference, 16),
    "deconv16": (deconv_reference, 256),
    "head": (head_reference, 16),
}


def abs_bound(kind, *args, **kwargs):
    """Largest per-output sum of absolute terms of reference `kind` on these inputs, in units of the output's least
    significant dyadic step (1 for the conv and FC kernels, 1/16 for the low-resolution heads and the k = 4 deconv,
    1/256 for the k = 16 deconv). A reference of several stages returns one tensor of sums per stage (see
    `conv12_reference`); the largest over all of them counts. A partial sum never exceeds the sum of the absolute values
    of its terms, so `abs_bound < LIMIT` makes every fp32 operation of every summation order exact."""
    fn, units = _ABS[kind]
    out = fn(*args, absolute=True, **kwargs)
    out = out if isinstance(out, tuple) else (out,)
    return max(float(t.max()) for t in out if t.numel()) * units if any(t.numel() for t in out) else 0.0


def wino43_closed_bound(cin, vmax, umax, bmax):
    """Worst case of the raw V / U family without looking at the data: 361 Cin vmax umax + bmax."""
    return AT6_ROW_SUM ** 2 * cin * vmax * umax + bmax


def fc_closed_bound(K, a, b, bmax, addmax=0):
    return K * a * b + bmax + addmax


# ---- failure report -------------------------------------------------------------------------------------------------
def first_mismatch(got, ref, meta=None, limit=6):
    """None when `got` (fp32, from the kernel) equals `ref` (float64) element for element BY VALUE (-0.0 == 0.0; a NaN
    in `got` never equals), else a report: the number of wrong elements and the first few coordinates with got / want.
    meta: {"name": str,
           "wino": (B, H, W, groups, pooled)  -> adds the 32-tile tile block, 64-channel channel block and wave (c % 64 // 16),
           "fc": True                         -> adds the 64 x 64 block}."""
    meta = meta or {}
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s, want %s" % (meta.get("name", ""), tuple(got.shape), tuple(ref.shape))
    bad = ~(got.double() == ref.to(got.device).double())
    n = int(bad.sum())
    if n == 0:
        return None
    idx = torch.nonzero(bad)[:limit].cpu().tolist()
    lines = ["%s: %d of %d elements differ from the float64 reference" % (meta.get("name", "output"), n, bad.numel())]
    for i in idx:
        g, w = float(got[tuple(i)]), float(ref[tuple(i)])
        where = ""
        if "wino" in meta and len(i) == 4:
            B, H, W, groups, pooled = meta["wino"]
            b, y, x, c = i
            Ht, Wt = (H + 3) // 4, (W + 3) // 4
            ty, tx = (y // 2, x // 2) if pooled else (y // 4, x // 4)
            t = (b * Ht + ty) * Wt + tx
            tpg = B * Ht * Wt // groups
            tb = (t // tpg) * ((tpg + 31) // 32) + (t % tpg) // 32
            where = "  tile %d (ty %d, tx %d) tile block %d, channel block %d, wave %d" % (t, ty, tx, tb, c // 64, c % 64 // 16)
        elif meta.get("fc") and len(i) == 2:
            where = "  block (rows %d.., cols %d..)" % (i[0] // 64 * 64, i[1] // 64 * 64)
        names = ("b", "y", "x", "c") if len(i) == 4 else ("row", "col") if len(i) == 2 else tuple("i%d" % k for k in range(len(i)))
        lines.append("  (%s) got %r want %r%s" % (", ".join("%s=%d" % p for p in zip(names, i)), g, w, where))
    return "\n".join(lines)


def check(got, ref, meta=None):
    msg = first_mismatch(got, ref, meta)
    assert msg is None, msg


def zero_bits(t):
    """True when every element of the fp32 tensor is +0.0 (all-zero bits: no -0.0, no NaN)."""
    return not bool(t.contiguous().view(torch.int32).any())


# ---- host-side dispatch of the trunk launcher (csrc/wino_mfma.hip) -------------------------------------------------------
def wino43_regime(shape, cout, groups):
    """What pcnn_winograd43_conv_fwd decides on the host for this launch: S (the Cin split, read back from the
    library's own pcnn_winograd43_conv_workspace_bytes: S = (bytes / 4 - groups Cout) / (B H W Cout), 1 when it asks for
    no workspace), ncb (64-channel blocks), nbt (32-tile blocks over all groups), tiles per group, and which side of
    the launcher's `u_bytes > v_bytes` rule the launch is on (the channel-block-major map needs ncb == 8)."""
    from posecnn_amd import _lib
    B, H, W, cin = shape
    n = ctypes.c_size_t()
    _lib.check("pcnn_winograd43_conv_workspace_bytes", _lib.lib().pcnn_winograd43_conv_workspace_bytes(B, H, W, cin, cout, groups, ctypes.byref(n)))
    words = n.value // 4
    S = 1 if n.value == 0 else (words - groups * cout) // (B * H * W * cout)
    assert n.value == 0 or (words - groups * cout) == S * B * H * W * cout
    T = B * ((H + 3) // 4) * ((W + 3) // 4)
    tpg = T // groups
    return {"S": S, "ncb": cout // 64, "nbt": groups * ((tpg + 31) // 32), "tpg": tpg,
            "u_heavier": 36.0 * cout * cin * 4.0 * groups > 36.0 * T * cin * 4.0}


# ---- case lists -----------------------------------------------------------------------------------------------------
def wino_cases():
    """(shape (B,H,W,Cin), Cout, pool, groups): the list of test_winograd43_mfma_conv_kernel plus what
    tests/test_exact_cpu.py's coverage check found missing from it (see WINO_EXTRA)."""
    from test_gpu_ops import WINO43_MFMA_CASES
    return list(WINO43_MFMA_CASES) + WINO_EXTRA


# What the coverage check of tests/test_exact_cpu.py found missing from the base list (S = the Cin split the library reports):
WINO_EXTRA = [
    ((1, 60, 80, 128), 128, 1, 1),     # S = 2 with pool 1 (the base list has S = 2 with pool 0 and 2 only)
    ((1, 120, 160, 512), 512, 1, 1),   # ncb == 8 with V heavier than U: eight channel blocks on the tile-block-major map
    ((1, 80, 100, 256), 512, 2, 1),    # ncb == 8, U heavier, 128 workgroups: the channel-block-major map WITHOUT a split
    ((1, 30, 40, 512), 512, 0, 1),     # conv5_x of one frame: S = 8 on the channel-block-major map, three tile blocks
    ((1, 60, 80, 512), 512, 0, 1),     # conv4_x of one frame: S = 4 on the channel-block-major map, ragged last tile block
]
WINO_VMAX, WINO_UMAX, WINO_BMAX = 8, 8, 1024
# run once more with no workspace handed to the entry: the launcher must fall back to S = 1 and give the same answer
WINO_NO_WORKSPACE_CASE = ((2, 30, 38, 256), 256, 2, 2)

# conv1_1 -> conv1_2 -> pool1: (B, H, W, groups); every one with both ut2 layouts and (relu1, relu2) in CONV12_RELUS
CONV12_CASES = [(1, 16, 16, 1), (2, 32, 48, 1), (3, 48, 16, 1), (4, 48, 32, 2), (2, 480, 640, 2)]
CONV12_RELUS = [(1, 1), (0, 1), (1, 0)]
CONV12_X, CONV12_U = 2, 2            # blob path: x in [-2, 2], |U| <= 2; w1 in {-1, 0, 1}, b1 in [-3, 3], b2 in [-64, 64]
CONV12_RAW_X, CONV12_RAW_U = 4, 1    # raw path: uint8 pixels within +-4 of the integer means, |U| <= 1
CONV12_RAW_CASES = [(1, 16, 16), (2, 32, 48), (3, 32, 32), (2, 96, 128)]
RAW_MEANS = (103.0, 116.0, 123.0)

# first layer: ((B, H, W), Cout, groups) — the shapes of test_conv3x3_c3_bias_relu and of
# test_first_conv_fused_into_winograd_input_transform, plus grouped ones
CONV1_CASES = [((2, 48, 64), 64, 1), ((1, 5, 131), 64, 1), ((1, 33, 7), 128, 1), ((1, 1, 1), 64, 1), ((1, 17, 300), 64, 1),
               ((2, 16, 32), 64, 2), ((1, 30, 50), 64, 1), ((1, 5, 7), 128, 1), ((4, 9, 13), 64, 2), ((1, 480, 640), 64, 1)]
CONV1_X, CONV1_W, CONV1_B = 128, 16, 1024     # |x| <= 128 (a colour blob), |w| <= 16, |b| <= 1024: (27 128 16 + 1024) 10^2 = 5.6 M after B^T d B

# FC family. x, w integers in [-FC_A, FC_A]; bias, addend in [-FC_BIAS, FC_BIAS]: K a b + |bias| + |addend| (closed form)
FC_A, FC_BIAS = 24, 1 << 16
# (capacity, K, N, with the device count, also with num_rows=None, addend): the configurations of the count sweep
FC_ROWS_CASES = [
    (3024, 8192, 4096, True, False, False),     # grid.y = 2, the balance split
    (3024, 4096, 4096, True, False, False),     # fc7: never splits
    (3024, 25088, 4096, True, False, False),    # fc6
    (200, 25088, 256, True, False, False),      # small capacity: up to 8 splits, the `live <= 512` exit
    (512, 2048, 1024, True, False, True),       # ... with an addend inside a split regime
    (600, 2048, 1024, True, True, False),       # capacity over the workspace's 512 rows
    (1100, 8192, 2048, True, True, False),
    (64, 128, 64, True, False, False),          # two K stages
]
FC_TALL_CASES = [(4800, 512, 64), (76800, 512, 128)]   # the tall map of the 1x1 heads: num_rows=None, with and without addend
FC_SPLIT_CASE = (700, 2048, 256, 128)           # fc_rows_split: capacity, K, out_a, out_b
FC_COLS_CASE = (700, 4096, 88, 128)             # fc_rows_cols: capacity, K, out_features, padded
FC_SKINNY_M = [1, 5, 16, 17, 21, 32]
FC_SKINNY_K = [25088, 4096, 2512]               # 2512 = 16 * 157: the K slices end in clamped steps
FC_SKINNY_N = [4096, 88, 128]
# Two more (K, N) pairs. In the nine above a clamped step (a slice of an odd number of 16-float steps) only ever runs in
# column group 0 (N <= 128: one group) or in the last K slice (N = 4096, K = 2512: 7 slices of 20 steps and one of 17);
# a value mutant of the clamped step in another group's first slice passed all nine. Here every full slice is odd (17
# resp. 25 steps) in two column groups, the second one ragged for N = 200.
FC_SKINNY_KN_EXTRA = [(2064, 200), (25088, 256)]


def fc_skinny_kn():
    return [(K, N) for K in FC_SKINNY_K for N in FC_SKINNY_N] + FC_SKINNY_KN_EXTRA


def fc_counts(capacity):
    """{0, 1, 2} + {64 k - 1, 64 k, 64 k + 1} + {capacity}, clipped to the capacity: every 64-row block boundary, where
    the device-side split decision (a function of the block count) can change. Nothing is thinned: the whole sweep of the
    largest configuration costs a fraction of a second on the GPU."""
    c = {0, 1, 2, capacity}
    for k in range(1, capacity // 64 + 2):
        c.update((64 * k - 1, 64 * k, 64 * k + 1))
    return sorted(v for v in c if 0 <= v <= capacity)


def skinny_counts(M):
    """Device counts on both sides of 16 (the second row block is skipped at <= 16), the ends, and None (= M)."""
    return [None] + sorted({c for c in (0, 1, 15, 16, 17, M - 1, M) if 0 <= c <= M})


# heads: (B, h, w, U, Cout, planted). Pixel counts that are no multiple of 32 / 64, B > 1 so a workgroup straddles images.
HEAD_CASES = [(3, 6, 10, 64, 22, True), (2, 10, 14, 128, 66, False), (3, 6, 10, 128, 96, True), (2, 14, 18, 64, 66, True),
              (5, 6, 6, 64, 96, False), (2, 60, 80, 128, 22, True)]
HEAD_X, HEAD_W = 64, 16              # scores / planted integers in [-64, 64], weights in [-16, 16]


def head_lowres_fits(U, Cout):
    """The one-launch vector-ALU head keeps 32 pixels x U plus the U x Cout filter in 60 KB of LDS (pcnn_head_lowres_fwd)."""
    return 4 * (32 * U + U * Cout) <= 60 * 1024


# deconv: the shapes of test_deconv_bilinear, each at both (k, s) of the network
DECONV_SHAPES = [(2, 30, 40, 64), (1, 60, 80, 128), (2, 7, 9, 66), (1, 5, 6, 22), (1, 3, 4, 5), (1, 4, 4, 3)]
DECONV_KS = [(4, 2), (16, 8)]
DECONV_X = 1 << 12                   # |x|, |add1|, |add2|, |bias| <= 4096: 4 * 4096 * 256 = 2^22 units of 1/256

# the chain family: integer activations through ops.winograd_input and then the trunk kernel (input-transform partials included)
CHAIN_CASES = [((1, 30, 40, 512), 512, 0, 1), ((2, 60, 80, 256), 256, 1, 2), ((1, 120, 160, 64), 64, 2, 1)]
CHAIN_X, CHAIN_U = 3, 2              # x in [0, 3] with half the entries zero (a ReLU's output), |U| <= 2


# ---- seeded inputs of the cases (the CPU file bounds exactly what the GPU file runs) -----------------------------------
def seed_of(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


def wino_inputs(case, device=None):
    """Raw integer V [36,T,Cin], U^T [groups,36,Cout,Cin] and bias [groups,Cout] of one trunk case: 36 independent random
    planes, so a mix-up of two transform planes shows."""
    (B, H, W, cin), cout, pool, groups = case
    T = B * ((H + 3) // 4) * ((W + 3) // 4)
    s = seed_of("wino", case)
    return (ints(s, (36, T, cin), -WINO_VMAX, WINO_VMAX, device=device), ints(s + 1, (groups, 36, cout, cin), -WINO_UMAX, WINO_UMAX, device=device),
            ints(s + 2, (groups, cout), -WINO_BMAX, WINO_BMAX, device=device))


def chain_inputs(case, device=None):
    (B, H, W, cin), cout, pool, groups = case
    s = seed_of("chain", case)
    return (ints(s, (B, H, W, cin), 0, CHAIN_X, zero_frac=0.5, device=device), ints(s + 1, (groups, 36, cout, cin), -CHAIN_U, CHAIN_U, device=device),
            ints(s + 2, (groups, cout), -WINO_BMAX, WINO_BMAX, device=device))


def conv12_inputs(B, H, W, groups, amp=CONV12_X, umax=CONV12_U, device=None):
    """x [B,H,W,3] in [-amp, amp], w1 in {-1, 0, 1}, b1 in [-3, 3], U2^T [groups,36,64,64] in [-umax, umax], b2 in [-64, 64]."""
    s = seed_of("conv12", B, H, W, groups, amp, umax)
    return (ints(s, (B, H, W, 3), -amp, amp, device=device), ints(s + 1, (groups, 3, 3, 3, 64), -1, 1, device=device),
            ints(s + 2, (groups, 64), -3, 3, device=device), ints(s + 3, (groups, 36, 64, 64), -umax, umax, device=device),
            ints(s + 4, (groups, 64), -64, 64, device=device))


def raw_frames(x, means=RAW_MEANS):
    """uint8 BGR frames whose blob (pixel - mean) is the integer tensor x [B,H,W,3] (|x| small against the means)."""
    return (x + torch.tensor(means, dtype=torch.float32, device=x.device)).to(torch.uint8)


def conv1_inputs(shape, cout, groups, device=None):
    B, H, W = shape
    s = seed_of("conv1", shape, cout, groups)
    return (ints(s, (B, H, W, 3), -CONV1_X, CONV1_X, device=device), ints(s + 1, (groups, 3, 3, 3, cout), -CONV1_W, CONV1_W, device=device),
            ints(s + 2, (groups, cout), -CONV1_B, CONV1_B, device=device))


def head_inputs(case, device=None):
    B, h, w, U, cout, plant = case
    s = seed_of("head", case)
    return (ints(s, (B, h, w, U), -HEAD_X, HEAD_X, device=device), ints(s + 1, (B, h // 2, w // 2, U), -HEAD_X, HEAD_X, device=device),
            ints(s + 2, (U, cout), -HEAD_W, HEAD_W, device=device), ints(s + 3, (B, h, w, U), -HEAD_X, HEAD_X, device=device) if plant else None)


def deconv_inputs(shape, stride, device=None):
    B, H, W, C = shape
    s = seed_of("deconv", shape, stride)
    out = (B, H * stride, W * stride, C)
    return (ints(s, shape, -DECONV_X, DECONV_X, device=device), ints(s + 1, out, -DECONV_X, DECONV_X, device=device),
            ints(s + 2, out, -DECONV_X, DECONV_X, device=device), ints(s + 3, (C,), -DECONV_X, DECONV_X, device=device))
