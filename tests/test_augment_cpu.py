"""CPU-side checks of the training augmentation (include/posecnn_hip_augment.h, posecnn_amd/augment.py): the restatement
(tests/augment_ref.py) against independent implementations, the sampler's distribution, and the C entry's host validation.

What is pinned here: the restatement's Philox4x64-10 to np.random.Philox; its 8-bit HLS to `colorsys` (float64, stdlib)
within one code, the colours on an exact rounding tie being the only disagreements (70 150 of the 132 768 test colours sit
on a tie in at least one of H, L, S — every odd max + min is a tie of L —, 22 785 of them disagree); known answers derived with exact fractions. OpenCV's own bytes are not pinned.

The float tolerance of the GPU test's Gaussian cases, max |float32 restatement - float64 restatement| over those cases, is
measured here: 1.935e-05 (printed by test_gauss_tolerance_of_the_gpu_cases; the GPU test allows 4 x that)."""
import colorsys
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import augment_cases as CS
import augment_ref as R

MASK = (1 << 64) - 1
TIES_EXPECTED = 70150


# ---- Philox ---------------------------------------------------------------------------------------------------------
def test_philox_equals_numpy():
    """np.random.Philox increments the counter before it generates: random_raw(4) of counter c is the block of c + 1."""
    rng = np.random.default_rng(3)
    cases = [((0, 0, 0, 0), (0, 0)), ((MASK, 0, 0, 0), (1, 2)), ((MASK, MASK, 5, 0), (MASK, 7)), ((12345, 1 << 40, 1, 0), CS.SEED_KEY)]
    cases += [(tuple(int(x) for x in rng.integers(0, 1 << 63, 4)), tuple(int(x) for x in rng.integers(0, 1 << 63, 2))) for _ in range(6)]
    for counter, key in cases:
        want = np.random.Philox(counter=np.array(counter, np.uint64), key=np.array(key, np.uint64)).random_raw(4)
        big = sum(c << (64 * i) for i, c in enumerate(counter)) + 1
        plus1 = [(big >> (64 * i)) & MASK for i in range(4)]
        got = R.philox4x64(plus1, key)[0]
        assert np.array_equal(got, want), (counter, key)
    # array form: consecutive counters are numpy's consecutive blocks
    want = np.random.Philox(counter=np.array([9, 8, 1, 0], np.uint64), key=np.array([5, 6], np.uint64)).random_raw(4 * 50)
    got = R.philox4x64((np.arange(10, 60, dtype=np.uint64), 8, 1, 0), (5, 6)).reshape(-1)
    assert np.array_equal(got, want)
    # and pixel_words takes word p & 3 of block p >> 2
    w = R.pixel_words(5, 7, 8, 1, (6 << 64) | 5)
    assert np.array_equal(w.reshape(-1), R.philox4x64((np.arange(9, dtype=np.uint64), 8, 1, 0), (5, 6)).reshape(-1)[:35])


# ---- 8-bit HLS against colorsys --------------------------------------------------------------------------------------
def _test_colours():
    lat = np.round(np.linspace(0, 255, 32)).astype(np.uint8)
    lattice = np.stack(np.meshgrid(lat, lat, lat, indexing="ij"), axis=-1).reshape(-1, 3)
    rand = np.random.default_rng(17).integers(0, 256, (100000, 3)).astype(np.uint8)
    return np.concatenate([lattice, rand])


def _on_a_tie(bgr):
    """Exact integer arithmetic: is 255 L, 255 S or H / 2 of the colour exactly half-way between two codes?"""
    c = bgr.astype(np.int64)
    b, g, r = c[:, 0], c[:, 1], c[:, 2]
    hi, lo = c.max(axis=1), c.min(axis=1)
    d, t = hi - lo, hi + lo
    tie_l = t % 2 == 1                                           # 255 L = (max + min) / 2
    den = np.where(t < 255, t, 510 - t)                          # 255 S = 255 d / den (either form at L = 1/2)
    den = np.where(d == 0, 1, den)
    tie_s = (d != 0) & ((510 * d) % (2 * den) == den)
    n = np.where(hi == r, g - b, np.where(hi == g, b - r, r - g))  # H / 2 = 30 n / d + a multiple of 60
    dd = np.where(d == 0, 1, d)
    tie_h = (d != 0) & ((60 * n) % (2 * dd) == dd)
    return tie_l | tie_s | tie_h


def test_hls8_is_within_one_code_of_colorsys():
    bgr = _test_colours()
    got = R.bgr_to_hls8(bgr).astype(np.int64)
    want = np.empty_like(got)
    for i, (b, g, r) in enumerate(bgr.tolist()):
        h, l, s = colorsys.rgb_to_hls(r / 255.0, g / 255.0, b / 255.0)
        want[i] = (round(h * 180.0), round(l * 255.0), round(s * 255.0))        # round(): half to even
    dh = np.abs(got[:, 0] - want[:, 0]) % 180
    dh = np.minimum(dh, 180 - dh)
    dist = np.maximum(dh, np.abs(got[:, 1:] - want[:, 1:]).max(axis=1))
    assert dist.max() <= 1
    ties = _on_a_tie(bgr)
    print("colours on a rounding tie: %d of %d; disagreements with colorsys: %d" % (ties.sum(), len(bgr), (dist > 0).sum()))
    assert int(ties.sum()) == TIES_EXPECTED
    assert not (dist > 0)[~ties].any(), "a colour off every rounding tie disagrees with colorsys"


# ---- known answers in exact fractions ---------------------------------------------------------------------------------
def _half_even(x):
    f = x.numerator // x.denominator
    rem = x - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return min(max(f, 0), 255)


def _exact_chromatic(b, g, r, d_h, d_l, d_s):
    """The header's steps 1-3 on one colour in exact rational arithmetic (the jitter is given as Fractions)."""
    fb, fg, fr = (Fraction(v, 255) for v in (b, g, r))
    vmax, vmin = max(fb, fg, fr), min(fb, fg, fr)
    l, diff = (vmax + vmin) / 2, vmax - vmin
    h = s = Fraction(0)
    if diff:
        s = diff / (vmax + vmin) if l < Fraction(1, 2) else diff / (2 - vmax - vmin)
        if vmax == fr:
            h = 60 * (fg - fb) / diff
        elif vmax == fg:
            h = 120 + 60 * (fb - fr) / diff
        else:
            h = 240 + 60 * (fr - fg) / diff
        if h < 0:
            h += 360
    H, L, S = _half_even(h / 2), _half_even(255 * l), _half_even(255 * s)
    x = (H + d_h) % 180
    H, L, S = int(x), int(min(max(L + d_l, 0), 255)), int(min(max(S + d_s, 0), 255))
    l, s = Fraction(L, 255), Fraction(S, 255)
    if S == 0:
        out = (l, l, l)
    else:
        p2 = l * (1 + s) if l <= Fraction(1, 2) else l + s - l * s
        p1 = 2 * l - p2
        sector, f = (H // 30) % 6, Fraction(H % 30, 30)
        up, down = p1 + (p2 - p1) * f, p1 + (p2 - p1) * (1 - f)
        rgb = [(p2, up, p1), (down, p2, p1), (p1, p2, up), (p1, down, p2), (up, p1, p2), (p2, p1, down)][sector]
        out = (rgb[2], rgb[1], rgb[0])
    return tuple(_half_even(255 * c) for c in out)


def test_greys_stay_grey():
    """S = 0 and d_s <= 0 keep S' = 0: the result is grey clip(trunc(v + d_l)) whatever d_h."""
    v = np.arange(256, dtype=np.uint8)
    grey = np.stack([v, v, v], axis=-1)
    for d_h, d_l, d_s in ((0.0, 0.0, 0.0), (1.7, 25.3, -25.1), (-1.7, -25.3, 0.0), (45.0, 0.999, -300.0), (-90.0, -0.5, -1e-9)):
        got = R.chromatic(grey, d_h, d_l, d_s)
        want = np.array([int(min(max(Fraction(int(x)) + Fraction(d_l), 0), 255)) for x in v], np.uint8)
        assert np.array_equal(got, np.stack([want] * 3, axis=-1)), (d_h, d_l, d_s)
        for x in (0, 1, 127, 128, 254, 255):
            assert _exact_chromatic(x, x, x, Fraction(d_h), Fraction(d_l), Fraction(d_s)) == (want[x],) * 3


def test_primaries_and_secondaries_at_zero_jitter():
    """L = 127.5 rounds to 128 (half to even), S = 255, H = 0, 30, .. 150: the round trip is NOT the identity."""
    colours = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255)]       # B, G, R
    hls = R.bgr_to_hls8(np.array(colours, np.uint8))
    assert hls[:, 1].tolist() == [128] * 6 and hls[:, 2].tolist() == [255] * 6
    assert hls[:, 0].tolist() == [120, 60, 0, 90, 150, 30]
    got = R.chromatic(np.array(colours, np.uint8), 0.0, 0.0, 0.0)
    want = [_exact_chromatic(b, g, r, Fraction(0), Fraction(0), Fraction(0)) for b, g, r in colours]
    assert got.tolist() == [list(w) for w in want]
    assert want[0] == (255, 1, 1) and want[3] == (255, 255, 1)          # blue and cyan: the 0 channels come back as 1
    # and a sweep of exact answers off the ties, jittered
    rng = np.random.default_rng(5)
    bgr = rng.integers(0, 256, (400, 3)).astype(np.uint8)
    bgr = bgr[~_on_a_tie(bgr)]
    d = (Fraction(-17, 10), Fraction(253, 10), Fraction(-251, 10))
    got = R.chromatic(bgr, *[float(x) for x in d])
    exact = np.array([_exact_chromatic(int(b), int(g), int(r), *d) for b, g, r in bgr])
    assert (np.abs(got.astype(int) - exact).max(axis=1) <= 1).all()
    assert (got == exact).all(axis=1).mean() > 0.9                      # the inverse has rounding ties of its own


# ---- sampler ----------------------------------------------------------------------------------------------------------
def test_sampler_ranges_frequencies_and_determinism():
    from posecnn_amd.augment import BLUR_SIZES, AugmentSampler
    n = 10000
    rows = AugmentSampler(seed=11).sample(n)
    assert np.array_equal(rows, AugmentSampler(seed=11).sample(n))
    assert not np.array_equal(rows, AugmentSampler(seed=12).sample(n))
    assert (np.abs(rows[:, 0]) <= 1.8).all() and (np.abs(rows[:, 1:3]) <= 25.6).all() and (rows[:, 6] == 1).all()
    assert rows[:, 0].std() > 0.9 and rows[:, 1].std() > 12                 # uniform: 3.6 / sqrt(12), 51.2 / sqrt(12)
    streams = np.concatenate([rows[:, 5], rows[:, 9]])
    assert len(np.unique(streams)) == 2 * n and (streams == np.round(streams)).all() and streams.min() >= 0
    noise = np.concatenate([rows[:, 3:5], rows[:, 7:9]])                    # 2 n draws of add_noise
    mode, arg = noise[:, 0], noise[:, 1]
    assert set(mode.tolist()) == {1.0, 2.0, 3.0}
    g = mode == 1
    assert (arg[g] >= 0).all() and (arg[g] <= np.sqrt(0.3 * 256)).all() and (arg[g] == arg[g].astype(np.float32)).all()
    assert set(arg[~g].tolist()) == set(float(s) for s in BLUR_SIZES)

    def within(count, total, p):
        return abs(count - total * p) <= 5 * np.sqrt(total * p * (1 - p))
    assert within(g.sum(), len(mode), 0.9) and within((~g).sum(), len(mode), 0.1)
    nb = int((~g).sum())
    assert within((mode == 2).sum(), nb, 0.5)
    for s in BLUR_SIZES:
        assert within((arg[~g] == s).sum(), nb, 1.0 / 6)
    # the switches of cfg.TRAIN
    off = AugmentSampler(seed=11, chromatic=False, add_noise=False).sample(50)
    assert (off[:, [0, 1, 2, 3, 4, 6, 7, 8]] == 0).all() and len(np.unique(off[:, [5, 9]])) == 100
    # consecutive calls continue the stream ids: a re-drawn frame never reuses one
    s = AugmentSampler(seed=1)
    a, b = s.sample(3), s.sample(2)
    assert len(np.unique(np.concatenate([a[:, [5, 9]].ravel(), b[:, [5, 9]].ravel()]))) == 10


def test_online_minibatches_builds_the_sampler_from_the_config(monkeypatch):
    from posecnn_amd import synthesize as syn, train
    assert train.TrainConfig.CHROMATIC is True and train.TrainConfig.ADD_NOISE is False      # lib/fcn/config.py:112-113
    seen = {}
    monkeypatch.setattr(syn, "synthetic_minibatches", lambda *a, **kw: seen.update(kw, called=True))

    class Cfg(train.TrainConfig):                      # experiments/cfgs/lov_color_2d.yml:19-20
        SYNTHESIZE = SYN_ONLINE = ADD_NOISE = True
        SYN_SAMPLE_OBJECT = False

    syn.online_minibatches(Cfg, [None] * 3, np.eye(3), 2, None, None, None)
    assert seen == {"called": True}                    # the default: no sampler, nothing changes
    syn.online_minibatches(Cfg, [None] * 3, np.eye(3), 2, None, None, None, augment_seed=9)
    s = seen["augment"]
    assert (s.seed, s.chromatic, s.add_noise) == (9, True, True)
    off = type("Off", (Cfg,), {"ADD_NOISE": False, "CHROMATIC": False})
    syn.online_minibatches(off, [None] * 3, np.eye(3), 2, None, None, None, augment_seed=1)
    assert (seen["augment"].chromatic, seen["augment"].add_noise) == (False, False)


# ---- Gaussian restatement ---------------------------------------------------------------------------------------------
def test_gaussian_restatement_statistics():
    w = R.pixel_words(256, 256, 77, 0, CS.SEED)
    for g in (R.gauss32(w).astype(np.float64), R.gauss64(w)):
        n = g.size
        assert n == 1 << 16
        assert abs(g.mean()) <= 5 / np.sqrt(n)
        assert abs(g.var() - 1) <= 5 * np.sqrt(2.0 / n)
    assert np.abs(R.gauss64(w)).max() <= R.G_MAX
    assert np.abs(R.gauss32(w)).max() <= np.float32(R.G_MAX)
    u1, u2 = R.uniforms(w)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    # another stream, another plane: other deviates
    assert not np.array_equal(w, R.pixel_words(256, 256, 78, 0, CS.SEED))
    assert not np.array_equal(w, R.pixel_words(256, 256, 77, 1, CS.SEED))


def test_gauss_tolerance_of_the_gpu_cases():
    tol = CS.gauss_tolerance()
    print("max |float32 restatement - float64 restatement| over the GPU test's Gaussian cases: %.3e" % tol)
    # sigma g up to 8.8 * 5.8 next to a byte of up to 255: a few ulps of 255 (1.5e-5 each)
    assert 0 < tol < 1e-4


# ---- the C-ABI --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from posecnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_argument_validation_happens_on_the_host(L):
    """Every call here returns before anything is launched: the device pointers are host addresses that are never read."""
    from posecnn_amd._lib import PCNN_EINVAL, PCNN_ENULL, PCNN_EWORKSPACE, PCNN_OK
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    n = ctypes.c_size_t(77)
    assert L.pcnn_augment_frames_workspace_bytes(3, 1, 0, ctypes.byref(n)) == PCNN_OK and n.value == 16
    assert L.pcnn_augment_frames_workspace_bytes(3, 1, 1, ctypes.byref(n)) == PCNN_OK and n.value == 0
    assert L.pcnn_augment_frames_workspace_bytes(3, 0, 0, ctypes.byref(n)) == PCNN_OK and n.value == 0
    assert L.pcnn_augment_frames_workspace_bytes(3, 1, 0, None) == PCNN_ENULL
    assert L.pcnn_augment_frames_workspace_bytes(0, 1, 0, ctypes.byref(n)) == PCNN_EINVAL
    assert L.pcnn_augment_frames_workspace_bytes(3, 1, 2, ctypes.byref(n)) == PCNN_EINVAL

    means = (ctypes.c_double * 3)(102.9801, 115.9465, 122.7717)
    good = np.stack([R.row((1.0, 2.0, 3.0), 1, 2.5, 4, 1, 2, 7.0, 5), R.row((0.0, 0.0, 0.0), 3, 15.0, 6, 0, 0, 0.0, 7)])
    base = dict(color=p, C=4, depth=p, rows=good, means=means, norm=0, B=2, H=8, W=8, data=p, data_p=p, ws=p, ws_bytes=16)

    def call(**kw):
        a = dict(base, **kw)
        rows = a["rows"]
        return L.pcnn_augment_frames_fwd(a["color"], a["C"], a["depth"], None if rows is None else rows.ctypes.data_as(ctypes.c_void_p),
                                         a["means"], 1, 2, a["norm"], a["B"], a["H"], a["W"], a["data"], a["data_p"], a["ws"],
                                         a["ws_bytes"], None)

    def refused(status, word, **kw):
        assert call(**kw) == status, kw
        msg = L.pcnn_last_error_string().decode()
        assert word in msg, (kw, msg)

    def edit(r, c, v):
        rows = good.copy()
        rows[r, c] = v
        return rows

    refused(PCNN_EINVAL, "batch", B=0)
    refused(PCNN_EINVAL, "height and width", H=7)
    refused(PCNN_EINVAL, "height and width", W=7)
    refused(PCNN_EINVAL, "2^30", B=2, H=1 << 15, W=1 << 15)
    refused(PCNN_EINVAL, "channels", C=2)
    refused(PCNN_EINVAL, "channels", C=5)
    refused(PCNN_EINVAL, "depth_norm", norm=2)
    refused(PCNN_ENULL, "color", color=None)
    refused(PCNN_ENULL, "params", rows=None)
    refused(PCNN_ENULL, "pixel_means", means=None)
    refused(PCNN_ENULL, "data is NULL", data=None)
    refused(PCNN_ENULL, "data_p", data_p=None)
    refused(PCNN_EINVAL, "aligned", data=odd)
    refused(PCNN_EINVAL, "aligned", color=odd)
    refused(PCNN_EINVAL, "pixel_means", means=(ctypes.c_double * 3)(1.0, float("nan"), 3.0))
    refused(PCNN_ENULL, "workspace", ws=None)
    refused(PCNN_EWORKSPACE, "workspace", ws_bytes=8)
    refused(PCNN_EINVAL, "workspace", ws=odd)
    for v in (4.0, -1.0, 1.5, float("nan")):
        refused(PCNN_EINVAL, "colour mode", rows=edit(1, 3, v))
        refused(PCNN_EINVAL, "depth mode", rows=edit(0, 7, v))
    for v in (4.0, 13.0, 1.0, 17.0, 3.5, 0.0, float("nan")):
        refused(PCNN_EINVAL, "colour blur size", rows=edit(1, 4, v))
        refused(PCNN_EINVAL, "depth blur size", rows=edit(0, 8, v))
    for v in (-0.5, float("inf"), float("nan")):
        refused(PCNN_EINVAL, "colour sigma", rows=edit(0, 4, v))
    for v in (-1.0, 0.5, 2.0 ** 53, float("nan")):
        refused(PCNN_EINVAL, "colour stream id", rows=edit(0, 5, v))
        refused(PCNN_EINVAL, "depth stream id", rows=edit(1, 9, v))
    for v in (91.0, -90.5, float("nan"), float("inf")):
        refused(PCNN_EINVAL, "d_h", rows=edit(1, 0, v))
    refused(PCNN_EINVAL, "d_l and d_s", rows=edit(0, 1, float("inf")))
    refused(PCNN_EINVAL, "d_l and d_s", rows=edit(0, 2, float("nan")))
    refused(PCNN_EINVAL, "chromatic", rows=edit(0, 6, 2.0))
    # a bad row anywhere is found before the first launch, also past the first launch's 32 frames
    many = np.tile(good[:1], (40, 1))
    many[37, 3] = 9.0
    refused(PCNN_EINVAL, "row 37", rows=many, B=40, ws_bytes=160)


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from posecnn_amd import ops
    rows = np.stack([R.row()])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.augment_frames(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), None, rows, 0)
    with pytest.raises(TypeError):
        ops.augment_frames(np.zeros((1, 8, 8, 3), np.uint8), None, rows, 0)
    assert "augment_frames" in ops.__all__
