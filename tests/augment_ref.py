"""numpy restatement of include/posecnn_hip_augment.h (TEST INFRASTRUCTURE): its own Philox4x64-10, the 8-bit HLS pair, the
float64 jitter, the blurs and the blobs with the header's exact f32 / f64 operations, and the Gaussian path twice — in
float32 numpy (the header's sequence with numpy's log and cos) and in float64 from the same generator words.

`augment_frames(...)` mirrors `ops.augment_frames`; with `gauss64=True` the Gaussian path is the float64 one."""
import numpy as np

F = np.float32
M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
MASK = (1 << 64) - 1
K255 = F(1.0 / 255.0)
K30 = F(1.0 / 30.0)
TWO_PI = F(2.0 * np.pi)
G_MAX = float(np.sqrt(48.0 * np.log(2.0)))        # u1 >= 2^-24


# ---- Philox4x64-10 --------------------------------------------------------------------------------------------------
def _mulhilo(a, b):
    """a: python int constant < 2^64, b: uint64 array -> (hi, lo) uint64 arrays of the 128-bit product"""
    a_lo, a_hi = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    b_lo, b_hi = b & m32, b >> s32
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> s32) + (lh & m32) + (hl & m32)
    lo = (ll & m32) | ((mid & m32) << s32)
    hi = hh + (lh >> s32) + (hl >> s32) + (mid >> s32)
    return hi, lo


def philox4x64(counter, key):
    """counter: 4 uint64 arrays (or ints) of one shape, key: 2 ints -> uint64 [..., 4], the block of exactly this counter"""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in counter]
    shape = np.broadcast_shapes(*[x.shape for x in c])
    c = [np.broadcast_to(x, shape).copy() for x in c]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    with np.errstate(over="ignore"):
        for _ in range(10):
            hi0, lo0 = _mulhilo(M0, c[0])
            hi1, lo1 = _mulhilo(M1, c[2])
            c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1)


def pixel_words(H, W, stream, plane, seed):
    """uint64 [H,W]: pixel p = y W + x takes word p & 3 of the block with counter (p >> 2, stream, plane, 0), key = seed"""
    n = H * W
    blocks = philox4x64((np.arange((n + 3) // 4, dtype=np.uint64), int(stream), int(plane), 0), (seed & MASK, seed >> 64))
    return blocks.reshape(-1)[:n].reshape(H, W)


def uniforms(words):
    hi, lo = (words >> np.uint64(32)).astype(np.uint32), (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    u1 = ((hi >> np.uint32(8)) + np.uint32(1)).astype(F) * F(2.0 ** -24)
    u2 = (lo >> np.uint32(8)).astype(F) * F(2.0 ** -24)
    return u1, u2


def gauss32(words):
    u1, u2 = uniforms(words)
    return np.sqrt(F(-2.0) * np.log(u1)) * np.cos(TWO_PI * u2)


def gauss64(words):
    u1, u2 = uniforms(words)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))


# ---- 8-bit HLS ------------------------------------------------------------------------------------------------------
def _byte(v):
    return np.clip(np.rint(v), F(0), F(255)).astype(np.uint8)


def bgr_to_hls8(bgr):
    """uint8 [...,3] BGR -> uint8 [...,3] (H8, L8, S8), header step 1"""
    b, g, r = (bgr[..., i].astype(F) * K255 for i in range(3))
    vmax, vmin = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    total, diff = vmax + vmin, vmax - vmin
    l = total * F(0.5)
    grey = diff == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = diff / np.where(l < F(0.5), total, (F(2.0) - vmax) - vmin)
        q = F(60.0) / diff
        h = np.where(vmax == r, (g - b) * q, np.where(vmax == g, (b - r) * q + F(120.0), (r - g) * q + F(240.0)))
    h = np.where(h < 0, h + F(360.0), h)
    h, s = np.where(grey, F(0), h).astype(F), np.where(grey, F(0), s).astype(F)
    return np.stack([_byte(h * F(0.5)), _byte(l * F(255.0)), _byte(s * F(255.0))], axis=-1)


def jitter(hls, d_h, d_l, d_s):
    """header step 2, float64 exactly as numpy: (h + d_h) % 180, clip(l + d_l), clip(s + d_s), astype(uint8)"""
    h = np.mod(hls[..., 0].astype(np.float64) + np.float64(d_h), 180.0)
    l = np.clip(hls[..., 1].astype(np.float64) + np.float64(d_l), 0, 255)
    s = np.clip(hls[..., 2].astype(np.float64) + np.float64(d_s), 0, 255)
    return np.stack([h, l, s], axis=-1).astype(np.uint8)


def hls8_to_bgr(hls):
    """uint8 [...,3] (H', L', S') -> uint8 [...,3] BGR, header step 3"""
    H = hls[..., 0].astype(np.int32)
    l, s = hls[..., 1].astype(F) * K255, hls[..., 2].astype(F) * K255
    p2 = np.where(l <= F(0.5), l * (F(1.0) + s), (l + s) - l * s)
    p1 = F(2.0) * l - p2
    d = p2 - p1
    sector = H // 30
    f = (H - 30 * sector).astype(F) * K30
    sector = np.where(sector >= 6, sector - 6, sector)
    up, down = p1 + d * f, p1 + d * (F(1.0) - f)
    pick = lambda table: np.choose(sector, table)
    r = pick([p2, down, p1, p1, up, p2])
    g = pick([up, p2, p2, down, p1, p1])
    b = pick([p1, p1, up, p2, p2, down])
    grey = hls[..., 2] == 0
    out = [np.where(grey, l, c).astype(F) for c in (b, g, r)]
    return np.stack([_byte(c * F(255.0)) for c in out], axis=-1)


def chromatic(bgr, d_h, d_l, d_s):
    return hls8_to_bgr(jitter(bgr_to_hls8(bgr), d_h, d_l, d_s))


# ---- depth value, noise, blob ---------------------------------------------------------------------------------------
def depth_value(depth, depth_norm):
    """uint16 [H,W] -> f32 [H,W], header step 4 (depth_norm 0: the frame's own maximum, 0 / 0 = NaN; 1: / 2000 clipped)"""
    d = depth.astype(F)
    if depth_norm == 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            return (d / F(depth.max())) * F(255.0)
    return np.clip(d / F(2000.0), F(0), F(1)) * F(255.0)


def reflect101(p, n):
    p = np.asarray(p).copy()
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def blur(values, size, vertical):
    """f32 [H,W,...] -> f32 accumulator of the header's modes 2 / 3: taps ascending, acc = acc + value * k"""
    H, W = values.shape[:2]
    r, k = size // 2, F(1.0 / size)
    acc = np.zeros(values.shape, F)
    for i in range(-r, r + 1):
        if vertical:
            tap = values[reflect101(np.arange(H) + i, H)]
        else:
            tap = values[:, reflect101(np.arange(W) + i, W)]
        acc = acc + tap * k
    return acc


def noise(values, mode, arg, stream, plane, seed, colour, use64=False):
    """values f32 [H,W] or [H,W,3] -> the plane's v of header step 5 (float64 when use64 and mode 1)"""
    mode = int(mode)
    if mode == 0:
        return values
    if mode == 1:
        words = pixel_words(values.shape[0], values.shape[1], stream, plane, seed)
        if use64:
            n = np.float64(F(arg)) * gauss64(words)
            v = values.astype(np.float64)
        else:
            n = F(arg) * gauss32(words)
            v = values
        if v.ndim == 3:
            n = n[..., None]
        v = v + n
        return np.where(v < 0, 0, np.where(v > 255, 255, v)).astype(v.dtype)      # keeps a NaN
    acc = blur(values, int(arg), vertical=(mode == 3))
    return np.clip(np.rint(acc), F(0), F(255)) if colour else acc


def blob(v, means):
    """header step 6: (float)((double)v - mean_c); v [H,W] is tiled to the three channels"""
    v = np.asarray(v)
    if v.ndim == 2:
        v = np.repeat(v[..., None], 3, axis=2)
    return (v.astype(np.float64) - np.asarray(means, np.float64).reshape(1, 1, 3)).astype(F if v.dtype != np.float64 else np.float64)


PIXEL_MEANS = np.array([102.9801, 115.9465, 122.7717], np.float64)


def augment_frames(color, depth, params, seed, pixel_means=None, depth_norm=0, use64=False):
    """color uint8 [B,H,W,3|4], depth uint16 [B,H,W] | None, params float64 [B,10] -> (data, data_p), both [B,H,W,3]
    (f32; float64 with use64, where only the Gaussian path differs from the f32 result)"""
    means = PIXEL_MEANS if pixel_means is None else np.asarray(pixel_means, np.float64).reshape(3)
    data, data_p = [], []
    for b, row in enumerate(np.asarray(params, np.float64)):
        bgr = color[b][..., :3]
        if row[6]:
            bgr = chromatic(bgr, row[0], row[1], row[2])
        v = noise(bgr.astype(F), row[3], row[4], int(row[5]), 0, seed, True, use64)
        data.append(blob(v, means))
        if depth is not None:
            v = noise(depth_value(depth[b], depth_norm), row[7], row[8], int(row[9]), 1, seed, False, use64)
            data_p.append(blob(v, means))
    dt = np.float64 if use64 else F
    return np.stack(data).astype(dt), (np.stack(data_p).astype(dt) if depth is not None else None)


def row(d=(0.0, 0.0, 0.0), mode=0, arg=0.0, stream=0, chroma=1, dmode=0, darg=0.0, dstream=0):
    return np.array([d[0], d[1], d[2], mode, arg, stream, chroma, dmode, darg, dstream], np.float64)
