"""numpy restatement of the input front end (include/posecnn_hip_frontend.h), independent of posecnn_amd: the normal map of
lib/normals/compute_normals.cu:30-101, its uint8 image (lib/fcn/test.py:91-93) and OpenCV's scalar 8-bit 3-channel
bilateral filter (:94). All arithmetic is float32 with one operation per numpy call, so nothing is contracted; the
filter walks its taps in OpenCV's order on whole-image arrays, which keeps each pixel's summation order.

The normal map is pinned to the reference's own kernel bodies through tests/golden/normals.npz (written by
tests/golden/make_normals_golden.py). The bilateral filter is restated from the published algorithm and pinned to
nothing: OpenCV is not available where this suite runs."""
import os

import numpy as np

F = np.float32
NAN_BITS = np.uint32(0x7fffffff)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "normals.npz")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def golden_cases():
    z = np.load(GOLDEN)
    return [dict(name=str(n), depth=z["%s/depth" % n], intrinsics=z["%s/intrinsics" % n], cutoff=float(z["%s/cutoff" % n]),
                 nmap=z["%s/nmap" % n]) for n in z["names"]]


def metres(depth_u16, factor_depth):
    """im_depth.astype(np.float32) / float(factor_depth): one float32 division."""
    return depth_u16.astype(F) / F(factor_depth)


def depth_normals(depth, intrinsics, cutoff=20.0):
    """depth f32 [B,H,W], intrinsics f32 [B,4] rows (fx, fy, cx, cy) -> nmap f32 [B,H,W,3]; NaN = 0x7fffffff."""
    depth = np.asarray(depth, F)
    B, H, W = depth.shape
    out = np.full((B, H, W, 3), NAN_BITS, np.uint32).view(F)
    u = np.arange(H, dtype=F)[:, None]
    v = np.arange(W, dtype=F)[None, :]
    with np.errstate(all="ignore"):
        for b in range(B):
            fx, fy, cx, cy = (F(k) for k in np.asarray(intrinsics, F)[b])
            fx_inv, fy_inv = F(1) / fx, F(1) / fy
            z = depth[b]
            valid = (z != 0) & (z < F(cutoff))
            vx = np.multiply(np.multiply(z, np.subtract(u, cx)), fx_inv)
            vy = np.multiply(np.multiply(z, np.subtract(v, cy)), fy_inv)
            vmap = np.stack([vx, vy, np.broadcast_to(z, vx.shape)], axis=-1).astype(F)
            vmap[~valid] = np.nan
            v00, v01, v10 = vmap[:-1, :-1], vmap[1:, :-1], vmap[:-1, 1:]
            ok = ~np.isnan(v00[..., 0]) & ~np.isnan(v01[..., 0]) & ~np.isnan(v10[..., 0])
            a = np.subtract(v01, v00)
            c = np.subtract(v10, v00)
            cr = np.stack([np.subtract(np.multiply(a[..., 1], c[..., 2]), np.multiply(a[..., 2], c[..., 1])),
                           np.subtract(np.multiply(a[..., 2], c[..., 0]), np.multiply(a[..., 0], c[..., 2])),
                           np.subtract(np.multiply(a[..., 0], c[..., 1]), np.multiply(a[..., 1], c[..., 0]))], axis=-1)
            sq = np.multiply(cr, cr)
            s2 = np.add(sq[..., 0], np.add(sq[..., 1], sq[..., 2]))
            n = np.where((s2 > 0)[..., None], np.divide(cr, np.sqrt(s2)[..., None]), cr).astype(F)
            inner = out[b, :-1, :-1]
            inner[ok] = n[ok]
    return out


def quantise(nmap):
    """(127.5 * nmap + 127.5).astype(np.uint8)[..., (2, 1, 0)] with NaN -> 0 (what the cast gives on x86)."""
    with np.errstate(all="ignore"):
        t = np.add(np.multiply(F(127.5), nmap), F(127.5))
        q = np.where(np.isnan(t), F(0), np.clip(np.trunc(t), 0, 255)).astype(np.uint8)
    return np.ascontiguousarray(q[..., ::-1])


def tables(d, sigma_color, sigma_space):
    """(color_weight f32 [768], space_weight f32 [K], offsets [(i, j)] * K) in OpenCV's order."""
    sc = float(sigma_color) if sigma_color > 0 else 1.0
    ss = float(sigma_space) if sigma_space > 0 else 1.0
    gc, gs = -0.5 / (sc * sc), -0.5 / (ss * ss)
    r = d // 2
    color = np.array([np.exp(i * i * gc) for i in range(768)], np.float64).astype(F)
    offsets, space = [], []
    for i in range(-r, r + 1):
        for j in range(-r, r + 1):
            rho = np.sqrt(np.float64(i * i + j * j))
            if rho > r:
                continue
            offsets.append((i, j))
            space.append(np.exp(rho * rho * gs))
    return color, np.array(space, np.float64).astype(F), offsets


def bilateral(image, d=9, sigma_color=75.0, sigma_space=75.0):
    """image uint8 [B,H,W,3] -> uint8 [B,H,W,3]; border reflect-101."""
    image = np.asarray(image, np.uint8)
    B, H, W, _ = image.shape
    color, space, offsets = tables(d, sigma_color, sigma_space)
    r = d // 2
    pad = np.pad(image, ((0, 0), (r, r), (r, r), (0, 0)), mode="reflect").astype(np.int32)
    centre = pad[:, r:r + H, r:r + W]
    acc = np.zeros((B, H, W, 3), F)
    wsum = np.zeros((B, H, W), F)
    for k, (i, j) in enumerate(offsets):
        q = pad[:, r + i:r + i + H, r + j:r + j + W]
        w = np.multiply(space[k], color[np.abs(q - centre).sum(axis=-1)])
        acc = np.add(acc, np.multiply(q.astype(F), w[..., None]))
        wsum = np.add(wsum, w)
    inv = np.divide(F(1), wsum)
    return np.rint(np.multiply(acc, inv[..., None])).astype(np.uint8)


def normal_image(depth, intrinsics, cutoff=20.0, d=9, sigma_color=75.0, sigma_space=75.0):
    """depth f32 [B,H,W] (metres) -> the uint8 image of lib/fcn/test.py:89-94; d = 0: without the filter."""
    q = quantise(depth_normals(depth, intrinsics, cutoff))
    return q if d == 0 else bilateral(q, d, sigma_color, sigma_space)
