"""Frames and parameter rows shared by tests/test_augment_cpu.py and tests/test_gpu_augment.py (TEST INFRASTRUCTURE).
Everything is seeded and built once per process; nobody modifies what these functions return."""
import functools

import numpy as np

import augment_ref as R

SEED = (0x0123456789ABCDEF << 64) | 0xFEDCBA9876543210
SEED_KEY = (SEED & ((1 << 64) - 1), SEED >> 64)
TILE_H, TILE_W = 16, 64                       # the kernel's LDS tile (posecnn_amd/csrc/augment.hip)
# 8 x 8: the smallest legal frame; 17 x 23: odd, W % 4 != 0, a Philox block straddles two rows; one tile + 1 in each
# dimension; two tiles + 3
GAUSS_SIZES = ((8, 8), (17, 23), (TILE_H + 1, TILE_W + 1), (2 * TILE_H + 3, 2 * TILE_W + 3))
BLUR_SIZES = (3, 5, 7, 9, 11, 15)
JITTER = (-1.7, 25.3, -25.1)                  # hue wrap at the bottom, L clipped at the top, S clipped at the bottom


@functools.lru_cache(maxsize=None)
def frames(H, W, B=1, channels=3, seed=1):
    """(color uint8 [B,H,W,channels], depth uint16 [B,H,W]): colours over the whole cube with saturated and grey patches,
    depths around 0..2600 (past the 2000 of depth_norm 1) with zeros"""
    rng = np.random.default_rng([seed, H, W, B])
    color = rng.integers(0, 256, (B, H, W, channels)).astype(np.uint8)
    color[:, : H // 4, : W // 4, :3] = rng.integers(0, 2, (B, H // 4, W // 4, 3)).astype(np.uint8) * 255
    color[:, H // 2:, : W // 4, :3] = color[:, H // 2:, : W // 4, :1]
    depth = rng.integers(0, 2600, (B, H, W)).astype(np.uint16)
    depth[:, ::3, ::5] = 0
    return color, depth


def gauss_rows(B):
    """Gaussian rows at the two ends and the middle of the reference's sigma range, chromatic on, streams far apart"""
    sig = [float(np.float32(np.sqrt(v))) for v in (76.8, 20.0, 0.5)]
    return np.stack([R.row(JITTER, 1, sig[b % 3], 1000 + 7 * b, 1, 1, sig[(b + 1) % 3], (1 << 40) + b) for b in range(B)])


@functools.lru_cache(maxsize=None)
def gauss_case(H, W):
    """One Gaussian case of the GPU test: inputs, rows, and the float32 and float64 restatements for both depth norms"""
    color, depth = frames(H, W, 2)
    rows = gauss_rows(2)
    out = {"color": color, "depth": depth, "rows": rows}
    for norm in (0, 1):
        out["f32", norm] = R.augment_frames(color, depth, rows, SEED, depth_norm=norm)
        out["f64", norm] = R.augment_frames(color, depth, rows, SEED, depth_norm=norm, use64=True)
    return out


@functools.lru_cache(maxsize=None)
def gauss_tolerance():
    """max |float32 restatement - float64 restatement| over the GPU test's own Gaussian cases: what one float32
    implementation of the header's sequence is away from the real-number result at these shapes and sigmas"""
    worst = 0.0
    for H, W in GAUSS_SIZES:
        c = gauss_case(H, W)
        for norm in (0, 1):
            for a, b in zip(c["f32", norm], c["f64", norm]):
                worst = max(worst, float(np.nanmax(np.abs(a.astype(np.float64) - b))))
    return worst
