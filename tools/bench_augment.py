#!/usr/bin/env python
"""Training augmentation (include/posecnn_hip_augment.h) at 16 frames of 480 x 640, colour only (BGRA in) and RGB-D, timed
in ONE process with alternating repeats (medians; device events around the call on resident inputs):

  fused      ops.augment_frames, one library call: with every frame in one mode (none with chromatic off, chromatic
             only, Gaussian, horizontal and vertical blur of 15) and with the rows AugmentSampler(seed 0) draws, the
             reference's recipe (90 % Gaussian, 10 % blur)
  framework  the same result composed from framework ops where that is possible: chromatic off + no noise is
             networks.raw_frame_blob (bit-identical, checked here); the chromatic transform is the header's formulas as
             elementwise tensor ops (the framework's f32 division is not correctly rounded, so a few bytes may differ by
             one code: the count is reported). The Gaussian path has no framework composition: its deviates are a
             function of (seed, stream id, pixel) that no framework generator reproduces.

Achieved bytes per second are the algorithmic bytes — 4 in (BGRA) and 12 out per pixel, plus 2 in and 12 out with
depth — over the median time. bench.py does not call this; the result goes to --out (default profiles/augment.json) and is
printed as one JSON line.

    python tools/bench_augment.py [--repeats 30] [--warmup 3] [--out profiles/augment.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from posecnn_amd import networks, ops  # noqa: E402
from posecnn_amd.augment import AugmentSampler  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def torch_chromatic(bgr, d_h, d_l, d_s):
    """Steps 1-3 of include/posecnn_hip_augment.h as elementwise tensor ops: uint8 [..., 3] -> uint8 [..., 3]"""
    f = torch.float32
    k255 = float(np.float32(1.0 / 255.0))
    b, g, r = (bgr[..., i].to(f) * k255 for i in range(3))
    vmax, vmin = torch.maximum(torch.maximum(b, g), r), torch.minimum(torch.minimum(b, g), r)
    total, diff = vmax + vmin, vmax - vmin
    l = total * 0.5
    grey = diff == 0
    safe = torch.where(grey, torch.ones_like(diff), diff)
    s = diff / torch.where(l < 0.5, total, (2.0 - vmax) - vmin).clamp_min(1e-30)
    q = 60.0 / safe
    h = torch.where(vmax == r, (g - b) * q, torch.where(vmax == g, (b - r) * q + 120.0, (r - g) * q + 240.0))
    h = torch.where(h < 0, h + 360.0, h)
    h, s = torch.where(grey, torch.zeros_like(h), h), torch.where(grey, torch.zeros_like(s), s)
    H8, L8, S8 = (torch.round(x).clamp(0, 255) for x in (h * 0.5, l * 255.0, s * 255.0))
    x = torch.remainder(H8.to(torch.float64) + d_h, 180.0).floor().to(torch.int32)
    Ln = (L8.to(torch.float64) + d_l).clamp(0, 255).floor()
    Sn = (S8.to(torch.float64) + d_s).clamp(0, 255).floor()
    l2, s2 = Ln.to(f) * k255, Sn.to(f) * k255
    p2 = torch.where(l2 <= 0.5, l2 * (1.0 + s2), (l2 + s2) - l2 * s2)
    p1 = 2.0 * l2 - p2
    d = p2 - p1
    sector = torch.div(x, 30, rounding_mode="floor")
    fr = (x - 30 * sector).to(f) * float(np.float32(1.0 / 30.0))
    sector = torch.where(sector >= 6, sector - 6, sector)
    up, down = p1 + d * fr, p1 + d * (1.0 - fr)

    def pick(table):
        out = table[5]
        for k in range(4, -1, -1):
            out = torch.where(sector == k, table[k], out)
        return torch.where(Sn == 0, l2, out)
    rr, gg, bb = pick([p2, down, p1, p1, up, p2]), pick([up, p2, p2, down, p1, p1]), pick([p1, p1, up, p2, p2, down])
    return torch.stack([torch.round(c * 255.0).clamp(0, 255) for c in (bb, gg, rr)], dim=-1).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_augment: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    B, H, W = a.frames, 480, 640
    rng = np.random.default_rng(0)
    color = torch.from_numpy(rng.integers(0, 256, (B, H, W, 4)).astype(np.uint8)).to(dev)
    depth = torch.from_numpy(rng.integers(0, 3000, (B, H, W)).astype(np.int16)).to(dev).view(torch.uint16)
    bgr = color[..., :3].contiguous()
    jitter = (-1.7, 25.3, -25.1)

    def rows(chroma, mode, arg):
        r = np.zeros((B, 10))
        r[:, :3] = jitter
        r[:, 3], r[:, 4], r[:, 5], r[:, 6] = mode, arg, np.arange(B), chroma
        r[:, 7], r[:, 8], r[:, 9] = mode, arg, B + np.arange(B)
        return r
    configs = {"none_chromatic_off": rows(0, 0, 0), "chromatic_only": rows(1, 0, 0), "gaussian": rows(1, 1, 6.0),
               "hblur15": rows(1, 2, 15), "vblur15": rows(1, 3, 15), "sampled_recipe": AugmentSampler(seed=0).sample(B)}
    routes = {}
    for name, r in configs.items():
        routes["fused/color/" + name] = lambda r=r: ops.augment_frames(color, None, r, 7)
        routes["fused/rgbd/" + name] = lambda r=r: ops.augment_frames(color, depth, r, 7)
    routes["fused/rgbd_fixed_2000/none_chromatic_off"] = lambda: ops.augment_frames(color, depth, configs["none_chromatic_off"], 7,
                                                                                    depth_norm="fixed_2000")
    from posecnn_amd.config import PIXEL_MEANS
    means = torch.from_numpy(np.asarray(PIXEL_MEANS, dtype=np.float64).reshape(1, 1, 1, 3)).to(dev)
    routes["framework/color/none_chromatic_off"] = lambda: networks.raw_frame_blob(color[..., :3].contiguous())
    routes["framework/rgbd_fixed_2000/none_chromatic_off"] = lambda: (networks.raw_frame_blob(color[..., :3].contiguous()),
                                                                       networks.raw_frame_blob(depth))
    routes["framework/color/chromatic_only"] = lambda: (torch_chromatic(color[..., :3], *jitter).to(torch.float64) - means).to(torch.float32)

    # the compositions compute what the fused call computes
    fused = ops.augment_frames(color, depth, configs["none_chromatic_off"], 7, depth_norm="fixed_2000")
    same = bool(torch.equal(fused[0], networks.raw_frame_blob(bgr)) and torch.equal(fused[1], networks.raw_frame_blob(depth)))
    diff = (ops.augment_frames(color, None, configs["chromatic_only"], 7)[0] - routes["framework/color/chromatic_only"]()).abs()
    checks = {"raw_frame_blob_bit_identical": same, "chromatic_framework_bytes_differing": int((diff > 0).sum()),
              "chromatic_framework_max_difference": float(diff.max())}

    for _ in range(a.warmup):
        for fn in routes.values():
            timed(fn)
    samples = {k: [] for k in routes}
    names = list(routes)
    for i in range(a.repeats):
        for k in (names if i % 2 == 0 else names[::-1]):
            samples[k].append(timed(routes[k]))
    pixels = B * H * W
    bytes_of = {"color": 16 * pixels, "rgbd": 30 * pixels, "rgbd_fixed_2000": 30 * pixels}
    result = {"what": "augmentation: fused call against framework compositions, medians of alternating repeats (ms)",
              "shape": {"frames": B, "height": H, "width": W, "color_channels": 4}, "device": torch.cuda.get_device_name(0),
              "repeats": a.repeats, "warmup": a.warmup, "checks": checks,
              "algorithmic_bytes": bytes_of, "routes": {}}
    for k, v in samples.items():
        med = statistics.median(v)
        result["routes"][k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v),
                               "algorithmic_gb_per_s": bytes_of[k.split("/")[1]] / (med * 1e-3) / 1e9}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
