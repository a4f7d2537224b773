#!/usr/bin/env python
"""The normal-image front end (include/posecnn_hip_frontend.h) at B = 16, 480 x 640, timed in ONE process with
alternating repeats (medians, device events around the library calls on preallocated buffers):

  fused     pcnn_normal_image_fwd: uint16 depth -> filtered uint8 image, nothing between in memory
  unfused   pcnn_depth_normals_fwd -> quantise (framework ops) -> pcnn_bilateral_u8c3_fwd
  floor     the bytes the fused entry has to move (2 B read + 3 B written per pixel) over the copy rate measured here: a
            device-to-device copy of a buffer of 16 frames' worth of float32 (20 MB: it stays in the caches, so this is
            a cache-rate floor, lower than an HBM floor would be)

Depth: the recorded demo frame tests/golden/demo_images/000001-depth.png, repeated over the batch with a per-frame
shift so that no two frames are equal. Both routes must give the same bytes before anything is timed. bench.py does
not call this; the result goes to --out (default profiles/normal_image.json) and is printed as one JSON line.

    python tools/bench_normals.py [--repeats 30] [--warmup 5] [--out profiles/normal_image.json]
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
from posecnn_amd import _lib, config, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--d", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_image.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_normals: needs the GPU (a CPU run measures nothing)")
    from PIL import Image
    dev = torch.device("cuda:0")
    frame = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "demo_images", "000001-depth.png"))).astype(np.uint16)
    H, W = frame.shape
    B = a.batch
    depth_np = np.stack([np.roll(frame, (3 * b, 5 * b), axis=(0, 1)) for b in range(B)])
    K = config.DEMO_INTRINSICS.astype(np.float32)
    intr_np = np.tile(np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], np.float32), (B, 1))
    factor, cutoff, d = float(config.DEMO_FACTOR_DEPTH), 20.0, a.d

    L = _lib.lib()
    P = ops._ptr
    depth, intr = torch.from_numpy(depth_np).to(dev), torch.from_numpy(intr_np).to(dev)
    color, space, _ = ops.bilateral_tables(d, 75.0, 75.0, dev)
    taps = space.numel()
    fused, unfused = (torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    nmap = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    copy_src, copy_dst = torch.empty((B, H, W), device=dev).fill_(1.0), torch.empty((B, H, W), device=dev)
    stream = ops._stream(depth)
    state = {}

    def quantise():
        t = nmap * 127.5 + 127.5
        state["q"] = torch.where(torch.isnan(t), torch.zeros_like(t), t).to(torch.uint8).flip(-1).contiguous()
        return 0

    calls = {
        "fused": lambda: L.pcnn_normal_image_fwd(None, P(depth), factor, P(intr), B, H, W, cutoff, d, P(color), P(space), taps,
                                                 P(fused), stream),
        "normals": lambda: L.pcnn_depth_normals_fwd(None, P(depth), factor, P(intr), B, H, W, cutoff, P(nmap), stream),
        "quantise": quantise,
        "bilateral": lambda: L.pcnn_bilateral_u8c3_fwd(P(state["q"]), B, H, W, d, P(color), P(space), taps, P(unfused), stream),
        "copy": lambda: copy_dst.copy_(copy_src).numel() * 0,
    }
    routes = {"fused": ("fused",), "unfused": ("normals", "quantise", "bilateral"), "roof": ("copy",)}

    def run_route(r):
        """-> per-call milliseconds of one pass over the route's calls (device events)."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(routes[r]) + 1)]
        ev[0].record()
        for k, name in enumerate(routes[r]):
            _lib.check(name, calls[name]())
            ev[k + 1].record()
        torch.cuda.synchronize()
        return {name: ev[k].elapsed_time(ev[k + 1]) for k, name in enumerate(routes[r])}

    run_route("fused"), run_route("unfused")
    same = bool(torch.equal(fused, unfused))
    if not same:
        sys.exit("bench_normals: the fused and the unfused route disagree (%d bytes)" % int((fused != unfused).sum()))

    for _ in range(a.warmup):
        for r in routes:
            run_route(r)
    samples = {}
    for i in range(a.repeats):
        for r in (("fused", "unfused", "roof") if i % 2 == 0 else ("unfused", "fused", "roof")):   # alternate who goes first
            for k, v in run_route(r).items():
                samples.setdefault(k, []).append(v)
    med = {k: statistics.median(v) for k, v in samples.items()}
    unfused_ms = statistics.median([sum(samples[k][i] for k in routes["unfused"]) for i in range(a.repeats)])
    pixels = B * H * W
    copy_rate = 2 * 4 * pixels / (med["copy"] * 1e-3)             # bytes read + bytes written per second
    moved = (2 + 3) * pixels
    result = {
        "what": "depth -> filtered normal image, fused against unfused, one process, alternating repeats, medians (ms)",
        "shape": {"batch": B, "height": H, "width": W, "d": d, "taps": taps, "pixels": pixels},
        "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
        "median_ms": med, "min_max_ms": {k: [min(v), max(v)] for k, v in samples.items()},
        "route_ms": {"fused": med["fused"], "unfused": unfused_ms}, "unfused_over_fused": unfused_ms / med["fused"],
        "fused_pixels_per_s": pixels / (med["fused"] * 1e-3),
        "fused_taps_per_s": pixels * taps / (med["fused"] * 1e-3),
        "bytes_floor": {"how": "2 B read + 3 B written per pixel over the rate of a device-to-device copy of %d float32 in this process (cache-resident: not an HBM floor)" % pixels,
                        "bytes": moved, "copy_bytes_per_s": copy_rate, "floor_ms": moved / copy_rate * 1e3,
                        "fused_over_floor": med["fused"] / (moved / copy_rate * 1e3)},
        "results_identical": same,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
