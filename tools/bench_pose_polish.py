#!/usr/bin/env python
"""The Nelder-Mead polish that ends both pose routes (include/posecnn_hip/pose_polish.h) on the frames of
tools/bench_pose3d.py: 16 frames of 480 x 640, 22 classes, five live classes per frame of 8 000 to 19 600 pixels, 256
hypotheses, the reference's defaults (max_pixels 1000, min_pixels 10, 100 evaluations). Timed in ONE process with alternating
repeats (medians; device events around the calls on resident inputs):

  depth / colour          ops.estimate_poses_3d / _2d as they are (three launches)
  depth+polish / colour+  the same with polish_evaluations = 100 (four launches)
  kernels                 the polished calls with the library's per-kernel events on (pcnn_profile_*): the polish launch alone

and, against the poses the frames were planted with, the displacement of the 8 box corners (metres) of every found class
without the polish, with 100 evaluations and with 400 — reported as found. No hardware counters are collected. bench.py does
not call this; the result goes to --out (default profiles/pose_polish.json) and is printed as one JSON line.

    python tools/bench_pose_polish.py [--repeats 20] [--warmup 3] [--out profiles/pose_polish.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_pose3d import C, FACTOR, H, K, REGIONS, W, rotation, scene, timed  # noqa: E402
from posecnn_amd import _lib, ops  # noqa: E402

EXTENT = 0.3


def planted(depth, dev):
    """the poses `bench_pose3d.scene` planted, recomputed from its depth frames and its seeded rotations: {(b, c): (R, t)}"""
    rng = np.random.RandomState(0)
    B = depth.shape[0]
    f64 = torch.float64
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=f64), torch.arange(W, device=dev, dtype=f64), indexing="ij")
    out = {}
    for b in range(B):
        zq = depth[b].view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).to(f64) / FACTOR
        eye = torch.stack([(x - K[2]) * zq / K[0], (y - K[3]) * zq / K[1], zq], dim=-1)
        for (c, y0, x0, w, h) in REGIONS:
            centre = eye[y0:y0 + h, x0:x0 + w].reshape(-1, 3).mean(0).cpu().numpy()
            out[(b, c)] = (rotation(rng), centre + np.array([0.0, 0.0, 0.1]))
    return out


def corner_displacements(poses64, truth):
    """largest corner distance per planted (frame, class) whose pose was found (t_z > 0)"""
    h = EXTENT / 2
    corners = np.array([[sx * h, sy * h, sz * h] for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)])
    out = []
    for (b, c), (R, t) in truth.items():
        P = poses64[b, c]
        if P[2, 3] > 0:
            out.append(float(np.linalg.norm((corners @ P[:, :3].T + P[:, 3]) - (corners @ R.T + t), axis=1).max()))
    return out


def summary(v):
    return {"median": float(np.median(v)), "max": float(np.max(v)), "classes": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--evaluations", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_polish.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pose_polish: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    B, seed = a.frames, 7
    label, depth, vertex, extents, intr, streams = scene(B, dev)
    truth = planted(depth, dev)
    kw = dict(seed=seed, streams=streams, hypotheses=a.hypotheses)

    def depth_route(evaluations=0):
        return ops.estimate_poses_3d(label, depth, vertex, extents, intr, FACTOR, polish_evaluations=evaluations, **kw)

    def colour_route(evaluations=0):
        return ops.estimate_poses_2d(label, vertex, extents, intr, polish_evaluations=evaluations, **kw)

    found, polished = {}, {}
    for name, route in (("depth", depth_route), ("colour", colour_route)):
        rows = {}
        for evaluations in (0, a.evaluations, 400):
            out = route(evaluations)
            rows[str(evaluations)] = summary(corner_displacements(out[1].cpu().numpy(), truth))
            if evaluations == a.evaluations:
                energy, evals, listed = (t.cpu().numpy() for t in out[5:])
                on = evals > 0
                polished[name] = {"classes": int(on.sum()), "listed_median": float(np.median(listed[on])),
                                  "energy_before_median": float(np.median(energy[on][:, 0])),
                                  "energy_after_median": float(np.median(energy[on][:, 1]))}
        found[name] = rows

    routes = {"depth": depth_route, "depth+polish": lambda: depth_route(a.evaluations), "colour": colour_route,
              "colour+polish": lambda: colour_route(a.evaluations)}
    for _ in range(a.warmup):
        for fn in routes.values():
            timed(fn)
    samples = {k: [] for k in routes}
    names = list(routes)
    for i in range(a.repeats):
        for k in (names if i % 2 == 0 else names[::-1]):
            samples[k].append(timed(routes[k]))
    kernels = {}
    _lib.profile_enable(True)
    for name in ("depth+polish", "colour+polish"):
        _lib.profile_report(reset=True)
        for _ in range(a.repeats):
            routes[name]()
        torch.cuda.synchronize()
        kernels[name] = {k: v["avg_us"] for k, v in _lib.profile_report(reset=True).items() if k.startswith(("pose_polish", "p3d_", "p2d_"))}
    _lib.profile_enable(False)

    result = {"what": "the final Nelder-Mead polish of both pose routes: each route without and with it, medians of alternating "
                      "repeats (ms); the polish launch alone by per-kernel events (us); corner displacement against the planted "
                      "poses (m) after 0 / %d / 400 evaluations; no hardware counters collected" % a.evaluations,
              "shape": {"frames": B, "height": H, "width": W, "classes": C, "hypotheses": a.hypotheses, "evaluations": a.evaluations,
                        "max_pixels": 1000, "min_pixels": 10},
              "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
              "polished": polished, "corner_displacement_m": found,
              "routes": {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in samples.items()},
              "kernels_avg_us": kernels}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
