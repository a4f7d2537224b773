#!/usr/bin/env python
"""3-D vertex route, colour-only pose stage (include/posecnn_hip_pose2d.h) on the frames of tools/bench_pose3d.py: 16 frames
of 480 x 640, 22 classes, five live classes per frame of 8 000 to 19 600 pixels (20 % gross outliers), 256 hypotheses, the
reference's thresholds (10 pixels). Timed in ONE process with alternating repeats (medians; device events around the calls
on resident inputs):

  driver       ops.estimate_poses_2d: prepare, sample and the whole preemptive loop as three launches, nothing read back
  kernels      the same call with the library's per-kernel events on (pcnn_profile_*): the three launches one by one
  host_loop    the shape of a direct port: ops.pose2d_prepare and ops.pose2d_sample, then one ops.pose2d_round per round
               with the class ids read back between rounds to decide, per (frame, class), whether it goes on
  depth_route  ops.estimate_poses_3d on the same frames with their depth, for scale

The host loop's poses, inlier counts, refinement steps and hypothesis counts are asserted bit-equal to the driver's at full
size before anything is timed. No hardware counters are collected. bench.py does not call this; the result goes to --out
(default profiles/pose2d.json) and is printed as one JSON line.

    python tools/bench_pose2d.py [--repeats 20] [--warmup 3] [--out profiles/pose2d.json]
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
from bench_pose3d import C, FACTOR, H, REF_IT, W, scene, timed  # noqa: E402
from posecnn_amd import _lib, ops  # noqa: E402


def host_loop(args, streams, hypotheses, seed):
    """prepare, sample, then one launch per round with a host read in between; -> (poses64, inliers, ref_steps, num_hyps, rounds)"""
    label, vertex, extents, intr = args
    B = label.shape[0]
    records, counts, offsets = ops.pose2d_prepare(label, vertex, extents)
    pose, cls, _, _ = ops.pose2d_sample(records, counts, offsets, extents, intr, H, W, seed=seed, streams=streams, hypotheses=hypotheses)
    cls_h = cls.cpu().numpy()
    poses64, inliers = np.zeros((B, C, 3, 4)), np.zeros((B, C), np.int32)
    ref_steps, num_hyps = np.zeros((B, C), np.int32), np.zeros((B, C), np.int32)
    for b in range(B):
        num_hyps[b] = np.bincount(cls_h[b], minlength=C)[:C]
    num_hyps[:, 0] = 0
    rnd = 0
    while (cls_h > 0).any():
        rnd += 1
        pose, cls, inl = ops.pose2d_round(records, counts, offsets, intr, pose, cls, H, W, rnd)
        cls_h = cls.cpu().numpy()                                   # the host decides who goes on
        done = []
        for b, c in zip(*np.nonzero(num_hyps)):
            alive = np.nonzero(cls_h[b] == c)[0]
            if len(alive) == 0:
                continue
            ref_steps[b, c] = rnd
            if len(alive) == 1 and rnd >= REF_IT:
                done.append((b, c, alive[0]))
        if done:
            pose_h, inl_h = pose.cpu().numpy(), inl.cpu().numpy()
            for b, c, h in done:
                poses64[b, c], inliers[b, c] = pose_h[b, h], inl_h[b, h]
                cls_h[b, h] = 0
            cls = torch.from_numpy(cls_h).to(cls.device)
    return poses64, inliers, ref_steps, num_hyps, rnd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose2d.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pose2d: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    B, seed = a.frames, 7
    label, depth, vertex, extents, intr, streams = scene(B, dev)
    args = (label, vertex, extents, intr)

    def driver():
        return ops.estimate_poses_2d(*args, seed=seed, streams=streams, hypotheses=a.hypotheses)

    def depth_route():
        return ops.estimate_poses_3d(label, depth, vertex, extents, intr, FACTOR, seed=seed, streams=streams, hypotheses=a.hypotheses)

    # the two routes compute the same thing, bit for bit, at full size
    poses, poses64, inliers, ref_steps, num_hyps = (t.cpu().numpy() for t in driver())
    h64, hin, hrs, hnh, rounds = host_loop(args, streams, a.hypotheses, seed)
    equal = {"poses64": bool((poses64.view(np.uint64) == h64.view(np.uint64)).all()), "inliers": bool((inliers == hin).all()),
             "ref_steps": bool((ref_steps == hrs).all()), "num_hyps": bool((num_hyps == hnh).all())}
    assert all(equal.values()), equal
    live = [int(c) for c in np.nonzero(num_hyps[0])[0]]
    pixels = [int((label[0] == c).sum()) for c in live]
    # how far the colour route lands from the depth route on the same frames (translation, metres)
    p3 = depth_route()[1].cpu().numpy()
    both = (poses64[:, :, 2, 3] > 0) & (p3[:, :, 2, 3] > 0)
    apart = np.linalg.norm(poses64[both][:, :, 3] - p3[both][:, :, 3], axis=1)

    routes = {"driver": driver, "host_loop": lambda: host_loop(args, streams, a.hypotheses, seed), "depth_route": depth_route}
    for _ in range(a.warmup):
        for fn in routes.values():
            timed(fn)
    samples = {k: [] for k in routes}
    names = list(routes)
    for i in range(a.repeats):
        for k in (names if i % 2 == 0 else names[::-1]):
            samples[k].append(timed(routes[k]))
    _lib.profile_enable(True)
    _lib.profile_report(reset=True)
    for _ in range(a.repeats):
        driver()
    torch.cuda.synchronize()
    kernels = _lib.profile_report(reset=True)
    _lib.profile_enable(False)

    result = {"what": "colour-only pose stage: three-launch driver against a host loop of single rounds and against the depth "
                      "route on the same frames, medians of alternating repeats (ms); no hardware counters collected",
              "shape": {"frames": B, "height": H, "width": W, "classes": C, "hypotheses": a.hypotheses, "live_classes": live,
                        "class_pixels": pixels, "rounds": rounds},
              "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
              "host_loop_bit_equal_to_driver": equal,
              "found": int((poses64[:, :, 2, 3] > 0).sum()), "inliers_frame0": [int(inliers[0, c]) for c in live],
              "translation_from_depth_route_m": {"median": float(np.median(apart)), "max": float(apart.max()), "classes": int(both.sum())},
              "routes": {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in samples.items()},
              "kernels_avg_us": {k: v["avg_us"] for k, v in kernels.items() if k.startswith("p2d_")}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
