#!/usr/bin/env python
"""3-D vertex route, pose stage (include/posecnn_hip_pose3d.h) at 16 frames of 480 x 640, 22 classes, five live classes per
frame of 8 000 to 19 600 pixels (20 % gross outliers, 5 % depth holes), 256 hypotheses, the reference's defaults. Timed in ONE
process with alternating repeats (medians; device events around the calls on resident inputs):

  driver       ops.estimate_poses_3d: prepare, sample and the whole preemptive loop as three launches, nothing read back
  kernels      the same call with the library's per-kernel events on (pcnn_profile_*): the three launches one by one
  host_loop    the shape of a direct port: ops.pose3d_prepare and ops.pose3d_sample, then one ops.pose3d_round per round
               with the class ids read back between rounds to decide, per (frame, class), whether it goes on

The host loop's poses, inlier counts, refinement steps and hypothesis counts are asserted bit-equal to the driver's at full
size before anything is timed. bench.py does not call this; the result goes to --out (default profiles/pose3d.json) and is
printed as one JSON line.

    python tools/bench_pose3d.py [--repeats 20] [--warmup 3] [--out profiles/pose3d.json]
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
from posecnn_amd import _lib, ops  # noqa: E402

H, W, C = 480, 640, 22
FACTOR = 10000.0
REGIONS = ((1, 20, 20, 100, 80), (5, 20, 200, 120, 100), (9, 200, 20, 125, 128), (13, 200, 250, 140, 140), (17, 360, 20, 100, 100))
K = (572.4, 573.6, 325.3, 242.0)
REF_IT = 8


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def scene(B, dev):
    """planted frames built on the device: every class region carries one rigid pose (tests/pose3d_cases.py at full size)"""
    rng = np.random.RandomState(0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    f64 = torch.float64
    label = torch.zeros((B, H, W), dtype=torch.int32, device=dev)
    vertex = torch.rand((B, H, W, 3 * C), dtype=torch.float32, device=dev, generator=g)
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=f64), torch.arange(W, device=dev, dtype=f64), indexing="ij")
    extents = np.zeros((C, 3), np.float32)
    extents[1:] = 0.3
    depths = []
    for b in range(B):
        z = 0.8 + 0.0002 * (b + 1) * x / 16 + 0.0001 * y
        d = torch.round(z * FACTOR)
        u = torch.rand((H, W), dtype=f64, device=dev, generator=g)
        d = torch.where((u >= 0.20) & (u < 0.25), torch.zeros_like(d), d)
        zq = d / FACTOR
        eye = torch.stack([(x - K[2]) * zq / K[0], (y - K[3]) * zq / K[1], zq], dim=-1)
        for (c, y0, x0, w, h) in REGIONS:
            label[b, y0:y0 + h, x0:x0 + w] = c
            e = eye[y0:y0 + h, x0:x0 + w]
            centre = e.reshape(-1, 3).mean(0).cpu().numpy()
            R, t = rotation(rng), centre + np.array([0.0, 0.0, 0.1])
            obj = (e - torch.from_numpy(t).to(dev)) @ torch.from_numpy(R).to(dev)
            off = torch.randn((h, w, 3), dtype=f64, device=dev, generator=g)
            off = off / off.norm(dim=-1, keepdim=True) * (0.05 + 0.1 * torch.rand((h, w, 1), dtype=f64, device=dev, generator=g))
            obj = torch.where((u[y0:y0 + h, x0:x0 + w] < 0.20)[..., None], obj + off, obj)
            vertex[b, y0:y0 + h, x0:x0 + w, 3 * c:3 * c + 3] = (obj / 0.3 + 0.5).to(torch.float32)
        depths.append(d.to(torch.int32).to(torch.int16))
    depth = torch.stack(depths).view(torch.uint16)
    intr = torch.tensor([K] * B, dtype=torch.float32, device=dev)
    streams = torch.arange(B, dtype=torch.int64, device=dev)
    return label, depth, vertex, torch.from_numpy(extents).to(dev), intr, streams


def host_loop(args, streams, hypotheses, seed):
    """prepare, sample, then one launch per round with a host read in between; -> (poses64, inliers, ref_steps, num_hyps, rounds)"""
    label, depth, vertex, extents, intr = args
    B = label.shape[0]
    records, counts, offsets = ops.pose3d_prepare(label, depth, vertex, extents, intr, FACTOR)
    pose, cls, _, _ = ops.pose3d_sample(records, counts, offsets, extents, intr, H, W, seed=seed, streams=streams, hypotheses=hypotheses)
    cls_h = cls.cpu().numpy()
    poses64, inliers = np.zeros((B, C, 3, 4)), np.zeros((B, C), np.int32)
    ref_steps, num_hyps = np.zeros((B, C), np.int32), np.zeros((B, C), np.int32)
    for b in range(B):
        num_hyps[b] = np.bincount(cls_h[b], minlength=C)[:C]
    num_hyps[:, 0] = 0
    rnd = 0
    while (cls_h > 0).any():
        rnd += 1
        pose, cls, inl = ops.pose3d_round(records, counts, offsets, pose, cls, H, W, rnd)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose3d.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pose3d: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    B, seed = a.frames, 7
    label, depth, vertex, extents, intr, streams = scene(B, dev)
    args = (label, depth, vertex, extents, intr)

    def driver():
        return ops.estimate_poses_3d(*args, FACTOR, seed=seed, streams=streams, hypotheses=a.hypotheses)

    # the two routes compute the same thing, bit for bit, at full size
    poses, poses64, inliers, ref_steps, num_hyps = (t.cpu().numpy() for t in driver())
    h64, hin, hrs, hnh, rounds = host_loop(args, streams, a.hypotheses, seed)
    equal = {"poses64": bool((poses64.view(np.uint64) == h64.view(np.uint64)).all()), "inliers": bool((inliers == hin).all()),
             "ref_steps": bool((ref_steps == hrs).all()), "num_hyps": bool((num_hyps == hnh).all())}
    assert all(equal.values()), equal
    live = [int(c) for c in np.nonzero(num_hyps[0])[0]]
    pixels = [int((label[0] == c).sum()) for c in live]

    routes = {"driver": driver, "host_loop": lambda: host_loop(args, streams, a.hypotheses, seed)}
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

    result = {"what": "3-D pose stage: three-launch driver against a host loop of single rounds, medians of alternating repeats (ms)",
              "shape": {"frames": B, "height": H, "width": W, "classes": C, "hypotheses": a.hypotheses, "live_classes": live,
                        "class_pixels": pixels, "rounds": rounds},
              "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
              "host_loop_bit_equal_to_driver": equal,
              "found": int((poses64[:, :, 2, 3] > 0).sum()), "inliers_frame0": [int(inliers[0, c]) for c in live],
              "vertex_pred_bytes_per_pixel_row": 12 * C, "vertex_pred_useful_bytes_per_class_pixel": 12,
              "routes": {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in samples.items()},
              "kernels_avg_us": {k: v["avg_us"] for k, v in kernels.items() if k.startswith("p3d_")}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
