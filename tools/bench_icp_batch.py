#!/usr/bin/env python
"""Depth-based pose refinement of a batch: `icp.refine_batch` (one call, no host round trip) against the per-frame
`Synthesizer.icp_python` loop, on the frames of the depth route's benchmarks — 16 frames of 480 x 640 with five live objects
per frame (tools/bench_icp.py's five ellipsoids of 81 920 triangles each, the size of a YCB `textured_simple.obj`, at poses
that differ from frame to frame; the network's poses 2 cm off in depth and a degree off). Timed in ONE process with
alternating repeats (medians; wall clock around each route, the device drained before and after):

  batch        icp.refine_batch on resident device tensors: 80 rows, 80 job slots
  per_frame    16 calls of Synthesizer.icp_python, as lib/fcn/test.py calls it (numpy label map and rows in, rows out)
  kernels      the batch call with the library's per-kernel events on (pcnn_profile_*)

The two routes' diagnostics (agree, pairs, choose, hits) are asserted equal, and their rows within 1e-6, before anything is
timed. bench.py does not call this; the result goes to --out (default profiles/icp_batch.json) and is printed as one JSON line.

    python tools/bench_icp_batch.py [--frames 16] [--repeats 20] [--warmup 2] [--subdivisions 6] [--out profiles/icp_batch.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from posecnn_amd import _lib, config, icp  # noqa: E402
from posecnn_amd.pose_error import quat2mat  # noqa: E402

H, W = 480, 640
FACTOR = 10000.0
SHAPES = [(0.05, (1.0, 0.7, 1.3)), (0.06, (0.8, 0.8, 1.2)), (0.045, (1.3, 1.0, 0.7)), (0.055, (1.0, 1.0, 1.0)), (0.05, (0.6, 1.2, 1.0))]
CENTRES = [(-0.18, -0.1, 0.75), (0.0, -0.1, 0.85), (0.18, -0.08, 0.8), (-0.1, 0.1, 0.7), (0.12, 0.1, 0.9)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def scene(B, sub, dev):
    import icp_scene as S
    K = config.DEMO_INTRINSICS.copy()
    rng = np.random.default_rng(7)
    meshes_np = [S.icosphere(r, sub, scale=sc) for r, sc in SHAPES]
    gm = [icp.Mesh(m[0], m[2], m[1], device=dev) for m in meshes_np]
    labels, depths, rois, poses, truths = [], [], [], [], []
    for b in range(B):
        depth, label = np.zeros((H, W), np.uint16), np.zeros((H, W), np.int32)
        for c, (g, ctr) in enumerate(zip(gm, CENTRES)):
            Tt = S.pose(S.rot(rng.standard_normal(3), rng.uniform(0, 3)), np.asarray(ctr) + rng.uniform(-0.01, 0.01, 3))
            v = icp.render(g, Tt[None], K, H, W, want=("vertices",))["vertices"][0].cpu().numpy()
            hit = np.isfinite(v[..., 2])
            depth = np.where(hit, np.clip(np.round(np.where(hit, v[..., 2], 0) * FACTOR), 0, 65535), depth).astype(np.uint16)
            label = np.where(hit, c + 1, label).astype(np.int32)
            est = S.pose(S.rot([0, 1, 0], 0.02) @ Tt[:, :3], Tt[:, 3] * (1 + 0.02 / Tt[2, 3]))
            rois.append([b, c + 1, 0, 0, 0, 0, 0])
            poses.append(np.concatenate([icp.mat2quat(est[:, :3]), est[:, 3]]))
            truths.append(Tt)
        labels.append(label)
        depths.append(depth)
    return (K, gm, np.stack(labels), np.stack(depths), np.asarray(rois, np.float32), np.asarray(poses, np.float32), truths,
            len(meshes_np[0][2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--subdivisions", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_batch.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_icp_batch: needs the GPU (a CPU run measures nothing)")
    import icp_scene as S
    dev = torch.device("cuda:0")
    B = a.frames
    K, gm, labels, depths, rois, poses, truths, triangles = scene(B, a.subdivisions, dev)
    R = len(rois)
    syn = icp.Synthesizer(meshes=gm, device=dev)
    syn.setup(W, H)
    bank = icp.MeshBank(gm, dev)
    up = lambda x: torch.from_numpy(x).to(dev)
    labels_t, depth_t = up(labels), up(depths.view(np.int16)).view(torch.uint16)
    intr = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]] * B, dtype=torch.float32, device=dev)
    rois_t, poses_t, count = up(rois), up(poses), torch.tensor([R], dtype=torch.int32, device=dev)
    params = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0.25, 6.0, FACTOR], np.float32)
    new, best, last = np.zeros((R, 7), np.float32), np.zeros((R, 7), np.float32), []

    def batch():
        return icp.refine_batch(labels_t, depth_t, intr, FACTOR, rois_t, poses_t, count, bank)

    def per_frame():
        del last[:]
        for b in range(B):
            rows = slice(5 * b, 5 * b + 5)
            syn.icp_python(labels[b], depths[b], params, H, W, 5, 7, rois[rows], poses[rows], new[rows], best[rows], 0.01)
            last.extend(syn.last)

    # the two routes compute the same thing at full size
    out = batch()
    pn, pi, info = (t.cpu().numpy() for t in out)
    per_frame()
    assert (info[:, 0] == icp.STATUS_REFINED).all() and len(last) == R
    unequal = 0
    for r, d in enumerate(last):
        assert (d["agree"], d["pairs"], d["choose"]) == tuple(info[r, 1:4]) and d["hits"].tolist() == info[r, 4:].tolist(), r
        for got, want in ((pn[r], new[r]), (pi[r], best[r])):
            assert np.abs(quat2mat(got[:4].astype(np.float64)) - quat2mat(want[:4].astype(np.float64))).max() < 1e-6
            assert np.abs(got[4:] - want[4:]).max() < 1e-6
            unequal += int((got.view(np.uint32) != want.view(np.uint32)).sum())
    errs = [S.pose_error(S.pose(quat2mat(pi[r, :4].astype(np.float64)), pi[r, 4:]), truths[r]) for r in range(R)]

    routes = {"batch": batch, "per_frame": per_frame}
    for _ in range(a.warmup):
        for fn in routes.values():
            wall(fn)
    samples = {k: [] for k in routes}
    names = list(routes)
    for i in range(a.repeats):
        for k in (names if i % 2 == 0 else names[::-1]):
            samples[k].append(wall(routes[k]))
    kernels = {}
    for name, fn in routes.items():
        _lib.profile_enable(True)
        _lib.profile_report(reset=True)
        fn()
        torch.cuda.synchronize()
        kernels[name] = _lib.profile_report(reset=True)
        _lib.profile_enable(False)
    need = ctypes.c_size_t()
    _lib.call("pcnn_icp_batch_workspace_bytes", R, H, W, ctypes.byref(need))
    med = {k: statistics.median(v) for k, v in samples.items()}
    result = {"what": "depth-based pose refinement: refine_batch (one call) against the per-frame icp_python loop, medians of alternating repeats (wall ms, device drained)",
              "shape": {"frames": B, "height": H, "width": W, "rows": R, "objects_per_frame": 5, "triangles_per_mesh": triangles,
                        "label_pixels_frame0": int((labels[0] > 0).sum()), "job_slots": R},
              "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
              "diagnostics_equal": True, "row_entries_not_bit_equal_to_icp_python": unequal, "row_entries": 14 * R,
              "translation_error_mm_max": max(e[1] for e in errs) * 1e3, "rotation_error_deg_max": max(e[0] for e in errs),
              "routes": {k: {"median_ms": med[k], "min_ms": min(v), "max_ms": max(v), "ms_per_object": med[k] / R} for k, v in samples.items()},
              "per_frame_over_batch": med["per_frame"] / med["batch"],
              "workspace_bytes": need.value, "workspace_bytes_per_job": need.value // R,
              "kernels_total_us": {route: {k: round(v["total_ms"] * 1e3, 1) for k, v in sorted(rep.items())} for route, rep in kernels.items()},
              "kernel_ms": {route: sum(v["total_ms"] for v in rep.values()) for route, rep in kernels.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
