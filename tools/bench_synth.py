#!/usr/bin/env python
"""Synthetic training scenes (include/posecnn_hip_synth.h) at 16 scenes of 480 x 640, 5-7 objects each, timed in ONE
process with alternating repeats (medians; device events around the library call on preallocated tensors):

  synth      pcnn_synth_scene_fwd, the whole call, and per kernel (the library's own event pairs, pcnn_profile_*, in
             passes of their own: the pairs serialise the launches, so their sum is not the call's time)
  one_by_one the same objects rendered one at a time with icp.render (geometry only: camera-frame vertex map, no
             lighting, no compositing, one depth buffer per object) — what the refinement renderer would cost as a feed
  train_step one SolverWrapper.train_step of the trainable graph at the same batch size, fed from the rendered batch
             (skipped with --no-train)

at two model sizes: icospheres of 20 480 faces (the order of the reference's 16 k-face models) and of 327 680 faces (the
order of a 260 k-face scan), eight differently scaled copies per bank. Scenes come from SceneSampler(seed 0). bench.py does
not call this; the result goes to --out (default profiles/synth_scene.json) and is printed as one JSON line.

    python tools/bench_synth.py [--repeats 20] [--warmup 3] [--no-train] [--out profiles/synth_scene.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from posecnn_amd import _lib, config, icp, synth, synthesize as syn  # noqa: E402


def ellipsoids(subdivisions, count, radius=0.06):
    """`count` differently scaled copies of one subdivided icosahedron (tests/icp_scene.py): (vertices, normals, faces)"""
    import icp_scene
    v, _, f = icp_scene.icosphere(1.0, subdivisions)
    v = v.astype(np.float64)
    for m in range(count):
        sc = radius * np.array([1.0 + 0.05 * m, 1.0 - 0.04 * m, 1.0 + 0.03 * (m % 3)])
        n = v / sc
        yield (v * sc).astype(np.float32), (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32), f


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_scene.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_synth: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    H, W, S = 480, 640, a.scenes
    K = config.DEMO_INTRINSICS
    rng = np.random.default_rng(0)
    bg = torch.from_numpy(rng.integers(0, 256, (S, H, W, 3)).astype(np.uint8)).to(dev)
    result = {"what": "synthetic scenes: one call per minibatch against one icp.render per object, medians (ms)",
              "shape": {"scenes": S, "height": H, "width": W}, "device": torch.cuda.get_device_name(0),
              "repeats": a.repeats, "warmup": a.warmup, "banks": {}}
    batch = None
    for subdiv in (5, 7):
        meshes = []
        for v, n, f in ellipsoids(subdiv, 8):
            meshes.append(icp.Mesh(v, f, n, device=dev))
            meshes[-1].colors = rng.uniform(0, 1, v.shape).astype(np.float32)
        bank = syn.MeshBank(meshes, device=dev)
        sampler = syn.SceneSampler(8, seed=0, tnear=0.5, tfar=1.5)
        scenes = [sampler.sample() for _ in range(S)]
        routes = {
            "synth": lambda: syn.render_scenes(bank, scenes, K, H, W, bg, min_pixels=800),
            "one_by_one": lambda: [icp.render(meshes[m], T[None], K, H, W, (syn.Z_NEAR, syn.Z_FAR), want=("vertices",))
                                   for sc in scenes for m, T, _ in sc.instances],
        }
        for _ in range(a.warmup):
            for r in routes.values():
                timed(r)
        samples = {r: [] for r in routes}
        for i in range(a.repeats):
            for r in (("synth", "one_by_one") if i % 2 == 0 else ("one_by_one", "synth")):
                samples[r].append(timed(routes[r]))
        _lib.profile_enable(True)
        _lib.profile_report()
        for _ in range(a.repeats):
            routes["synth"]()
        torch.cuda.synchronize()
        kernels = {k: v["total_ms"] / a.repeats for k, v in _lib.profile_report().items()}
        _lib.profile_enable(False)
        batch = routes["synth"]()
        counts = batch.pixel_counts.cpu().numpy()
        n_inst = sum(len(sc.instances) for sc in scenes)
        med = {r: statistics.median(v) for r, v in samples.items()}
        result["banks"]["%d_faces" % len(meshes[0].faces_np)] = {
            "faces_per_mesh": int(len(meshes[0].faces_np)), "instances": n_inst,
            "triangles_per_batch": int(sum(len(meshes[m].faces_np) for sc in scenes for m, _, _ in sc.instances)),
            "median_ms": med, "min_max_ms": {r: [min(v), max(v)] for r, v in samples.items()},
            "per_kernel_ms_serialised": kernels, "one_by_one_over_synth": med["one_by_one"] / med["synth"],
            "valid_scenes": int(batch.valid.sum()), "mean_pixels_per_instance": float(counts.mean()),
            "covered_fraction": float((batch.label > 0).float().mean()),
        }
    if not a.no_train:
        from posecnn_amd import train
        from posecnn_amd.networks import vgg16_convs
        torch.manual_seed(0)
        net = vgg16_convs("COLOR", 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=True, is_train=True,
                          device=dev, seed=3, init="he")
        feed = batch.feed(config.LOV_EXTENTS, synth.make_model_points(22, 64), config.LOV_SYMMETRY)

        class Cfg(train.TrainConfig):
            LEARNING_RATE = 1e-6

        solver = train.SolverWrapper(net, Cfg)
        solver.train_step(feed)
        steps = [timed(lambda: solver.train_step(feed)) for _ in range(3)]
        result["train_step_ms"] = {"median": statistics.median(steps), "samples": steps, "batch": S}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
