#!/usr/bin/env python
"""Three routes to one training step's vertex loss (forward + backward w.r.t. vertex_pred) at B = 16, 480 x 640, C = 22,
timed in ONE process with alternating repeats (medians):

  (a) host      numpy builds vertex_targets / vertex_weights as the reference's minibatch code does, then uploads them
                (2 x 1.30 GB) — generation + upload only, the loss kernels of (b) would follow
  (b) generator pcnn_vertex_targets_fwd on the device + pcnn_smooth_l1_vertex_fwd / _bwd on the materialised tensors
  (c) fused     pcnn_smooth_l1_vertex_gt_fwd / _bwd straight from the label map and the object table

(b) and (c) are timed with device events around the library calls on preallocated buffers; (a) with a host clock that
ends in a device synchronise. The write roof is measured here too: a plain fill of a 1.30 GB tensor. bench.py does not
call this; the result goes to profiles/vertex_loss.json.

    python tools/bench_vertex_loss.py [--repeats 20] [--host-repeats 20] [--out profiles/vertex_loss.json]
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
import vertex_ref  # noqa: E402  (the numpy restatement of the reference's host code)
from posecnn_amd import _lib, config, ops, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--classes", type=int, default=22)
    ap.add_argument("--objects", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_loss.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vertex_loss: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    B, H, W, C, sigma = a.batch, a.height, a.width, a.classes, 1.0
    K = config.DEMO_INTRINSICS.copy()
    K[:2] *= W / 640.0
    label, _, frames = synth.make_batch(4000, B, H=H, W=W, C=C, n_obj=a.objects, K=K)
    label = label.astype(np.int32)
    obj = np.zeros((B, a.objects, 6), np.float32)
    for b, fr in enumerate(frames):
        for j, (cls, cx, cy, z) in enumerate(fr["objects"]):
            obj[b, j] = (cls, 0, np.float32(cx), np.float32(cy), np.float32(np.log(z)), 10.0)
    n = B * H * W * 3 * C
    tensor_bytes = 4 * n

    L = _lib.lib()
    P = ops._ptr
    d_label, d_obj = torch.from_numpy(label).to(dev), torch.from_numpy(obj).to(dev)
    pred = torch.randn((B, H, W, 3 * C), device=dev)
    targets, weights, grad_b, grad_c = (torch.empty_like(pred) for _ in range(4))
    out_b, out_c = torch.empty(3, device=dev), torch.empty(3, device=dev)
    nbytes = ctypes.c_size_t(0)
    _lib.check("workspace", L.pcnn_smooth_l1_vertex_workspace_bytes(ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    up = torch.full((1,), 5.0, device=dev)
    stream = ops._stream(pred)
    M = obj.shape[1]

    calls = {
        "b_generate": lambda: L.pcnn_vertex_targets_fwd(P(d_label), None, P(d_obj), B, H, W, C, M, P(targets), P(weights), stream),
        "b_forward": lambda: L.pcnn_smooth_l1_vertex_fwd(P(pred), P(targets), P(weights), n, sigma, P(out_b), P(ws), ws.numel(), stream),
        "b_backward": lambda: L.pcnn_smooth_l1_vertex_bwd(P(pred), P(targets), P(weights), P(out_b), P(up), n, sigma, P(grad_b), stream),
        "c_forward": lambda: L.pcnn_smooth_l1_vertex_gt_fwd(P(pred), P(d_label), None, P(d_obj), B, H, W, C, M, sigma, P(out_c), P(ws),
                                                            ws.numel(), stream),
        "c_backward": lambda: L.pcnn_smooth_l1_vertex_gt_bwd(P(pred), P(d_label), None, P(d_obj), P(out_c), P(up), B, H, W, C, M, sigma,
                                                             P(grad_c), stream),
        "fill": lambda: grad_c.fill_(1.0).numel() * 0,
    }
    routes = {"b": ("b_generate", "b_forward", "b_backward"), "c": ("c_forward", "c_backward"), "roof": ("fill",)}

    def run_route(r):
        """-> per-call milliseconds of one pass over the route's calls (device events)."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(routes[r]) + 1)]
        ev[0].record()
        for k, name in enumerate(routes[r]):
            _lib.check(name, calls[name]())
            ev[k + 1].record()
        torch.cuda.synchronize()
        return {name: ev[k].elapsed_time(ev[k + 1]) for k, name in enumerate(routes[r])}

    def host_route():
        t0 = time.perf_counter()
        t, w = vertex_ref.vertex_targets(label, obj, C)
        t1 = time.perf_counter()
        dt, dw = torch.from_numpy(t).to(dev), torch.from_numpy(w).to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return {"a_generate_host": (t1 - t0) * 1e3, "a_upload": (t2 - t1) * 1e3}, dt, dw

    # same results before any timing
    run_route("b"), run_route("c")
    same_out = bool(torch.equal(out_b.view(torch.int32), out_c.view(torch.int32)))
    same_grad = bool(torch.equal(grad_b, grad_c))
    _, dt, dw = host_route()
    same_host = bool(torch.equal(dt.view(torch.int32), targets.view(torch.int32)) and torch.equal(dw.view(torch.int32), weights.view(torch.int32)))
    del dt, dw
    if not (same_out and same_grad and same_host):
        sys.exit("bench_vertex_loss: the routes disagree (loss %s, grad %s, host targets %s)" % (same_out, same_grad, same_host))

    for _ in range(a.warmup):
        for r in ("b", "c", "roof"):
            run_route(r)
    samples = {}
    for i in range(max(a.repeats, a.host_repeats)):
        order = ("b", "c", "roof") if i % 2 == 0 else ("c", "b", "roof")     # alternate who goes first
        for r in order:
            if i < a.repeats:
                for k, v in run_route(r).items():
                    samples.setdefault(k, []).append(v)
        if i < a.host_repeats:
            t, dt, dw = host_route()
            del dt, dw
            for k, v in t.items():
                samples.setdefault(k, []).append(v)

    med = {k: statistics.median(v) for k, v in samples.items()}
    spread = {k: [min(v), max(v)] for k, v in samples.items()}
    total = lambda r: statistics.median([sum(samples[k][i] for k in routes[r]) for i in range(a.repeats)])
    b_ms, c_ms = total("b"), total("c")
    roof = tensor_bytes / (med["fill"] * 1e-3)
    written = {"b_generate": 2 * tensor_bytes, "b_backward": tensor_bytes, "c_backward": tensor_bytes}
    result = {
        "what": "vertex loss forward + backward, three routes, one process, alternating repeats, medians (ms)",
        "shape": {"batch": B, "height": H, "width": W, "classes": C, "objects_per_frame": M, "elements": n,
                  "tensor_bytes": tensor_bytes, "foreground_fraction": float((label > 0).mean())},
        "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "host_repeats": a.host_repeats, "warmup": a.warmup,
        "median_ms": med, "min_max_ms": spread,
        "route_ms": {"a_host_generation_plus_upload": med["a_generate_host"] + med["a_upload"] if a.host_repeats > 0 else None,
                     "b_generator_plus_unfused_loss": b_ms, "c_fused_loss": c_ms},
        "b_over_c": b_ms / c_ms, "fused_is_faster_than_generator_route": bool(c_ms < b_ms),
        "write_roof": {"how": "torch fill_ of one [B,H,W,3C] f32 tensor in this process", "bytes": tensor_bytes, "ms": med["fill"],
                       "bytes_per_s": roof},
        "fraction_of_write_roof": {k: written[k] / (med[k] * 1e-3) / roof for k in written},
        "bytes_written": written,
        "results_identical": {"loss_bits": same_out, "grad_equal": same_grad, "host_targets_bits": same_host},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
