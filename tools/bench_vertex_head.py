#!/usr/bin/env python
"""The training vertex head, fused against today's lowres_train_heads route, at B = 16, 480 x 640, C = 22, on one GPU.

  op     forward + backward of the vertex head from the 128-channel 1/8-resolution feature x [B,60,80,128]:
           lowres   framework 1x1 conv of x -> ops.deconv_bilinear(z, 16, 8, bias) (vertex_pred [B,480,640,66] materialised,
                    bias added by the framework) -> ops.smooth_l1_loss_vertex_gt, autograd back to x, weights and bias:
                    what vgg16_convs(lowres_train_heads=True) runs today
           fused    the same 1x1 conv -> ops.vertex_head_loss, autograd back to the same three
         and the peak memory of one forward + backward above the inputs
  sl1    ops.smooth_l1_loss_vertex_gt alone on a resident vertex_pred: forward and backward, device events
  step   one SolverWrapper.train_step of the trainable RGB-D graph (lowres_train_heads=True) on a synthetic training batch
         with the object-table vertex feed, fused_vertex_loss off and on: wall time per step
  memory torch.cuda.max_memory_allocated of one such step, each graph alone in a process of its own

Each part runs in a child process of its own under a time limit; inside it the two sides alternate (who goes first
changes every repeat) and medians and min / max of `--repeats` samples are reported. The comparison is always the other
route in the same run. bench.py does not call this; the result goes to profiles/vertex_head.json.

    python tools/bench_vertex_head.py [--repeats 20] [--parts op,sl1,step,memory] [--out profiles/vertex_head.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"op": 240, "sl1": 180, "step": 420, "mem_lowres": 180, "mem_fused": 180}     # seconds per child process
MODES = {"lowres": False, "fused": True}


def _stats(samples):
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} for k, v in samples.items()}


def _scene(a, dev, n_obj=5, seed=4000):
    """label map int32 [B,H,W] and object table f32 [B,n_obj,6] of a synthetic scene, on the device"""
    import numpy as np
    import torch
    from posecnn_amd import synth
    label, _, frames = synth.make_batch(seed, a.batch, H=a.height, W=a.width, C=a.classes, n_obj=n_obj)
    objects = np.zeros((a.batch, n_obj, 6), np.float32)
    for n in range(a.batch):
        for j, (cls, cx, cy, z) in enumerate(frames[n]["objects"]):
            objects[n, j] = (cls, 0, np.float32(cx), np.float32(cy), np.float32(np.log(z)), 1.0)
    foreground = float(((label > 0) & (label < a.classes)).mean())
    return torch.from_numpy(label.astype(np.int32)).to(dev), torch.from_numpy(objects).to(dev), foreground


def part_op(a):
    import torch
    import torch.nn.functional as F
    from posecnn_amd import ops
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    B, H, W, C, U, k, s = a.batch, a.height, a.width, a.classes, 128, 16, 8
    h, w = H // s, W // s
    g = torch.Generator(device="cpu").manual_seed(7)
    gt, objects, foreground = _scene(a, dev)
    x = torch.randn((B, h, w, U), generator=g).to(dev).requires_grad_(True)
    wt = (torch.randn((3 * C, U, 1, 1), generator=g) * 0.1).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bias = (torch.randn(3 * C, generator=g) * 0.1).to(dev).requires_grad_(True)
    nchw, nhwc = (lambda t: t.permute(0, 3, 1, 2)), (lambda t: t.permute(0, 2, 3, 1))

    def lowres():
        z = nhwc(F.conv2d(nchw(x), wt, None)).contiguous()
        return ops.smooth_l1_loss_vertex_gt(ops.deconv_bilinear(z, k, s, bias=bias), gt, objects)

    def fused():
        z = nhwc(F.conv2d(nchw(x), wt, None)).contiguous()
        return ops.vertex_head_loss(z, bias, gt, objects, k, s)[0]

    def once(route):
        for t in (x, wt, bias):
            t.grad = None
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        with torch.enable_grad():
            loss = route()
            ev[1].record()
            loss.backward()
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), loss.detach(), [t.grad.clone() for t in (x, wt, bias)]

    _, _, l_low, g_low = once(lowres)
    _, _, l_fus, g_fus = once(fused)
    rel = lambda p, q: float((p.double() - q.double()).norm() / q.double().norm())
    agreement = {"loss_lowres": float(l_low), "loss_fused": float(l_fus), "loss_bits_equal": bool(torch.equal(l_low, l_fus)),
                 "x_grad_bits_equal": bool(torch.equal(g_low[0], g_fus[0])),
                 "grad_rel_err": {n: rel(p, q) for n, p, q in zip(("x", "weights", "bias"), g_fus, g_low)}}
    if not agreement["loss_bits_equal"] or max(agreement["grad_rel_err"].values()) > 1e-4:
        sys.exit("bench_vertex_head: the routes disagree: %s" % json.dumps(agreement))
    del g_low, g_fus
    routes = {"lowres": lowres, "fused": fused}
    peak = {}
    for name, r in routes.items():
        for _ in range(a.warmup):
            once(r)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        once(r)
        peak[name] = int(torch.cuda.max_memory_allocated() - base)
    samples = {}
    for i in range(a.repeats):
        for name in (("lowres", "fused") if i % 2 == 0 else ("fused", "lowres")):
            f, b, _, _ = once(routes[name])
            for key, v in ((name + "_forward_ms", f), (name + "_backward_ms", b), (name + "_ms", f + b)):
                samples.setdefault(key, []).append(v)
    st = _stats(samples)
    return {"what": "vertex head forward + backward from the 1/8-resolution feature, device events, alternating repeats",
            "shape": {"batch": B, "height": H, "width": W, "classes": C, "units": U, "kernel": k, "stride": s,
                      "foreground_fraction": foreground},
            "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "ms": st,
            "lowres_over_fused": st["lowres_ms"]["median"] / st["fused_ms"]["median"],
            "fused_is_faster": bool(st["fused_ms"]["median"] < st["lowres_ms"]["median"]),
            "peak_bytes_above_inputs": peak, "agreement": agreement}


def part_sl1(a):
    import torch
    from posecnn_amd import ops
    dev = torch.device("cuda:0")
    B, H, W, C = a.batch, a.height, a.width, a.classes
    gt, objects, foreground = _scene(a, dev)
    g = torch.Generator(device="cpu").manual_seed(9)
    pred = torch.randn((B, H, W, 3 * C), generator=g).to(dev).requires_grad_(True)

    def once():
        pred.grad = None
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        with torch.enable_grad():
            loss = ops.smooth_l1_loss_vertex_gt(pred, gt, objects)
            ev[1].record()
            loss.backward()
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    for _ in range(a.warmup):
        once()
    samples = {"forward_ms": [], "backward_ms": []}
    for _ in range(a.repeats):
        f, b = once()
        samples["forward_ms"].append(f)
        samples["backward_ms"].append(b)
    nbytes = pred.numel() * 4
    st = _stats(samples)
    return {"what": "ops.smooth_l1_loss_vertex_gt alone on a resident vertex_pred, device events; the backward includes "
                    "autograd's handling of the 1.3 GB gradient it writes",
            "shape": {"batch": B, "height": H, "width": W, "classes": C, "foreground_fraction": foreground},
            "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "ms": st, "tensor_bytes": nbytes,
            "backward_write_GBps": nbytes / st["backward_ms"]["median"] / 1e6}


def _step_setup(a, modes):
    """-> once(mode): one train_step of that graph, (milliseconds, losses)."""
    import numpy as np
    import torch
    from posecnn_amd import config, synth, train
    from posecnn_amd.networks import vgg16_convs
    dev = torch.device("cuda:0")
    B, H, W, C = a.batch, a.height, a.width, a.classes
    K = config.DEMO_INTRINSICS.copy()
    K[:2] *= W / 640.0
    f32 = np.float32
    label, _, frames = synth.make_batch(100000, B, H=H, W=W, C=C, n_obj=3, K=K)
    planted_np, scenes = synth.make_planted_batch(100000, B, H=H, W=W, C=C, num_units=64, n_obj=3, K=K)
    g = torch.Generator(device="cpu").manual_seed(1234)
    means = torch.from_numpy(config.PIXEL_MEANS)
    data = (torch.randint(0, 256, (B, H, W, 3), generator=g).float() - means).float()
    depth = torch.randint(0, 3000, (B, H, W, 1), generator=g).float()
    data_p = ((torch.clamp(depth / 2000.0, 0, 1) * 255).expand(B, H, W, 3) - means).float().contiguous()
    objects = np.zeros((B, 3, 6), f32)
    for n in range(B):
        for j, (cls, cx, cy, z) in enumerate(frames[n]["objects"]):
            objects[n, j] = (cls, 0, f32(cx), f32(cy), f32(np.log(z)), 1.0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    feed = {"data": data.to(dev), "data_p": data_p.to(dev), "gt_label_2d": t(label.astype(np.int32)), "keep_prob": 1.0,
            "poses": t(synth.make_gt_poses(scenes, K)), "extents": t(config.LOV_EXTENTS),
            "meta_data": t(np.stack([config.make_meta_data(K)] * B).reshape(B, 1, 1, 48)),
            "points": t(synth.make_model_points(C, 64)), "symmetry": t(config.LOV_SYMMETRY), "vertex_objects": t(objects)}
    planted = {k: t(v) for k, v in planted_np.items()}

    class Cfg(train.TrainConfig):
        LEARNING_RATE = 1e-6

    solvers = {}
    for name in modes:
        torch.manual_seed(0)
        net = vgg16_convs("RGBD", C, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=True, is_train=True,
                          device=dev, seed=3, init="he", lowres_train_heads=True, fused_vertex_loss=MODES[name])
        synth.init_calibrated(net)
        run = net.run
        net.run = lambda f, run=run: run(f, planted=planted)      # the planted scene of bench.py's workload
        solvers[name] = train.SolverWrapper(net, Cfg)

    def once(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = solvers[name].train_step(feed)      # ends in float(loss): a device synchronise
        torch.cuda.synchronize()
        assert ("loss_vertex_sl1" in solvers[name].net.layers) == MODES[name]
        return (time.perf_counter() - t0) * 1e3, losses

    return once


def part_memory(a, mode):
    import torch
    once = _step_setup(a, (mode,))
    for _ in range(2):
        once(mode)
    torch.cuda.reset_peak_memory_stats()
    once(mode)
    return {"max_memory_allocated_bytes": int(torch.cuda.max_memory_allocated()), "graph": mode,
            "what": "torch.cuda.max_memory_allocated over the third train_step of this graph, alone in its process"}


def part_step(a):
    import torch
    B, H, W, C = a.batch, a.height, a.width, a.classes
    once = _step_setup(a, tuple(MODES))
    first = {}
    for name in MODES:
        for _ in range(max(a.warmup, 2)):
            _, first[name] = once(name)
    samples = {}
    for i in range(a.repeats):
        for name in (("lowres", "fused") if i % 2 == 0 else ("fused", "lowres")):
            samples.setdefault(name + "_ms", []).append(once(name)[0])
    st = _stats(samples)
    return {"what": "SolverWrapper.train_step, trainable RGB-D graph with lowres_train_heads=True, host clock around a step that "
                    "ends in a synchronise, alternating repeats",
            "shape": {"batch": B, "height": H, "width": W, "classes": C, "input": "RGBD"},
            "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "ms": st,
            "lowres_over_fused": st["lowres_ms"]["median"] / st["fused_ms"]["median"],
            "step_is_shorter": bool(st["fused_ms"]["median"] < st["lowres_ms"]["median"]),
            "losses_after_warmup": first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--classes", type=int, default=22)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="op,sl1,step,memory")
    ap.add_argument("--part", default=None, choices=sorted(LIMITS), help="(internal) run one part in this process, print its JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_head.json"))
    a = ap.parse_args()
    if a.part is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_vertex_head: needs the GPU (a CPU run measures nothing)")
        fn = {"op": part_op, "sl1": part_sl1, "step": part_step, "mem_lowres": lambda a_: part_memory(a_, "lowres"),
              "mem_fused": lambda a_: part_memory(a_, "fused")}[a.part]
        print("RESULT " + json.dumps(fn(a), sort_keys=True))
        return
    if a.repeats < 20:
        print("bench_vertex_head: fewer than 20 repeats: a rehearsal, not a measurement", file=sys.stderr)
    result = {}
    parts = [q for p in a.parts.split(",") for q in (("mem_lowres", "mem_fused") if p == "memory" else (p,))]
    for part in parts:
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part] + [
            "--%s=%s" % (k, getattr(a, k)) for k in ("batch", "height", "width", "classes", "repeats", "warmup")]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=LIMITS[part], cwd=ROOT)
        except subprocess.TimeoutExpired:
            sys.exit("bench_vertex_head: part %s ran into its %d s limit; nothing further is started" % (part, LIMITS[part]))
        if p.returncode != 0:
            sys.exit("bench_vertex_head: part %s ended with status %d; nothing further is started" % (part, p.returncode))
        line = [l for l in p.stdout.decode().splitlines() if l.startswith("RESULT ")][-1]
        result[part] = json.loads(line[len("RESULT "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
