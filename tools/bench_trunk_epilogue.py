#!/usr/bin/env python
"""The trunk's training epilogues (csrc/trunk_epilogue.hip) against the framework composition, at B = 16, 480 x 640, on one GPU.

  layers  per distinct layer shape of a VGG16 tower, forward + backward of the epilogue ALONE on a resident raw convolution
          output, device events:
            pool    conv -> pool pairs (conv1_2, conv2_2, conv3_3): ops.bias_relu_pool2_train
                    against max_pool2d(relu(y + bias), 2)
            dual    conv4_3: ops.bias_relu_pool2_train(want_act=True) against the same composition with both outputs read
            plain   every other layer: ops.bias_relu_train_ against relu(y + bias)
          with the GB/s of the fused route's algorithmic bytes (computed from the shape below) and, once per shape, the
          assertion that dy of the two routes is equal bit for bit at this size
  step    one SolverWrapper.train_step of the trainable RGB-D graph on top of lowres_train_heads + fused_vertex_loss,
          fused_train_epilogue off and on in the same process: wall time per step
  memory  torch.cuda.max_memory_allocated of one such step, each graph alone in a process of its own

Each part runs in a child process of its own under a time limit; inside it the two sides alternate (who goes first changes
every repeat) and medians and min / max of `--repeats` samples are reported. bench.py does not call this; the result goes to
profiles/trunk_epilogue.json.

    python tools/bench_trunk_epilogue.py [--repeats 20] [--parts layers,step,memory] [--out profiles/trunk_epilogue.json]
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
LIMITS = {"layers": 420, "step": 420, "mem_off": 180, "mem_on": 180}     # seconds per child process
MODES = {"off": False, "on": True}
ACHIEVABLE_GBPS = 6300.0
# (kind, divisor of the frame, channels, the layers of one tower with this shape)
LAYERS = (("pool", 1, 64, ("conv1_2",)), ("pool", 2, 128, ("conv2_2",)), ("pool", 4, 256, ("conv3_3",)),
          ("dual", 8, 512, ("conv4_3",)),
          ("plain", 1, 64, ("conv1_1",)), ("plain", 2, 128, ("conv2_1",)), ("plain", 4, 256, ("conv3_1", "conv3_2")),
          ("plain", 8, 512, ("conv4_1", "conv4_2")), ("plain", 16, 512, ("conv5_1", "conv5_2", "conv5_3")))


def _stats(samples):
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} for k, v in samples.items()}


def fused_bytes(kind, n):
    """Algorithmic bytes of the fused route, forward + backward, for a layer output of n floats (sel: one byte per pooled
    element, n / 4 of them)."""
    pooled, sel = n, n // 4                                   # bytes: n / 4 floats, n / 4 bytes
    if kind == "pool":       # fwd: read y, write pooled + sel; bwd: read dpooled + sel, write dy
        return 4 * n + pooled + sel + pooled + sel + 4 * n
    if kind == "dual":       # fwd: + write act; bwd: + read dact and act
        return 4 * n + 4 * n + pooled + sel + pooled + sel + 8 * n + 4 * n
    return 8 * n + 12 * n    # fwd in place: read + write; bwd: read da and a, write dy


def part_layers(a):
    import torch
    import torch.nn.functional as F
    from posecnn_amd import ops
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    nchw, nhwc = (lambda t: t.permute(0, 3, 1, 2)), (lambda t: t.permute(0, 2, 3, 1).contiguous())
    anchor = torch.zeros((), device=dev, requires_grad=True)

    class Stem(torch.autograd.Function):
        """A fresh copy of the raw convolution output that requires grad without being a leaf; its backward keeps dy."""
        got = None

        @staticmethod
        def forward(ctx, anchor_, raw):
            return raw.clone()

        @staticmethod
        def backward(ctx, g):
            Stem.got = g
            return torch.zeros((), device=g.device), None

    out = {}
    for kind, div, C, names in LAYERS:
        h, w = H // div, W // div
        g = torch.Generator(device=dev).manual_seed(div * 1000 + C)
        raw = torch.randn((B, h, w, C), generator=g, device=dev)
        bias = (torch.randn(C, generator=g, device=dev) * 0.5).requires_grad_(True)
        dp = torch.randn((B, h // 2, w // 2, C), generator=g, device=dev) if kind != "plain" else None
        da = torch.randn((B, h, w, C), generator=g, device=dev) if kind != "pool" else None

        def fused(y):
            if kind == "pool":
                return [ops.bias_relu_pool2_train(y, bias)], [dp]
            if kind == "dual":
                return list(ops.bias_relu_pool2_train(y, bias, want_act=True)), [da, dp]
            return [ops.bias_relu_train_(y, bias)], [da]

        def composition(y):      # Network._bias_act under grad, Network.max_pool
            act = F.relu(y + bias)
            if kind == "plain":
                return [act], [da]
            pooled = nhwc(F.max_pool2d(nchw(act), (2, 2), (2, 2)))
            return ([pooled], [dp]) if kind == "pool" else ([act, pooled], [da, dp])

        def once(route):
            bias.grad = None
            with torch.enable_grad():
                y = Stem.apply(anchor, raw)
                torch.cuda.synchronize()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                outs, grads = route(y)
                ev[1].record()
                torch.autograd.backward(outs, grads)
            ev[2].record()
            torch.cuda.synchronize()
            dy, Stem.got = Stem.got, None
            return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), dy, bias.grad

        _, _, dy_f, db_f = once(fused)
        _, _, dy_c, db_c = once(composition)
        if not torch.equal(dy_f, dy_c):
            sys.exit("bench_trunk_epilogue: dy of the two routes differs at %s %s" % (kind, (B, h, w, C)))
        db_rel = float((db_f.double() - db_c.double()).abs().max() / db_c.double().abs().max())
        del dy_f, dy_c
        routes = {"fused": fused, "composition": composition}
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
            for name in (("composition", "fused") if i % 2 == 0 else ("fused", "composition")):
                f, b, _, _ = once(routes[name])
                for key, v in ((name + "_forward_ms", f), (name + "_backward_ms", b), (name + "_ms", f + b)):
                    samples.setdefault(key, []).append(v)
        st = _stats(samples)
        n = raw.numel()
        nbytes = fused_bytes(kind, n)
        gbps = nbytes / st["fused_ms"]["median"] / 1e6
        out["%s_%dx%dx%d" % (kind, h, w, C)] = {
            "kind": kind, "shape": [B, h, w, C], "layers_per_tower": list(names), "ms": st, "dy_bits_equal": True,
            "dbias_max_rel_diff": db_rel, "fused_algorithmic_bytes": nbytes, "fused_GBps": gbps,
            "fused_share_of_achievable": gbps / ACHIEVABLE_GBPS, "peak_bytes_above_inputs": peak,
            "composition_over_fused": st["composition_ms"]["median"] / st["fused_ms"]["median"]}
        del raw, dp, da
        torch.cuda.empty_cache()
    towers = {k: sum(2 * len(v["layers_per_tower"]) * v["ms"][k + "_ms"]["median"] for v in out.values())
              for k in ("fused", "composition")}
    return {"what": "forward + backward of the epilogue alone per layer shape, device events, alternating repeats; "
                    "fused_GBps = algorithmic bytes of the fused route / its median time, against %g GB/s achievable" % ACHIEVABLE_GBPS,
            "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "layers": out,
            "both_towers_ms": towers, "both_towers_composition_over_fused": towers["composition"] / towers["fused"]}


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
                          device=dev, seed=3, init="he", lowres_train_heads=True, fused_vertex_loss=True,
                          fused_train_epilogue=MODES[name])
        synth.init_calibrated(net)
        run = net.run
        net.run = lambda f, run=run: run(f, planted=planted)      # the planted scene of bench.py's workload
        assert net.fused_train_epilogue == MODES[name]
        solvers[name] = train.SolverWrapper(net, Cfg)

    def once(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = solvers[name].train_step(feed)      # ends in float(loss): a device synchronise
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, losses

    return once


def part_memory(a, mode):
    import torch
    once = _step_setup(a, (mode,))
    for _ in range(2):
        once(mode)
    torch.cuda.reset_peak_memory_stats()
    once(mode)
    return {"max_memory_allocated_bytes": int(torch.cuda.max_memory_allocated()), "fused_train_epilogue": MODES[mode],
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
        for name in (("off", "on") if i % 2 == 0 else ("on", "off")):
            samples.setdefault(name + "_ms", []).append(once(name)[0])
    st = _stats(samples)
    five = samples["off_ms"][:5]
    return {"what": "SolverWrapper.train_step, trainable RGB-D graph with lowres_train_heads + fused_vertex_loss, "
                    "fused_train_epilogue off / on, host clock around a step that ends in a synchronise, alternating repeats",
            "shape": {"batch": B, "height": H, "width": W, "classes": C, "input": "RGBD"},
            "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "ms": st,
            "off_spread_of_first_five_ms": max(five) - min(five),
            "off_over_on": st["off_ms"]["median"] / st["on_ms"]["median"],
            "on_not_slower_beyond_spread": bool(st["on_ms"]["median"] <= st["off_ms"]["median"] + (max(five) - min(five))),
            "losses_after_warmup": first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--classes", type=int, default=22)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="layers,step,memory")
    ap.add_argument("--part", default=None, choices=sorted(LIMITS), help="(internal) run one part in this process, print its JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trunk_epilogue.json"))
    a = ap.parse_args()
    if a.part is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_trunk_epilogue: needs the GPU (a CPU run measures nothing)")
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False
        fn = {"layers": part_layers, "step": part_step, "mem_off": lambda a_: part_memory(a_, "off"),
              "mem_on": lambda a_: part_memory(a_, "on")}[a.part]
        print("RESULT " + json.dumps(fn(a), sort_keys=True))
        return
    if a.repeats < 20:
        print("bench_trunk_epilogue: fewer than 20 repeats: a rehearsal, not a measurement", file=sys.stderr)
    result = {}
    parts = [q for p in a.parts.split(",") for q in (("mem_off", "mem_on") if p == "memory" else (p,))]
    for part in parts:
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part] + [
            "--%s=%s" % (k, getattr(a, k)) for k in ("batch", "height", "width", "classes", "repeats", "warmup")]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=LIMITS[part], cwd=ROOT)
        except subprocess.TimeoutExpired:
            sys.exit("bench_trunk_epilogue: part %s ran into its %d s limit; nothing further is started" % (part, LIMITS[part]))
        if p.returncode != 0:
            sys.exit("bench_trunk_epilogue: part %s ended with status %d; nothing further is started" % (part, p.returncode))
        line = [l for l in p.stdout.decode().splitlines() if l.startswith("RESULT ")][-1]
        result[part] = json.loads(line[len("RESULT "):])
        print("bench_trunk_epilogue: part %s done" % part, file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
