"""The pose polish (include/posecnn_hip/pose_polish.h) on the GPU: every output bit for bit equal to the numpy restatement
tests/pose_polish_ref.py, for both routes, on the cases of tests/pose_polish_cases.py — what each case exercises is proved
on the CPU by tests/test_pose_polish_cpu.py (test_case_claims, test_colour_case_meets_infinity, test_edge_case_is_clamped,
test_shrink_case)."""
import contextlib
import ctypes

import numpy as np
import pytest

import memguard
import pose2d_cases as C2
import pose2d_ref as R2
import pose3d_cases as C3
import pose3d_ref as R3
import pose_polish_cases as PC
import pose_polish_ref as PR

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
SEED = (0x1234_5678_9ABC_DEF0 << 64) | 0x0FED_CBA9_8765_4321
STREAMS = (11, 5, 1 << 63)
NAMES = ("poses32", "poses64", "energy", "evals", "listed")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def assert_bits(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        name, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def u16(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(gpu).view(torch.uint16)


def stream_tensor(gpu, ids):
    return dev(gpu, np.array(ids, dtype=np.uint64).view(np.int64))


def run_polish(gpu, case, route, frames=None, **kw):
    """ops.pose_polish on the frames `frames` (default: all) of a case dict -> {name: numpy}"""
    from posecnn_amd import ops
    sl = slice(None) if frames is None else list(frames)
    B = case["records"][sl].shape[0]
    out = ops.pose_polish(dev(gpu, case["records"][sl]), dev(gpu, case["counts"][sl]), dev(gpu, case["offsets"][sl]),
                          dev(gpu, case["poses"][sl].reshape(B, -1, 3, 4)), dev(gpu, case["gate"][sl]), route,
                          dev(gpu, case["K"][sl]) if route == 1 else None, height=PC.H, width=PC.W, min_pixels=PC.MIN_PIXELS, **kw)
    return dict(zip(NAMES, (t.cpu().numpy() for t in out)))


def check_frame(what, got, b, want):
    """frame b of the GPU's outputs against one frame's dict of pose_polish_ref.polish"""
    C = len(want["evals"])
    assert_bits(what + " evals", got["evals"][b], want["evals"])
    assert_bits(what + " listed", got["listed"][b], want["listed"])
    assert_bits(what + " energy", got["energy"][b], want["energy"])
    assert_bits(what + " poses64", got["poses64"][b].reshape(C, 12), want["poses64"])
    assert_bits(what + " poses32", got["poses32"][b].reshape(C, 12), want["poses32"])


# ---- the stand-alone polish ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_pixels,evaluations", PC.RUNS, ids=["%d-%d" % r for r in PC.RUNS])
@pytest.mark.parametrize("route", [0, 1], ids=["depth", "colour"])
def test_batch(gpu, route, max_pixels, evaluations):
    """the four-frame batch: thinned and unthinned lists in LDS (37, 1000) and in the workspace (1025, 2000), list lengths 5,
    63, 64, 65, 129, empty classes, gate == min_pixels against min_pixels + 1, 0 / 7 / 8 / 100 evaluations"""
    got = run_polish(gpu, PC.batch(route), route, max_pixels=max_pixels, evaluations=evaluations, inlier_threshold=PC.THRESHOLD[route])
    want = PC.reference(route, max_pixels, evaluations)
    for b in range(4):
        check_frame("frame %d" % b, got, b, want[b])
    if evaluations >= 7:
        assert (got["energy"][..., 1] <= got["energy"][..., 0]).all() and got["evals"].max() == evaluations
    else:
        assert not got["evals"].any() and not got["energy"].any()


@pytest.mark.parametrize("route", [0, 1], ids=["depth", "colour"])
def test_batch_slot(gpu, route):
    """a frame's result does not depend on its batch slot: frame 2 alone, and the batch reversed, against the batch; a
    second run repeats the first"""
    kw = dict(max_pixels=1000, evaluations=100, inlier_threshold=PC.THRESHOLD[route])
    full = run_polish(gpu, PC.batch(route), route, **kw)
    again = run_polish(gpu, PC.batch(route), route, **kw)
    alone = run_polish(gpu, PC.batch(route), route, frames=[2], **kw)
    rev = run_polish(gpu, PC.batch(route), route, frames=[3, 2, 1, 0], **kw)
    for k in NAMES:
        assert_bits("second run " + k, again[k], full[k])
        assert_bits("alone " + k, alone[k][0], full[k][2])
        assert_bits("reversed " + k, rev[k][::-1], full[k])


def test_colour_meets_infinity(gpu):
    for evaluations in PC.NEAR_RUNS:
        got = run_polish(gpu, PC.near(), 1, max_pixels=1000, evaluations=evaluations, inlier_threshold=PC.NEAR_THRESHOLD)
        check_frame("near, %d evaluations" % evaluations, got, 0, PC.near_reference(evaluations))
        assert np.isfinite(got["energy"]).all()


@pytest.mark.parametrize("route", [0, 1], ids=["depth", "colour"])
def test_edge_is_clamped(gpu, route):
    got = run_polish(gpu, PC.edge(route), route, max_pixels=1000, evaluations=100, inlier_threshold=PC.EDGE_THRESHOLD[route])
    check_frame("edge", got, 0, PC.edge_reference(route))


@pytest.mark.parametrize("evaluations", PC.SHRINK_RUNS)
def test_shrink(gpu, evaluations):
    got = run_polish(gpu, PC.shrink(), 1, max_pixels=1000, evaluations=evaluations, inlier_threshold=PC.THRESHOLD[1])
    check_frame("shrink, %d evaluations" % evaluations, got, 0, PC.shrink_reference(evaluations))


def test_argument_errors(gpu):
    from posecnn_amd import ops
    bt = PC.batch(0)
    args = [dev(gpu, bt["records"]), dev(gpu, bt["counts"]), dev(gpu, bt["offsets"]), dev(gpu, bt["poses"].reshape(4, PC.C, 3, 4)),
            dev(gpu, bt["gate"])]
    for kw in (dict(evaluations=6), dict(evaluations=4097), dict(evaluations=-1), dict(max_pixels=0), dict(min_pixels=-1),
               dict(inlier_threshold=float("nan"))):
        with pytest.raises(ValueError):
            ops.pose_polish(*args, 0, height=PC.H, width=PC.W, **kw)
    for route in (2, "rgb"):
        with pytest.raises(ValueError):
            ops.pose_polish(*args, route, height=PC.H, width=PC.W)
    with pytest.raises(ValueError):
        ops.pose_polish(*args, 1, height=PC.H, width=PC.W)                     # the colour route without intrinsics
    with pytest.raises(ValueError):
        ops.pose_polish(*args, 0, height=PC.H, width=PC.W + 1)
    with pytest.raises(ValueError):
        ops.estimate_poses_3d(*scene3(gpu)[0], polish_evaluations=-1)
    with pytest.raises(ValueError):
        ops.estimate_poses_3d(*scene3(gpu)[0], polish_evaluations=5)


# ---- the polished drivers -----------------------------------------------------------------------------------------------------
DRIVER = ("poses32", "poses64", "inliers", "ref_steps", "num_hyps")


def scene3(gpu):
    label, depth, vertex, extents, K, frames = C3.batch(range(1, 4), C3.INTRINSICS)
    return (dev(gpu, label), u16(gpu, depth), dev(gpu, vertex), dev(gpu, extents), dev(gpu, K), C3.FACTOR), frames, extents


def scene2(gpu):
    label, vertex, extents, K, frames = C2.batch(range(1, 4), C2.INTRINSICS)
    return (dev(gpu, label), dev(gpu, vertex), dev(gpu, extents), dev(gpu, K)), frames, extents


@pytest.mark.parametrize("route", [0, 1], ids=["depth", "colour"])
def test_polished_driver(gpu, route):
    """polish_evaluations = 100: the driver equals estimate followed by pose_polish on the prepared records, and the
    restatement's estimate followed by its polish; polish_evaluations = 0: today's driver, today's tuple"""
    from posecnn_amd import ops
    if route == 0:
        args, frames, extents = scene3(gpu)
        kw = dict(seed=SEED, streams=stream_tensor(gpu, STREAMS), hypotheses=64)
        estimate, records = ops.estimate_poses_3d, ops.pose3d_prepare(*args)
        thr = 0.01
    else:
        args, frames, extents = scene2(gpu)
        kw = dict(seed=SEED, streams=stream_tensor(gpu, STREAMS), hypotheses=64, **C2.PARAMS)
        estimate, records = ops.estimate_poses_2d, ops.pose2d_prepare(*args[:3])
        thr = C2.INLIER_THRESHOLD
    plain = estimate(*args, **kw)
    zero = estimate(*args, polish_evaluations=0, **kw)
    assert len(plain) == len(zero) == 5
    polished = estimate(*args, polish_evaluations=100, min_pixels=10, **kw)
    assert len(polished) == 8
    for name, a, b in zip(DRIVER, plain, zero):
        assert_bits("polish_evaluations = 0: " + name, b.cpu().numpy(), a.cpu().numpy())
    for name, a, b in zip(DRIVER[2:], plain[2:], polished[2:5]):
        assert_bits("the loop's own outputs: " + name, b.cpu().numpy(), a.cpu().numpy())
    chained = ops.pose_polish(*records, plain[1], plain[2], route, args[4] if route == 0 else args[3], height=C3.H, width=C3.W,
                              min_pixels=10, evaluations=100, inlier_threshold=thr)
    got = dict(zip(NAMES, (t.cpu().numpy() for t in (polished[0], polished[1]) + tuple(polished[5:]))))
    for name, t in zip(NAMES, chained):
        assert_bits("driver against estimate + pose_polish: " + name, got[name], t.cpu().numpy())
    assert (got["evals"][:, list(C3.POSED)] == 100).all() and not got["evals"][:, [0, 4, 5, 6]].any()
    # (whether the polish moves a pose the loop has already refitted is not assumed: on these exact scenes it may not)
    for b, f in enumerate(frames):
        if route == 0:
            est = R3.estimate(f["label"], f["depth"], f["vertex_pred"], extents, f["K"], C3.FACTOR, STREAMS[b], SEED, hypotheses=64)
            rec, cnt, off = R3.prepare(f["label"], f["depth"], f["vertex_pred"], extents, f["K"], C3.FACTOR)
        else:
            est = R2.estimate(f["label"], f["vertex_pred"], extents, f["K"], STREAMS[b], SEED, hypotheses=64, **C2.PARAMS)
            rec, cnt, off = R2.prepare(f["label"], f["vertex_pred"], extents)
        want = PR.polish(route, rec, cnt, off, est["poses64"], est["inliers"], K=f["K"], max_pixels=1000, min_pixels=10, evaluations=100,
                         inlier_threshold=thr)
        check_frame("restatement, frame %d" % b, got, b, want)


def test_polished_entry_without_evaluations(gpu):
    """the C entries with evaluations == 0 are the existing drivers: same pose bits, polish outputs NULL and unread"""
    import torch
    from posecnn_amd import ops
    args, _, _ = scene3(gpu)
    streams = stream_tensor(gpu, STREAMS)
    plain = ops.estimate_poses_3d(*args, seed=SEED, streams=streams, hypotheses=64)
    B, C = 3, C3.C
    n = ctypes.c_size_t()
    ops.call("pcnn_pose3d_estimate_polished_workspace_bytes", B, C3.H, C3.W, C, 64, 1000, ctypes.byref(n))
    ws = torch.empty(n.value, dtype=torch.uint8, device=gpu)
    outs = (torch.empty((B, C, 3, 4), dtype=torch.float64, device=gpu), torch.empty((B, C, 3, 4), dtype=torch.float32, device=gpu),
            torch.empty((B, C), dtype=torch.int32, device=gpu), torch.empty((B, C), dtype=torch.int32, device=gpu),
            torch.empty((B, C), dtype=torch.int32, device=gpu))
    p = ops._ptr
    ops.call("pcnn_pose3d_estimate_polished_fwd", *map(p, args[:5]), p(streams), C3.FACTOR, SEED & (1 << 64) - 1, SEED >> 64, B, C3.H, C3.W,
             C, 64, 1000, 1000, 8, 400, 0.01, 0.01, 1024, 10, 0, *map(p, outs), None, None, None, p(ws), n.value, ops._stream(ws))
    for name, a, b in zip(("poses64", "poses32", "inliers", "ref_steps", "num_hyps"), outs, (plain[1], plain[0]) + tuple(plain[2:])):
        assert_bits(name, a.cpu().numpy(), b.cpu().numpy())


def test_synthesizer_and_single_frame(gpu):
    """`Synthesizer.estimate_poses_3d / _2d` and `fcn.poses_from_vertmap_3d` pass polish_evaluations on: their poses are the
    polished driver's"""
    from posecnn_amd import fcn, ops
    from posecnn_amd.icp import Synthesizer
    f = C3.make_frame(1)
    K = f["K"]
    poses = np.full((3, 4, C3.C), -7.0, dtype=F)
    Synthesizer(meshes=[], device=gpu).estimate_poses_3d(f["label"], f["depth"], f["vertex_pred"], f["extents"], poses, C3.C, K[0], K[1],
                                                         K[2], K[3], C3.FACTOR, seed=SEED, polish_evaluations=100)
    want = ops.estimate_poses_3d(dev(gpu, f["label"][None]), u16(gpu, f["depth"][None]), dev(gpu, f["vertex_pred"][None]),
                                 dev(gpu, f["extents"]), dev(gpu, np.array([K], dtype=F)), C3.FACTOR, seed=SEED, polish_evaluations=100)
    w32, evals = want[0].cpu().numpy()[0], want[6].cpu().numpy()[0]
    for c in range(C3.C):
        if c in C3.POSED:
            assert evals[c] == 100
            assert_bits("class %d" % c, poses[:, :, c], w32[c])
        else:
            assert (poses[:, :, c] == -7.0).all()
    meta = {"intrinsic_matrix": np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dtype=D), "factor_depth": C3.FACTOR}
    _, rows = fcn.poses_from_vertmap_3d(f["label"], f["depth"], f["vertex_pred"], meta, f["extents"], C3.C, seed=SEED, device=gpu,
                                        polish_evaluations=100)
    _, rows0 = fcn.poses_from_vertmap_3d(f["label"], f["depth"], f["vertex_pred"], meta, f["extents"], C3.C, seed=SEED, device=gpu)
    assert rows.shape == rows0.shape == (3, 7)
    assert_bits("translation rows", rows[:, 4:], np.stack([w32[c][:, 3] for c in C3.POSED]))
    g = C2.make_frame(1)
    poses2 = np.full((3, 4, C2.C), -7.0, dtype=F)
    Synthesizer(meshes=[], device=gpu).estimate_poses_2d(g["label"], g["vertex_pred"], g["extents"], poses2, C2.C, K[0], K[1], K[2], K[3],
                                                         seed=SEED, polish_evaluations=100)
    want2 = ops.estimate_poses_2d(dev(gpu, g["label"][None]), dev(gpu, g["vertex_pred"][None]), dev(gpu, g["extents"]),
                                  dev(gpu, np.array([K], dtype=F)), seed=SEED, polish_evaluations=100)[0].cpu().numpy()[0]
    for c in C2.POSED:
        assert_bits("colour class %d" % c, poses2[:, :, c], want2[c])


# ---- memory contract ------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def guarded(pattern):
    from posecnn_amd import _lib, ops
    g = memguard.GuardedTorch(pattern, devices=("cuda",))
    rec = memguard.Recorder(_lib.lib())
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "torch", g)
        mp.setattr(ops, "lib", lambda: rec)
        mp.setattr(ops, "_default_ws", {})
        yield g, rec


@pytest.mark.parametrize("route", [0, 1], ids=["depth", "colour"])
def test_memory_contract(gpu, route):
    """Guard bands around every output, the workspaces and the inputs of the stand-alone polish (list in LDS and in the
    workspace) and of the polished driver, both poison patterns: guards and inputs intact, results independent of the
    poison, and equal to the restatement's."""
    import torch
    from posecnn_amd import ops
    bt = PC.batch(route)
    runs, calls = {}, set()
    for pat in memguard.PATTERNS:
        with guarded(pat) as (g, rec):
            ins = [g.embed(bt["records"], "cuda"), g.embed(bt["counts"], "cuda"), g.embed(bt["offsets"], "cuda"),
                   g.embed(bt["poses"].reshape(4, PC.C, 3, 4), "cuda"), g.embed(bt["gate"], "cuda")]
            K = g.embed(bt["K"], "cuda")
            kw = dict(height=PC.H, width=PC.W, min_pixels=PC.MIN_PIXELS, evaluations=100, inlier_threshold=PC.THRESHOLD[route])
            lds = ops.pose_polish(*ins, route, K if route == 1 else None, max_pixels=1000, **kw)
            wsp = ops.pose_polish(*ins, route, K if route == 1 else None, max_pixels=2000, **kw)
            if route == 0:
                label, depth, vertex, extents, Ks, _ = C3.batch(range(1, 4), C3.INTRINSICS)
                fr = [g.embed(label, "cuda"), g.embed(depth, "cuda"), g.embed(vertex, "cuda"), g.embed(extents, "cuda"), g.embed(Ks, "cuda")]
                streams = g.embed(np.array(STREAMS, dtype=np.uint64).view(np.int64), "cuda")
                est = ops.estimate_poses_3d(*fr, C3.FACTOR, seed=SEED, streams=streams, hypotheses=32, polish_evaluations=20)
            else:
                label, vertex, extents, Ks, _ = C2.batch(range(1, 4), C2.INTRINSICS)
                fr = [g.embed(label, "cuda"), g.embed(vertex, "cuda"), g.embed(extents, "cuda"), g.embed(Ks, "cuda")]
                streams = g.embed(np.array(STREAMS, dtype=np.uint64).view(np.int64), "cuda")
                est = ops.estimate_poses_2d(*fr, seed=SEED, streams=streams, hypotheses=32, polish_evaluations=20, **C2.PARAMS)
            torch.cuda.synchronize()
            g.check()
            assert sum(a.kind == "empty" for a in g.arenas) == (5 + 1) + (5 + 1) + (8 + 1)       # outputs + a workspace, three calls
            names = ["lds_" + n for n in NAMES] + ["ws_" + n for n in NAMES] + ["est_%d" % i for i in range(8)]
            runs[pat] = {k: memguard.to_numpy(t) for k, t in zip(names, tuple(lds) + tuple(wsp) + tuple(est))}
            calls |= set(rec.calls)
    memguard.compare_patterns(runs)
    route_name = ("pose3d", "pose2d")[route]
    assert {"pcnn_pose_polish_workspace_bytes", "pcnn_pose_polish_fwd", "pcnn_%s_estimate_polished_workspace_bytes" % route_name,
            "pcnn_%s_estimate_polished_fwd" % route_name} <= calls
    for b in range(4):
        check_frame("LDS list, frame %d" % b, {n: runs["P2"]["lds_" + n] for n in NAMES}, b, PC.reference(route, 1000, 100)[b])
        check_frame("workspace list, frame %d" % b, {n: runs["P1"]["ws_" + n] for n in NAMES}, b, PC.reference(route, 2000, 100)[b])
