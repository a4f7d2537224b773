"""The 3-D vertex route's pose kernels (include/posecnn_hip_pose3d.h) on the GPU: every output bit for bit equal to the
numpy restatement tests/pose3d_ref.py, on the planted 64 x 96 scenes of tests/pose3d_cases.py."""
import contextlib
import functools

import numpy as np
import pytest

import memguard
import pose3d_cases as CS
import pose3d_ref as R

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
SEED = (0x1234_5678_9ABC_DEF0 << 64) | 0x0FED_CBA9_8765_4321
STREAMS = (11, 5, 1 << 63)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def assert_bits(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        name, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def u16(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(gpu).view(torch.uint16)


def dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def stream_tensor(gpu, ids):
    return dev(gpu, np.array(ids, dtype=np.uint64).view(np.int64))


@functools.lru_cache(maxsize=None)
def scene(n):
    """B = n frames with their own intrinsics; the restatement's records are computed once and shared"""
    label, depth, vertex, extents, K, frames = CS.batch(range(1, n + 1), CS.INTRINSICS[:n])
    prep = [R.prepare(f["label"], f["depth"], f["vertex_pred"], extents, f["K"], CS.FACTOR) for f in frames]
    return label, depth, vertex, extents, K, frames, prep


def gpu_prepare(gpu, n, vertex_tensor=None):
    from posecnn_amd import ops
    label, depth, vertex, extents, K, _, _ = scene(n)
    v = dev(gpu, vertex) if vertex_tensor is None else vertex_tensor
    return ops.pose3d_prepare(dev(gpu, label), u16(gpu, depth), v, dev(gpu, extents), dev(gpu, K), CS.FACTOR)


# ---- prepare --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True])
def test_prepare(gpu, misaligned):
    """records, counts and order of three frames (labels >= C and < 0 are in every frame); `misaligned`: vertex_pred is a
    view 4 bytes into its allocation"""
    import torch
    label, depth, vertex, extents, K, frames, prep = scene(3)
    v = None
    if misaligned:
        flat = torch.empty(vertex.size + 1, dtype=torch.float32, device=gpu)
        v = flat[1:].view(vertex.shape)
        v.copy_(dev(gpu, vertex))
        assert v.data_ptr() % 16 == 4
    records, counts, offsets = (t.cpu().numpy() for t in gpu_prepare(gpu, 3, v))
    for b, (rec, cnt, off) in enumerate(prep):
        assert [int(cnt[c]) for c in range(1, CS.C)] == [CS.SIZES[c] for c in range(1, CS.C)]
        assert_bits("counts[%d]" % b, counts[b], cnt)
        assert_bits("offsets[%d]" % b, offsets[b], off)
        assert_bits("records[%d]" % b, records[b, :len(rec)], rec)


# ---- sample ---------------------------------------------------------------------------------------------------------------
def test_sample(gpu):
    from posecnn_amd import ops
    label, depth, vertex, extents, K, frames, prep = scene(3)
    records, counts, offsets = gpu_prepare(gpu, 3)
    got = ops.pose3d_sample(records, counts, offsets, dev(gpu, extents), dev(gpu, K), CS.H, CS.W, seed=SEED,
                            streams=stream_tensor(gpu, STREAMS), hypotheses=256)
    pose, cls, att, rec3 = (t.cpu().numpy() for t in got)
    for b, (rec, cnt, off) in enumerate(prep):
        want = R.sample(rec, cnt, off, extents, frames[b]["K"], CS.H, CS.W, STREAMS[b], SEED, hypotheses=256)
        assert set(np.unique(want[1])) == {1, 2, 3}                   # every posed class drew hypotheses, the all-hole class none
        assert want[2].max() > 0                                      # some first attempts were refused
        assert_bits("hyp_class[%d]" % b, cls[b], want[1])
        assert_bits("hyp_attempt[%d]" % b, att[b], want[2])
        assert_bits("hyp_rec[%d]" % b, rec3[b], want[3])
        assert_bits("hyp_pose[%d]" % b, pose[b].reshape(-1, 12), want[0])


def test_sample_dead(gpu):
    """only the all-hole class is live: with max_attempts = 16 every hypothesis is dead"""
    from posecnn_amd import ops
    f = CS.make_frame(1)
    label = np.where(f["label"] == 5, 5, 0).astype(np.int32)
    args = (dev(gpu, label[None]), u16(gpu, f["depth"][None]), dev(gpu, f["vertex_pred"][None]), dev(gpu, f["extents"]),
            dev(gpu, np.array([f["K"]], dtype=F)))
    records, counts, offsets = ops.pose3d_prepare(*args, CS.FACTOR)
    assert counts.cpu().numpy()[0].tolist() == [0, 0, 0, 0, 0, 448, 0]
    pose, cls, att, rec3 = (t.cpu().numpy() for t in ops.pose3d_sample(records, counts, offsets, args[3], args[4], CS.H, CS.W,
                                                                        seed=SEED, hypotheses=70, max_attempts=16))
    assert not pose.any() and not cls.any() and (att == -1).all() and (rec3 == -1).all()
    out = ops.estimate_poses_3d(*args, CS.FACTOR, seed=SEED, hypotheses=70, max_attempts=16)
    assert all(not t.cpu().numpy().any() for t in out)


# ---- one round ------------------------------------------------------------------------------------------------------------
def run_round(gpu, records, counts, offsets, pose, cls, rnd, **kw):
    from posecnn_amd import ops
    got = ops.pose3d_round(records, counts, offsets, dev(gpu, pose), dev(gpu, cls), CS.H, CS.W, rnd, **kw)
    return [t.cpu().numpy() for t in got]


def check_rounds(gpu, pose, cls, rounds, **kw):
    """chained rounds on frame 0 of the 3-frame scene (frames 1, 2 carry empty slots): GPU against the restatement, each fed
    the GPU's previous output"""
    label, depth, vertex, extents, K, frames, prep = scene(3)
    records, counts, offsets = gpu_prepare(gpu, 3)
    rec, cnt, off = prep[0]
    n = len(cls)
    poses = np.zeros((3, n, 3, 4), D)
    classes = np.zeros((3, n), np.int32)
    poses[0], classes[0] = pose.reshape(n, 3, 4), cls
    classes[1, :3] = (0, -4, 70)                      # not hypotheses: come back as class 0, pose unchanged
    seen = []
    for rnd in rounds:
        p, c, i = run_round(gpu, records, counts, offsets, poses, classes, rnd, **kw)
        wp, wc, wi = R.round_fwd(rec, cnt, off, poses[0].reshape(n, 12), classes[0], rnd, **kw)
        assert_bits("class_out round %d" % rnd, c[0], wc)
        assert_bits("inliers_out round %d" % rnd, i[0], wi)
        assert_bits("pose_out round %d" % rnd, p[0].reshape(n, 12), wp)
        assert not c[1:].any() and not i[1:].any()
        assert_bits("empty slots", p[1:], poses[1:])
        seen.append((c[0].copy(), i[0].copy(), p[0].copy(), poses[0].copy()))
        poses[0], classes[0] = p[0], c[0]
    return seen


def sampled(n_hyp):
    label, depth, vertex, extents, K, frames, prep = scene(3)
    rec, cnt, off = prep[0]
    pose, cls, _, _ = R.sample(rec, cnt, off, extents, frames[0]["K"], CS.H, CS.W, STREAMS[0], SEED, hypotheses=n_hyp)
    return pose, cls


def test_round_ties_and_thinning(gpu):
    """planted duplicates (equal counts: the lower index wins), default batch: class 1 reaches m = n = 2500 in round 3 with
    more than max_pixels = 1000 inliers (thinned refit)"""
    pose, cls = sampled(64)
    first = np.nonzero(cls == 1)[0]
    pose[first[1]], pose[first[2]] = pose[first[0]], pose[first[0]]
    seen = check_rounds(gpu, pose, cls, (1, 2, 3, 4))
    c, i, p, before = seen[2]
    best = np.nonzero(c == 1)[0]
    assert len(best) and i[best].max() > 1000 and (p[best] != before[best]).any()
    c0, i0 = seen[0][0], seen[0][1]
    assert i0[first[0]] == i0[first[1]] == i0[first[2]]
    assert not (c0[first[0]] == 0 and c0[first[1]] != 0) and not (c0[first[1]] == 0 and c0[first[2]] != 0)


def test_round_small_batch(gpu):
    """pixel_batch = 128: m crosses n = 401 (class 3) in round 4 and n = 900 (class 2) in round 8; max_pixels = 100 thins"""
    pose, cls = sampled(32)
    check_rounds(gpu, pose, cls, range(1, 10), pixel_batch=128, max_pixels=100)


def test_round_three_inliers(gpu):
    """a lone hypothesis with 3 inliers is not refitted, one with 4 is; hand-made records"""
    from posecnn_amd import ops
    rng = np.random.RandomState(5)
    n3, n4 = 40, 50
    obj = rng.uniform(-0.1, 0.1, size=(n3 + n4, 3)).astype(F)
    eye = (obj.astype(D) + np.array([0.0, 0.0, 1.0])).astype(F)          # identity rotation, t = (0, 0, 1) up to f32
    bad = np.ones(n3 + n4, bool)
    bad[[3, 17, 30]] = False
    bad[[n3 + 1, n3 + 9, n3 + 20, n3 + 41]] = False
    eye[bad] += F(0.5)
    HW = CS.H * CS.W
    records = np.zeros((1, HW, 6), F)
    records[0, :n3 + n4] = np.concatenate([eye, obj], axis=1)
    counts, offsets = np.array([[0, n3, n4]], np.int32), np.array([[0, 0, n3]], np.int32)
    pose = np.zeros((1, 2, 12), D)
    pose[0, :, [0, 5, 10]] = 1.0
    pose[0, :, 11] = 1.0 + 1e-4
    cls = np.array([[1, 2]], np.int32)
    p, c, i = (t.cpu().numpy() for t in ops.pose3d_round(dev(gpu, records), dev(gpu, counts), dev(gpu, offsets),
                                                           dev(gpu, pose.reshape(1, 2, 3, 4)), dev(gpu, cls), CS.H, CS.W, 1))
    wp, wc, wi = R.round_fwd(records[0], counts[0], offsets[0], pose[0], cls[0], 1)
    assert wi.tolist() == [3, 4] and wc.tolist() == [1, 2]
    assert_bits("class_out", c[0], wc)
    assert_bits("inliers_out", i[0], wi)
    assert_bits("pose_out", p[0].reshape(2, 12), wp)
    assert_bits("three inliers: untouched", p[0, 0].reshape(12), pose[0, 0])
    assert (p[0, 1].reshape(12) != pose[0, 1]).any()


def threshold_inputs(gpu):
    f = CS.threshold_frame()
    return f, (dev(gpu, f["label"][None]), u16(gpu, f["depth"][None]), dev(gpu, f["vertex_pred"][None]), dev(gpu, f["extents"]),
               dev(gpu, np.array([f["K"]], dtype=F)))


def test_round_at_threshold(gpu):
    """a record whose residual EQUALS the threshold is no inlier (`<`, countInliers3D :1276): the lone hypothesis of
    tests/pose3d_cases.threshold_frame has 3 inliers and is not refitted; with `<=` it would have 4 and move"""
    from posecnn_amd import ops
    f, args = threshold_inputs(gpu)
    rec, cnt, off = R.prepare(f["label"], f["depth"], f["vertex_pred"], f["extents"], f["K"], f["factor"])
    assert R.residual(CS.THRESHOLD_POSE[None], rec)[0].tolist() == [0.25, 0.0, 0.0, 0.0] and D(F(0.25)) == 0.25
    records, counts, offsets = ops.pose3d_prepare(*args, f["factor"])
    assert_bits("records", records.cpu().numpy()[0, :4], rec)
    pose, cls = CS.THRESHOLD_POSE.reshape(1, 1, 3, 4), np.array([[1]], np.int32)
    p, c, i = (t.cpu().numpy() for t in ops.pose3d_round(records, counts, offsets, dev(gpu, pose), dev(gpu, cls), 8, 8, 1,
                                                           inlier_threshold=0.25))
    wp, wc, wi = R.round_fwd(rec, cnt, off, pose.reshape(1, 12), cls[0], 1, inlier_threshold=0.25)
    assert wi.tolist() == [3] and wc.tolist() == [1]
    assert_bits("inliers_out", i[0], wi)
    assert_bits("class_out", c[0], wc)
    assert_bits("pose_out", p[0].reshape(1, 12), wp)
    assert_bits("not refitted", p[0].reshape(12), CS.THRESHOLD_POSE)


def test_driver_at_threshold(gpu):
    """the same frame through the sampler and the whole loop: every accepted three-point fit is exactly R = I, t = (0, 0, 2),
    the record at the threshold is counted in every round by `<`, so the survivor has 3 inliers throughout: it is never
    refitted, its pose comes out unchanged and ref_steps still reaches ref_it"""
    from posecnn_amd import ops
    f, args = threshold_inputs(gpu)
    rec, cnt, off = R.prepare(f["label"], f["depth"], f["vertex_pred"], f["extents"], f["K"], f["factor"])
    streams = stream_tensor(gpu, [3])
    records, counts, offsets = ops.pose3d_prepare(*args, f["factor"])
    kw = {k: v for k, v in CS.THRESHOLD.items() if k != "hypotheses"}
    got = ops.pose3d_sample(records, counts, offsets, args[3], args[4], 8, 8, seed=SEED, streams=streams, hypotheses=13, **kw)
    pose, cls, att, rec3 = (t.cpu().numpy()[0] for t in got)
    want = R.sample(rec, cnt, off, f["extents"], f["K"], 8, 8, 3, SEED, **CS.THRESHOLD)
    assert (want[1] == 1).all() and want[2].max() > 0 and (want[0] == CS.THRESHOLD_POSE).all()
    for name, g, w in zip(("hyp_pose", "hyp_class", "hyp_attempt", "hyp_rec"), (pose.reshape(-1, 12), cls, att, rec3), want):
        assert_bits(name, g, w)
    out = ops.estimate_poses_3d(*args, f["factor"], seed=SEED, streams=streams, **CS.THRESHOLD)
    out = dict(zip(("poses32", "poses64", "inliers", "ref_steps", "num_hyps"), (t.cpu().numpy()[0] for t in out)))
    want = R.estimate(f["label"], f["depth"], f["vertex_pred"], f["extents"], f["K"], f["factor"], 3, SEED, **CS.THRESHOLD)
    assert want["inliers"].tolist() == [0, 3] and want["ref_steps"].tolist() == [0, 8] and want["num_hyps"].tolist() == [0, 13]
    for k in ("inliers", "ref_steps", "num_hyps"):
        assert_bits(k, out[k], want[k])
    assert_bits("poses64", out["poses64"].reshape(-1, 12), want["poses64"])
    assert_bits("poses32", out["poses32"].reshape(-1, 12), want["poses32"])
    assert_bits("unchanged pose", out["poses64"][1].reshape(12), CS.THRESHOLD_POSE)


# ---- the driver -----------------------------------------------------------------------------------------------------------
def estimate(gpu, n, order=None, **kw):
    from posecnn_amd import ops
    label, depth, vertex, extents, K, _, _ = scene(3)
    order = list(range(n)) if order is None else order
    out = ops.estimate_poses_3d(dev(gpu, label[order]), u16(gpu, depth[order]), dev(gpu, vertex[order]), dev(gpu, extents),
                                dev(gpu, K[order]), CS.FACTOR, seed=SEED, streams=stream_tensor(gpu, [STREAMS[b] for b in order]), **kw)
    return dict(zip(("poses32", "poses64", "inliers", "ref_steps", "num_hyps"), (t.cpu().numpy() for t in out)))


@pytest.mark.parametrize("hypotheses", [1, 13, 256])
def test_driver(gpu, hypotheses):
    label, depth, vertex, extents, K, frames, prep = scene(3)
    got = estimate(gpu, 3, hypotheses=hypotheses)
    again = estimate(gpu, 3, hypotheses=hypotheses)
    single = estimate(gpu, 1, order=[2], hypotheses=hypotheses)
    for k in got:
        assert_bits("second run " + k, again[k], got[k])
        assert_bits("slot 0 of B = 1 against slot 2 of B = 3, " + k, single[k][0], got[k][2])
    for b, f in enumerate(frames):
        want = R.estimate(f["label"], f["depth"], f["vertex_pred"], extents, f["K"], CS.FACTOR, STREAMS[b], SEED, hypotheses=hypotheses)
        assert want["num_hyps"].sum() == hypotheses and not want["num_hyps"][[0, 4, 5, 6]].any()
        for k in ("num_hyps", "ref_steps", "inliers"):
            assert_bits("%s[%d]" % (k, b), got[k][b], want[k])
        assert_bits("poses64[%d]" % b, got["poses64"][b].reshape(-1, 12), want["poses64"])
        assert_bits("poses32[%d]" % b, got["poses32"][b].reshape(-1, 12), want["poses32"])
        for c in range(CS.C):
            if want["num_hyps"][c] == 0:                           # not live, all holes, absent, or no hypothesis drawn
                assert not got["poses64"][b, c].any() and got["inliers"][b, c] == 0 and got["ref_steps"][b, c] == 0
        if hypotheses == 256:
            for c in CS.POSED:
                assert CS.corner_displacement(got["poses64"][b, c], *f["poses"][c], extents[c]) < 1e-3


def test_driver_no_live_class(gpu):
    """a frame whose only class has 400 pixels (not live) between two ordinary frames"""
    from posecnn_amd import ops
    label, depth, vertex, extents, K, frames, prep = scene(3)
    label = label.copy()
    label[1] = np.where(label[1] == 4, 4, 0)
    out = ops.estimate_poses_3d(dev(gpu, label), u16(gpu, depth), dev(gpu, vertex), dev(gpu, extents), dev(gpu, K), CS.FACTOR,
                                seed=SEED, streams=stream_tensor(gpu, STREAMS), hypotheses=13)
    out = [t.cpu().numpy() for t in out]
    assert all(not t[1].any() for t in out)
    ref = estimate(gpu, 3, hypotheses=13)
    for t, k in zip(out, ("poses32", "poses64", "inliers", "ref_steps", "num_hyps")):
        assert_bits(k, t[[0, 2]], ref[k][[0, 2]])


def test_argument_errors(gpu):
    from posecnn_amd import ops
    label, depth, vertex, extents, K, _, _ = scene(3)
    args = (dev(gpu, label), u16(gpu, depth), dev(gpu, vertex), dev(gpu, extents), dev(gpu, K), CS.FACTOR)
    for kw in (dict(hypotheses=0), dict(hypotheses=1025), dict(max_attempts=0), dict(pixel_batch=0), dict(max_pixels=0),
               dict(ref_it=-1), dict(min_area=-1), dict(inlier_threshold=float("nan"))):
        with pytest.raises(ValueError):
            ops.estimate_poses_3d(*args, **kw)
    with pytest.raises(ValueError):
        ops.estimate_poses_3d(*args[:5], 0.0)


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


def test_memory_contract(gpu):
    """Guard bands around every output, the driver's workspace and the inputs of the four launching entries, both poison
    patterns: guards and inputs intact, results independent of the poison (records past a frame's total are documented as
    untouched), and equal to the restatement's."""
    import torch
    from posecnn_amd import ops
    label, depth, vertex, extents, K, frames, prep = scene(3)
    totals = [len(p[0]) for p in prep]
    runs, calls = {}, set()
    for pat in memguard.PATTERNS:
        with guarded(pat) as (g, rec):
            ins = [g.embed(label, "cuda"), g.embed(depth, "cuda"), g.embed(vertex, "cuda"), g.embed(extents, "cuda"),
                   g.embed(K, "cuda")]
            streams = g.embed(np.array(STREAMS, dtype=np.uint64).view(np.int64), "cuda")
            records, counts, offsets = ops.pose3d_prepare(*ins, CS.FACTOR)
            hyp = ops.pose3d_sample(records, counts, offsets, ins[3], ins[4], CS.H, CS.W, seed=SEED, streams=streams, hypotheses=70)
            rnd = ops.pose3d_round(records, counts, offsets, hyp[0], hyp[1], CS.H, CS.W, 1)
            est = ops.estimate_poses_3d(*ins, CS.FACTOR, seed=SEED, streams=streams, hypotheses=70)
            torch.cuda.synchronize()
            g.check()
            assert sum(a.kind == "empty" for a in g.arenas) == 3 + 4 + 3 + 5 + 1          # the last one: the workspace
            names = ("records", "counts", "offsets", "hyp_pose", "hyp_class", "hyp_attempt", "hyp_rec", "pose_out", "class_out",
                     "inliers_out", "poses32", "poses64", "inliers", "ref_steps", "num_hyps")
            runs[pat] = {k: memguard.to_numpy(t) for k, t in zip(names, (records, counts, offsets) + tuple(hyp) + tuple(rnd) + tuple(est))}
            calls |= set(rec.calls)
    keep = np.zeros((3, CS.H * CS.W, 6), bool)
    for b, n in enumerate(totals):
        keep[b, n:] = True
    memguard.compare_patterns(runs, keep={"records": keep})
    assert {"pcnn_pose3d_workspace_bytes", "pcnn_pose3d_prepare_fwd", "pcnn_pose3d_sample_fwd", "pcnn_pose3d_round_fwd",
            "pcnn_pose3d_estimate_fwd"} <= calls
    for b, f in enumerate(frames):
        want = R.estimate(f["label"], f["depth"], f["vertex_pred"], extents, f["K"], CS.FACTOR, STREAMS[b], SEED, hypotheses=70)
        assert_bits("poses64[%d]" % b, runs["P2"]["poses64"][b].reshape(-1, 12), want["poses64"])


# ---- the reference's call and the single-frame driver ---------------------------------------------------------------------
def test_synthesizer_layout(gpu):
    """`Synthesizer.estimate_poses_3d` fills poses [3,4,C] in place: class j in poses[:, :, j], the others untouched"""
    from posecnn_amd.icp import Synthesizer
    f = CS.make_frame(1)
    K = f["K"]
    poses = np.full((3, 4, CS.C), -7.0, dtype=F)
    Synthesizer(meshes=[], device=gpu).estimate_poses_3d(f["label"], f["depth"], f["vertex_pred"], f["extents"], poses, CS.C,
                                                         K[0], K[1], K[2], K[3], CS.FACTOR, seed=SEED)
    want = R.estimate(f["label"], f["depth"], f["vertex_pred"], f["extents"], K, CS.FACTOR, 0, SEED)
    for c in range(CS.C):
        if c in CS.POSED:
            assert_bits("class %d" % c, poses[:, :, c].reshape(12), want["poses32"][c])
            assert poses[2, 3, c] > 0
        else:
            assert (poses[:, :, c] == -7.0).all()


def quat2mat_ref(q):
    """(w, x, y, z) -> R with the 2 / |q|^2 scaling, float64"""
    w, x, y, z = [float(v) for v in q]
    s = 2.0 / (w * w + x * x + y * y + z * z)
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]])


def mat2quat_ref(R):
    """rotation matrix -> (w, x, y, z), w >= 0, float64: the trace branch or the largest diagonal element"""
    R = np.asarray(R, dtype=D)
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[1 + i], q[0] = 0.25 * s, (R[k, j] - R[j, k]) / s
        q[1 + j], q[1 + k] = (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q /= np.linalg.norm(q)
    return q if q[0] >= 0 else -q


def bb2d_ref(extent, pose, K):
    """lib/fcn/test.py:1115-1148 in the reference's own types: float32 corners and RT, the float64 intrinsic matrix"""
    h = [extent[0] * 0.5, extent[1] * 0.5, extent[2] * 0.5]
    x3d = np.ones((4, 8), dtype=F)
    x3d[:3] = np.array([[h[0], -h[0]] * 4, [h[1], h[1], -h[1], -h[1]] * 2, [h[2]] * 4 + [-h[2]] * 4], dtype=F)
    RT = np.zeros((3, 4), dtype=F)
    RT[:3, :3] = quat2mat_ref(pose[:4])
    RT[:, 3] = pose[4:7]
    x2d = np.matmul(K, np.matmul(RT, x3d))
    u, v = x2d[0] / x2d[2], x2d[1] / x2d[2]
    return np.array([u.min(), v.min(), u.max(), v.max()], dtype=F)


def test_single_frame_rows(gpu):
    """The post-network half of im_segment_single_frame_3d on planted arrays (the network's planted-layer mechanism adds to
    the 1/8-resolution head features and cannot set `vertex_pred`): the rows equal, bit for bit, this file's restatement of
    mat2quat / _get_bb2D applied to the driver's poses, and go through icp_python(channel_roi = 6) without error. Then the whole function on a small
    `vertex_reg_3d` network: it returns the rows of its own label map and field."""
    import torch
    from posecnn_amd import fcn
    from posecnn_amd.icp import Mesh, Synthesizer
    from posecnn_amd.networks import vgg16_convs
    f = CS.make_frame(1)
    K = f["K"]
    meta = {"intrinsic_matrix": np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dtype=D), "factor_depth": CS.FACTOR}
    rois, poses = fcn.poses_from_vertmap_3d(f["label"], f["depth"], f["vertex_pred"], meta, f["extents"], CS.C, seed=SEED, device=gpu)
    want = R.estimate(f["label"], f["depth"], f["vertex_pred"], f["extents"], K, CS.FACTOR, 0, SEED)
    assert rois.shape == (3, 6) and poses.shape == (3, 7) and rois[:, 1].tolist() == [1.0, 2.0, 3.0] and not rois[:, 0].any()
    for row, c in enumerate(CS.POSED):
        P = want["poses32"][c].reshape(3, 4)
        wq = np.zeros(7, F)
        wq[:4], wq[4:] = mat2quat_ref(P[:, :3]), P[:, 3]                    # the restated mat2quat of the driver's f32 pose
        assert_bits("pose row %d" % row, poses[row], wq)
        assert_bits("box row %d" % row, rois[row, 2:], bb2d_ref(f["extents"][c], wq, meta["intrinsic_matrix"]))
        assert abs(np.linalg.norm(wq[:4].astype(D)) - 1) < 1e-6 and wq[0] >= 0
        assert np.abs(quat2mat_ref(wq[:4]) - P[:, :3]).max() < 1e-6         # and it is the rotation it came from
    # the rows feed icp_python with 6-column ROIs
    import icp_scene
    v, n, faces = icp_scene.box_mesh((CS.EXTENT / 2,) * 3)
    syn = Synthesizer(meshes=[Mesh(v, faces, n, device=gpu)] * (CS.C - 1), device=gpu)
    out, out_icp = np.zeros((3, 7), F), np.zeros((3, 7), F)
    syn.icp_python(f["label"], f["depth"], (K[0], K[1], K[2], K[3], 0.25, 6.0, CS.FACTOR), CS.H, CS.W, 3, 6, rois, poses, out,
                   out_icp, 0.01)
    assert np.isfinite(out).all() and np.isfinite(out_icp).all()

    net = vgg16_convs("COLOR", CS.C, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=False, vertex_reg_3d=True, pose_reg=False,
                      trainable=False, is_train=False, seed=3, init="he", with_losses=False, device=gpu)
    im = np.random.RandomState(0).randint(0, 256, size=(CS.H, CS.W, 3)).astype(np.uint8)
    with torch.no_grad():
        labels, probs, vertex_pred, rois2, poses2 = fcn.im_segment_single_frame_3d(net, im, f["depth"], meta, f["extents"], CS.C,
                                                                                    seed=SEED, device=gpu)
    assert labels.shape == (CS.H, CS.W) and vertex_pred.shape == (CS.H, CS.W, 3 * CS.C) and rois2.shape[1] == 6
    r3, p3 = fcn.poses_from_vertmap_3d(labels, f["depth"], vertex_pred, meta, f["extents"], CS.C, seed=SEED, device=gpu)
    assert_bits("rois", rois2, r3)
    assert_bits("poses", poses2, p3)
