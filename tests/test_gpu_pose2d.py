"""The colour-only pose kernels of the 3-D vertex route (include/posecnn_hip_pose2d.h) on the GPU: every output bit for bit
equal to the numpy restatement tests/pose2d_ref.py, on the planted 64 x 96 scenes of tests/pose2d_cases.py."""
import contextlib
import functools

import numpy as np
import pytest

import memguard
import pose2d_cases as CS
import pose2d_ref as R

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
SEED = (0x1234_5678_9ABC_DEF0 << 64) | 0x0FED_CBA9_8765_4321
STREAMS = (11, 5, 1 << 63)
PARAMS = CS.PARAMS
OUT = ("poses32", "poses64", "inliers", "ref_steps", "num_hyps")


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


def stream_tensor(gpu, ids):
    return dev(gpu, np.array(ids, dtype=np.uint64).view(np.int64))


@functools.lru_cache(maxsize=None)
def scene():
    """B = 3 frames with their own intrinsics; the restatement's records are computed once and shared"""
    label, vertex, extents, K, frames = CS.batch((1, 2, 3), CS.INTRINSICS)
    prep = [R.prepare(f["label"], f["vertex_pred"], extents) for f in frames]
    return label, vertex, extents, K, frames, prep


@functools.lru_cache(maxsize=None)
def reference(b, hypotheses):
    """the restatement's whole loop on frame b: computed once per hypothesis count"""
    label, vertex, extents, K, frames, prep = scene()
    f = frames[b]
    return R.estimate(f["label"], f["vertex_pred"], extents, f["K"], STREAMS[b], SEED, hypotheses=hypotheses, **PARAMS)


def gpu_prepare(gpu, vertex_tensor=None):
    from posecnn_amd import ops
    label, vertex, extents, K, _, _ = scene()
    v = dev(gpu, vertex) if vertex_tensor is None else vertex_tensor
    return ops.pose2d_prepare(dev(gpu, label), v, dev(gpu, extents))


# ---- prepare --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True])
def test_prepare(gpu, misaligned):
    """records, counts and order of three frames (labels >= C and < 0 are in every frame); `misaligned`: vertex_pred is a
    view 4 bytes into its allocation"""
    import torch
    label, vertex, extents, K, frames, prep = scene()
    v = None
    if misaligned:
        flat = torch.empty(vertex.size + 1, dtype=torch.float32, device=gpu)
        v = flat[1:].view(vertex.shape)
        v.copy_(dev(gpu, vertex))
        assert v.data_ptr() % 16 == 4
    records, counts, offsets = (t.cpu().numpy() for t in gpu_prepare(gpu, v))
    for b, (rec, cnt, off) in enumerate(prep):
        assert [int(cnt[c]) for c in range(1, CS.C)] == [CS.SIZES[c] for c in range(1, CS.C)]
        assert not rec[:, 2].any() and rec[:, 0].max() == 94 and rec[:, 1].max() == 63  # (x, y, 0, obj): class 4 ends at column 94
        assert_bits("counts[%d]" % b, counts[b], cnt)
        assert_bits("offsets[%d]" % b, offsets[b], off)
        assert_bits("records[%d]" % b, records[b, :len(rec)], rec)


# ---- sample ---------------------------------------------------------------------------------------------------------------
def test_sample(gpu):
    from posecnn_amd import ops
    label, vertex, extents, K, frames, prep = scene()
    records, counts, offsets = gpu_prepare(gpu)
    got = ops.pose2d_sample(records, counts, offsets, dev(gpu, extents), dev(gpu, K), CS.H, CS.W, seed=SEED,
                            streams=stream_tensor(gpu, STREAMS), hypotheses=256, **PARAMS)
    pose, cls, att, rec4 = (t.cpu().numpy() for t in got)
    for b, (rec, cnt, off) in enumerate(prep):
        want = R.sample(rec, cnt, off, extents, frames[b]["K"], CS.H, CS.W, STREAMS[b], SEED, hypotheses=256, **PARAMS)
        assert set(np.unique(want[1])) == {1, 2, 3}                   # every posed class drew hypotheses, the all-empty class none
        assert want[2].max() > 0                                      # some first attempts were refused
        assert_bits("hyp_class[%d]" % b, cls[b], want[1])
        assert_bits("hyp_attempt[%d]" % b, att[b], want[2])
        assert_bits("hyp_rec[%d]" % b, rec4[b], want[3])
        assert_bits("hyp_pose[%d]" % b, pose[b].reshape(-1, 12), want[0])


def test_sample_dead(gpu):
    """only the all-empty class is live: with max_attempts = 16 every hypothesis is dead"""
    from posecnn_amd import ops
    f = CS.make_frame(1)
    label = np.where(f["label"] == 5, 5, 0).astype(np.int32)
    args = (dev(gpu, label[None]), dev(gpu, f["vertex_pred"][None]), dev(gpu, f["extents"]))
    K = dev(gpu, np.array([f["K"]], dtype=F))
    records, counts, offsets = ops.pose2d_prepare(*args)
    assert counts.cpu().numpy()[0].tolist() == [0, 0, 0, 0, 0, 448, 0]
    pose, cls, att, rec4 = (t.cpu().numpy() for t in ops.pose2d_sample(records, counts, offsets, args[2], K, CS.H, CS.W, seed=SEED,
                                                                        hypotheses=70, max_attempts=16, **PARAMS))
    assert not pose.any() and not cls.any() and (att == -1).all() and (rec4 == -1).all()
    out = ops.estimate_poses_2d(*args, K, seed=SEED, hypotheses=70, max_attempts=16, **PARAMS)
    assert all(not t.cpu().numpy().any() for t in out)


# ---- one round ------------------------------------------------------------------------------------------------------------
def check_rounds(gpu, pose, cls, rounds, **kw):
    """chained rounds on frame 0 of the scene (frames 1, 2 carry empty slots): GPU against the restatement, each fed the
    GPU's previous output"""
    from posecnn_amd import ops
    label, vertex, extents, K, frames, prep = scene()
    records, counts, offsets = gpu_prepare(gpu)
    rec, cnt, off = prep[0]
    n = len(cls)
    poses = np.zeros((3, n, 3, 4), D)
    classes = np.zeros((3, n), np.int32)
    poses[0], classes[0] = pose.reshape(n, 3, 4), cls
    classes[1, :3] = (0, -4, 70)                      # not hypotheses: come back as class 0, pose unchanged
    kw = dict(inlier_threshold=CS.INLIER_THRESHOLD, **kw)
    seen = []
    for rnd in rounds:
        p, c, i = (t.cpu().numpy() for t in ops.pose2d_round(records, counts, offsets, dev(gpu, K), dev(gpu, poses), dev(gpu, classes),
                                                               CS.H, CS.W, rnd, **kw))
        wp, wc, wi = R.round_fwd(rec, cnt, off, poses[0].reshape(n, 12), classes[0], rnd, frames[0]["K"], **kw)
        assert_bits("class_out round %d" % rnd, c[0], wc)
        assert_bits("inliers_out round %d" % rnd, i[0], wi)
        assert_bits("pose_out round %d" % rnd, p[0].reshape(n, 12), wp)
        assert not c[1:].any() and not i[1:].any()
        assert_bits("empty slots", p[1:], poses[1:])
        seen.append((c[0].copy(), i[0].copy(), p[0].copy(), poses[0].copy()))
        poses[0], classes[0] = p[0], c[0]
    return seen


def sampled(n_hyp):
    label, vertex, extents, K, frames, prep = scene()
    rec, cnt, off = prep[0]
    pose, cls, _, _ = R.sample(rec, cnt, off, extents, frames[0]["K"], CS.H, CS.W, STREAMS[0], SEED, hypotheses=n_hyp, **PARAMS)
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


def moved(pose):
    """every pose 1 mm off along each axis (0.15 pixel): the refit has an increment far above the rounding of its sums"""
    pose = np.array(pose, dtype=D).reshape(-1, 12).copy()
    pose[:, [3, 7, 11]] += 1e-3
    return pose


def test_round_moved_poses(gpu):
    """the refit at work: from poses 1 mm off, three chained rounds, the last one thinned"""
    pose, cls = sampled(32)
    seen = check_rounds(gpu, moved(pose), cls, (1, 2, 3))
    c, i, p, before = seen[0]
    assert (np.abs(p - before).max(axis=(1, 2))[c > 0] > 1e-4).all()          # every survivor moved back


def three_inlier_case():
    """hand-made records: class 1 has 3 pixels that reproject within the threshold under the given pose, class 2 has 4"""
    rng = np.random.RandomState(5)
    n3, n4 = 40, 50
    K = (120.0, 118.0, 48.0, 32.0)
    obj = rng.uniform(-0.1, 0.1, size=(n3 + n4, 3)).astype(F)
    q = obj.astype(D) + np.array([0.0, 0.0, 1.0])                        # identity rotation, t = (0, 0, 1)
    pix = np.stack([K[0] * q[:, 0] / q[:, 2] + K[2], K[1] * q[:, 1] / q[:, 2] + K[3]], axis=1)
    bad = np.ones(n3 + n4, bool)
    bad[[3, 17, 30]] = False
    bad[[n3 + 1, n3 + 9, n3 + 20, n3 + 41]] = False
    pix[bad] += 40.0
    pix[~bad] += rng.uniform(-0.3, 0.3, size=(7, 2))                     # not exact: the refit has something to do
    HW = CS.H * CS.W
    records = np.zeros((1, HW, 6), F)
    records[0, :n3 + n4, :2], records[0, :n3 + n4, 3:] = pix, obj
    counts, offsets = np.array([[0, n3, n4]], np.int32), np.array([[0, 0, n3]], np.int32)
    pose = np.zeros((1, 2, 12), D)
    pose[0, :, [0, 5, 10]] = 1.0
    pose[0, :, 11] = 1.0 + 1e-4
    return records, counts, offsets, pose, np.array([[1, 2]], np.int32), K


def test_round_three_inliers(gpu):
    """a lone hypothesis with 3 inliers is not refitted, one with 4 is"""
    from posecnn_amd import ops
    records, counts, offsets, pose, cls, K = three_inlier_case()
    p, c, i = (t.cpu().numpy() for t in ops.pose2d_round(dev(gpu, records), dev(gpu, counts), dev(gpu, offsets),
                                                           dev(gpu, np.array([K], F)), dev(gpu, pose.reshape(1, 2, 3, 4)), dev(gpu, cls),
                                                           CS.H, CS.W, 1, inlier_threshold=1.0))
    wp, wc, wi = R.round_fwd(records[0], counts[0], offsets[0], pose[0], cls[0], 1, K, inlier_threshold=1.0)
    assert wi.tolist() == [3, 4] and wc.tolist() == [1, 2]
    assert_bits("class_out", c[0], wc)
    assert_bits("inliers_out", i[0], wi)
    assert_bits("pose_out", p[0].reshape(2, 12), wp)
    assert_bits("three inliers: untouched", p[0, 0].reshape(12), pose[0, 0])
    assert (p[0, 1].reshape(12) != pose[0, 1]).any()


def test_round_at_threshold(gpu):
    """a record whose reprojection distance EQUALS the threshold is no inlier (`<`): the lone hypothesis of
    tests/pose2d_cases.threshold_frame has 3 inliers and is not refitted; with `<=` it would have 4 and move"""
    from posecnn_amd import ops
    f = CS.threshold_frame()
    rec, cnt, off = R.prepare(f["label"], f["vertex_pred"], f["extents"])
    d, front = R.reproj(CS.THRESHOLD_POSE[None], rec, f["K"])
    assert sorted(d[0].tolist()) == [0.0, 0.0, 0.0, CS.THRESHOLD] and front.all() and D(F(CS.THRESHOLD)) == CS.THRESHOLD
    records, counts, offsets = ops.pose2d_prepare(dev(gpu, f["label"][None]), dev(gpu, f["vertex_pred"][None]), dev(gpu, f["extents"]))
    assert_bits("records", records.cpu().numpy()[0, :4], rec)
    pose, cls = CS.THRESHOLD_POSE.reshape(1, 1, 3, 4), np.array([[1]], np.int32)
    p, c, i = (t.cpu().numpy() for t in ops.pose2d_round(records, counts, offsets, dev(gpu, np.array([f["K"]], F)), dev(gpu, pose),
                                                           dev(gpu, cls), 8, 8, 1, inlier_threshold=CS.THRESHOLD))
    wp, wc, wi = R.round_fwd(rec, cnt, off, pose.reshape(1, 12), cls[0], 1, f["K"], inlier_threshold=CS.THRESHOLD)
    assert wi.tolist() == [3] and wc.tolist() == [1]
    assert_bits("inliers_out", i[0], wi)
    assert_bits("class_out", c[0], wc)
    assert_bits("pose_out", p[0].reshape(1, 12), wp)
    assert_bits("not refitted", p[0].reshape(12), CS.THRESHOLD_POSE)


# ---- the driver -----------------------------------------------------------------------------------------------------------
def estimate(gpu, order=(0, 1, 2), **kw):
    from posecnn_amd import ops
    label, vertex, extents, K, _, _ = scene()
    order = list(order)
    out = ops.estimate_poses_2d(dev(gpu, label[order]), dev(gpu, vertex[order]), dev(gpu, extents), dev(gpu, K[order]), seed=SEED,
                                streams=stream_tensor(gpu, [STREAMS[b] for b in order]), **PARAMS, **kw)
    return dict(zip(OUT, (t.cpu().numpy() for t in out)))


def staged(gpu, hypotheses, ref_it=8):
    """the driver's result from the staged calls: prepare, sample, then one pose2d_round per round of the schedule with the
    class ids read back in between"""
    from posecnn_amd import ops
    label, vertex, extents, K, _, _ = scene()
    records, counts, offsets = gpu_prepare(gpu)
    Kt = dev(gpu, K)
    pose, cls, _, _ = ops.pose2d_sample(records, counts, offsets, dev(gpu, extents), Kt, CS.H, CS.W, seed=SEED,
                                        streams=stream_tensor(gpu, STREAMS), hypotheses=hypotheses, **PARAMS)
    num = np.stack([np.bincount(c, minlength=CS.C) for c in cls.cpu().numpy()]).astype(np.int32)
    rounds = max(len(R.halving_schedule(int(v), ref_it)) for v in num[:, 1:].reshape(-1))
    inl = None
    for rnd in range(1, rounds + 1):
        pose, cls, inl = ops.pose2d_round(records, counts, offsets, Kt, pose, cls, CS.H, CS.W, rnd, inlier_threshold=CS.INLIER_THRESHOLD)
    pose, cls, inl = pose.cpu().numpy(), cls.cpu().numpy(), inl.cpu().numpy()
    poses64, inliers = np.zeros((3, CS.C, 3, 4), D), np.zeros((3, CS.C), np.int32)
    for b in range(3):
        for c in range(1, CS.C):
            h = np.nonzero(cls[b] == c)[0]
            if len(h):
                assert len(h) == 1
                poses64[b, c], inliers[b, c] = pose[b, h[0]], inl[b, h[0]]
    return poses64, inliers, num


@pytest.mark.parametrize("hypotheses", [1, 13, 256])
def test_driver(gpu, hypotheses):
    label, vertex, extents, K, frames, prep = scene()
    got = estimate(gpu, hypotheses=hypotheses)
    again = estimate(gpu, hypotheses=hypotheses)
    for k in got:
        assert_bits("second run " + k, again[k], got[k])
    for b, f in enumerate(frames):
        want = reference(b, hypotheses)
        assert want["num_hyps"].sum() == hypotheses and not want["num_hyps"][[0, 4, 5, 6]].any()
        for k in ("num_hyps", "ref_steps", "inliers"):
            assert_bits("%s[%d]" % (k, b), got[k][b], want[k])
        assert_bits("poses64[%d]" % b, got["poses64"][b].reshape(-1, 12), want["poses64"])
        assert_bits("poses32[%d]" % b, got["poses32"][b].reshape(-1, 12), want["poses32"])
        for c in range(CS.C):
            if want["num_hyps"][c] == 0:                           # not live, all empty, absent, or no hypothesis drawn
                assert not got["poses64"][b, c].any() and got["inliers"][b, c] == 0 and got["ref_steps"][b, c] == 0
    # every round of a class with one hypothesis left is the same computation in both: the staged calls give the same bits
    poses64, inliers, num = staged(gpu, hypotheses)
    assert_bits("staged num_hyps", num, got["num_hyps"])
    same_rounds = np.array([[len(R.halving_schedule(int(v), 8)) for v in row] for row in num])
    full = same_rounds == same_rounds[:, 1:].max()                 # the classes whose own schedule is the longest one
    full &= num > 0
    assert full.any()
    assert_bits("staged poses64", poses64[full], got["poses64"][full])
    assert_bits("staged inliers", inliers[full], got["inliers"][full])


def test_driver_no_live_class(gpu):
    """a frame whose only class has 400 pixels (not live) between two ordinary frames"""
    from posecnn_amd import ops
    label, vertex, extents, K, frames, prep = scene()
    label = label.copy()
    label[1] = np.where(label[1] == 4, 4, 0)
    out = ops.estimate_poses_2d(dev(gpu, label), dev(gpu, vertex), dev(gpu, extents), dev(gpu, K), seed=SEED,
                                streams=stream_tensor(gpu, STREAMS), hypotheses=13, **PARAMS)
    out = [t.cpu().numpy() for t in out]
    assert all(not t[1].any() for t in out)
    for t, k in zip(out, OUT):
        for b in (0, 2):
            want = reference(b, 13)
            assert_bits(k, t[b].reshape(want[k].shape), want[k])


def test_batch_slot_independence(gpu):
    """a frame's result does not depend on its batch slot: the frames permuted, each with its own stream id"""
    ref = estimate(gpu, hypotheses=13)
    order = (2, 0, 1)
    got = estimate(gpu, order=order, hypotheses=13)
    single = estimate(gpu, order=(2,), hypotheses=13)
    for k in OUT:
        assert_bits("permuted " + k, got[k], ref[k][list(order)])
        assert_bits("alone " + k, single[k][0], ref[k][2])


def test_argument_errors(gpu):
    from posecnn_amd import ops
    label, vertex, extents, K, _, _ = scene()
    args = (dev(gpu, label), dev(gpu, vertex), dev(gpu, extents), dev(gpu, K))
    for kw in (dict(hypotheses=0), dict(hypotheses=1025), dict(max_attempts=0), dict(pixel_batch=0), dict(max_pixels=0),
               dict(ref_it=-1), dict(min_area=-1), dict(inlier_threshold=float("nan")), dict(min_dist2d=float("inf")),
               dict(min_dist3d=float("nan"))):
        with pytest.raises(ValueError):
            ops.estimate_poses_2d(*args, **kw)
    with pytest.raises(ValueError):
        ops.estimate_poses_2d(args[0], args[1], args[2], args[3][:2])
    with pytest.raises(ValueError):
        ops.pose2d_round(*gpu_prepare(gpu), args[3], dev(gpu, np.zeros((3, 4, 3, 4))), dev(gpu, np.zeros((3, 4), np.int32)), CS.H, CS.W, 0)


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
    label, vertex, extents, K, frames, prep = scene()
    totals = [len(p[0]) for p in prep]
    runs, calls = {}, set()
    for pat in memguard.PATTERNS:
        with guarded(pat) as (g, rec):
            ins = [g.embed(label, "cuda"), g.embed(vertex, "cuda"), g.embed(extents, "cuda"), g.embed(K, "cuda")]
            streams = g.embed(np.array(STREAMS, dtype=np.uint64).view(np.int64), "cuda")
            records, counts, offsets = ops.pose2d_prepare(*ins[:3])
            hyp = ops.pose2d_sample(records, counts, offsets, ins[2], ins[3], CS.H, CS.W, seed=SEED, streams=streams, hypotheses=13, **PARAMS)
            rnd = ops.pose2d_round(records, counts, offsets, ins[3], hyp[0], hyp[1], CS.H, CS.W, 1, inlier_threshold=CS.INLIER_THRESHOLD)
            est = ops.estimate_poses_2d(*ins, seed=SEED, streams=streams, hypotheses=13, **PARAMS)
            torch.cuda.synchronize()
            g.check()
            assert sum(a.kind == "empty" for a in g.arenas) == 3 + 4 + 3 + 5 + 1          # the last one: the workspace
            names = ("records", "counts", "offsets", "hyp_pose", "hyp_class", "hyp_attempt", "hyp_rec", "pose_out", "class_out",
                     "inliers_out") + OUT
            runs[pat] = {k: memguard.to_numpy(t) for k, t in zip(names, (records, counts, offsets) + tuple(hyp) + tuple(rnd) + tuple(est))}
            calls |= set(rec.calls)
    keep = np.zeros((3, CS.H * CS.W, 6), bool)
    for b, n in enumerate(totals):
        keep[b, n:] = True
    memguard.compare_patterns(runs, keep={"records": keep})
    assert {"pcnn_pose2d_workspace_bytes", "pcnn_pose2d_prepare_fwd", "pcnn_pose2d_sample_fwd", "pcnn_pose2d_round_fwd",
            "pcnn_pose2d_estimate_fwd"} <= calls
    for b in range(3):
        assert_bits("poses64[%d]" % b, runs["P2"]["poses64"][b].reshape(-1, 12), reference(b, 13)["poses64"])


# ---- the reference's call and the single-frame driver ---------------------------------------------------------------------
def test_synthesizer_layout(gpu):
    """`Synthesizer.estimate_poses_2d` fills poses [3,4,C] in place: class j in poses[:, :, j], the others untouched.
    The reference's thresholds (10 pixels) on the 96-pixel frame: the layout is checked against the restatement, not the
    planted pose."""
    from posecnn_amd.icp import Synthesizer
    f = CS.make_frame(1)
    K = f["K"]
    poses = np.full((3, 4, CS.C), -7.0, dtype=F)
    Synthesizer(meshes=[], device=gpu).estimate_poses_2d(f["label"], f["vertex_pred"], f["extents"], poses, CS.C, K[0], K[1], K[2], K[3],
                                                         seed=SEED)
    want = R.estimate(f["label"], f["vertex_pred"], f["extents"], K, 0, SEED)
    assert (want["num_hyps"][list(CS.POSED)] > 0).all()
    for c in range(CS.C):
        if c in CS.POSED:
            assert_bits("class %d" % c, poses[:, :, c].reshape(12), want["poses32"][c])
            assert poses[2, 3, c] > 0
        else:
            assert (poses[:, :, c] == -7.0).all()


def test_single_frame_rows(gpu):
    """`poses_from_vertmap_2d` on planted arrays: the rows are the depth leg's row builder (tests/test_gpu_pose3d.py checks
    it against the reference's mat2quat / _get_bb2D) applied to the colour driver's poses. Then the whole function on a small
    `vertex_reg_3d` network with rgb_poses=True and no depth frame: it returns the rows of its own label map and field, and
    the default call still needs its depth frame."""
    import torch
    from posecnn_amd import fcn
    from posecnn_amd.icp import mat2quat
    from posecnn_amd.networks import vgg16_convs
    f = CS.make_frame(1)
    K = f["K"]
    meta = {"intrinsic_matrix": np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dtype=D)}
    rois, poses = fcn.poses_from_vertmap_2d(f["label"], f["vertex_pred"], meta, f["extents"], CS.C, seed=SEED, device=gpu)
    want = R.estimate(f["label"], f["vertex_pred"], f["extents"], K, 0, SEED)
    assert rois.shape == (3, 6) and poses.shape == (3, 7) and rois[:, 1].tolist() == [1.0, 2.0, 3.0] and not rois[:, 0].any()
    for row, c in enumerate(CS.POSED):
        P = want["poses32"][c].reshape(3, 4)
        wq = np.zeros(7, F)
        wq[:4], wq[4:] = mat2quat(P[:, :3]), P[:, 3]
        assert_bits("pose row %d" % row, poses[row], wq)
        assert_bits("box row %d" % row, rois[row, 2:], fcn._get_bb2D(f["extents"][c], wq, meta["intrinsic_matrix"]))
        assert abs(np.linalg.norm(wq[:4].astype(D)) - 1) < 1e-6 and wq[0] >= 0

    net = vgg16_convs("COLOR", CS.C, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=False, vertex_reg_3d=True, pose_reg=False,
                      trainable=False, is_train=False, seed=3, init="he", with_losses=False, device=gpu)
    im = np.random.RandomState(0).randint(0, 256, size=(CS.H, CS.W, 3)).astype(np.uint8)
    with torch.no_grad():
        labels, probs, vertex_pred, rois2, poses2 = fcn.im_segment_single_frame_3d(net, im, None, meta, f["extents"], CS.C, seed=SEED,
                                                                                    device=gpu, rgb_poses=True)
        with pytest.raises(ValueError):
            fcn.im_segment_single_frame_3d(net, im, None, meta, f["extents"], CS.C, seed=SEED, device=gpu)
    assert labels.shape == (CS.H, CS.W) and vertex_pred.shape == (CS.H, CS.W, 3 * CS.C) and rois2.shape[1] == 6 and poses2.shape[1] == 7
    r2, p2 = fcn.poses_from_vertmap_2d(labels, vertex_pred, meta, f["extents"], CS.C, seed=SEED, device=gpu)
    assert_bits("rois", rois2, r2)
    assert_bits("poses", poses2, p2)
