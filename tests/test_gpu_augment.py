"""pcnn_augment_frames_fwd on the GPU against the numpy restatement tests/augment_ref.py (include/posecnn_hip_augment.h):
the chromatic transform over all 2^24 colours, the blurs and both depth blobs bit for bit; the Gaussian path against the
float64 restatement within 4 x the distance the float32 restatement has from it (tests/test_augment_cpu.py measures
1.935e-05 on these very cases: the device's log and cos are another float32 implementation, not a better or worse one);
batch independence; the memory contract; the training feed."""
import contextlib
import functools

import numpy as np
import pytest

import augment_cases as CS
import augment_ref as R
import memguard

pytestmark = pytest.mark.gpu
F = np.float32


def run(gpu, color, depth, rows, seed=CS.SEED, depth_norm="frame_max", pixel_means=None):
    import torch
    from posecnn_amd import ops
    c = torch.from_numpy(np.ascontiguousarray(color)).to(gpu)
    d = None if depth is None else torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(gpu).view(torch.uint16)
    data, data_p = ops.augment_frames(c, d, rows, seed, pixel_means, depth_norm)
    torch.cuda.synchronize()
    return data.cpu().numpy(), (None if data_p is None else data_p.cpu().numpy())


def assert_bits(name, got, want):
    assert got.dtype == want.dtype == F and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r vs %r" % (name, (~same).sum(), same.size, i, got[i], want[i]))


# ---- chromatic transform --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _all_colours():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=-1).astype(np.uint8).reshape(1, 4096, 4096, 3)


def test_all_colours_byte_for_byte(gpu):
    """All 2^24 colours as one 4096 x 4096 frame, mode 0, jitter (-1.7, +25.3, -25.1): hue wrap, L clipped at the top, S
    clipped at the bottom. Zero means: the blob is the transformed byte itself."""
    color = _all_colours()
    rows = np.stack([R.row(CS.JITTER, 0, 0.0, 0, 1)])
    got, _ = run(gpu, color, None, rows, pixel_means=(0.0, 0.0, 0.0))
    want = np.concatenate([R.chromatic(color[0, y:y + 256], *CS.JITTER) for y in range(0, 4096, 256)])
    assert_bits("data", got[0], want.astype(F))
    assert (want != color[0]).any()


def test_opposite_jitter_on_a_sample(gpu):
    """(+1.7, -25.3, +25.1) on 2^20 colours: hue wrap at the top, L clipped at the bottom, S at the top; and zero jitter,
    which is not the identity."""
    rng = np.random.default_rng(9)
    color = rng.integers(0, 256, (2, 512, 1024, 3)).astype(np.uint8)
    rows = np.stack([R.row((1.7, -25.3, 25.1), 0, 0.0, 0, 1), R.row((0.0, 0.0, 0.0), 0, 0.0, 1, 1)])
    got, _ = run(gpu, color, None, rows)
    want, _ = R.augment_frames(color, None, rows, CS.SEED)
    assert_bits("data", got, want)
    assert (R.chromatic(color[1], 0.0, 0.0, 0.0) != color[1]).any()


# ---- Gaussian ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", CS.GAUSS_SIZES, ids=["%dx%d" % s for s in CS.GAUSS_SIZES])
def test_gaussian_against_the_float64_restatement(gpu, size):
    case = CS.gauss_case(*size)
    bound = 4 * CS.gauss_tolerance()
    for norm, name in ((0, "frame_max"), (1, "fixed_2000")):
        got = run(gpu, case["color"], case["depth"], case["rows"], depth_norm=name)
        for plane, g, w in zip(("data", "data_p"), got, case["f64", norm]):
            err = np.abs(g.astype(np.float64) - w)
            print("%s %s %s: max |kernel - float64| = %.3e (bound %.3e)" % (size, name, plane, err.max(), bound))
            assert err.max() <= bound, (plane, name)
            # the value before the means: where it is well inside (0, 255) or well outside, the clip decision agrees
            v64 = w + R.PIXEL_MEANS
            inside = (v64 >= bound) & (v64 <= 255 - bound)
            at_0, at_255 = (0.0 - R.PIXEL_MEANS).astype(F), (255.0 - R.PIXEL_MEANS).astype(F)
            assert not ((g == at_0) | (g == at_255))[inside].any(), (plane, name)
            assert inside.mean() > 0.5 and not inside.all()          # the cases do clip somewhere
        # the noise is there, and it is the same deviate on the three channels of the colour plane
        clean = R.augment_frames(case["color"], case["depth"], np.stack([R.row(CS.JITTER, 0, 0, 0, 1)] * 2), CS.SEED, depth_norm=norm)
        assert np.abs(got[0] - clean[0]).max() > 1 and np.abs(got[1] - clean[1]).max() > 1


# ---- blur -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(8, 8), (CS.TILE_H + 1, CS.TILE_W + 1)], ids=["8x8", "tile+1"])
def test_blurs_bit_for_bit(gpu, size):
    """All six lengths x both orientations as one batch of 12 frames; at 8 x 8 a radius of 7 reflects off the far edge.
    Colour bytes (chromatic on) and depth floats equal the restatement bit for bit; BGRA input equals BGR input."""
    H, W = size
    color4, depth = CS.frames(H, W, 12, 4)
    color3 = np.ascontiguousarray(color4[..., :3])
    rows = np.stack([R.row(CS.JITTER, 2 + k % 2, CS.BLUR_SIZES[k // 2], k, 1, 3 - k % 2, CS.BLUR_SIZES[5 - k // 2], 50 + k) for k in range(12)])
    for norm, name in ((0, "frame_max"), (1, "fixed_2000")):
        want = R.augment_frames(color3, depth, rows, CS.SEED, depth_norm=norm)
        got3 = run(gpu, color3, depth, rows, depth_norm=name)
        got4 = run(gpu, color4, depth, rows, depth_norm=name)
        for plane, g3, g4, w in zip(("data", "data_p"), got3, got4, want):
            assert_bits("%s (BGR, %s)" % (plane, name), g3, w)
            assert_bits("%s (BGRA, %s)" % (plane, name), g4, w)
    assert np.abs(want[0] - R.augment_frames(color3, None, np.stack([R.row(CS.JITTER, 0, 0, 0, 1)] * 12), CS.SEED)[0]).max() > 1


# ---- batch independence -------------------------------------------------------------------------------------------------
def test_a_frame_does_not_depend_on_its_slot(gpu):
    H, W = 17, 23
    color, depth = CS.frames(H, W, 3)
    rows = CS.gauss_rows(3)
    alone = run(gpu, color[:1], depth[:1], rows[:1])
    for slot in range(3):
        order = [(slot + k) % 3 for k in (0, 1, 2)]           # frame 0 sits in slot (3 - slot) % 3
        at = order.index(0)
        got = run(gpu, color[order], depth[order], rows[order])
        assert_bits("data in slot %d" % at, got[0][at:at + 1], alone[0])
        assert_bits("data_p in slot %d" % at, got[1][at:at + 1], alone[1])
    again = run(gpu, color[:1], depth[:1], rows[:1])
    assert_bits("second run, data", again[0], alone[0])
    assert_bits("second run, data_p", again[1], alone[1])
    other = rows[:1].copy()
    other[0, 5] += 1
    other[0, 9] += 1
    diff = run(gpu, color[:1], depth[:1], other)
    assert (diff[0] != alone[0]).mean() > 0.5 and (diff[1] != alone[1]).mean() > 0.5
    reseeded = run(gpu, color[:1], depth[:1], rows[:1], seed=CS.SEED ^ (1 << 100))
    assert (reseeded[0] != alone[0]).mean() > 0.5


def test_more_frames_than_one_launch_takes(gpu):
    """40 frames: the rows travel as kernel arguments, 32 frames per launch."""
    color, depth = CS.frames(8, 12, 40, 4)
    rows = np.stack([R.row((0.3 * (b % 5), -b, b), b % 4, (0.5 + b if b % 4 == 1 else CS.BLUR_SIZES[b % 6]), 3 * b, b % 2,
                           (b + 1) % 4, (1.5 if (b + 1) % 4 == 1 else CS.BLUR_SIZES[(b + 2) % 6]), 3 * b + 1) for b in range(40)])
    blur_or_none = np.array([b % 4 != 1 for b in range(40)]), np.array([(b + 1) % 4 != 1 for b in range(40)])
    got = run(gpu, color, depth, rows)
    want = R.augment_frames(color, depth, rows, CS.SEED)
    want64 = R.augment_frames(color, depth, rows, CS.SEED, use64=True)
    for plane, g, w, w64, exact in zip(("data", "data_p"), got, want, want64, blur_or_none):
        assert_bits(plane, g[exact], w[exact])
        assert np.nanmax(np.abs(g[~exact].astype(np.float64) - w64[~exact])) <= 4 * CS.gauss_tolerance()


# ---- depth blobs --------------------------------------------------------------------------------------------------------
def test_chromatic_off_equals_the_raw_frame_blob(gpu):
    """Chromatic off + mode 0 + depth_norm 1 is `networks.raw_frame_blob` of the same frames, bit for bit."""
    import torch
    from posecnn_amd import networks, ops
    H, W = 2 * CS.TILE_H + 3, 2 * CS.TILE_W + 3
    color, depth = CS.frames(H, W, 2, 4)
    c = torch.from_numpy(color).to(gpu)
    d = torch.from_numpy(depth.view(np.int16)).to(gpu).view(torch.uint16)
    rows = np.stack([R.row((1.0, 2.0, 3.0), 0, 0.0, b, 0, 0, 0.0, 9 + b) for b in range(2)])
    data, data_p = ops.augment_frames(c, d, rows, CS.SEED, depth_norm="fixed_2000")
    assert torch.equal(data, networks.raw_frame_blob(c[..., :3].contiguous()))
    assert torch.equal(data_p, networks.raw_frame_blob(d))
    want = R.augment_frames(color, depth, rows, CS.SEED, depth_norm=1)
    assert_bits("data", data.cpu().numpy(), want[0])
    assert_bits("data_p", data_p.cpu().numpy(), want[1])


@pytest.mark.parametrize("size", [(9, 10), (37, 64)], ids=["9x10", "37x64"])
def test_frame_max_depth_blob(gpu, size):
    """depth_norm 0: the frame's own maximum, found on the device; an all-zero frame is NaN everywhere, as numpy's is.
    Frame 1's maximum sits in its last element, frame 2's in its first (the max kernel's scalar head and tail)."""
    H, W = size
    color, depth = CS.frames(H, W, 4)
    depth = depth.copy()
    depth[0] = 0
    depth[1, -1, -1] = 65535
    depth[2, 0, 0] = 40000
    rows = np.stack([R.row((0, 0, 0), 0, 0, b, 0, (0, 2, 3, 0)[b], (0, 5, 3, 0)[b], b) for b in range(4)])
    got = run(gpu, color, depth, rows)
    want = R.augment_frames(color, depth, rows, CS.SEED, depth_norm=0)
    assert np.isnan(want[1][0]).all() and np.isnan(got[1][0]).all()
    assert_bits("data", got[0], want[0])
    assert_bits("data_p", got[1], want[1])


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


@pytest.mark.parametrize("channels", [3, 4])
def test_memory_contract(gpu, channels):
    """Guard bands around both outputs, the workspace and the inputs, both poison patterns: identical results (every
    element is written), guards and inputs intact. 35 x 131: partial tiles on both edges, W % 4 != 0; 20 x 72: the
    float4 path with a partial tile."""
    import torch
    from posecnn_amd import ops
    for H, W in ((35, 131), (20, 72)):
        color, depth = CS.frames(H, W, 4, channels)
        rows = np.stack([R.row(CS.JITTER, b, (0, 3.0, 15, 11)[b], b, 1, 3 - b, (7, 9, 2.0, 0)[b], 20 + b) for b in range(4)])
        runs, calls = {}, set()
        for p in memguard.PATTERNS:
            with guarded(p) as (g, rec):
                c = g.embed(color, "cuda")
                d = g.embed(depth, "cuda")
                data, data_p = ops.augment_frames(c, d, rows, CS.SEED)
                torch.cuda.synchronize()
                g.check()
                assert sum(a.kind == "empty" for a in g.arenas) == 3            # data, data_p, workspace
                runs[p] = {"data": memguard.to_numpy(data), "data_p": memguard.to_numpy(data_p)}
                calls |= set(rec.calls)
        memguard.compare_patterns(runs)
        assert {"pcnn_augment_frames_workspace_bytes", "pcnn_augment_frames_fwd"} <= calls
        want = R.augment_frames(color, depth, rows, CS.SEED)
        exact = np.array([True, False, True, True]), np.array([True, True, False, True])
        for k, w, e in zip(("data", "data_p"), want, exact):
            assert_bits(k, runs["P1"][k][e], w[e])


# ---- feed -------------------------------------------------------------------------------------------------------------------
def test_feed_with_a_sampler(gpu):
    """The two-object scene of tests/synth_cases.py rendered at 160 x 208: feed(augment=sampler) carries the blobs of
    ops.augment_frames on batch.color with the sampler's rows; feed(augment=None) is today's; one training step on the
    augmented feed returns finite losses."""
    import torch
    import synth_cases as C
    from posecnn_amd import config, ops, synth, synthesize as syn, train
    from posecnn_amd.augment import AugmentSampler
    from posecnn_amd.networks import vgg16_convs
    H, W = 160, 208
    K = C.intrinsics(H, W)
    scenes, lights = C.main_scenes()
    bank = syn.MeshBank(C.bank_meshes(K), C.CLASSES, device=gpu)
    bg = torch.from_numpy(C.backgrounds(1, H, W)).to(gpu)
    batch = syn.render_scenes(bank, [syn.Scene(scenes[0], lights[0])], K, H, W, bg, (C.Z_NEAR, C.Z_FAR), 1000.0, 100, False)
    assert len(batch.scenes[0].instances) == 2
    points = synth.make_model_points(22, 64)
    args = (config.LOV_EXTENTS, points, config.LOV_SYMMETRY)

    plain = batch.feed(*args, rgbd=True)
    assert plain["data"].dtype == torch.uint8 and torch.equal(plain["data"], batch.color[..., :3]) and plain["data_p"] is batch.depth
    assert not hasattr(batch, "augment_rows")

    feed = batch.feed(*args, rgbd=True, augment=AugmentSampler(seed=5))
    rows = batch.augment_rows
    assert np.array_equal(rows, AugmentSampler(seed=5).sample(1))
    data, data_p = ops.augment_frames(batch.color, batch.depth, rows, 5)
    assert feed["data"].dtype == torch.float32 and torch.equal(feed["data"], data) and torch.equal(feed["data_p"], data_p)
    want = R.augment_frames(batch.color.cpu().numpy(), memguard.to_numpy(batch.depth), rows, 5, use64=True)
    for g, w in zip((data, data_p), want):
        assert np.abs(g.cpu().numpy().astype(np.float64) - w).max() <= 4 * CS.gauss_tolerance()
    assert sorted(feed) == sorted(plain)
    for k in plain:
        if k not in ("data", "data_p"):
            same = torch.equal(feed[k], plain[k]) if isinstance(plain[k], torch.Tensor) else feed[k] == plain[k]
            assert same, k
    colour_only = batch.feed(*args, augment=AugmentSampler(seed=5))
    assert "data_p" not in colour_only and torch.equal(colour_only["data"], data)

    torch.manual_seed(0)
    net = vgg16_convs("COLOR", 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=True, is_train=True,
                      device=gpu, seed=3, init="he")

    class Cfg(train.TrainConfig):
        LEARNING_RATE = 1e-6

    losses = train.SolverWrapper(net, Cfg).train_step(colour_only)
    for k in ("loss", "loss_cls", "loss_vertex", "loss_pose", "loss_regu"):
        assert np.isfinite(losses[k]), (k, losses)
