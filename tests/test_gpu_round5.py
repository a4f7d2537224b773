"""GPU tests added in round 5 (VERDICT r4 "Next" #1, #7):
  * the mode the headline is measured in — THREE HIP streams, 16 RGB-D frames of 480x640, the fused first-layers
    kernel (138 KB of LDS, one workgroup per CU) co-resident with other batches' kernels — against the serial run,
    bit for bit, 24 batches (rows, fc7, poses_tanh, loss_pose);
  * `bench.py` itself: `outputs_equal_serial` is true on a short --full run; a plain run times K steps and dumps its last one;
  * the multi-rank path rehearsed on one GPU: two ranks under the real launcher, both computing on cuda:0, gloo
    carrying the detection block (RCCL refuses duplicate devices) — real kernels, real shard offsets, `ranks_seen == 2`.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from posecnn_amd import config, synth
from test_gpu_ops import N, T, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _rgbd_batch(g, B, H, W):
    import torch
    im = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).float()
    data = (im - torch.from_numpy(config.PIXEL_MEANS)).float().contiguous()
    depth = torch.randint(0, 3000, (B, H, W, 1), generator=g).float()
    d = (torch.clamp(depth / 2000.0, 0, 1) * 255).expand(B, H, W, 3)
    return data, (d - torch.from_numpy(config.PIXEL_MEANS)).float().contiguous()


def test_three_streams_full_size_batches_equal_the_serial_run(gpu):
    """bench.py's default since round 4 (`--streams 3`, batch 16, 480x640 RGB-D, train-mode Hough, fused conv1_1 ->
    conv1_2 -> pool1): consecutive batches on three alternating HIP streams must reproduce the one-stream run bit
    for bit. The reference has one frame in flight (lib/fcn/test.py:1867-1888), so there is exactly one right answer
    per batch. 4 distinct batches x 6 rounds = 24 batches in flight three at a time; every tensor of the pose branch
    that round 3's LDS-ring race corrupted (fc7 rows, a flipped quaternion) is compared, plus the detection rows
    (labels -> Hough -> RoI pooling) and the scalar pose loss (all 9 x count rows)."""
    import torch
    from posecnn_amd import fcn
    from posecnn_amd.networks import vgg16_convs
    B, H, W, C = 16, 480, 640, 22
    net = vgg16_convs("RGBD", C, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=False,
                      is_train=True, seed=3, init="he", with_losses=False, device=gpu)
    synth.init_calibrated(net)
    assert net.fused_conv12, "the headline runs on the fused first-layers kernel"
    K = config.DEMO_INTRINSICS.copy()
    pts = T(gpu, synth.make_model_points(C, config.NUM_MODEL_POINTS, extents=config.LOV_EXTENTS))
    g = torch.Generator(device="cpu").manual_seed(77)
    batches = []
    for i in range(4):
        data, data_p = _rgbd_batch(g, B, H, W)
        planted_np, scenes = synth.make_planted_batch(700 + i * B, B, H=H, W=W, K=K, C=C, extents=config.LOV_EXTENTS)
        batches.append((data.to(gpu), data_p.to(gpu), {k: T(gpu, v) for k, v in planted_np.items()},
                        T(gpu, synth.make_gt_poses(scenes, K, seed=i))))

    def one(b):
        det = fcn.im_segment_batch(net, b[0], K, config.LOV_EXTENTS, pts, config.LOV_SYMMETRY, data_p=b[1], planted=b[2],
                                   with_losses=True, gt_poses=b[3])
        # (rows past 9 x count of fc7 / poses_tanh are not defined — dead_rows="keep" — and are not compared below)
        return (det.rows.clone(), det.count.clone(), net.get_output("loss_pose").clone(), net.get_output("fc7").clone(),
                net.get_output("poses_tanh").clone(), net.get_output("label_2d").clone())

    with torch.no_grad():
        serial = []
        for b in batches:
            serial.append(one(b))
            torch.cuda.synchronize()              # one batch in flight, the device idle in between
        streams = [torch.cuda.current_stream(gpu), torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)]
        got = []
        for rep in range(6):
            for i, b in enumerate(batches):
                with torch.cuda.stream(streams[(rep * len(batches) + i) % 3]):
                    got.append(one(b))
        torch.cuda.synchronize()
    assert len(got) == 24
    for j, (rows, count, loss, fc7, ptanh, lab) in enumerate(got):
        want = serial[j % len(batches)]
        n = int(count)
        assert n == int(want[1]) and n >= 3 * B, "batch %d: %d detections" % (j, n)
        live = 9 * n
        same(N(lab), N(want[5]), "label_2d of batch %d" % j)
        same(N(rows), N(want[0]), "rows of batch %d" % j)
        same(N(loss).reshape(-1), N(want[2]).reshape(-1), "loss_pose of batch %d" % j)
        same(N(fc7[:live]), N(want[3][:live]), "fc7 of batch %d" % j)
        same(N(ptanh[:live]), N(want[4][:live]), "poses_tanh of batch %d" % j)


def _env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    return env


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_bench_reports_outputs_equal_serial(gpu):
    """`bench.py` (three streams) holds its own timed run to a serial re-run of the same batches and says so in the
    JSON line; a short run of the real configuration."""
    r = subprocess.run([sys.executable, BENCH, "--full", "--steps", "6", "--warmup", "2", "--prewarm-seconds", "0", "--no-cpu-baseline",
                        "--no-secondary"], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = _json_line(r.stdout)
    assert out["outputs_equal_serial"] is True, out["outputs_equal_serial_detail"]
    d = out["outputs_equal_serial_detail"]
    assert d["batches_compared"] == 6 and d["mismatches"] == 0 and min(d["rows_per_batch"]) > 0
    assert "3 HIP streams" in out["step_submission"]
    # round 6: the spread of the timed region and the per-rank block travel with every --full line (--repeats defaults to 5)
    assert out["repeats"] == 5 and len(out["value_all"]) == 5 and abs(out["value_all"][0] - out["value"]) < 0.01
    assert out["value_min"] <= out["value_median"] <= out["value_max"] and out["value_min"] > 0.8 * out["value_max"]
    pr = out["per_rank"]
    assert pr["ranks"] == 1 and abs(pr["ms_per_step_by_rank"][0] - out["ms_per_step"]) < 0.05 * out["ms_per_step"] and pr["h2d_GBps_per_rank"][0] > 1.0
    # the Hough counters are this build's (source-hash gate) and say what bounds the vote kernel: its vector ALUs
    assert out["roofline"]["traffic"] and 0.5 < out["roofline"]["valu_active_share"] < 1.3


def test_plain_bench_run_is_the_headline_and_dumps_its_last_step(gpu, tmp_path):
    """`bench.py` without --full: K timed steps and the headline fields, none of the --full measurements; --dump-outputs
    writes the last timed step's outputs in float32, and a second process with the same arguments writes the same bits."""
    dumped = []
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-seconds", "0",
                            "--dump-outputs", str(d)], env=_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = _json_line(r.stdout)
        assert out["steps"] == 3 and out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert "frames/sec" in out["metric"] and abs(out["value"] - 16 * 1000.0 / out["ms_per_step"]) < 1e-6 * out["value"]
        assert not {"value_cold", "repeats", "outputs_equal_serial", "roofline", "kernels_us", "secondary", "cpu_baseline"} & set(out)
        files = {f[:-4]: np.load(str(d / f)) for f in os.listdir(str(d)) if f.endswith(".npy")}
        assert set(files) == {"detections", "rois", "poses", "labels"}
        assert all(a.dtype == np.float32 for a in files.values())
        assert sum(os.path.getsize(str(d / f)) for f in os.listdir(str(d))) <= 64 << 20
        assert files["labels"].shape == (16, 480, 640) and files["labels"].max() > 0
        assert files["rois"].shape[0] > 0 and files["rois"].shape == files["poses"].shape and files["detections"].shape[1] == 14
        dumped.append(files)
    for name in dumped[0]:
        assert np.array_equal(dumped[0][name], dumped[1][name]), name


def test_two_ranks_on_one_gpu_through_the_real_launcher(gpu):
    """The multi-rank path without an 8-GPU node: `python bench.py --gpus 2` self-spawns two ranks under
    torch.distributed.run; with --shared-device both compute on cuda:0 (three streams each) and gloo carries the packed
    detection block. Everything except the transport is the real thing: kernels, per-rank shard offsets (global frame
    indices rank * B + i), barrier + MAX-over-ranks timing, one gather per step. Rank 0 must see both ranks' frames and
    twice one rank's detections. (the partitioning follows the reference's independent per-image loop,
    lib/hough_voting_gpu_layer/hough_voting_gpu_op.cc:369-377.)"""
    r = subprocess.run([sys.executable, BENCH, "--full", "--gpus", "2", "--backend", "gloo", "--shared-device", "--steps", "4", "--warmup", "2",
                        "--prewarm-seconds", "0", "--no-cpu-baseline", "--no-secondary"],
                       env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = _json_line(r.stdout)
    pg = out["process_group"]
    assert out["n_gpus"] == 2 and pg["world_size"] == 2 and pg["backend"] == "gloo" and pg["shared_device"] is True
    assert pg["ranks_seen"] == 2
    assert out["config"]["global_batch"] == 32 and out["config"]["per_gpu_batch"] == 16
    assert out["outputs_equal_serial"] is True, out["outputs_equal_serial_detail"]
    assert out["config"]["detections_per_step"] >= 2 * 3 * 16    # both ranks' frames carry their planted objects
    assert pg["all_gather_us"] is not None and pg["all_gather_us"] > 0
    assert out["per_rank"]["ranks"] == 2 and len(out["per_rank"]["ms_per_step_by_rank"]) == 2 and len(out["per_rank"]["h2d_GBps_per_rank"]) == 2
    assert out["per_rank"]["ms_per_step_max"] <= out["ms_per_step"] * 1.02    # the contract's MAX over ranks (taken after the barrier) bounds them


def test_head_lowres_mfma_equals_the_op_sequence_it_replaces(gpu):
    """csrc/heads_small.hip head_lowres_mfma_kernel (what `vgg16_convs` launches per head from a few frames on: vgg16_convs.py:128-142,
    :151-163 in the fused-heads form): add_score = score_conv4 + deconv(4,2)(score_conv5) [+ planted] must carry the bits of
    pcnn_deconv_bilinear_fwd + two framework adds (and of the few-frame kernel head_lowres); the 1x1 product, now on the
    matrix cores, is checked against float64. Shapes: the two heads at 16 frames' scale, a pixel count that is no multiple
    of the 64-pixel workgroup, 93 outputs (6 column tiles, the last one ragged), 5 outputs (one ragged tile)."""
    import torch
    from posecnn_amd import ops
    F = np.float32
    rng = np.random.default_rng(21)
    for (B, h, w, U, Cout, plant) in ((4, 60, 80, 64, 22, True), (2, 60, 80, 128, 66, False), (3, 6, 10, 64, 5, True), (1, 2, 2, 16, 3, False),
                                      (1, 12, 16, 128, 93, True)):
        a = T(gpu, rng.standard_normal((B, h, w, U)).astype(F))
        b5 = T(gpu, rng.standard_normal((B, h // 2, w // 2, U)).astype(F))
        pl = T(gpu, rng.standard_normal((B, h, w, U)).astype(F)) if plant else None
        wt = T(gpu, (rng.standard_normal((U, Cout)) / U ** 0.5).astype(F))
        add, z = ops.head_lowres_mfma(a, b5, ops.head_lowres_mfma_filter(wt), Cout, planted=pl)
        want = a + ops.deconv_bilinear(b5, 4, 2)
        if plant:
            want = want + pl
        same(N(add), N(want), "add_score %s" % ((B, h, w, U),))
        if 4 * (32 * U + U * Cout) <= 60 * 1024:
            add_v, z_v = ops.head_lowres(a, b5, wt, planted=pl)
            same(N(add), N(add_v), "add_score vs the few-frame kernel")
            assert float((z - z_v).abs().max()) < 1e-5 * max(1.0, float(z_v.abs().max()))
        zr = want.double().reshape(-1, U) @ wt.double()
        assert float((z.double().reshape(-1, Cout) - zr).abs().max()) < 1e-5 * max(1.0, float(zr.abs().max()))
    with pytest.raises(Exception):
        ops.head_lowres_mfma(a, b5, ops.head_lowres_mfma_filter(wt)[:16], Cout)          # filter rows != ceil(Cout / 16) * 16


def test_fc_rows_cols_is_fc8_and_tanh_in_one_launch(gpu):
    """pcnn_fc_rows_cols_fwd (`Network.fc_tanh` at more rows than the skinny kernel takes: fc8 4096 -> 4 C = 88 and
    poses_tanh, lib/networks/vgg16_convs.py:192-193): the row kernel on a zero-padded filter, only the 88 real columns
    stored, tanh in the epilogue, rows at or past the device-side count zero. Against float64."""
    import torch
    from posecnn_amd import ops
    g = torch.Generator(device="cpu").manual_seed(5)
    for (M, K, N_, cnt) in ((300, 4096, 88, 131), (64, 256, 56, 64), (130, 128, 4, 1), (70, 512, 128, 0)):
        x = torch.randn((M, K), generator=g).to(gpu)
        w = (torch.randn((N_, K), generator=g) / K ** 0.5).to(gpu)
        b = torch.randn((N_,), generator=g).to(gpu)
        npad = (N_ + 63) // 64 * 64
        wp = torch.zeros((npad, K), device=gpu); wp[:N_] = w
        bp = torch.zeros((npad,), device=gpu); bp[:N_] = b
        count = torch.tensor([cnt], dtype=torch.int32, device=gpu)
        y, t = ops.fc_rows_cols(x, wp, bp, N_, "tanh", num_rows=count)
        ref = x.double() @ w.double().t() + b.double()
        assert tuple(y.shape) == (M, N_) and tuple(t.shape) == (M, N_)
        assert float((y[:cnt].double() - ref[:cnt]).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())) if cnt else True
        assert float((t[:cnt].double() - torch.tanh(y[:cnt].double())).abs().max()) < 1e-6 if cnt else True   # tanh of ITS OWN linear output
        assert not bool(y[cnt:].any()) and not bool(t[cnt:].any())
        yr = ops.fc_rows_cols(x, wp, bp, N_, "relu", num_rows=count)
        assert float((yr[:cnt].double() - torch.relu(ref[:cnt])).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())) if cnt else True
    with pytest.raises(Exception):
        ops.fc_rows_cols(x, wp, bp, 30, "none")        # 30 is no multiple of 4


def test_pose_l2_normalize_and_the_packed_detection_block(gpu):
    """Two launches that replace ten framework ones per step: poses_pred = l2_normalize(poses_tanh * poses_weight, dim 1)
    (vgg16_convs.py:195-197) and the all-gather block of posecnn_amd/dist.py::pack_detections written by det_assemble."""
    import torch
    from posecnn_amd import dist as pdist, ops
    rng = np.random.default_rng(8)
    F = np.float32
    for (R, C, cnt) in ((45, 22, 30), (9, 14, 9), (200, 64, 0)):
        x = T(gpu, np.tanh(rng.standard_normal((R, 4 * C))).astype(F))
        w = np.zeros((R, 4 * C), F)
        for r in range(R):
            if r % 3:
                c = int(rng.integers(1, C)); w[r, 4 * c:4 * c + 4] = 1
        w = T(gpu, w)
        count = torch.tensor([cnt], dtype=torch.int32, device=gpu)
        got = ops.pose_l2_normalize(x, w, num_rows=count)
        mul = (x * w).double()
        want = mul * torch.rsqrt(torch.clamp((mul * mul).sum(dim=1, keepdim=True), min=1e-12))
        assert float((got[:cnt].double() - want[:cnt]).abs().max()) < 3e-7 if cnt else True
        assert not bool(got[cnt:].any())
    # the packed block
    C, R, n = 22, 27, 18
    rois = rng.standard_normal((R, 7)).astype(F)
    rois[:, 0] = rng.integers(0, 16, R)
    rois[:, 1] = rng.integers(0, C, R)
    pt = np.tanh(rng.standard_normal((R, 4 * C))).astype(F)
    tp = rng.standard_normal((R, 7)).astype(F)
    count = torch.tensor([n], dtype=torch.int32, device=gpu)
    for stride in (1, 9):
        rows0, c0 = ops.det_assemble(T(gpu, rois), T(gpu, pt), T(gpu, tp), count, row_stride=stride)
        for off in (0, 48):
            rows, c1, block = ops.det_assemble(T(gpu, rois), T(gpu, pt), T(gpu, tp), count, row_stride=stride, frame_offset=off)
            want = pdist.pack_detections(rows0, c0, off)
            same(N(block), N(want), "packed block, stride %d offset %d" % (stride, off))
            assert int(c1) == int(c0) and rows.data_ptr() == block.data_ptr()


def test_merged_head_convs_equal_the_separate_products(gpu):
    """COLOR networks run `score_conv5` + `score_conv5_vertex` (both on conv5_3) and `score_conv4` + `score_conv4_vertex` (both on
    conv4_3; vgg16_convs.py:128-133,151-157) as one product per source (pcnn_fc_rows_split_fwd): every layer downstream must carry
    the bits of the four separate launches."""
    import torch
    from posecnn_amd import fcn
    from posecnn_amd.networks import vgg16_convs
    C, H, W = 22, 96, 128
    rng = np.random.default_rng(4)
    K = config.DEMO_INTRINSICS.copy(); K[:2] *= W / 640.0
    pts = synth.make_model_points(C, 32)
    outs = []
    for merge in (True, False):
        net = vgg16_convs("COLOR", C, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=False, is_train=False,
                          seed=3, init="he", with_losses=False, device=gpu)
        synth.init_calibrated(net)
        net.merge_head_convs = merge
        data = T(gpu, (np.random.default_rng(9).integers(0, 256, (2, H, W, 3)).astype(np.float32) - config.PIXEL_MEANS).astype(np.float32))
        feed = fcn._feed(net, data, None, K, config.LOV_EXTENTS, pts, config.LOV_SYMMETRY, C, gpu)
        planted_np, _ = synth.make_planted_batch(3, 2, H=H, W=W, K=K, C=C, n_obj=2)
        with torch.no_grad():
            net.run(feed, planted={k: T(gpu, v) for k, v in planted_np.items()})
        outs.append({n: N(net.get_output(n)) for n in ("score_conv5", "score_conv4", "score_conv5_vertex", "score_conv4_vertex", "add_score",
                                                      "add_score_vertex", "label_2d", "vertex_pred_lowres", "rois", "poses_tanh")})
    for n in outs[0]:
        same(outs[0][n], outs[1][n], n)


@pytest.mark.parametrize("shape,k,s", [((2, 30, 40, 22), 16, 8), ((1, 7, 9, 22), 16, 8), ((1, 5, 21, 40), 16, 8), ((1, 6, 7, 3), 16, 8),
                                       ((1, 9, 5, 14), 4, 2)])
def test_hard_label_from_the_label_heads_launch_equals_the_op(gpu, shape, k, s):
    """pcnn_upscore_softmax_argmax_hard_fwd: the Hardlabel op (hard_label_op_gpu.cu.cc:17-29) evaluated on the probabilities
    while they are still in LDS. Same bits as the op run on the prob tensor afterwards and as the CPU checker, for the
    compile-time class counts (22, 14), the generic kernels (40 -> <64>, 3 -> <24>), a ragged last segment (21 * 8 = 168
    columns = 128 + 40), ground-truth labels -1 (no label), 0 (background: hot only below the threshold), out of range
    (ignored); prob / score / label themselves unchanged by the extra output; prob not requested at all."""
    import torch
    from posecnn_amd import ops
    import oracle
    B, H, W, C = shape
    rng = np.random.default_rng(31)
    z = (rng.standard_normal(shape) * 2).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    gt = rng.integers(-1, C, (B, H * s, W * s)).astype(np.int32)
    gt[rng.random(gt.shape) < 0.4] = 0           # plenty of background pixels: the prob[0] < threshold branch
    gt[0, 0, :3] = [C, C + 5, -7]                # out of range: no channel is set
    for thr in (1.0 / C, 0.5, 1.5):              # below / around / above every probability
        score, prob, label, hard = ops.upscore_softmax_argmax(T(gpu, z), T(gpu, bias), k, s, relu=True, want_score=True,
                                                              hard_gt=T(gpu, gt), hard_threshold=thr)
        s0, p0, l0 = ops.upscore_softmax_argmax(T(gpu, z), T(gpu, bias), k, s, relu=True, want_score=True)
        same(N(score), N(s0), "score"); same(N(prob), N(p0), "prob"); same(N(label), N(l0), "label")
        want = ops.hard_label(p0, T(gpu, gt), thr)
        same(N(hard), N(want), "hard label (fused vs op) thr=%g" % thr)
        same(N(hard), oracle.hard_label(N(p0), gt, thr), "hard label (fused vs CPU checker) thr=%g" % thr)
        in_range = (gt >= 0) & (gt < C)
        assert np.array_equal(N(hard).sum(-1) > 0, in_range & ((gt > 0) | (np.take_along_axis(N(p0), np.clip(gt, 0, C - 1)[..., None], -1)[..., 0] < thr)))
        _, p1, l1, h1 = ops.upscore_softmax_argmax(T(gpu, z), T(gpu, bias), k, s, relu=True, want_prob=False, hard_gt=T(gpu, gt),
                                                   hard_threshold=thr)
        assert p1 is None
        same(N(h1), N(want), "hard label without the prob output"); same(N(l1), N(l0), "label")
    with pytest.raises(Exception, match="threshold"):
        ops.upscore_softmax_argmax(T(gpu, z), T(gpu, bias), k, s, hard_gt=T(gpu, gt), hard_threshold=0.0)


def test_pipeline_takes_gt_label_weight_from_the_label_head(gpu):
    """fcn.im_segment_batch(with_losses=True): `gt_label_weight` (vgg16_convs.py:148-149) comes out of the label head's launch —
    on a graph built with the loss layers and on one built without them — and equals the Hardlabel op on prob_normalized."""
    import torch
    from posecnn_amd import fcn, ops, _lib
    from posecnn_amd.networks import vgg16_convs
    C, B, H, W = 22, 2, 96, 128
    K = config.DEMO_INTRINSICS.copy(); K[:2] *= W / 640.0
    pts = synth.make_model_points(C, 32)
    g = torch.Generator().manual_seed(5)
    data, data_p = _rgbd_batch(g, B, H, W)
    planted_np, scenes = synth.make_planted_batch(7, B, H=H, W=W, K=K, C=C, n_obj=2)
    gtp = synth.make_gt_poses(scenes, K, seed=3)
    for graph_losses in (True, False):
        net = vgg16_convs("RGBD", C, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=False, is_train=True,
                          seed=3, init="he", with_losses=graph_losses, device=gpu)
        synth.init_calibrated(net)
        _lib.profile_enable(True)
        with torch.no_grad():
            fcn.im_segment_batch(net, T(gpu, data.numpy()), K, config.LOV_EXTENTS, pts, config.LOV_SYMMETRY, data_p=T(gpu, data_p.numpy()),
                                 planted={k: T(gpu, v) for k, v in planted_np.items()}, with_losses=True, gt_poses=T(gpu, gtp))
        torch.cuda.synchronize()
        rep = _lib.profile_report(); _lib.profile_enable(False)
        assert not any(k.startswith("hard_label") for k in rep), sorted(rep)   # no separate launch
        hard = net.get_output("gt_label_weight")
        want = ops.hard_label(net.get_output("prob_normalized"), net.get_output("gt_label_2d"), net.threshold_label)
        same(N(hard), N(want), "gt_label_weight")
        assert float(hard.sum()) > 0
