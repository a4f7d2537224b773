"""CPU checks of the training feed's vertex targets: the numpy restatement (tests/vertex_ref.py) against recorded outputs
of the reference's `_generate_vertex_targets` (tests/golden/vertex_targets.npz, written by
tests/golden/make_vertex_targets_golden.py), `datasets.training_blobs` on a YCB-Video tree written here, and the host-side argument checks of the entries of
include/posecnn_hip_train.h (nothing is launched)."""
import ctypes
import os

import numpy as np
import pytest

import vertex_ref
from posecnn_amd import config, datasets, pose_error

F = np.float32


# ---- the reference pin ---------------------------------------------------------------------------------------------
def test_golden_covers_the_cases_it_is_there_for():
    cases = {c["name"]: c for c in vertex_ref.golden_cases()}
    assert len(cases) >= 6
    for c in cases.values():
        assert c["label"].shape[0] <= 96 and c["label"].shape[1] <= 128
        assert c["targets"].dtype == F and c["weights"].dtype == F and c["weights"].any()
    c = cases["several_classes"]
    assert len(np.unique(c["label"][c["label"] > 0])) >= 4
    c = cases["label_without_object"]       # class 4 is painted, has no object, gets no weight
    assert (c["label"] == 4).any() and 4 not in c["cls_indexes"] and not c["weights"][c["label"] == 4].any()
    c = cases["object_without_label"]
    assert 3 in c["cls_indexes"] and not (c["label"] == 3).any()
    c = cases["centre_outside"]
    assert (c["center"][:, 0] < 0).any() and (c["center"][:, 0] >= c["label"].shape[1]).any()
    c = cases["pixel_on_centre"]
    for cls, (cx, cy) in zip(c["cls_indexes"], c["center"]):
        cls, cx, cy = int(cls), int(cx), int(cy)
        assert c["label"][cy, cx] == cls and c["weights"][cy, cx, 3 * cls] == 10
        assert c["targets"][cy, cx, 3 * cls] == 0 and c["targets"][cy, cx, 3 * cls + 1] == 0
    c = cases["two_class_multi_instance"]
    assert c["multi"] == 1 and c["num_classes"] == 2 and len(c["cls_indexes"]) == 3 and c["mask"].max() == 5


@pytest.mark.parametrize("case", vertex_ref.golden_cases(), ids=lambda c: c["name"])
def test_restatement_equals_the_reference_bit_for_bit(case):
    inst = None if case["instance"] is None else case["instance"][None]
    targets, weights = vertex_ref.vertex_targets(case["label"][None], case["objects"][None], case["num_classes"], inst)
    assert vertex_ref.same_bits(targets[0], case["targets"])
    assert vertex_ref.same_bits(weights[0], case["weights"])


def test_restatement_takes_the_highest_matching_row_and_ignores_dead_ones():
    label = np.zeros((1, 8, 8), np.int32)
    label[0, 2:6, 2:6] = 3
    label[0, 7, 7] = 9                                           # >= C: no channels of its own
    obj = np.array([[[3, 0, 1.5, 2.5, 0.1, 10], [0, 0, 9, 9, 9, 9], [3, 0, 6.5, 1.5, 0.2, 5], [-1, 0, 4, 4, 4, 4]]], F)
    t, w = vertex_ref.vertex_targets(label, obj, 5)
    assert (w[0, 2:6, 2:6, 9:12] == 5).all() and (t[0, 2:6, 2:6, 11] == F(0.2)).all()
    assert w.sum() == 5 * 3 * 16
    t0, w0 = vertex_ref.vertex_targets(label, obj[:, :0], 5)   # M = 0
    assert not t0.any() and not w0.any()


# ---- datasets.training_blobs ---------------------------------------------------------------------------------------
def write_tree(root, rng, H=40, W=52):
    """Two frames, three / two objects, rotations and fractional centres; H, W are not multiples of 16."""
    import scipy.io
    from PIL import Image
    os.makedirs(os.path.join(root, "data", "0007"))
    np.savetxt(os.path.join(root, "extents.txt"), config.LOV_EXTENTS[1:], fmt="%.6f")
    frames, idx = [], []
    for f, classes in enumerate(((2, 11, 21), (5, 11))):
        name = "0007/%06d" % (f + 1)
        idx.append(name)
        label = np.zeros((H, W), np.uint8)
        yy, xx = np.mgrid[0:H, 0:W]
        n = len(classes)
        center = np.stack([rng.uniform(5, W - 5, n), rng.uniform(5, H - 5, n)], axis=1)
        poses = np.zeros((3, 4, n))
        for j, cls in enumerate(classes):
            label[(xx - center[j, 0]) ** 2 + (yy - center[j, 1]) ** 2 <= 36] = cls
            poses[:, :3, j] = pose_error.quat2mat(rng.standard_normal(4))
            poses[:, 3, j] = (rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.5, 1.5))
        for what, im in (("color", rng.integers(0, 256, (H, W, 3), dtype=np.uint8)),
                         ("depth", rng.integers(0, 30000, (H, W)).astype(np.uint16)), ("label", label)):
            Image.fromarray(im).save(os.path.join(root, "data", "%s-%s.png" % (name, what)))
        meta = {"intrinsic_matrix": config.DEMO_INTRINSICS, "factor_depth": np.array([[10000]]), "poses": poses,
                "cls_indexes": np.array(classes).reshape(-1, 1), "center": center}
        scipy.io.savemat(os.path.join(root, "data", name + "-meta.mat"), meta)
        frames.append(dict(label=label, classes=classes, center=center, poses=poses))
    with open(os.path.join(root, "keyframe.txt"), "w") as fh:
        fh.write("\n".join(idx) + "\n")
    return frames


@pytest.mark.parametrize("im_scale", [1.0, 0.5])
def test_training_blobs_on_a_synthetic_tree(tmp_path, im_scale):
    raw = write_tree(str(tmp_path), np.random.default_rng(11))
    ds = datasets.YCBVideo(str(tmp_path), "keyframe")
    blobs = datasets.training_blobs([ds.frame(i) for i in range(len(ds))], ds.num_classes, im_scale=im_scale, w_inside=10.0)
    Hp, Wp = int(48 * im_scale), int(64 * im_scale)                               # 40 x 52 padded to a multiple of 16
    label, obj = blobs["gt_label_2d"], blobs["vertex_objects"]
    assert label.shape == (2, Hp, Wp) and label.dtype == np.int32
    assert obj.shape == (2, 3, 6) and obj.dtype == F and not obj[1, 2].any()      # frame 1 has two objects: a zero row
    assert "vertex_instance" not in blobs
    assert blobs["meta_data"].shape == (2, 1, 1, 48) and blobs["meta_data"].dtype == F
    for b, fr in enumerate(raw):
        assert np.array_equal(blobs["meta_data"][b, 0, 0], config.make_meta_data(config.DEMO_INTRINSICS, im_scale))
        if im_scale == 1.0:
            assert np.array_equal(label[b, :40, :52], fr["label"]) and not label[b, 40:].any() and not label[b, :, 52:].any()
        else:
            assert np.array_equal(label[b, :20, :26], fr["label"][::2, ::2])      # nearest: every second pixel
        # the table says what the raw meta says
        want = vertex_ref.object_table(np.array(fr["classes"]), fr["center"], fr["poses"], 10.0, im_scale)
        got_t, got_w = vertex_ref.vertex_targets(label[b:b + 1], obj[b:b + 1], ds.num_classes)
        ref_t, ref_w = vertex_ref.vertex_targets(label[b:b + 1], want[None], ds.num_classes)
        assert vertex_ref.same_bits(got_t, ref_t) and vertex_ref.same_bits(got_w, ref_w) and ref_w.any()
    # pose blob: (frame, cls, 0 x 4, unit quaternion that reproduces R, T)
    poses = blobs["poses"]
    assert poses.shape == (5, 13) and poses.dtype == F
    rows = [(b, j) for b, fr in enumerate(raw) for j in range(len(fr["classes"]))]
    for row, (b, j) in zip(poses, rows):
        assert row[0] == b and row[1] == raw[b]["classes"][j] and not row[2:6].any()
        q = row[6:10].astype(np.float64)
        assert abs(np.linalg.norm(q) - 1) < 1e-6
        assert np.abs(pose_error.quat2mat(q) - raw[b]["poses"][:, :3, j]).max() < 1e-6
        assert np.array_equal(row[10:], raw[b]["poses"][:, 3, j].astype(F))


def test_training_blobs_two_class_multi_instance_equals_the_reference():
    """The frame of the golden two-class case, handed over as a dataset frame: cls_index + mask."""
    c = next(c for c in vertex_ref.golden_cases() if c["multi"])
    full_cls = np.zeros(int(c["mask"].max()))                    # five objects; the kept class sits at cls_indexes_old
    full_cls[:] = 1
    full_cls[c["cls_indexes_old"]] = 6
    n = len(full_cls)
    center, poses = np.zeros((n, 2)), np.zeros((3, 4, n))
    poses[2, 3, :] = 1.0
    center[c["cls_indexes_old"]], poses[:, :, c["cls_indexes_old"]] = c["center"], c["poses"]
    label6 = c["label"] * 6
    frame = {"label": label6, "mask": c["mask"], "cls_index": 6,
             "meta": {"cls_indexes": full_cls, "center": center, "poses": poses, "intrinsic_matrix": config.DEMO_INTRINSICS}}
    blobs = datasets.training_blobs([frame], 2)
    assert np.array_equal(blobs["gt_label_2d"][0], c["label"]) and blobs["vertex_objects"].shape == (1, 3, 6)
    assert np.array_equal(blobs["vertex_objects"][0, :, 1], c["cls_indexes_old"] + 1)
    t, w = vertex_ref.vertex_targets(blobs["gt_label_2d"], blobs["vertex_objects"], 2, blobs["vertex_instance"])
    assert vertex_ref.same_bits(t[0], c["targets"]) and vertex_ref.same_bits(w[0], c["weights"])
    with pytest.raises(ValueError, match="repeats a class"):
        datasets.training_blobs([dict(frame, cls_index=0)], 22)
    with pytest.raises(ValueError, match="no 'mask'"):
        datasets.training_blobs([dict(frame, mask=None)], 2)


# ---- the C boundary ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from posecnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_argument_validation_happens_on_the_host(L):
    """Every call here returns before anything is launched: the pointers are host addresses that are never read."""
    from posecnn_amd import _lib
    buf = ctypes.create_string_buffer(1 << 14)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    n = ctypes.c_size_t(0)
    assert L.pcnn_smooth_l1_vertex_workspace_bytes(ctypes.byref(n)) == 0 and 0 < n.value <= 1 << 13
    tg = lambda C, M: L.pcnn_vertex_targets_fwd(p, None, p, 1, 4, 4, C, M, p, p, None)
    fw = lambda C, M, sigma, ws=n.value: L.pcnn_smooth_l1_vertex_gt_fwd(p, p, None, p, 1, 4, 4, C, M, sigma, p, p, ws, None)
    bw = lambda C, M, sigma: L.pcnn_smooth_l1_vertex_gt_bwd(p, p, None, p, p, None, 1, 4, 4, C, M, sigma, p, None)
    for call in (tg, lambda C, M: fw(C, M, 1.0), lambda C, M: bw(C, M, 1.0)):
        assert call(1, 3) == _lib.PCNN_EINVAL and b"num_classes" in L.pcnn_last_error_string()
        assert call(65, 3) == _lib.PCNN_EINVAL
        assert call(22, -1) == _lib.PCNN_EINVAL and b"num_objects" in L.pcnn_last_error_string()
        assert call(22, 65) == _lib.PCNN_EINVAL
    for call in (fw, bw):
        assert call(22, 3, 0.0) == _lib.PCNN_EINVAL and b"sigma" in L.pcnn_last_error_string()
        assert call(22, 3, -1.0) == _lib.PCNN_EINVAL
    # NULL pointers are reported, not dereferenced
    assert L.pcnn_vertex_targets_fwd(None, None, p, 1, 4, 4, 22, 3, p, p, None) == _lib.PCNN_ENULL
    assert L.pcnn_vertex_targets_fwd(p, None, None, 1, 4, 4, 22, 3, p, p, None) == _lib.PCNN_ENULL      # objects with M > 0
    assert L.pcnn_vertex_targets_fwd(p, None, p, 1, 4, 4, 22, 3, p, None, None) == _lib.PCNN_ENULL
    assert L.pcnn_smooth_l1_vertex_gt_fwd(None, p, None, p, 1, 4, 4, 22, 3, 1.0, p, p, n.value, None) == _lib.PCNN_ENULL
    assert L.pcnn_smooth_l1_vertex_gt_fwd(p, p, None, p, 1, 4, 4, 22, 3, 1.0, None, p, n.value, None) == _lib.PCNN_ENULL
    assert L.pcnn_smooth_l1_vertex_gt_bwd(p, p, None, p, None, None, 1, 4, 4, 22, 3, 1.0, p, None) == _lib.PCNN_ENULL
    assert L.pcnn_smooth_l1_vertex_gt_bwd(p, p, None, p, p, None, 1, 4, 4, 22, 3, 1.0, None, None) == _lib.PCNN_ENULL
    # workspace: NULL or one byte short
    assert fw(22, 3, 1.0, n.value - 1) == _lib.PCNN_EWORKSPACE
    assert L.pcnn_smooth_l1_vertex_gt_fwd(p, p, None, p, 1, 4, 4, 22, 3, 1.0, p, None, n.value, None) == _lib.PCNN_EWORKSPACE
    # misaligned outputs
    q = ctypes.c_void_p(p.value + 4)
    assert L.pcnn_vertex_targets_fwd(p, None, p, 1, 4, 4, 22, 3, q, p, None) == _lib.PCNN_EINVAL
    assert L.pcnn_smooth_l1_vertex_gt_bwd(p, p, None, p, p, None, 1, 4, 4, 22, 3, 1.0, q, None) == _lib.PCNN_EINVAL


def test_ops_check_shapes_before_touching_the_device():
    import torch
    from posecnn_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vertex_targets(torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 2, 6), 22)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.smooth_l1_loss_vertex_gt(torch.zeros(1, 4, 4, 66), torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 2, 6))
