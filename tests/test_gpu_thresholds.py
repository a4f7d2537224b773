"""Threshold-crossing parity: every new case of tests/thresholds.py through the public call, every output bit for bit against
oracle/ (tests/vertex_ref.py for the vertex targets). tests/test_thresholds_cpu.py proves on the CPU which staged path each
case reaches; this file only has to run them. No tolerance anywhere: bit equality is the contract of these kernels
(include/posecnn_hip.h, "Conventions")."""
import numpy as np
import pytest

import thresholds as TH
from test_gpu_hough import NAMES as HOUGH_NAMES
from test_gpu_ops import N, T, same

pytestmark = pytest.mark.gpu
F = np.float32


def cases(op):
    found = TH.new_cases(op)
    return pytest.mark.parametrize("case", found, ids=[c["id"] for c in found])


def zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


@cases("adl")
def test_average_distance(gpu, case):
    """Host-side row count, then the same rows as a device-side count inside a larger buffer whose rows past the count hold
    targets of their own: same bits, zeros past the count."""
    import torch
    from posecnn_amd import ops
    d, want = TH.build(case["id"]), TH.reference(case["id"])
    R, cap = d["R"], d["pred"].shape[0]
    assert cap > R and d["wgt"][R:].any()
    pts, sym = T(gpu, d["pts"]), T(gpu, d["sym"])
    loss, diff = ops.average_distance_loss(T(gpu, d["pred"][:R]), T(gpu, d["tgt"][:R]), T(gpu, d["wgt"][:R]), pts, sym, d["margin"])
    assert want["loss"][0] > 0
    same(N(loss), want["loss"], "loss")
    same(N(diff), want["diff"], "bottom_diff")
    count = torch.tensor([R], dtype=torch.int32, device=gpu)
    loss, diff = ops.average_distance_loss(T(gpu, d["pred"]), T(gpu, d["tgt"]), T(gpu, d["wgt"]), pts, sym, d["margin"], num_rows=count)
    diff = N(diff)
    same(N(loss), want["loss"], "loss (device-side count)")
    same(diff[:R], want["diff"], "bottom_diff (device-side count)")
    assert diff.shape[0] == cap and zero_bits(diff[R:]), "rows past the count must be +0"


@cases("hough")
def test_hough_voting(gpu, case):
    from posecnn_amd import ops
    d, want = TH.build(case["id"]), TH.reference(case["id"])
    out = ops.hough_voting_gpu_padded(T(gpu, d["label"]), T(gpu, d["vertex"]), T(gpu, d["ext"]), T(gpu, d["meta"]), None, 0,
                                      case["vote_thr"], TH.HOUGH_PER_THR, case["skip"], label_threshold=case["label_thr"])
    assert int(want["num_rois"][1]) >= 1
    for name, got in zip(HOUGH_NAMES, out):
        same(N(got), want[name], name)


@cases("roi_fwd")
def test_roi_pool_forward(gpu, case):
    import torch
    from posecnn_amd import ops
    d, want = TH.build(case["id"]), TH.reference(case["id"])
    data, rois = T(gpu, d["data"]), T(gpu, d["rois"])
    if d["argmax"]:
        top, arg = ops.roi_pool(data, rois, d["PH"], d["PW"], d["scale"], 0)
        same(N(arg), want["argmax"], "argmax")
    else:      # argmax may be NULL (include/posecnn_hip.h): half the LDS words per column
        B, H, W, C = d["data"].shape
        top = torch.full(want["top"].shape, float("nan"), dtype=torch.float32, device=gpu)
        ops.check("pcnn_roi_pool_fwd",
                  ops.lib().pcnn_roi_pool_fwd(ops._ptr(data), ops._ptr(rois), B, H, W, C, rois.shape[0], rois.shape[1], d["PH"], d["PW"],
                                              float(d["scale"]), 0, ops._ptr(top), ops._ptr(None), ops._stream(data)))
    same(N(top), want["top"], "top")


@cases("roi_bwd")
def test_roi_pool_backward(gpu, case):
    from posecnn_amd import ops
    d, want = TH.build(case["id"]), TH.reference(case["id"])
    data = T(gpu, d["data"]).requires_grad_(True)
    top, arg = ops.roi_pool(data, T(gpu, d["rois"]), d["PH"], d["PW"], d["scale"], 0)
    same(N(top), want["top"], "top")
    same(N(arg), want["argmax"], "argmax")
    top.backward(T(gpu, d["grad"]))
    assert np.abs(want["bottom_diff"]).sum() > 0
    same(N(data.grad), want["bottom_diff"], "bottom_diff")


@cases("render")
def test_render(gpu, case):
    from posecnn_amd import icp
    d, want = TH.build(case["id"]), TH.reference(case["id"])
    mesh = icp.Mesh(d["vertices"], d["faces"], TH.smooth_normals(d["vertices"], d["faces"]), device=gpu)
    got = icp.render(mesh, d["pose"], d["K"], d["H"], d["W"], want=("vertices", "normals", "canonical"))
    assert np.isfinite(want["vertices"][..., 0]).any()
    for key in ("vertices", "normals", "canonical"):
        same(N(got[key]), want[key], key)


@cases("backproject")
def test_backproject(gpu, case):
    from posecnn_amd import ops
    d, want = TH.build(case["id"]), TH.reference(case["id"])
    m4 = d["meta"].reshape(d["meta"].shape[0], 1, 1, -1)
    td, tl, tf = ops.backproject(T(gpu, d["data"]), T(gpu, d["label"]), T(gpu, d["depth"]), T(gpu, m4), T(gpu, d["label3d"]),
                                 d["G"], d["k"], d["thr"])
    assert want["top_flag"].sum() > 0
    same(N(td), want["top_data"], "top_data")
    same(N(tf), want["top_flag"], "top_flag")
    same(N(tl), want["top_label"], "top_label")


@cases("vertex")
def test_vertex_targets(gpu, case):
    import torch
    from posecnn_amd import _lib, ops
    d, want = TH.build(case["id"]), TH.reference(case["id"])
    label, inst, obj = T(gpu, d["label"]), T(gpu, d["inst"]), T(gpu, d["obj"])
    if case["M"] <= 64:
        t, w = ops.vertex_targets(label, obj, d["C"], inst)
        same(N(t), want["targets"], "targets")
        same(N(w), want["weights"], "weights")
        return
    # one row too many: PCNN_EINVAL, and nothing is launched (the outputs keep what they held)
    B, H, W = d["label"].shape
    outs = [torch.full((B, H, W, 3 * d["C"]), 7.0, dtype=torch.float32, device=gpu) for _ in range(2)]
    st = ops.lib().pcnn_vertex_targets_fwd(ops._ptr(label), ops._ptr(inst), ops._ptr(obj), B, H, W, d["C"], case["M"], ops._ptr(outs[0]),
                                           ops._ptr(outs[1]), ops._stream(label))
    torch.cuda.synchronize()
    assert st == _lib.PCNN_EINVAL
    assert all(bool((o == 7.0).all()) for o in outs)
    with pytest.raises(ValueError):
        ops.vertex_targets(label, obj, d["C"], inst)
