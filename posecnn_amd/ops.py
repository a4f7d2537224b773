"""Host-side operator surface of the PoseCNN custom layers on MI355X.

Names, argument order and attribute names mirror the reference's layer wrappers in
lib/networks/network.py (`hough_voting_gpu` :256-259, `roi_pool` :321-332, `hard_label` :338-340,
`average_distance_loss` :236-238, `backproject` :224-226) and the output tuples follow the
`REGISTER_OP` output order of each `*_op.cc`. Tensors are NHWC, float32 / int32, resident on the
GPU; every call enqueues hand-written gfx950 kernels from libposecnn_hip.so on torch's current
stream. There is no eager/PyTorch fallback: a missing library or a CPU tensor raises.
"""
import ctypes
from ctypes import c_size_t

import numpy as np

import torch

from . import _lib  # noqa: F401  (tests and tools reach the binding as ops._lib)
from ._lib import HOUGH_ROWS_CAPACITY, MAX_ROI, POSE_CHANNELS, VERTEX_CHANNELS, check, lib

__all__ = [
    "hough_voting_gpu", "hough_voting_gpu_padded", "roi_pool", "roi_pool_add2", "hard_label", "conv1_1_conv1_2_fused",
    "conv1_1_conv1_2_fused_raw",
    "average_distance_loss", "backproject", "softmax_argmax", "deconv_bilinear", "bias_act_",
    "hough_voting_grad", "hard_label_grad", "hough_rows_capacity",
    "upscore_softmax_argmax", "Workspace", "vertex_targets", "smooth_l1_loss_vertex_gt",
    "depth_normals", "bilateral_filter_u8", "normal_image", "bilateral_tables", "augment_frames",
    "label_head_loss", "label_head_loss_grad", "vertex_head_loss", "vertex_head_loss_grad",
    "bias_relu_train_", "bias_relu_train_grad", "bias_relu_pool2_train", "bias_relu_pool2_train_grad",
    "estimate_poses_3d", "pose3d_prepare", "pose3d_sample", "pose3d_round",
    "estimate_poses_2d", "pose2d_prepare", "pose2d_sample", "pose2d_round",
    "pose_polish", "icp_refine_batch", "winograd43_conv_fused",
]

INLIER_THRESHOLD = 0.9  # hough_voting_gpu_op.cc:356
LABEL_THRESHOLD = 500   # hough_voting_gpu_op.cc:357


def call(name, *args):
    """`_lib.call` with the handle taken from THIS module's `lib`: the memory-contract tests stand a recorder in for it,
    module by module (icp.py and synthesize.py have the same two lines for the same reason)."""
    check(name, getattr(lib(), name)(*args))


def _dev(t, name, dtype):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (got %s); posecnn_amd has no CPU path" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _aligned16(t):
    """The float4 loads of the MFMA / reduction kernels need 16-byte aligned bases; a view that starts
    mid-allocation (e.g. one row of a packed bias table) is copied — the C-ABI itself rejects it (EINVAL)."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class Workspace:
    """Caller-owned scratch (the reference uses context->allocate_temp inside every launcher,
    e.g. hough_voting_gpu_op.cu.cc:633-640). Grows monotonically; one per stream."""

    def __init__(self):
        self._buf = None

    def get(self, nbytes, device):
        if self._buf is None or self._buf.numel() < nbytes or self._buf.device != device:
            self._buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return self._buf


_default_ws = {}


def _ws(device, key):
    k = (device.index, key, torch.cuda.current_stream(device).cuda_stream)
    if k not in _default_ws:
        _default_ws[k] = Workspace()
    return _default_ws[k]


def _workspace(device, key, query, *dims, workspace=None, at_least=1):
    """The scratch of one entry: ask its `query` (a pcnn_*_workspace_bytes entry, called with `dims`) for the size and fetch
    max(that, at_least) bytes from `workspace` (a caller's Workspace) or from this stream's own under `key`.
    -> (buffer, bytes asked for). at_least=0 is for the entries that take NULL when they need nothing: the buffer is then
    None and no Workspace is touched."""
    nbytes = c_size_t(0)
    call(query, *dims, ctypes.byref(nbytes))
    need = max(nbytes.value, at_least)
    return ((workspace or _ws(device, key)).get(need, device) if need else None), nbytes.value


def icp_refine_batch(*args, **kwargs):
    """`icp.refine_batch` (depth-based refinement of every detection row of a batch, one call): see posecnn_amd/icp.py."""
    from . import icp
    return icp.refine_batch(*args, **kwargs)


# ------------------------------------------------------------------------------------------------
def hough_rows_capacity(batch, is_train, rois_per_image=0):
    """Rows each Hough output needs: the reference's scratch size MAX_ROI * 9
    (hough_voting_gpu_op.cc:94) under its own capacity rule, batch * k * (9 | 1) for k maxima per image."""
    if not rois_per_image:
        return HOUGH_ROWS_CAPACITY
    return max(1, int(batch) * int(rois_per_image) * (9 if is_train else 1))


def _hough_common(label_2d, field, extents, meta_data, poses, threshold, skip_pixels, workspace, out, lowres,
                  is_train=0, rois_per_image=0):
    label_2d = _dev(label_2d, "label_2d", torch.int32)
    field = _dev(field, "vertex_pred", torch.float32)
    extents = _dev(extents, "extents", torch.float32)
    meta_data = _dev(meta_data, "meta_data", torch.float32)
    if label_2d.dim() != 3:
        raise ValueError("label must be 3-dimensional")  # hough_voting_gpu_op.cc:328-329
    if field.dim() != 4:
        raise ValueError("vertex must be 4-dimensional")  # :331-332
    B, H, W = label_2d.shape
    if lowres is None:
        want = (B, H, W)
    else:
        stride = int(lowres)
        if stride < 1 or H % stride or W % stride:
            raise ValueError("label map %dx%d is not a multiple of the stride %d" % (H, W, stride))
        want = (B, H // stride, W // stride)
    if tuple(field.shape[:3]) != want or field.shape[3] % VERTEX_CHANNELS:
        raise ValueError("vertex must be [B,%d,%d,3*num_classes] matching label" % want[1:])
    C = field.shape[3] // VERTEX_CHANNELS
    if extents.numel() != C * 3:
        raise ValueError("extents must be [num_classes,3]")
    num_meta = meta_data.shape[-1]
    if meta_data.numel() != B * num_meta:
        raise ValueError("meta_data must be [B,1,1,num_meta]")
    if poses is None or poses.numel() == 0:
        num_gt, gt = 0, None
    else:
        gt = _dev(poses, "poses", torch.float32)
        if gt.dim() != 2 or gt.shape[1] != 13:
            raise ValueError("poses (gt) must be [N,13]")
        num_gt = gt.shape[0]
    dev = label_2d.device
    ws, _ = _workspace(dev, "hough", "pcnn_hough_voting_workspace_bytes", B, H, W, C, float(threshold), int(skip_pixels),
                       int(rois_per_image), workspace=workspace)
    if out is None:
        cap = hough_rows_capacity(B, is_train, rois_per_image)
        out = (torch.empty((cap, 7), dtype=torch.float32, device=dev),
               torch.empty((cap, 7), dtype=torch.float32, device=dev),
               torch.empty((cap, POSE_CHANNELS * C), dtype=torch.float32, device=dev),
               torch.empty((cap, POSE_CHANNELS * C), dtype=torch.float32, device=dev),
               torch.empty((cap,), dtype=torch.int32, device=dev),
               torch.empty((2,), dtype=torch.int32, device=dev))
    return label_2d, field, extents, meta_data, gt, num_gt, (B, H, W, C, num_meta), ws, out


def hough_voting_gpu_padded(label_2d, vertex_pred, extents, meta_data, poses, is_train, threshold,
                            per_threshold, skip_pixels, workspace=None, out=None,
                            inlier_threshold=INLIER_THRESHOLD, label_threshold=LABEL_THRESHOLD,
                            rois_per_image=0):
    """Sync-free form: returns capacity-sized buffers and the device-side row counts.

    Returns (top_box[cap,7], top_pose[cap,7], top_target[cap,4C], top_weight[cap,4C],
    top_domain[cap] int32, num_rois[2] int32) where num_rois[0] is the number of rows the
    reference op returns (>= 1) and num_rois[1] the true detection row count; cap =
    `hough_rows_capacity(B, is_train, rois_per_image)` (1152 under the reference's capacity rule).
    rois_per_image: 0 = the reference's index_size = MAX_ROI / B per image; k > 0 = k maxima per
    image whatever B (include/posecnn_hip.h, "Capacity").
    """
    label_2d, vertex_pred, extents, meta_data, gt, num_gt, (B, H, W, C, num_meta), ws, out = _hough_common(
        label_2d, vertex_pred, extents, meta_data, poses, threshold, skip_pixels, workspace, out, None,
        is_train, rois_per_image)
    top_box, top_pose, top_target, top_weight, top_domain, num_rois = out
    call("pcnn_hough_voting_fwd", _ptr(label_2d), _ptr(vertex_pred), _ptr(extents), _ptr(meta_data), _ptr(gt), B, H, W, C, num_meta,
         num_gt, int(is_train), float(threshold), float(per_threshold), int(skip_pixels), float(inlier_threshold),
         int(label_threshold), int(rois_per_image), int(top_box.shape[0]), _ptr(top_box), _ptr(top_pose), _ptr(top_target),
         _ptr(top_weight), _ptr(top_domain), _ptr(num_rois), _ptr(ws), ws.numel(), _stream(label_2d))
    return out


def hough_voting_gpu_lowres_padded(label_2d, z, bias, kernel, stride, extents, meta_data, poses, is_train,
                                   threshold, per_threshold, skip_pixels, workspace=None, out=None,
                                   inlier_threshold=INLIER_THRESHOLD, label_threshold=LABEL_THRESHOLD,
                                   rois_per_image=0):
    """Fused vertex head -> Hough voting: identical results to
    `hough_voting_gpu_padded(label_2d, deconv_bilinear(z, kernel, stride, bias=bias), ...)` without
    ever building the [B,H,W,3C] `vertex_pred` (vgg16_convs.py:152-163).
    z is the 1x1 `vertex_pred` conv evaluated at 1/stride resolution, [B,H/stride,W/stride,3C]."""
    label_2d, z, extents, meta_data, gt, num_gt, (B, H, W, C, num_meta), ws, out = _hough_common(
        label_2d, z, extents, meta_data, poses, threshold, skip_pixels, workspace, out, stride,
        is_train, rois_per_image)
    bias = _dev(bias, "bias", torch.float32)
    if bias.numel() != VERTEX_CHANNELS * C:
        raise ValueError("bias must be [3*num_classes]")
    top_box, top_pose, top_target, top_weight, top_domain, num_rois = out
    call("pcnn_hough_voting_lowres_fwd", _ptr(label_2d), _ptr(z), _ptr(bias), int(kernel), int(stride), _ptr(extents),
         _ptr(meta_data), _ptr(gt), B, H, W, C, num_meta, num_gt, int(is_train), float(threshold), float(per_threshold),
         int(skip_pixels), float(inlier_threshold), int(label_threshold), int(rois_per_image), int(top_box.shape[0]), _ptr(top_box),
         _ptr(top_pose), _ptr(top_target), _ptr(top_weight), _ptr(top_domain), _ptr(num_rois), _ptr(ws), ws.numel(),
         _stream(label_2d))
    return out


def hough_voting_grad(label_2d, vertex_pred):
    """HoughvotinggpuGrad (hough_voting_gpu_op.cc:440-484 -> set_gradients, .cu.cc:608-612): the op
    is not differentiable; its registered gradient hands zeros to both inputs. Returns
    (grad_label f32 [B,H,W], grad_vertex f32 [B,H,W,3C])."""
    B, H, W = label_2d.shape
    C = vertex_pred.shape[3] // VERTEX_CHANNELS
    dev = vertex_pred.device
    gl = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    gv = torch.empty((B, H, W, VERTEX_CHANNELS * C), dtype=torch.float32, device=dev)
    call("pcnn_hough_voting_bwd", _ptr(gl), _ptr(gv), B, H, W, C, _stream(gv))
    return gl, gv


class _HoughVotingFn(torch.autograd.Function):
    """The op inside an autograd graph (training graph, vgg16_convs.py:167-168): outputs carry no
    gradient information; backward = the registered zero gradient of the reference."""

    @staticmethod
    def forward(ctx, label_2d, vertex_pred, extents, meta_data, poses, cfg):
        is_train, threshold, per_threshold, skip_pixels, workspace, consts = cfg
        out = hough_voting_gpu_padded(label_2d, vertex_pred, extents, meta_data, poses, is_train, threshold,
                                      per_threshold, skip_pixels, workspace=workspace, **consts)
        ctx.save_for_backward(label_2d, vertex_pred)
        ctx.mark_non_differentiable(out[4], out[5])
        return out

    @staticmethod
    def backward(ctx, *_grads):
        label_2d, vertex_pred = ctx.saved_tensors
        _, gv = hough_voting_grad(label_2d, vertex_pred)
        return None, gv, None, None, None, None   # label is int32: no gradient slot


def hough_voting_gpu(label_2d, vertex_pred, extents, meta_data, poses, is_train, threshold,
                     per_threshold, skip_pixels, name=None, workspace=None, **consts):
    """Drop-in for `Network.hough_voting_gpu` (network.py:256-259): returns exactly-sized
    (top_box[R,7], top_pose[R,7], top_target[R,4C], top_weight[R,4C], top_domain[R]).
    Like the reference (hough_voting_gpu_op.cc:379-383) this reads the row count back to the host.
    """
    if torch.is_grad_enabled() and isinstance(vertex_pred, torch.Tensor) and vertex_pred.requires_grad:
        top_box, top_pose, top_target, top_weight, top_domain, num_rois = _HoughVotingFn.apply(
            label_2d, vertex_pred, extents, meta_data, poses,
            (is_train, threshold, per_threshold, skip_pixels, workspace, consts))
    else:
        top_box, top_pose, top_target, top_weight, top_domain, num_rois = hough_voting_gpu_padded(
            label_2d, vertex_pred, extents, meta_data, poses, is_train, threshold, per_threshold,
            skip_pixels, workspace=workspace, **consts)
    r = int(num_rois[0].item())
    return top_box[:r], top_pose[:r], top_target[:r], top_weight[:r], top_domain[:r]


# ------------------------------------------------------------------------------------------------
class _RoiPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, rois, pooled_height, pooled_width, spatial_scale, pool_channel):
        B, H, W, C = data.shape
        R, cols = rois.shape
        Cout = 1 if pool_channel else C
        top = torch.empty((R, pooled_height, pooled_width, Cout), dtype=torch.float32, device=data.device)
        argmax = torch.empty((R, pooled_height, pooled_width, Cout), dtype=torch.int32, device=data.device)
        call("pcnn_roi_pool_fwd", _ptr(data), _ptr(rois), B, H, W, C, R, cols, int(pooled_height), int(pooled_width),
             float(spatial_scale), int(pool_channel), _ptr(top), _ptr(argmax), _stream(data))
        ctx.save_for_backward(rois, argmax)
        ctx.cfg = (B, H, W, C, R, cols, int(pooled_height), int(pooled_width), float(spatial_scale), int(pool_channel))
        ctx.mark_non_differentiable(argmax)
        return top, argmax

    @staticmethod
    def backward(ctx, grad_top, _grad_argmax):
        rois, argmax = ctx.saved_tensors
        B, H, W, C, R, cols, PH, PW, scale, pc = ctx.cfg
        grad_top = grad_top.contiguous()
        bottom = torch.empty((B, H, W, C), dtype=torch.float32, device=grad_top.device)
        call("pcnn_roi_pool_bwd", _ptr(grad_top), _ptr(rois), _ptr(argmax), B, H, W, C, R, cols, PH, PW, scale, pc, _ptr(bottom),
             _stream(grad_top))
        return bottom, None, None, None, None, None


def roi_pool(data, rois, pooled_height, pooled_width, spatial_scale, pool_channel, name=None):
    """Drop-in for `Network.roi_pool` (network.py:321-332): NHWC max pooling of 7-column ROIs.
    Returns (top_data[R,PH,PW,C or 1], argmax int32)."""
    data = _dev(data, "data", torch.float32)
    rois = _dev(rois, "rois", torch.float32)
    if data.dim() != 4:
        raise ValueError("data must be 4-dimensional")  # roi_pooling_op.cc:313-314
    if rois.dim() != 2:
        raise ValueError("rois must be 2-dimensional")  # :317-318
    return _RoiPoolFn.apply(data, rois, pooled_height, pooled_width, spatial_scale, pool_channel)


def roi_pool_add2(data_a, scale_a, data_b, scale_b, rois, pooled_height=7, pooled_width=7, num_rows=None, dead_rows="zero", out=None):
    """Fused `pool_score` = roi_pool(conv5_3, 1/16) + roi_pool(conv4_3, 1/8)
    (vgg16_convs.py:177-187), inference only (no argmax). `num_rows` (device int32[1]): true row
    count of a capacity-sized `rois` buffer; rows past it pool to zero — or, with dead_rows="keep", are not
    written at all (for consumers that mask them by the same count: ops.fc_rows / ops.fc_skinny)."""
    data_a = _dev(data_a, "data_a", torch.float32)
    data_b = _dev(data_b, "data_b", torch.float32)
    rois = _dev(rois, "rois", torch.float32)
    B, Ha, Wa, C = data_a.shape
    Bb, Hb, Wb, Cb = data_b.shape
    if (B, C) != (Bb, Cb):
        raise ValueError("feature maps must share batch and channel dimensions")
    if dead_rows not in ("zero", "keep"):
        raise ValueError("dead_rows must be 'zero' or 'keep'")
    if dead_rows == "keep" and num_rows is None:
        raise ValueError("dead_rows='keep' needs num_rows")
    R, cols = rois.shape
    if out is None:
        out = torch.empty((R, pooled_height, pooled_width, C), dtype=torch.float32, device=data_a.device)
    else:
        out = _dev(out, "out", torch.float32)
        if tuple(out.shape) != (R, pooled_height, pooled_width, C):
            raise ValueError("out must be [R, PH, PW, C]")
    name = "pcnn_roi_pool_add2_live_fwd" if dead_rows == "keep" else "pcnn_roi_pool_add2_fwd"
    call(name, _ptr(data_a), Ha, Wa, float(scale_a), _ptr(data_b), Hb, Wb, float(scale_b), _ptr(rois), B, C, R, cols,
         int(pooled_height), int(pooled_width), _ptr(_dev(num_rows, "num_rows", torch.int32) if num_rows is not None else None),
         _ptr(out), _stream(data_a))
    return out


# ------------------------------------------------------------------------------------------------
def _hard_label_raw(prob, gt_label, threshold):
    C = prob.shape[-1]
    N = prob.numel() // C
    out = torch.empty_like(prob)
    call("pcnn_hard_label_fwd", _ptr(prob), _ptr(gt_label), N, C, float(threshold), _ptr(out), _stream(prob))
    return out


def hard_label_grad(prob, gt_label):
    """HardlabelGrad (hard_label_op_gpu.cu.cc:55-85): zeros for both inputs.
    Returns (grad_prob f32 like prob, grad_gt f32 [N])."""
    C = prob.shape[-1]
    N = prob.numel() // C
    gp = torch.empty_like(prob)
    gg = torch.empty(gt_label.shape, dtype=torch.float32, device=prob.device)
    call("pcnn_hard_label_bwd", _ptr(gp), _ptr(gg), N, C, _stream(prob))
    return gp, gg


class _HardLabelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, gt_label, threshold):
        ctx.save_for_backward(prob, gt_label)
        return _hard_label_raw(prob, gt_label, threshold)

    @staticmethod
    def backward(ctx, _grad):
        prob, gt_label = ctx.saved_tensors
        return hard_label_grad(prob, gt_label)[0], None, None


def hard_label(prob, gt_label, threshold, name=None):
    """Drop-in for `Network.hard_label` (network.py:338-340); GPU-kernel semantics
    (hard_label_op_gpu.cu.cc:17-29). prob [B,H,W,C] f32, gt_label [B,H,W] int32 -> [B,H,W,C].
    Inside an autograd graph the registered zero gradient (HardlabelGrad) is what flows back."""
    prob = _dev(prob, "prob", torch.float32)
    gt_label = _dev(gt_label, "gt_label", torch.int32)
    C = prob.shape[-1]
    N = prob.numel() // C
    if gt_label.numel() != N:
        raise ValueError("gt_label must have one entry per pixel of prob")
    if torch.is_grad_enabled() and prob.requires_grad:
        return _HardLabelFn.apply(prob, gt_label, float(threshold))
    return _hard_label_raw(prob, gt_label, threshold)


def softmax_argmax(score, want_prob=True):
    """softmax_high_dimension + argmax_2d (network.py:474-488, 432-434) in one pass.
    score [..., C] f32 -> (prob_normalized [..., C] or None, label_2d [...] int32)."""
    score = _dev(score, "score", torch.float32)
    C = score.shape[-1]
    N = score.numel() // C
    prob = torch.empty_like(score) if want_prob else None
    label = torch.empty(score.shape[:-1], dtype=torch.int32, device=score.device)
    call("pcnn_softmax_argmax_fwd", _ptr(score), N, C, _ptr(prob), _ptr(label), _stream(score))
    return prob, label


def bias_act_(x, bias, relu=True):
    """In place: x[..., c] = [ReLU](x[..., c] + bias[c]) for an NHWC-contiguous tensor."""
    x = _dev(x, "x", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    C = x.shape[-1]
    if bias.numel() != C:
        raise ValueError("bias must have one entry per channel")
    call("pcnn_bias_act_fwd", _ptr(x), _ptr(bias), x.numel() // C, C, 1 if relu else 0, _ptr(x), _stream(x))
    return x


def conv3x3_c3(x, weights, bias, relu=True):
    """[ReLU](conv3x3_SAME(x) + bias) for a 3-channel NHWC input: x [B,H,W,3], weights [3,3,3,Cout]
    laid out (ky, kx, ci, co) like the TF variable, Cout a multiple of 64. Returns [B,H,W,Cout]."""
    x = _dev(x, "x", torch.float32)
    weights = _dev(weights, "weights", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError("x must be [B,H,W,3]")
    B, H, W, _ = x.shape
    Cout = weights.shape[-1]
    if tuple(weights.shape) != (3, 3, 3, Cout) or bias.numel() != Cout:
        raise ValueError("weights must be [3,3,3,Cout] (ky,kx,ci,co) and bias [Cout]")
    y = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
    call("pcnn_conv3x3_c3_fwd", _ptr(x), _ptr(weights), _ptr(bias), B, H, W, Cout, 1 if relu else 0, _ptr(y), _stream(x))
    return y


def conv3x3_c3_winograd43(x, weights, bias, relu=True, groups=1):
    """winograd_input(conv3x3_c3(x, weights, bias, relu), tile=4) in one kernel: V [36, T, Cout].
    groups > 1: weights [groups,3,3,3,Cout], bias [groups,Cout]; image b uses set b // (B // groups)."""
    x = _dev(x, "x", torch.float32)
    weights = _dev(weights, "weights", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError("x must be [B,H,W,3]")
    B, H, W, _ = x.shape
    Cout = weights.shape[-1]
    if weights.numel() != groups * 27 * Cout or tuple(weights.shape[-4:]) != (3, 3, 3, Cout) or bias.numel() != groups * Cout:
        raise ValueError("weights must be [groups,3,3,3,Cout] (ky,kx,ci,co) and bias [groups,Cout]")
    v = torch.empty((36, B * ((H + 3) // 4) * ((W + 3) // 4), Cout), dtype=torch.float32, device=x.device)
    call("pcnn_conv3x3_c3_winograd43_fwd", _ptr(x), _ptr(weights), _ptr(bias), B, H, W, Cout, int(groups), 1 if relu else 0,
         _ptr(v), _stream(x))
    return v


def _raw_frames(color_bgr, depth, pixel_means):
    """The checked frames of the two raw-frame entries: color_bgr uint8 [B,H,W,3] (or None), depth uint16 [B,H,W] or
    [B,H,W,1] (or None). Returns (c, nc, d, nd, H, W, device, means): the contiguous tensors with their frame counts and
    the pixel means (config.PIXEL_MEANS unless given) as the c_double[3] the C entries take."""
    from .config import PIXEL_MEANS
    c = _dev(color_bgr, "color_bgr", torch.uint8) if color_bgr is not None else None
    d = _dev(depth, "depth", torch.uint16) if depth is not None else None
    if c is None and d is None:
        raise ValueError("need colour and / or depth frames")
    if c is not None and (c.dim() != 4 or c.shape[3] != 3):
        raise ValueError("color_bgr must be uint8 [B,H,W,3]")
    if d is not None and d.dim() == 4 and d.shape[3] == 1:
        d = d.reshape(d.shape[:3])
    if d is not None and d.dim() != 3:
        raise ValueError("depth must be uint16 [B,H,W]")
    H, W = (c.shape[1], c.shape[2]) if c is not None else (d.shape[1], d.shape[2])
    if c is not None and d is not None and tuple(d.shape[1:]) != (H, W):
        raise ValueError("colour and depth frames must have the same size")
    means = (ctypes.c_double * 3)(*[float(m) for m in np.asarray(PIXEL_MEANS if pixel_means is None else pixel_means, dtype=np.float64).reshape(-1)[:3]])
    return c, (0 if c is None else c.shape[0]), d, (0 if d is None else d.shape[0]), H, W, (c if c is not None else d).device, means


def conv3x3_c3_winograd43_raw(color_bgr, depth, weights, bias, relu=True, pixel_means=None):
    """conv3x3_c3_winograd43 on the frames as the sensor delivers them: color_bgr uint8 [B,H,W,3] (or None), depth uint16
    [B,H,W] (or None); the blobs of lib/fcn/test.py:56-74 are formed inside the kernel, bit for bit. Colour frames first
    (filter set 0), depth frames after (next set): weights [sets,3,3,3,Cout], bias [sets,Cout]. Returns V [36, T, Cout]."""
    c, nc, d, nd, H, W, dev, means = _raw_frames(color_bgr, depth, pixel_means)
    sets = (nc > 0) + (nd > 0)
    weights = _dev(weights, "weights", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    Cout = weights.shape[-1]
    if weights.numel() != sets * 27 * Cout or tuple(weights.shape[-4:]) != (3, 3, 3, Cout) or bias.numel() != sets * Cout:
        raise ValueError("weights must be [sets,3,3,3,Cout] (ky,kx,ci,co) and bias [sets,Cout]")
    v = torch.empty((36, (nc + nd) * ((H + 3) // 4) * ((W + 3) // 4), Cout), dtype=torch.float32, device=dev)
    call("pcnn_conv3x3_c3_winograd43_raw_fwd", _ptr(c), nc, _ptr(d), nd, means, _ptr(weights), _ptr(bias), H, W, Cout,
         1 if relu else 0, _ptr(v), _stream(v))
    return v


def conv12_fragment_major(ut2):
    """U^T [..., 36, 64, 64] (plane, out channel, in channel) -> the fragment-major layout of pcnn_conv1_1_conv1_2_fused_fwd's
    ut2_layout = 1: [..., 36, 4, 4, 64, 4] with (k, w, g, lane, i) = U^T[k][16 w + (lane & 15)][16 g + 4 (lane >> 4) + i]."""
    lead = ut2.shape[:-3]
    t = ut2.reshape(*lead, 36, 4, 16, 4, 4, 4)          # k, w, lr, g, lk, i
    t = t.permute(*range(len(lead)), len(lead), len(lead) + 1, len(lead) + 3, len(lead) + 4, len(lead) + 2, len(lead) + 5)   # k, w, g, lk, lr, i
    return t.reshape(*lead, 36, 4, 4, 64, 4).contiguous()


def conv1_1_conv1_2_fused(x, w1, b1, ut2, b2, relu1=True, relu2=True, groups=1, ut2_layout=0):
    """max_pool_2x2(relu(conv1_2(relu(conv1_1(x))))) in one kernel (csrc/conv_first.hip): x [B,H,W,3] f32 blobs, H and W multiples
    of 16; w1 [groups,3,3,3,64], b1 [groups,64]; ut2 [groups,36,64,64] = winograd_filter(w2, 4).transpose(1, 2) per set;
    b2 [groups,64]. Bit-identical to conv3x3_c3_winograd43 + winograd43_conv(pool=1). Returns [B,H/2,W/2,64]."""
    x = _dev(x, "x", torch.float32)
    w1, b1, ut2, b2 = (_dev(t, n, torch.float32) for t, n in ((w1, "w1"), (b1, "b1"), (ut2, "ut2"), (b2, "b2")))
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError("x must be [B,H,W,3]")
    B, H, W, _ = x.shape
    if w1.numel() != groups * 27 * 64 or b1.numel() != groups * 64 or ut2.numel() != groups * 36 * 64 * 64 or b2.numel() != groups * 64:
        raise ValueError("w1 [groups,3,3,3,64], b1 [groups,64], ut2 [groups,36,64,64], b2 [groups,64]")
    y = torch.empty((B, H // 2, W // 2, 64), dtype=torch.float32, device=x.device)
    call("pcnn_conv1_1_conv1_2_fused_fwd", _ptr(x), _ptr(w1), _ptr(b1), _ptr(ut2), int(ut2_layout), _ptr(b2), B, H, W, int(groups),
         1 if relu1 else 0, 1 if relu2 else 0, _ptr(y), _stream(x))
    return y


def conv1_1_conv1_2_fused_raw(color_bgr, depth, w1, b1, ut2, b2, relu1=True, relu2=True, pixel_means=None, ut2_layout=0):
    """conv1_1_conv1_2_fused on the frames as the sensor delivers them (see conv3x3_c3_winograd43_raw): colour frames first
    (filter set 0), depth frames after (next set)."""
    c, nc, d, nd, H, W, dev, means = _raw_frames(color_bgr, depth, pixel_means)
    sets = (nc > 0) + (nd > 0)
    w1, b1, ut2, b2 = (_dev(t, n, torch.float32) for t, n in ((w1, "w1"), (b1, "b1"), (ut2, "ut2"), (b2, "b2")))
    if w1.numel() != sets * 27 * 64 or b1.numel() != sets * 64 or ut2.numel() != sets * 36 * 64 * 64 or b2.numel() != sets * 64:
        raise ValueError("w1 [sets,3,3,3,64], b1 [sets,64], ut2 [sets,36,64,64], b2 [sets,64]")
    y = torch.empty((nc + nd, H // 2, W // 2, 64), dtype=torch.float32, device=dev)
    call("pcnn_conv1_1_conv1_2_fused_raw_fwd", _ptr(c), nc, _ptr(d), nd, means, _ptr(w1), _ptr(b1), _ptr(ut2), int(ut2_layout),
         _ptr(b2), H, W, 1 if relu1 else 0, 1 if relu2 else 0, _ptr(y), _stream(y))
    return y


_WINO_G = {
    2: [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]],
    4: [[1 / 4, 0.0, 0.0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
        [1 / 24, -1 / 12, 1 / 6], [0.0, 0.0, 1.0]],
}


def _wino_tiles(B, H, W, tile):
    if tile == 2:
        return B * (H // 2) * (W // 2)
    return B * ((H + 3) // 4) * ((W + 3) // 4)


def winograd_filter(weights, tile=2):
    """torch filter [Cout, Cin, 3, 3] -> U f32 [(tile+2)^2, Cin, Cout], U[n*i+j] = (G g G^T)[i][j]
    (float64 arithmetic, one rounding). Host-side plumbing, done once per filter."""
    g = weights.detach().to(torch.float64)
    G = torch.tensor(_WINO_G[tile], dtype=torch.float64, device=g.device)
    u = torch.einsum("ir,ocrs,js->ijco", G, g, G)   # [n,n,Cin,Cout]
    n = tile + 2
    return u.reshape(n * n, g.shape[1], g.shape[0]).to(torch.float32).contiguous()


def winograd_input(x, tile=2):
    """x [B,H,W,C] -> V [(tile+2)^2, T, C]: the input transform B^T d B of every input patch
    (tile = 2: F(2x2,3x3), T = B*H/2*W/2; tile = 4: F(4x4,3x3), T = B*ceil(H/4)*ceil(W/4))."""
    x = _dev(x, "x", torch.float32)
    B, H, W, C = x.shape
    n = tile + 2
    v = torch.empty((n * n, _wino_tiles(B, H, W, tile), C), dtype=torch.float32, device=x.device)
    fn = "pcnn_winograd_input_fwd" if tile == 2 else "pcnn_winograd43_input_fwd"
    call(fn, _ptr(x), B, H, W, C, _ptr(v), _stream(x))
    return v


def winograd_output(m, bias, B, H, W, relu=True, pool=False, tile=2):
    """M [(tile+2)^2, T, C] -> [ReLU](A^T M A + bias) as [B,H,W,C], or its 2x2 max-pool [B,H/2,W/2,C]."""
    m = _dev(m, "m", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    C = m.shape[2]
    n = tile + 2
    if m.shape[0] != n * n or m.shape[1] != _wino_tiles(B, H, W, tile) or bias.numel() != C:
        raise ValueError("m must be [%d, tiles, C] and bias [C]" % (n * n))
    shape = (B, H // 2, W // 2, C) if pool else (B, H, W, C)
    y = torch.empty(shape, dtype=torch.float32, device=m.device)
    fn = "pcnn_winograd_output_fwd" if tile == 2 else "pcnn_winograd43_output_fwd"
    call(fn, _ptr(m), _ptr(bias), B, H, W, C, 1 if relu else 0, 1 if pool else 0, _ptr(y), _stream(m))
    return y


def winograd43_output_both(m, bias, B, H, W, relu=True):
    """F(4x4,3x3) output transform returning (y [B,H,W,C], max_pool_2x2(y) [B,H/2,W/2,C]) from one pass."""
    m = _dev(m, "m", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    C = m.shape[2]
    if m.shape[0] != 36 or m.shape[1] != _wino_tiles(B, H, W, 4) or bias.numel() != C:
        raise ValueError("m must be [36, tiles, C] and bias [C]")
    y = torch.empty((B, H, W, C), dtype=torch.float32, device=m.device)
    yp = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=m.device)
    call("pcnn_winograd43_output_both_fwd", _ptr(m), _ptr(bias), B, H, W, C, 1 if relu else 0, _ptr(y), _ptr(yp), _stream(m))
    return y, yp


def winograd43_pack_filters(ut):
    """ut [groups,36,Cout,Cin] (or [36,Cout,Cin]) -> the fragment-major filter bank of winograd43_conv(packed=True), same
    shape and size: viewed as [groups,36,Cout/16,Cin/64,4,64,4], element [g,k,n16,kc,j,16*lk+lr,e] is
    ut[g,k,16*n16+lr,64*kc+16*j+4*lk+e] — the order in which a wave's lanes consume the operand. Once per filter."""
    ut = _dev(ut, "ut", torch.float32)
    if ut.dim() not in (3, 4) or ut.shape[-3] != 36:
        raise ValueError("ut must be [groups, 36, Cout, Cin] or [36, Cout, Cin]")
    groups = ut.shape[0] if ut.dim() == 4 else 1
    Cout, Cin = ut.shape[-2], ut.shape[-1]
    utp = torch.empty_like(ut)
    call("pcnn_winograd43_pack_filters_fwd", _ptr(ut), Cin, Cout, int(groups), _ptr(utp), _stream(ut))
    return utp


def winograd43_conv(v, ut, bias, B, H, W, relu=True, pool=0, groups=1, packed=False):
    """The 36 Winograd-domain contractions + output transform of F(4x4,3x3) in one fp32-MFMA kernel:
    v [36,T,Cin], ut [groups,36,Cout,Cin] (= winograd_filter(w, 4).transpose(1, 2) per group), bias
    [groups,Cout] -> y [B,H,W,Cout] (pool=0), its 2x2 max-pool [B,H/2,W/2,Cout] (pool=1) or both (pool=2,
    returns (y, y_pool)). `groups`: image b uses filter set b // (B // groups). `packed`: ut is the bank of
    winograd43_pack_filters (same shape), which the kernel takes straight into registers; same bits."""
    v = _dev(v, "v", torch.float32)
    ut = _dev(ut, "ut", torch.float32)
    bias = _aligned16(_dev(bias, "bias", torch.float32))
    Cin = v.shape[2]
    if ut.dim() == 3:
        ut = ut.unsqueeze(0)
    Cout = ut.shape[2]
    if (v.shape[0] != 36 or v.shape[1] != _wino_tiles(B, H, W, 4) or tuple(ut.shape) != (groups, 36, Cout, Cin)
            or bias.numel() != groups * Cout):
        raise ValueError("v must be [36, tiles, Cin], ut [groups, 36, Cout, Cin], bias [groups, Cout]")
    pool = int(pool)
    y = torch.empty((B, H // 2, W // 2, Cout) if pool == 1 else (B, H, W, Cout), dtype=torch.float32, device=v.device)
    yp = torch.empty((B, H // 2, W // 2, Cout), dtype=torch.float32, device=v.device) if pool == 2 else None
    # Cin-split partials (small launches only)
    ws, nbytes = _workspace(v.device, "wino43_conv", "pcnn_winograd43_conv_workspace_bytes", B, H, W, Cin, Cout, int(groups), at_least=0)
    fn = "pcnn_winograd43_conv_packed_fwd" if packed else "pcnn_winograd43_conv_fwd"
    call(fn, _ptr(v), _ptr(ut), _ptr(bias), B, H, W, Cin, Cout, int(groups), 1 if relu else 0, pool, _ptr(y), _ptr(yp), _ptr(ws),
         nbytes, _stream(v))
    return (y, yp) if pool == 2 else y


def winograd43_conv_fused(x, utp, bias, relu=True, pool=0, groups=1):
    """A 3x3 / stride 1 / SAME convolution with 64 or 128 input and 128 output channels in ONE kernel (csrc/conv2_fused.hip):
    x [B,H,W,Cin], H and W multiples of 16; utp [groups,36,128,Cin] the bank of winograd43_pack_filters; bias [groups,128]
    -> y [B,H,W,128] (pool=0) or its 2x2 max-pool [B,H/2,W/2,128] (pool=1). The transformed input never leaves the CU.
    Bit-identical to winograd_input(x, 4) + winograd43_conv(..., packed=True) on the same tensors wherever that op runs one K
    chain per accumulator: always with Cin = 64, and with Cin = 128 in every launch of at least 128 of this kernel's 16 x 16
    pixel blocks (a smaller one the op splits over Cin when it has its workspace: two partial outputs summed afterwards,
    another rounding order; without the workspace the entry pcnn_winograd43_conv_packed_fwd never splits)."""
    x = _dev(x, "x", torch.float32)
    utp = _dev(utp, "utp", torch.float32)
    bias = _aligned16(_dev(bias, "bias", torch.float32))
    if x.dim() != 4:
        raise ValueError("x must be [B,H,W,Cin]")
    B, H, W, Cin = x.shape
    if utp.dim() == 3:
        utp = utp.unsqueeze(0)
    Cout = utp.shape[2]
    if tuple(utp.shape) != (groups, 36, Cout, Cin) or bias.numel() != groups * Cout:
        raise ValueError("utp must be [groups, 36, Cout, Cin], bias [groups, Cout]")
    pool = int(pool)
    y = torch.empty((B, H // 2, W // 2, Cout) if pool == 1 else (B, H, W, Cout), dtype=torch.float32, device=x.device)
    call("pcnn_winograd43_conv_fused_fwd", _ptr(x), _ptr(utp), _ptr(bias), B, H, W, Cin, Cout, int(groups), 1 if relu else 0, pool,
         _ptr(y), _stream(x))
    return y


def fc_rows(x, wt, bias, relu=True, num_rows=None, addend=None):
    """`Network.fc` on a capacity-sized row buffer: y[m] = [ReLU](x[m] @ wt.T + bias [+ addend[m]]) for
    m < *num_rows (device int32[1]; None = every row), zeros past it. x [M, K], wt [N, K] (the TF weight
    [K, N] transposed), K % 64 == 0, N % 64 == 0. One fp32-MFMA kernel, no host synchronisation."""
    x = _dev(x, "x", torch.float32)
    wt = _dev(wt, "wt", torch.float32)
    bias = _aligned16(_dev(bias, "bias", torch.float32))
    if x.dim() != 2 or wt.dim() != 2 or wt.shape[1] != x.shape[1] or bias.numel() != wt.shape[0]:
        raise ValueError("x must be [M, K], wt [N, K], bias [N]")
    M, K = x.shape
    N = wt.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    nr = _dev(num_rows, "num_rows", torch.int32) if num_rows is not None else None
    ad = _dev(addend, "addend", torch.float32) if addend is not None else None
    if ad is not None and tuple(ad.shape) != (M, N):
        raise ValueError("addend must be [M, N]")
    ws, nbytes = _workspace(x.device, "fc_rows", "pcnn_fc_rows_workspace_bytes", M, K, N, at_least=0)   # split-K partials (few live rows)
    call("pcnn_fc_rows_fwd", _ptr(x), _ptr(wt), _ptr(bias), M, K, N, 1 if relu else 0, _ptr(nr), _ptr(ad), _ptr(y), _ptr(ws),
         nbytes, _stream(x))
    return y


def fc_rows_split(x, wt, bias, out_a, relu_a=True, relu_b=False, num_rows=None):
    """Two layers on the same rows as one product: wt [out_a + out_b, K] and bias [out_a + out_b] hold the two filters one
    after the other; returns (y_a [M, out_a], y_b [M, out_b]) with a ReLU flag each. Bit-identical to two `fc_rows` calls."""
    x = _dev(x, "x", torch.float32)
    wt = _dev(wt, "wt", torch.float32)
    bias = _aligned16(_dev(bias, "bias", torch.float32))
    if x.dim() != 2 or wt.dim() != 2 or wt.shape[1] != x.shape[1] or bias.numel() != wt.shape[0] or not 0 < out_a < wt.shape[0]:
        raise ValueError("x must be [M, K], wt [out_a + out_b, K], bias [out_a + out_b]")
    M, K = x.shape
    out_b = wt.shape[0] - int(out_a)
    ya = torch.empty((M, int(out_a)), dtype=torch.float32, device=x.device)
    yb = torch.empty((M, out_b), dtype=torch.float32, device=x.device)
    nr = _dev(num_rows, "num_rows", torch.int32) if num_rows is not None else None
    call("pcnn_fc_rows_split_fwd", _ptr(x), _ptr(wt), _ptr(bias), M, K, int(out_a), out_b, 1 if relu_a else 0, 1 if relu_b else 0,
         _ptr(nr), _ptr(ya), _ptr(yb), _stream(x))
    return ya, yb


def fc_rows_cols(x, wt_padded, bias_padded, out_features, activation="none", num_rows=None):
    """`fc_rows` for a width that is no multiple of 64 (fc8: 88): wt_padded [Npad, K] / bias_padded [Npad] zero-padded to a
    multiple of 64, y [M, out_features]. activation "none" | "relu" | "tanh"; "tanh" returns (linear, tanh(linear))."""
    x = _dev(x, "x", torch.float32)
    wt_padded = _dev(wt_padded, "wt_padded", torch.float32)
    bias_padded = _aligned16(_dev(bias_padded, "bias_padded", torch.float32))
    if x.dim() != 2 or wt_padded.dim() != 2 or wt_padded.shape[1] != x.shape[1] or bias_padded.numel() != wt_padded.shape[0]:
        raise ValueError("x must be [M, K], wt_padded [Npad, K], bias_padded [Npad]")
    M, K = x.shape
    act = {"none": 0, "relu": 1, "tanh": 2}[activation]
    y = torch.empty((M, int(out_features)), dtype=torch.float32, device=x.device)
    y2 = torch.empty_like(y) if act == 2 else None
    nr = _dev(num_rows, "num_rows", torch.int32) if num_rows is not None else None
    call("pcnn_fc_rows_cols_fwd", _ptr(x), _ptr(wt_padded), _ptr(bias_padded), M, K, wt_padded.shape[0], int(out_features), act,
         _ptr(nr), _ptr(y), _ptr(y2), _stream(x))
    return (y, y2) if act == 2 else y


_tickets = {}


def _ticket_buffer(device, n):
    """int32 ticket counters of the split-K kernels that finish in their last workgroup: zero on entry, zero on
    exit (the kernel resets them), so one zero-filled buffer per stream serves every launch on that stream."""
    k = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _tickets.get(k)
    if buf is None or buf.numel() < n:
        buf = torch.zeros(max(int(n), 256), dtype=torch.int32, device=device)
        _tickets[k] = buf
    return buf


# The crossover between the two few-row paths of fc6 / fc7 / fc8: at or below it csrc/fc_skinny.hip streams the
# weights with split-K over the whole chip; above it `fc_rows` / `fc_rows_cols` take the layer on 64-row blocks. fc8 through
# `fc_rows_cols` has no split-K: with tens of live rows a couple of workgroups stream its padded 128 x 4096 filter (2 MB) —
# ~10 us, launch-bound either way, and only cheaper per row from there.
SKINNY_MAX_ROWS = 32


def fc_skinny(x, wt, bias, activation="none", num_rows=None):
    """`Network.fc` for <= 32 rows (the single-frame loop): y = act(x @ wt.T + bias) as one weight-streaming
    launch (csrc/fc_skinny.hip). x [M <= 32, K % 16 == 0], wt [N, K] (the TF weight transposed), bias [N].
    activation "none" | "relu" | "tanh"; "tanh" returns (linear, tanh(linear)) — fc8 and poses_tanh."""
    x = _dev(x, "x", torch.float32)
    wt = _dev(wt, "wt", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    if x.dim() != 2 or wt.dim() != 2 or wt.shape[1] != x.shape[1] or bias.numel() != wt.shape[0]:
        raise ValueError("x must be [M, K], wt [N, K], bias [N]")
    act = {"none": 0, "relu": 1, "tanh": 2}[activation]
    M, K = x.shape
    N = wt.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    y2 = torch.empty((M, N), dtype=torch.float32, device=x.device) if act == 2 else None
    nr = _dev(num_rows, "num_rows", torch.int32) if num_rows is not None else None
    nbytes, ncnt = ctypes.c_size_t(), ctypes.c_int()
    call("pcnn_fc_skinny_workspace_bytes", M, K, N, ctypes.byref(nbytes), ctypes.byref(ncnt))
    ws = _ws(x.device, "fc_skinny").get(nbytes.value, x.device)
    cnt = _ticket_buffer(x.device, ncnt.value)
    call("pcnn_fc_skinny_fwd", _ptr(x), _ptr(wt), _ptr(bias), M, K, N, act, _ptr(nr), _ptr(y), _ptr(y2), _ptr(ws), nbytes.value,
         _ptr(cnt), cnt.numel(), _stream(x))
    return (y, y2) if act == 2 else y


def _head_lowres_args(score4, score5, filt, filt_name, planted, stride):
    """What `head_lowres` and `head_lowres_mfma` check and allocate alike: the tensors on the device, the dimensions of score4,
    whether score5, the 2-D filter and `planted` fit them (each wrapper adds its own filter shape and raises), and `add`."""
    score4 = _dev(score4, "score4", torch.float32)
    score5 = _dev(score5, "score5", torch.float32)
    filt = _dev(filt, filt_name, torch.float32)
    pl = _dev(planted, "planted", torch.float32) if planted is not None else None
    B, h, w, U = score4.shape
    fits = (tuple(score5.shape) == (B, h // stride, w // stride, U) and filt.dim() == 2
            and (pl is None or tuple(pl.shape) == tuple(score4.shape)))
    return score4, score5, filt, pl, B, h, w, U, fits, torch.empty_like(score4)


def head_lowres(score4, score5, weights_t, planted=None, kernel=4, stride=2):
    """add = score4 + deconv_{kernel,stride}(score5) [+ planted]; z = add . weights_t (1x1 conv, no bias) in one
    launch. score4 [B,h,w,U], score5 [B,h/stride,w/stride,U], weights_t [U, Cout] -> (add [B,h,w,U], z [B,h,w,Cout])."""
    score4, score5, weights_t, pl, B, h, w, U, fits, add = _head_lowres_args(score4, score5, weights_t, "weights_t", planted, stride)
    if not fits or weights_t.shape[0] != U:
        raise ValueError("score4 [B,h,w,U], score5 [B,h/s,w/s,U], weights_t [U,Cout], planted like score4")
    Cout = weights_t.shape[1]
    z = torch.empty((B, h, w, Cout), dtype=torch.float32, device=score4.device)
    call("pcnn_head_lowres_fwd", _ptr(score4), _ptr(score5), _ptr(pl), _ptr(weights_t), B, h, w, U, Cout, int(kernel), int(stride),
         _ptr(add), _ptr(z), _stream(score4))
    return add, z


def head_lowres_mfma_filter(weights_t):
    """The filter of `head_lowres_mfma`: weights_t [U, Cout] (the TF variable [1,1,U,Cout] as it is) -> [ceil(Cout/16)*16, U],
    N-major with K contiguous, zero rows past Cout (cache it per weight version)."""
    U, Cout = weights_t.shape
    npad = (Cout + 15) // 16 * 16
    w = torch.zeros((npad, U), dtype=torch.float32, device=weights_t.device)
    w[:Cout] = weights_t.t()
    return w


def head_lowres_mfma(score4, score5, weights_nk, out_channels, planted=None, kernel=4, stride=2):
    """`head_lowres` for many pixels per launch: the same add (bit-identical `add`), the 1x1 product on the matrix cores.
    weights_nk from `head_lowres_mfma_filter`. U % 16 == 0, out_channels <= 96."""
    score4, score5, weights_nk, pl, B, h, w, U, fits, add = _head_lowres_args(score4, score5, weights_nk, "weights_nk", planted, stride)
    Cout = int(out_channels)
    if not fits or tuple(weights_nk.shape) != ((Cout + 15) // 16 * 16, U):
        raise ValueError("score4 [B,h,w,U], score5 [B,h/s,w/s,U], weights_nk [ceil(Cout/16)*16, U], planted like score4")
    z = torch.empty((B, h, w, Cout), dtype=torch.float32, device=score4.device)
    call("pcnn_head_lowres_mfma_fwd", _ptr(score4), _ptr(score5), _ptr(pl), _ptr(weights_nk), B, h, w, U, Cout, int(kernel),
         int(stride), _ptr(add), _ptr(z), _stream(score4))
    return add, z


def pose_l2_normalize(poses_tanh, poses_weight, num_rows=None):
    """poses_pred = l2_normalize(poses_tanh * poses_weight, dim=1) (vgg16_convs.py:195-197) in one launch; rows at or past
    the device-side count are zeros."""
    x = _dev(poses_tanh, "poses_tanh", torch.float32)
    w = _dev(poses_weight, "poses_weight", torch.float32)
    if x.dim() != 2 or tuple(w.shape) != tuple(x.shape):
        raise ValueError("poses_tanh and poses_weight must be [R, 4C]")
    nr = _dev(num_rows, "num_rows", torch.int32) if num_rows is not None else None
    out = torch.empty_like(x)
    call("pcnn_pose_l2_normalize_fwd", _ptr(x), _ptr(w), _ptr(nr), x.shape[0], x.shape[1], _ptr(out), _stream(x))
    return out


def det_assemble(rois, poses_tanh, top_pose, num_rows, row_stride=1, frame_offset=None):
    """lib/fcn/test.py:206-211 on the device: rows [ceil(R / stride), 14] = box7 | quaternion of the row's class |
    translation, zeros past the device-side count; count [1] int32 = *num_rows // stride.
    With `frame_offset` (a rank's first global frame index) the same launch writes the block that rank hands to the
    detection all-gather — rows with column 0 shifted to global frame numbering + a last row (count, 0, ...) — and
    returns (rows, count, block) with `rows` a view of the block's first rows. Rows are written, and shifted in the block,
    for every i * stride < *num_rows; when that count is no multiple of the stride, the partial last group's row is written
    but not counted (count = *num_rows // stride)."""
    rois = _dev(rois, "rois", torch.float32)
    poses_tanh = _dev(poses_tanh, "poses_tanh", torch.float32)
    top_pose = _dev(top_pose, "top_pose", torch.float32)
    nr = _dev(num_rows, "num_rows", torch.int32)
    R = rois.shape[0]
    if rois.dim() != 2 or rois.shape[1] != 7 or tuple(top_pose.shape) != (R, 7) or poses_tanh.shape[0] != R or poses_tanh.shape[1] % 4:
        raise ValueError("rois [R,7], top_pose [R,7], poses_tanh [R,4C]")
    n_out = (R + row_stride - 1) // row_stride
    count = torch.empty((1,), dtype=torch.int32, device=rois.device)
    if frame_offset is not None:
        block = torch.empty((n_out + 1, 14), dtype=torch.float32, device=rois.device)
        call("pcnn_det_assemble_packed_fwd", _ptr(rois), _ptr(poses_tanh), _ptr(top_pose), _ptr(nr), R, int(row_stride),
             poses_tanh.shape[1] // 4, float(frame_offset), _ptr(block), _ptr(count), _stream(rois))
        return block[:n_out], count, block
    rows = torch.empty((n_out, 14), dtype=torch.float32, device=rois.device)
    call("pcnn_det_assemble_fwd", _ptr(rois), _ptr(poses_tanh), _ptr(top_pose), _ptr(nr), R, int(row_stride),
         poses_tanh.shape[1] // 4, _ptr(rows), _ptr(count), _stream(rois))
    return rows, count


def conv3x3_winograd(x, u, bias, relu=True, pool=False, tile=2):
    """3x3 / stride 1 / SAME convolution + bias [+ ReLU] [+ 2x2 max-pool] as Winograd F(tile x tile, 3x3):
    input transform (gfx950 kernel) -> (tile+2)^2 fp32 GEMMs (library, MFMA) -> output transform
    (gfx950 kernel). `u` comes from `winograd_filter(weights, tile)`."""
    B, H, W, _ = x.shape
    v = winograd_input(x, tile)
    m = torch.bmm(v, u)
    return winograd_output(m, bias, B, H, W, relu, pool, tile)


def bias_relu_pool2(x, bias, relu=True):
    """max_pool_2x2(ReLU(x + bias)) from the raw convolution output [B,H,W,C] (H, W even)."""
    x = _dev(x, "x", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    B, H, W, C = x.shape
    if bias.numel() != C:
        raise ValueError("bias must have one entry per channel")
    y = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    call("pcnn_bias_relu_pool2_fwd", _ptr(x), _ptr(bias), B, H, W, C, 1 if relu else 0, _ptr(y), _stream(x))
    return y


def _deconv_bilinear_raw(input, kernel, stride, add1=None, add2=None, bias=None, relu=False):
    input = _dev(input, "input", torch.float32)
    if input.dim() != 4:
        raise ValueError("deconv input must be 4-dimensional")
    B, H, W, C = input.shape
    out = torch.empty((B, H * stride, W * stride, C), dtype=torch.float32, device=input.device)
    a1 = _dev(add1, "add1", torch.float32) if add1 is not None else None
    a2 = _dev(add2, "add2", torch.float32) if add2 is not None else None
    bs = _dev(bias, "bias", torch.float32) if bias is not None else None
    for t in (a1, a2):
        if t is not None and tuple(t.shape) != tuple(out.shape):
            raise ValueError("addend must have the output shape %s" % (tuple(out.shape),))
    call("pcnn_deconv_bilinear_fwd", _ptr(input), B, H, W, C, int(kernel), int(stride), _ptr(a1), _ptr(a2), _ptr(bs),
         1 if relu else 0, _ptr(out), _stream(input))
    return out


def deconv_bilinear_grad(grad_out, kernel, stride):
    """Gradient of `deconv_bilinear` w.r.t. its input: [B,H*s,W*s,C] -> [B,H,W,C]."""
    grad_out = _dev(grad_out, "grad_out", torch.float32)
    B, Ho, Wo, C = grad_out.shape
    if Ho % stride or Wo % stride:
        raise ValueError("grad_out is not a multiple of the stride")
    gin = torch.empty((B, Ho // stride, Wo // stride, C), dtype=torch.float32, device=grad_out.device)
    call("pcnn_deconv_bilinear_bwd", _ptr(grad_out), B, Ho // stride, Wo // stride, C, int(kernel), int(stride), _ptr(gin),
         _stream(grad_out))
    return gin


class _DeconvBilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, kernel, stride):
        ctx.ks = (kernel, stride)
        return _deconv_bilinear_raw(input, kernel, stride)

    @staticmethod
    def backward(ctx, grad_out):
        return deconv_bilinear_grad(grad_out.contiguous(), *ctx.ks), None, None


def deconv_bilinear(input, kernel, stride, add1=None, add2=None, bias=None, relu=False):
    """The fixed bilinear `deconv` layer (network.py:207-222 with make_deconv_filter :141-157) as a
    per-channel interpolation: [B,H,W,C] -> [B,H*s,W*s,C], optionally fused with up to two addends
    (same shape as the output), a per-channel bias and ReLU. Differentiable w.r.t. `input` (the
    filter is not trainable in the reference: deconv(..., trainable=False)); when a gradient is
    needed the extras are applied as separate framework ops."""
    needs_grad = torch.is_grad_enabled() and any(
        isinstance(t, torch.Tensor) and t.requires_grad for t in (input, add1, add2, bias))
    if not needs_grad:
        return _deconv_bilinear_raw(input, kernel, stride, add1, add2, bias, relu)
    out = _DeconvBilinearFn.apply(_dev(input, "input", torch.float32), int(kernel), int(stride))
    for t in (add1, add2, bias):
        if t is not None:
            out = out + t
    return torch.relu(out) if relu else out


class _SmoothL1VertexFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, sigma):
        n = pred.numel()
        out = torch.empty(3, dtype=torch.float32, device=pred.device)
        ws, _ = _workspace(pred.device, "smooth_l1", "pcnn_smooth_l1_vertex_workspace_bytes")
        call("pcnn_smooth_l1_vertex_fwd", _ptr(pred), _ptr(target), _ptr(weight), n, float(sigma), _ptr(out), _ptr(ws), ws.numel(),
             _stream(pred))
        ctx.save_for_backward(pred, target, weight, out)
        ctx.sigma = float(sigma)
        return out[0], out[1:].clone()

    @staticmethod
    def backward(ctx, grad_loss, _grad_sums):
        pred, target, weight, out = ctx.saved_tensors
        grad = torch.empty_like(pred)
        up = grad_loss.reshape(1).to(torch.float32).contiguous()
        call("pcnn_smooth_l1_vertex_bwd", _ptr(pred), _ptr(target), _ptr(weight), _ptr(out), _ptr(up), pred.numel(), ctx.sigma,
             _ptr(grad), _stream(pred))
        return grad, None, None, None


def smooth_l1_loss_vertex(vertex_pred, vertex_targets, vertex_weights, sigma=1.0):
    """lib/fcn/train.py:564-573 as two streaming kernels (forward, backward w.r.t. vertex_pred).
    Returns the scalar loss = sum(in_loss) / (sum(weights) + 1e-10)."""
    pred = _dev(vertex_pred, "vertex_pred", torch.float32)
    target = _dev(vertex_targets, "vertex_targets", torch.float32)
    weight = _dev(vertex_weights, "vertex_weights", torch.float32)
    if pred.shape != target.shape or pred.shape != weight.shape:
        raise ValueError("vertex_pred, vertex_targets and vertex_weights must have the same shape")
    return _SmoothL1VertexFn.apply(pred, target, weight, float(sigma))[0]


def _vertex_gt_args(gt_label_2d, objects, instance):
    """(label int32 [B,H,W], objects f32 [B,M,6], instance int32 [B,H,W] | None) of include/posecnn_hip_train.h, checked."""
    label = _dev(gt_label_2d, "gt_label_2d", torch.int32)
    obj = _dev(objects, "objects", torch.float32)
    if label.dim() != 3:
        raise ValueError("gt_label_2d must be [B,H,W] (got %s)" % (tuple(label.shape),))
    if obj.dim() != 3 or obj.shape[0] != label.shape[0] or obj.shape[2] != 6:
        raise ValueError("objects must be [B,M,6] with B = %d (got %s)" % (label.shape[0], tuple(obj.shape)))
    if instance is not None:
        instance = _dev(instance, "instance", torch.int32)
        if instance.shape != label.shape:
            raise ValueError("instance must have the shape of gt_label_2d")
    return label, obj, instance


def vertex_targets(gt_label_2d, objects, num_classes, instance=None):
    """lib/gt_synthesize_layer/minibatch.py:543-602 (`_generate_vertex_targets`, VERTEX_REG_2D) on the device:
    gt_label_2d int32 [B,H,W], objects f32 [B,M,6] rows (cls, mask_id, cx, cy, log_z, w) as `datasets.training_blobs`
    builds them, instance int32 [B,H,W] (multi-instance frames) -> (vertex_targets, vertex_weights) f32 [B,H,W,3C],
    numpy's bits. Training itself does not need them: `smooth_l1_loss_vertex_gt` takes the same three inputs."""
    label, obj, instance = _vertex_gt_args(gt_label_2d, objects, instance)
    B, H, W = label.shape
    C = int(num_classes)
    targets = torch.empty((B, H, W, 3 * C), dtype=torch.float32, device=label.device)
    weights = torch.empty((B, H, W, 3 * C), dtype=torch.float32, device=label.device)
    call("pcnn_vertex_targets_fwd", _ptr(label), _ptr(instance), _ptr(obj), B, H, W, C, obj.shape[1], _ptr(targets), _ptr(weights),
         _stream(label))
    return targets, weights


class _SmoothL1VertexGtFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label, instance, obj, sigma):
        B, H, W, C3 = pred.shape
        out = torch.empty(3, dtype=torch.float32, device=pred.device)
        ws, _ = _workspace(pred.device, "smooth_l1", "pcnn_smooth_l1_vertex_workspace_bytes")
        call("pcnn_smooth_l1_vertex_gt_fwd", _ptr(pred), _ptr(label), _ptr(instance), _ptr(obj), B, H, W, C3 // 3, obj.shape[1],
             float(sigma), _ptr(out), _ptr(ws), ws.numel(), _stream(pred))
        ctx.save_for_backward(pred, label, obj, out, instance)
        ctx.sigma = float(sigma)
        return out[0], out[1:].clone()

    @staticmethod
    def backward(ctx, grad_loss, _grad_sums):
        pred, label, obj, out, instance = ctx.saved_tensors
        B, H, W, C3 = pred.shape
        grad = torch.empty_like(pred)
        up = grad_loss.reshape(1).to(torch.float32).contiguous()
        call("pcnn_smooth_l1_vertex_gt_bwd", _ptr(pred), _ptr(label), _ptr(instance), _ptr(obj), _ptr(out), _ptr(up), B, H, W,
             C3 // 3, obj.shape[1], ctx.sigma, _ptr(grad), _stream(pred))
        return grad, None, None, None, None


def smooth_l1_loss_vertex_gt(vertex_pred, gt_label_2d, objects, instance=None, sigma=1.0):
    """`smooth_l1_loss_vertex(vertex_pred, *vertex_targets(gt_label_2d, objects, C, instance), sigma)` — the same bits,
    forward and backward — without the two [B,H,W,3C] tensors: both kernels read the label map and the object table.
    vertex_pred must be finite where the weight is zero (include/posecnn_hip_train.h)."""
    pred = _dev(vertex_pred, "vertex_pred", torch.float32)
    label, obj, instance = _vertex_gt_args(gt_label_2d, objects, instance)
    if pred.dim() != 4 or pred.shape[:3] != label.shape or pred.shape[3] % 3 != 0:
        raise ValueError("vertex_pred must be [B,H,W,3C] over gt_label_2d %s (got %s)" % (tuple(label.shape), tuple(pred.shape)))
    return _SmoothL1VertexGtFn.apply(pred, label, instance, obj, float(sigma))[0]



def upscore_softmax_argmax(z, bias, kernel, stride, relu=True, want_score=False, want_prob=True, hard_gt=None,
                           hard_threshold=None):
    """Label-head epilogue in one pass: score = [ReLU](deconv(z) + bias) -> softmax -> first argmax.
    z [B,H,W,C] f32. Returns (score or None, prob or None, label int32 [B,H*s,W*s]); with `hard_gt` (int32
    [B,H*s,W*s]) and `hard_threshold` a fourth element: hard_label(prob, hard_gt, hard_threshold) f32 [B,H*s,W*s,C]
    from the same launch (no gradient flows through the Hardlabel op: hard_label_op_gpu.cu.cc:55-63)."""
    z = _dev(z, "z", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    B, H, W, C = z.shape
    Ho, Wo = H * stride, W * stride
    dev = z.device
    score = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=dev) if want_score else None
    prob = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=dev) if want_prob else None
    label = torch.empty((B, Ho, Wo), dtype=torch.int32, device=dev)
    if hard_gt is not None:
        if hard_threshold is None:
            raise ValueError("hard_gt needs hard_threshold (the Hardlabel op's `threshold` attribute)")
        # the Hardlabel op on the probabilities of the same launch (vgg16_convs.py:148-149): same bits as
        # hard_label(prob, gt, threshold), 432 MB of stores per 16 frames that fit under the head's own arithmetic
        gt = _dev(hard_gt, "hard_gt", torch.int32)
        if tuple(gt.shape) != (B, Ho, Wo):
            raise ValueError("hard_gt must be int32 [B, H*stride, W*stride]")
        hard = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=dev)
        call("pcnn_upscore_softmax_argmax_hard_fwd", _ptr(z), _ptr(bias), B, H, W, C, int(kernel), int(stride), 1 if relu else 0,
             _ptr(score), _ptr(prob), _ptr(label), _ptr(gt), float(hard_threshold), _ptr(hard), _stream(z))
        return score, prob, label, hard
    call("pcnn_upscore_softmax_argmax_fwd", _ptr(z), _ptr(bias), B, H, W, C, int(kernel), int(stride), 1 if relu else 0,
         _ptr(score), _ptr(prob), _ptr(label), _stream(z))
    return score, prob, label


def _label_head_loss_args(z, bias, gt_label_2d, kernel, stride):
    z = _dev(z, "z", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    gt = _dev(gt_label_2d, "gt_label_2d", torch.int32)
    if z.dim() != 4 or bias.dim() != 1 or bias.shape[0] != z.shape[3]:
        raise ValueError("z must be [B,H,W,C] and bias [C] (got %s, %s)" % (tuple(z.shape), tuple(bias.shape)))
    B, H, W, C = z.shape
    if tuple(gt.shape) != (B, H * stride, W * stride):
        raise ValueError("gt_label_2d must be int32 [B, H*stride, W*stride] = %s (got %s)"
                         % ((B, H * stride, W * stride), tuple(gt.shape)))
    ws, _ = _workspace(z.device, "label_head_loss", "pcnn_label_head_loss_workspace_bytes", B, H, W, C, int(kernel), int(stride))
    return z, bias, gt, ws


def _label_head_loss_raw(z, bias, gt_label_2d, threshold, kernel, stride, relu=True, want_terms=False):
    """-> (loss f32 [], sums f64 [2] = (S, count), label_2d int32 [B,Ho,Wo], terms f32 [B,Ho,Wo] | None): one call of
    pcnn_label_head_loss_fwd (include/posecnn_hip_loss.h)."""
    z, bias, gt, ws = _label_head_loss_args(z, bias, gt_label_2d, kernel, stride)
    B, H, W, C = z.shape
    dev = z.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    label = torch.empty(gt.shape, dtype=torch.int32, device=dev)
    terms = torch.empty(gt.shape, dtype=torch.float32, device=dev) if want_terms else None
    call("pcnn_label_head_loss_fwd", _ptr(z), _ptr(bias), _ptr(gt), B, H, W, C, int(kernel), int(stride), 1 if relu else 0,
         float(threshold), _ptr(loss), _ptr(sums), _ptr(label), _ptr(terms), _ptr(ws), ws.numel(), _stream(z))
    return loss, sums, label, terms


def label_head_loss_grad(z, bias, gt_label_2d, threshold, kernel, stride, relu=True, upstream=None, sums=None):
    """The backward kernel of `label_head_loss` on its own: -> (dscore f32 [B,H*s,W*s,C], dbias f32 [C]), the gradient of
    upstream * loss w.r.t. the full-resolution score and the bias; `deconv_bilinear_grad(dscore, kernel, stride)` is the
    one w.r.t. z. `upstream` is a one-element f32 tensor on the device (None: 1), `sums` what the forward saved (None: the
    forward is run for it)."""
    if sums is None:
        sums = _label_head_loss_raw(z, bias, gt_label_2d, threshold, kernel, stride, relu)[1]
    z, bias, gt, ws = _label_head_loss_args(z, bias, gt_label_2d, kernel, stride)
    sums = _dev(sums, "sums", torch.float64)
    up = _dev(upstream, "upstream", torch.float32).reshape(1) if upstream is not None else None
    B, H, W, C = z.shape
    dscore = torch.empty(tuple(gt.shape) + (C,), dtype=torch.float32, device=z.device)
    dbias = torch.empty(C, dtype=torch.float32, device=z.device)
    call("pcnn_label_head_loss_bwd", _ptr(z), _ptr(bias), _ptr(gt), _ptr(sums), _ptr(up), B, H, W, C, int(kernel), int(stride),
         1 if relu else 0, float(threshold), _ptr(dscore), _ptr(dbias), _ptr(ws), ws.numel(), _stream(z))
    return dscore, dbias


class _LabelHeadLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, bias, gt, threshold, kernel, stride, relu, want_terms):
        loss, sums, label, terms = _label_head_loss_raw(z, bias, gt, threshold, kernel, stride, relu, want_terms)
        ctx.save_for_backward(z, bias, gt, sums)
        ctx.cfg = (threshold, kernel, stride, relu)
        ctx.mark_non_differentiable(label)
        if terms is None:
            return loss, label
        ctx.mark_non_differentiable(terms)
        return loss, label, terms

    @staticmethod
    def backward(ctx, grad_loss, *_unused):
        z, bias, gt, sums = ctx.saved_tensors
        threshold, kernel, stride, relu = ctx.cfg
        up = grad_loss.reshape(1).to(torch.float32).contiguous()
        dscore, dbias = label_head_loss_grad(z, bias, gt, threshold, kernel, stride, relu, upstream=up, sums=sums)
        dz = deconv_bilinear_grad(dscore, kernel, stride)
        return dz, dbias, None, None, None, None, None, None


def label_head_loss(z, bias, gt_label_2d, threshold, kernel, stride, relu=True, want_terms=False):
    """The label head of the training graph in one pass from the 1/8-resolution class scores z [B,H,W,C] (without bias):
    score = [ReLU](deconv(z) + bias) -> softmax -> first argmax, the Hardlabel rule on (prob, gt_label_2d, threshold) and
    loss_cross_entropy_single_frame (lib/fcn/train.py:41-44) over its weights, without a [B,H*s,W*s,C] tensor.
    Returns (loss f32 [], label_2d int32 [B,H*s,W*s]) and, with `want_terms`, the per-pixel terms f32 [B,H*s,W*s].
    Differentiable w.r.t. z and bias; no gradient flows through the Hardlabel rule or the argmax, as the reference
    registers them (hard_label_op_gpu.cu.cc:55-63)."""
    z = _dev(z, "z", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    gt = _dev(gt_label_2d, "gt_label_2d", torch.int32)
    return _LabelHeadLossFn.apply(z, bias, gt, float(threshold), int(kernel), int(stride), bool(relu), bool(want_terms))


def _vertex_head_loss_args(z, bias, gt_label_2d, objects, instance, kernel, stride):
    z = _dev(z, "z", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    label, obj, instance = _vertex_gt_args(gt_label_2d, objects, instance)
    if z.dim() != 4 or z.shape[3] % VERTEX_CHANNELS or bias.dim() != 1 or bias.shape[0] != z.shape[3]:
        raise ValueError("z must be [B,H,W,3C] and bias [3C] (got %s, %s)" % (tuple(z.shape), tuple(bias.shape)))
    B, H, W, C3 = z.shape
    if tuple(label.shape) != (B, H * stride, W * stride):
        raise ValueError("gt_label_2d must be int32 [B, H*stride, W*stride] = %s (got %s)"
                         % ((B, H * stride, W * stride), tuple(label.shape)))
    ws, _ = _workspace(z.device, "vertex_head_loss", "pcnn_vertex_head_loss_workspace_bytes", B, H, W, C3 // VERTEX_CHANNELS,
                       int(kernel), int(stride))
    return z, bias, label, obj, instance, ws


def _vertex_head_loss_raw(z, bias, gt_label_2d, objects, kernel, stride, instance=None, sigma=1.0):
    """-> out f32 [3] = (loss, sum(in_loss), sum(w)): one call of pcnn_vertex_head_loss_fwd (include/posecnn_hip_vertex_loss.h)."""
    z, bias, label, obj, instance, ws = _vertex_head_loss_args(z, bias, gt_label_2d, objects, instance, kernel, stride)
    B, H, W, C3 = z.shape
    out = torch.empty(3, dtype=torch.float32, device=z.device)
    call("pcnn_vertex_head_loss_fwd", _ptr(z), _ptr(bias), _ptr(label), _ptr(instance), _ptr(obj), B, H, W, C3 // VERTEX_CHANNELS,
         obj.shape[1], int(kernel), int(stride), float(sigma), _ptr(out), _ptr(ws), ws.numel(), _stream(z))
    return out


def vertex_head_loss_grad(z, bias, gt_label_2d, objects, kernel, stride, instance=None, sigma=1.0, upstream=None, out=None):
    """The backward kernel of `vertex_head_loss` on its own: -> (dz f32 [B,H,W,3C], dbias f32 [3C]), the gradient of
    upstream * loss w.r.t. the low-resolution field and the bias. `upstream` is a one-element f32 tensor on the device
    (None: 1), `out` the three floats the forward saved (None: the forward is run for them)."""
    if out is None:
        out = _vertex_head_loss_raw(z, bias, gt_label_2d, objects, kernel, stride, instance, sigma)
    z, bias, label, obj, instance, ws = _vertex_head_loss_args(z, bias, gt_label_2d, objects, instance, kernel, stride)
    out = _dev(out, "out", torch.float32)
    up = _dev(upstream, "upstream", torch.float32).reshape(1) if upstream is not None else None
    B, H, W, C3 = z.shape
    dz = torch.empty_like(z)
    dbias = torch.empty(C3, dtype=torch.float32, device=z.device)
    call("pcnn_vertex_head_loss_bwd", _ptr(z), _ptr(bias), _ptr(label), _ptr(instance), _ptr(obj), _ptr(out), _ptr(up), B, H, W,
         C3 // VERTEX_CHANNELS, obj.shape[1], int(kernel), int(stride), float(sigma), _ptr(dz), _ptr(dbias), _ptr(ws), ws.numel(),
         _stream(z))
    return dz, dbias


class _VertexHeadLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, bias, label, obj, instance, kernel, stride, sigma):
        out = _vertex_head_loss_raw(z, bias, label, obj, kernel, stride, instance, sigma)
        ctx.save_for_backward(z, bias, label, obj, out, instance)
        ctx.cfg = (kernel, stride, sigma)
        return out[0], out[1:].clone()

    @staticmethod
    def backward(ctx, grad_loss, _grad_sums):
        z, bias, label, obj, out, instance = ctx.saved_tensors
        kernel, stride, sigma = ctx.cfg
        up = grad_loss.reshape(1).to(torch.float32).contiguous()
        dz, dbias = vertex_head_loss_grad(z, bias, label, obj, kernel, stride, instance, sigma, upstream=up, out=out)
        return dz, dbias, None, None, None, None, None, None


def vertex_head_loss(z, bias, gt_label_2d, objects, kernel, stride, instance=None, sigma=1.0):
    """The vertex head of the training graph from the 1/stride-resolution field z [B,H,W,3C] (without bias):
    `smooth_l1_loss_vertex_gt(deconv_bilinear(z, kernel, stride) + bias, gt_label_2d, objects, instance, sigma)` — the same
    bits, loss and gradient w.r.t. z — without vertex_pred [B,H*s,W*s,3C] or its gradient ever being written: the
    interpolation runs only under a matching row, for the three channels that carry weight. Returns (loss f32 [],
    sums f32 [2] = (sum(in_loss), sum(w))). Differentiable w.r.t. z and bias; z and bias must be finite."""
    z, bias, label, obj, instance, _ = _vertex_head_loss_args(z, bias, gt_label_2d, objects, instance, kernel, stride)
    return _VertexHeadLossFn.apply(z, bias, label, obj, instance, int(kernel), int(stride), float(sigma))


# ---- the trunk's training epilogues (include/posecnn_hip_trunk_train.h, csrc/trunk_epilogue.hip) ---------------------------
def _channels_first(t):
    """Is `t` a 4-D [B,C,H,W] tensor whose memory is NHWC-dense (channels_last) — what the framework's convolution returns
    for the NHWC activations of this package? The epilogues take it as it is: an NHWC *view* of it could not be written in
    place without autograd copying the whole tensor back and forth. A tensor that is contiguous as it stands is NHWC."""
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def _trunk_dbias_ws(fn_name, shape, device, want):
    if not want:
        return None, None
    return torch.empty(shape[-1], dtype=torch.float32, device=device), _workspace(device, "trunk_epilogue", fn_name, *shape)[0]


def bias_relu_train_grad(da, a, relu=True, want_dbias=True):
    """The backward kernel of `bias_relu_train_` on its own: -> (dy, dbias f32 [C] | None) from the gradient `da` and the
    layer's output `a`, both [..., C] contiguous (`a` may be None when `relu` is off): dy = relu ? (a > 0 ? da : 0) : da,
    dbias the sum of dy over pixels in the order of the header."""
    da = _dev(da, "da", torch.float32)
    a = _dev(a, "a", torch.float32) if a is not None else None
    if relu and (a is None or a.shape != da.shape):
        raise ValueError("a must have da's shape %s (got %s)" % (tuple(da.shape), None if a is None else tuple(a.shape)))
    if da.dim() < 2:
        raise ValueError("da must be [..., C]")
    C = da.shape[-1]
    rows = da.numel() // C
    dy = torch.empty_like(da)
    dbias, ws = _trunk_dbias_ws("pcnn_bias_relu_train_workspace_bytes", (rows, C), da.device, want_dbias)
    call("pcnn_bias_relu_train_bwd", _ptr(da), _ptr(a if relu else None), rows, C, 1 if relu else 0, _ptr(dy), _ptr(dbias),
         _ptr(ws), ws.numel() if ws is not None else 0, _stream(da))
    return dy, dbias


class _BiasReluTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bias, relu):
        cf = _channels_first(y)
        bias_act_(y.permute(0, 2, 3, 1) if cf else y, bias, relu)
        ctx.mark_dirty(y)
        ctx.cfg = (relu, cf)
        ctx.save_for_backward(*((y,) if relu else ()))
        return y

    @staticmethod
    def backward(ctx, grad):
        relu, cf = ctx.cfg
        a = ctx.saved_tensors[0] if relu else None
        if cf:
            grad, a = grad.permute(0, 2, 3, 1), (a.permute(0, 2, 3, 1) if relu else None)
        dy, dbias = bias_relu_train_grad(grad, a, relu, want_dbias=ctx.needs_input_grad[1])
        return (dy.permute(0, 3, 1, 2) if cf else dy), dbias, None


def bias_relu_train_(y, bias, relu=True):
    """`bias_act_` under autograd: in place y[..., c] = [ReLU](y[..., c] + bias[c]), differentiable w.r.t. y and bias, one
    kernel each way; the output itself is what the backward keeps. `y` is NHWC-contiguous [..., C], or the channels_last
    [B,C,H,W] result of a framework convolution (returned in the same form); it must not be a leaf that requires grad."""
    y = _dev_dense(y, "y")
    bias = _dev(bias, "bias", torch.float32)
    C = y.shape[1] if _channels_first(y) else y.shape[-1]
    if bias.dim() != 1 or bias.numel() != C:
        raise ValueError("bias must have one entry per channel (%d, got %s)" % (C, tuple(bias.shape)))
    return _BiasReluTrainFn.apply(y, bias, bool(relu))


def _dev_dense(t, name):
    """`_dev` without its copy: the in-place epilogues write the tensor they are given."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        _dev(t, name, torch.float32)
    if not (t.is_contiguous() or _channels_first(t)):
        raise ValueError("%s must be contiguous as NHWC, or channels_last as [B,C,H,W] (got strides %s)" % (name, t.stride()))
    return t


def _bias_relu_pool2_train_raw(y, bias, relu=True, want_act=False):
    """-> (act | None, pooled f32 [B,H/2,W/2,C], sel u8 [B,H/2,W/2,C]): one call of pcnn_bias_relu_pool2_train_fwd on the
    NHWC-contiguous y; with `want_act`, act IS y, overwritten."""
    y = _dev(y, "y", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    if y.dim() != 4 or bias.dim() != 1 or bias.shape[0] != y.shape[3]:
        raise ValueError("y must be [B,H,W,C] and bias [C] (got %s, %s)" % (tuple(y.shape), tuple(bias.shape)))
    B, H, W, C = y.shape
    pooled = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=y.device)
    sel = torch.empty((B, H // 2, W // 2, C), dtype=torch.uint8, device=y.device)
    act = y if want_act else None
    call("pcnn_bias_relu_pool2_train_fwd", _ptr(y), _ptr(bias), B, H, W, C, 1 if relu else 0, _ptr(act), _ptr(pooled), _ptr(sel),
         _stream(y))
    return act, pooled, sel


def bias_relu_pool2_train_grad(dpooled, sel, dact=None, act=None, want_dbias=True):
    """The backward kernel of `bias_relu_pool2_train` on its own: -> (dy f32 [B,H,W,C], dbias f32 [C] | None) from dpooled
    f32 and sel u8 [B,H/2,W/2,C] and, for the dual form, the gradient and the value of the activated tensor [B,H,W,C]:
    dy_k = (act_k > 0 ? dact_k : 0) + (sel == k ? dpooled : 0)."""
    dpooled = _dev(dpooled, "dpooled", torch.float32)
    sel = _dev(sel, "sel", torch.uint8)
    if dpooled.dim() != 4 or sel.shape != dpooled.shape:
        raise ValueError("dpooled and sel must both be [B,H/2,W/2,C] (got %s, %s)" % (tuple(dpooled.shape), tuple(sel.shape)))
    B, Ho, Wo, C = dpooled.shape
    H, W = 2 * Ho, 2 * Wo
    if (dact is None) != (act is None):
        raise ValueError("dact and act are both None or both given")
    if dact is not None:
        dact, act = _dev(dact, "dact", torch.float32), _dev(act, "act", torch.float32)
        if tuple(dact.shape) != (B, H, W, C) or act.shape != dact.shape:
            raise ValueError("dact and act must be %s (got %s, %s)" % ((B, H, W, C), tuple(dact.shape), tuple(act.shape)))
    dy = torch.empty((B, H, W, C), dtype=torch.float32, device=dpooled.device)
    dbias, ws = _trunk_dbias_ws("pcnn_bias_relu_pool2_train_workspace_bytes", (B, H, W, C), dpooled.device, want_dbias)
    call("pcnn_bias_relu_pool2_train_bwd", _ptr(dpooled), _ptr(sel), _ptr(dact), _ptr(act), B, H, W, C, _ptr(dy), _ptr(dbias),
         _ptr(ws), ws.numel() if ws is not None else 0, _stream(dpooled))
    return dy, dbias


class _BiasReluPool2TrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bias, relu, want_act):
        cf = _channels_first(y)
        act, pooled, sel = _bias_relu_pool2_train_raw(y.permute(0, 2, 3, 1) if cf else y, bias, relu, want_act)
        ctx.cf = cf
        ctx.set_materialize_grads(False)
        if cf:
            pooled = pooled.permute(0, 3, 1, 2)
        if not want_act:
            ctx.save_for_backward(sel)
            return pooled
        ctx.mark_dirty(y)
        ctx.save_for_backward(sel, y)
        return y, pooled

    @staticmethod
    def backward(ctx, *grads):
        sel = ctx.saved_tensors[0]
        dact, dpooled = grads if len(grads) == 2 else (None, grads[0])
        nhwc = (lambda t: t.permute(0, 2, 3, 1)) if ctx.cf else (lambda t: t)
        act = nhwc(ctx.saved_tensors[1]) if dact is not None else None
        dpooled = nhwc(dpooled) if dpooled is not None else torch.zeros(sel.shape, dtype=torch.float32, device=sel.device)
        dy, dbias = bias_relu_pool2_train_grad(dpooled, sel, nhwc(dact) if dact is not None else None, act,
                                               want_dbias=ctx.needs_input_grad[1])
        return (dy.permute(0, 3, 1, 2) if ctx.cf else dy), dbias, None, None


def bias_relu_pool2_train(y, bias, relu=True, want_act=False):
    """The conv -> pool pairs of the trunk under autograd: pooled = max_pool_2x2([ReLU](y + bias)) from the raw convolution
    output y [B,H,W,C] (H, W even), one kernel each way. What the backward keeps is one byte per pooled element (which
    of the window's four values it was, or that the ReLU closed the window): neither the activated full-resolution tensor nor
    an index tensor exists. With `want_act` (conv4_3, whose un-pooled output other layers read) returns (act, pooled), act
    being y overwritten in place and kept for the backward; only the ReLU form has that backward. `y` is NHWC-contiguous, or
    the channels_last [B,C,H,W] result of a framework convolution (the outputs then come in the same form).
    Differentiable w.r.t. y and bias."""
    if want_act and not relu:
        raise ValueError("bias_relu_pool2_train(want_act=True) is the ReLU layer's form: its backward gates on act > 0")
    if isinstance(y, torch.Tensor) and (want_act or _channels_first(y)):
        y = _dev_dense(y, "y")
    else:
        y = _dev(y, "y", torch.float32)
    bias = _dev(bias, "bias", torch.float32)
    if y.dim() != 4:
        raise ValueError("y must be [B,H,W,C] (got %s)" % (tuple(y.shape),))
    C = y.shape[1] if _channels_first(y) else y.shape[-1]
    if bias.dim() != 1 or bias.numel() != C:
        raise ValueError("bias must have one entry per channel (%d, got %s)" % (C, tuple(bias.shape)))
    return _BiasReluPool2TrainFn.apply(y, bias, bool(relu), bool(want_act))


# ------------------------------------------------------------------------------------------------
class _AverageDistanceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction, target, weight, point, symmetry, margin, num_rows=None):
        R, CH = prediction.shape
        C, P = point.shape[0], point.shape[1]
        dev = prediction.device
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        bottom_diff = torch.empty((R, CH), dtype=torch.float32, device=dev)
        ws, _ = _workspace(dev, "adl", "pcnn_average_distance_workspace_bytes", R, C, P)
        call("pcnn_average_distance_fwd", _ptr(prediction), _ptr(target), _ptr(weight), _ptr(point), _ptr(symmetry), R, C, P,
             float(margin), _ptr(num_rows), _ptr(loss), _ptr(bottom_diff), _ptr(ws), ws.numel(), _stream(prediction))
        ctx.save_for_backward(bottom_diff)
        ctx.mark_non_differentiable(bottom_diff)
        return loss, bottom_diff

    @staticmethod
    def backward(ctx, grad_loss, _grad_diff):
        (bottom_diff,) = ctx.saved_tensors
        R, CH = bottom_diff.shape
        grad_loss = grad_loss.contiguous()
        out = torch.empty_like(bottom_diff)
        if R > 0:
            call("pcnn_average_distance_bwd", _ptr(grad_loss), _ptr(bottom_diff), R, CH, _ptr(out), _stream(bottom_diff))
        return out, None, None, None, None, None, None


def average_distance_loss(poses_pred, poses_target, poses_weight, points, symmetry, margin, name=None, num_rows=None):
    """Drop-in for `Network.average_distance_loss` (network.py:236-238).
    Returns (loss[1], bottom_diff[R,4C]). `num_rows` (device int32[1]): the op's true row count when
    the inputs are capacity-sized buffers of the sync-free Hough op (normalisation by that count)."""
    poses_pred = _dev(poses_pred, "prediction", torch.float32)
    poses_target = _dev(poses_target, "target", torch.float32)
    poses_weight = _dev(poses_weight, "weight", torch.float32)
    points = _dev(points, "point", torch.float32)
    symmetry = _dev(symmetry, "symmetry", torch.float32)
    for t, n in ((poses_pred, "prediction"), (poses_target, "target"), (poses_weight, "weight")):
        if t.dim() != 2:
            raise ValueError("%s must be 2-dimensional" % n)  # average_distance_loss_op.cc:278-285
    if points.dim() != 3:
        raise ValueError("point must be 3-dimensional")
    if symmetry.dim() != 1:
        raise ValueError("symmetry must be 1-dimensional")
    if poses_pred.shape[1] != POSE_CHANNELS * points.shape[0]:
        raise ValueError("prediction must be [R, 4*num_classes]")
    if num_rows is not None:
        num_rows = _dev(num_rows, "num_rows", torch.int32)
    return _AverageDistanceFn.apply(poses_pred, poses_target, poses_weight, points, symmetry, margin, num_rows)


# ------------------------------------------------------------------------------------------------
class _BackprojectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, label, depth, meta_data, label_3d, grid_size, kernel_size, threshold):
        B, H, W, Cd = data.shape
        Cl = label.shape[3]
        num_meta = meta_data.shape[-1]
        G = int(grid_size)
        dev = data.device
        top_data = torch.empty((B, G, G, G, Cd), dtype=torch.float32, device=dev)
        top_flag = torch.empty((B, G, G, G, Cd), dtype=torch.float32, device=dev)
        top_label = torch.empty((B, G, G, G, Cl), dtype=torch.float32, device=dev)
        # caller-owned scratch for the window-range table that lets 85 % of the voxels skip their depth scan
        ws, need = _workspace(dev, "backproject", "pcnn_backproject_workspace_bytes", B, H, W, int(kernel_size), at_least=0)
        call("pcnn_backproject_ws_fwd", _ptr(data), _ptr(label), _ptr(depth), _ptr(meta_data), _ptr(label_3d), B, H, W, Cd, Cl,
             num_meta, G, int(kernel_size), float(threshold), _ptr(top_data), _ptr(top_label), _ptr(top_flag), _ptr(ws), need,
             _stream(data))
        ctx.save_for_backward(depth, meta_data)
        ctx.cfg = (B, H, W, Cd, num_meta, G)
        ctx.mark_non_differentiable(top_label, top_flag)
        return top_data, top_label, top_flag

    @staticmethod
    def backward(ctx, grad_data, _gl, _gf):
        depth, meta_data = ctx.saved_tensors
        B, H, W, Cd, num_meta, G = ctx.cfg
        grad_data = grad_data.contiguous()
        bottom = torch.empty((B, H, W, Cd), dtype=torch.float32, device=grad_data.device)
        call("pcnn_backproject_bwd", _ptr(grad_data), _ptr(depth), _ptr(meta_data), B, H, W, Cd, num_meta, G, _ptr(bottom),
             _stream(grad_data))
        return bottom, None, None, None, None, None, None, None


def backproject(data, label, depth, meta_data, label_3d, grid_size, kernel_size, threshold, name=None):
    """Drop-in for `Network.backproject` (network.py:224-226).
    Returns (top_data[B,G,G,G,Cd], top_label[B,G,G,G,Cl], top_flag[B,G,G,G,Cd])."""
    data = _dev(data, "data", torch.float32)
    label = _dev(label, "label", torch.float32)
    depth = _dev(depth, "depth", torch.float32)
    meta_data = _dev(meta_data, "meta_data", torch.float32)
    label_3d = _dev(label_3d, "label_3d", torch.float32)
    if data.dim() != 4:
        raise ValueError("data must be 4-dimensional")       # backprojecting_op.cc:332-333
    if label.dim() != 4:
        raise ValueError("label must be 4-dimensional")      # :335-336
    if depth.dim() != 4:
        raise ValueError("depth must be 4-dimensional")      # :338-339
    if meta_data.dim() != 4:
        raise ValueError("meta data must be 4-dimensional")  # :341-342
    if label_3d.dim() != 5:
        raise ValueError("label 3D must be 5-dimensional")   # :344-345
    return _BackprojectFn.apply(data, label, depth, meta_data, label_3d, grid_size, kernel_size, threshold)


# ------------------------------------------------------------------------------------------------
# input front end (include/posecnn_hip_frontend.h): the network input of cfg.INPUT = 'NORMAL'
_bilateral_cache = {}


def bilateral_tables(d, sigma_color, sigma_space, device=None):
    """The two weight tables of the 8-bit 3-channel bilateral filter as OpenCV's scalar code builds them, with numpy on
    the host: color_weight f32 [768], entry i = float32(exp(i i (-0.5 / sigma_color^2))); space_weight f32 [K] and
    offsets int32 [K,2], one row (i, j) per tap of [-r, r]^2 (r = d // 2, i outer, j inner) with
    rho = sqrt(float64(i i + j j)) <= r, entry = float32(exp(rho rho (-0.5 / sigma_space^2))); a sigma <= 0 counts as 1.
    Returns (color_weight, space_weight, offsets): numpy arrays, or with `device` the two tables as tensors there
    (cached per device and parameter triple) and the offsets as numpy."""
    d = int(d)
    if d < 3 or d > 15 or d % 2 == 0:
        raise ValueError("d must be odd, 3 <= d <= 15 (got %d)" % d)
    if device is not None:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:   # 'cuda' and 'cuda:0' are one cache entry
            device = torch.device("cuda", torch.cuda.current_device())
    key = (None if device is None else str(device), d, float(sigma_color), float(sigma_space))
    if key not in _bilateral_cache:
        host = _bilateral_cache.get((None,) + key[1:])
        if host is None:
            sc = float(sigma_color) if sigma_color > 0 else 1.0
            ss = float(sigma_space) if sigma_space > 0 else 1.0
            r = d // 2
            i = np.arange(768, dtype=np.float64)
            color = np.exp(i * i * (-0.5 / (sc * sc))).astype(np.float32)
            offsets = np.array([(a, b) for a in range(-r, r + 1) for b in range(-r, r + 1)
                                if np.sqrt(np.float64(a * a + b * b)) <= r], dtype=np.int32)
            rho = np.sqrt((offsets.astype(np.float64) ** 2).sum(axis=1))
            space = np.exp(rho * rho * (-0.5 / (ss * ss))).astype(np.float32)
            host = _bilateral_cache[(None,) + key[1:]] = (color, space, offsets)
        if device is not None:
            _bilateral_cache[key] = (torch.from_numpy(host[0]).to(device), torch.from_numpy(host[1]).to(device), host[2])
    return _bilateral_cache[key]


def _depth_args(depth, intrinsics, factor_depth):
    """The checked depth inputs of include/posecnn_hip_frontend.h: depth f32 [B,H,W] in metres (factor_depth None) or
    uint16 [B,H,W] with its factor_depth; intrinsics f32 [B,4] rows (fx, fy, cx, cy).
    Returns (depth_f32 | None, depth_u16 | None, factor, intrinsics, B, H, W)."""
    if not isinstance(depth, torch.Tensor):
        raise TypeError("depth must be a torch.Tensor")
    raw = depth.dtype == torch.uint16
    depth = _dev(depth, "depth", torch.uint16 if raw else torch.float32)
    intrinsics = _dev(intrinsics, "intrinsics", torch.float32)
    if depth.dim() == 4 and depth.shape[3] == 1:
        depth = depth.reshape(depth.shape[:3])
    if depth.dim() != 3:
        raise ValueError("depth must be [B,H,W] (got %s)" % (tuple(depth.shape),))
    if raw and factor_depth is None:
        raise ValueError("a uint16 depth frame needs its factor_depth")
    if not raw and factor_depth is not None:
        raise ValueError("factor_depth goes with a uint16 depth frame; a float32 frame is in metres")
    B, H, W = depth.shape
    if tuple(intrinsics.shape) != (B, 4):
        raise ValueError("intrinsics must be [B,4] rows (fx, fy, cx, cy) with B = %d (got %s)" % (B, tuple(intrinsics.shape)))
    return (None if raw else depth), (depth if raw else None), (float(factor_depth) if raw else 0.0), intrinsics, B, H, W


def depth_normals(depth, intrinsics, depth_cutoff=20.0, factor_depth=None):
    """gpu_normals (lib/normals/compute_normals.cu:30-101) of B depth frames, one IEEE rounding per operation:
    depth f32 [B,H,W] in metres, or uint16 [B,H,W] with `factor_depth` (z = float32(d) / factor_depth);
    intrinsics f32 [B,4] rows (fx, fy, cx, cy). Returns nmap f32 [B,H,W,3]; NaN (0x7fffffff) where the reference's is."""
    f32, u16, factor, intr, B, H, W = _depth_args(depth, intrinsics, factor_depth)
    nmap = torch.empty((B, H, W, 3), dtype=torch.float32, device=intr.device)
    call("pcnn_depth_normals_fwd", _ptr(f32), _ptr(u16), factor, _ptr(intr), B, H, W, float(depth_cutoff), _ptr(nmap),
         _stream(nmap))
    return nmap


def bilateral_filter_u8(image, d=9, sigma_color=75.0, sigma_space=75.0):
    """cv2.bilateralFilter(image, d, sigma_color, sigma_space) of uint8 [B,H,W,3] frames (border reflect-101) with the
    arithmetic of OpenCV's scalar code (include/posecnn_hip_frontend.h). Returns uint8 [B,H,W,3]."""
    image = _dev(image, "image", torch.uint8)
    if image.dim() != 4 or image.shape[3] != 3:
        raise ValueError("image must be uint8 [B,H,W,3] (got %s)" % (tuple(image.shape),))
    color, space, _ = bilateral_tables(d, sigma_color, sigma_space, image.device)
    B, H, W, _ = image.shape
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=image.device)
    call("pcnn_bilateral_u8c3_fwd", _ptr(image), B, H, W, int(d), _ptr(color), _ptr(space), space.numel(), _ptr(out), _stream(out))
    return out


def normal_image(depth, intrinsics, factor_depth=None, depth_cutoff=20.0, d=9, sigma_color=75.0, sigma_space=75.0):
    """The uint8 image lib/fcn/test.py:89-94 forms under cfg.INPUT = 'NORMAL', in one kernel:
    bilateral_filter_u8(uint8(127.5 depth_normals(depth) + 127.5)[..., (2, 1, 0)], d, sigma_color, sigma_space); d = 0
    leaves the filter out. Arguments as `depth_normals`. Returns uint8 [B,H,W,3], which the network takes as `data`
    (the first kernel subtracts PIXEL_MEANS: ops.conv1_1_conv1_2_fused_raw)."""
    f32, u16, factor, intr, B, H, W = _depth_args(depth, intrinsics, factor_depth)
    color, space, taps = None, None, 0
    if int(d) != 0:
        color, space, _ = bilateral_tables(d, sigma_color, sigma_space, intr.device)
        taps = space.numel()
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=intr.device)
    call("pcnn_normal_image_fwd", _ptr(f32), _ptr(u16), factor, _ptr(intr), B, H, W, float(depth_cutoff), int(d), _ptr(color),
         _ptr(space), taps, _ptr(out), _stream(out))
    return out


# ------------------------------------------------------------------------------------------------
# training augmentation (include/posecnn_hip_augment.h): chromatic_transform + add_noise + the blob, one kernel
AUGMENT_ROW = 10
DEPTH_NORMS = {"frame_max": 0, "fixed_2000": 1}


def augment_frames(color, depth=None, params=None, seed=0, pixel_means=None, depth_norm="frame_max"):
    """`chromatic_transform` and `add_noise` (lib/utils/blob.py:74-129) in the order of
    lib/gt_synthesize_layer/minibatch.py:170-201, fused with the blob formation: color uint8 [B,H,W,3] BGR or [B,H,W,4]
    BGRA (the fourth byte is ignored: `SceneBatch.color` goes in as it is), depth uint16 [B,H,W] or None.
    params: host float64 [B,10], one row per frame (`augment.AugmentSampler.sample`; columns and arithmetic:
    include/posecnn_hip_augment.h). seed: an integer below 2^128, the Philox key. depth_norm: "frame_max" (the frame's own
    maximum, minibatch.py:189) or "fixed_2000" (clip(d / 2000, 0, 1) 255, what `networks.raw_frame_blob` forms).
    Returns (data, data_p): f32 [B,H,W,3] blobs with PIXEL_MEANS subtracted; data_p is None without depth."""
    from .config import PIXEL_MEANS
    color = _dev(color, "color", torch.uint8)
    if color.dim() != 4 or color.shape[3] not in (3, 4):
        raise ValueError("color must be uint8 [B,H,W,3] or [B,H,W,4] (got %s)" % (tuple(color.shape),))
    B, H, W, C = color.shape
    if depth is not None:
        depth = _dev(depth, "depth", torch.uint16)
        if depth.dim() == 4 and depth.shape[3] == 1:
            depth = depth.reshape(depth.shape[:3])
        if tuple(depth.shape) != (B, H, W):
            raise ValueError("depth must be uint16 [%d,%d,%d] (got %s)" % (B, H, W, tuple(depth.shape)))
    if depth_norm not in DEPTH_NORMS:
        raise ValueError("depth_norm must be one of %s (got %r)" % (sorted(DEPTH_NORMS), depth_norm))
    if params is None:
        raise ValueError("augment_frames needs params: one row of %d doubles per frame" % AUGMENT_ROW)
    rows = np.ascontiguousarray(params, dtype=np.float64)
    if rows.shape != (B, AUGMENT_ROW):
        raise ValueError("params must be [%d,%d] (got %s)" % (B, AUGMENT_ROW, rows.shape))
    seed = int(seed)
    if not 0 <= seed < 1 << 128:
        raise ValueError("seed must be in [0, 2^128)")
    means = (ctypes.c_double * 3)(*[float(m) for m in np.asarray(PIXEL_MEANS if pixel_means is None else pixel_means, dtype=np.float64).reshape(-1)[:3]])
    color, depth = _aligned16(color), (_aligned16(depth) if depth is not None else None)
    dev = color.device
    data = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    data_p = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev) if depth is not None else None
    norm = DEPTH_NORMS[depth_norm]
    ws, nbytes = _workspace(dev, "augment_frames", "pcnn_augment_frames_workspace_bytes", B, 1 if depth is not None else 0, norm,
                            at_least=0)
    call("pcnn_augment_frames_fwd", _ptr(color), C, _ptr(depth), ctypes.c_void_p(rows.ctypes.data), means, seed & (1 << 64) - 1,
         seed >> 64, norm, B, H, W, _ptr(data), _ptr(data_p), _ptr(ws), nbytes, _stream(data))
    return data, data_p


# ------------------------------------------------------------------------------------------------
# 3-D vertex route: preemptive RANSAC + Kabsch poses from object coordinates (include/posecnn_hip_pose3d.h)
POSE3D_DEFAULTS = dict(hypotheses=256, pixel_batch=1000, max_pixels=1000, ref_it=8, min_area=400, inlier_threshold=0.01,
                       min_dist=0.01, min_pixels=10, max_attempts=1024)   # synthesize.cpp:1783-1799; max_attempts is ours


POSE2D_DEFAULTS = dict(hypotheses=256, pixel_batch=1000, max_pixels=1000, ref_it=8, min_area=400, inlier_threshold=10.0,
                       min_dist2d=10.0, min_dist3d=0.01, min_pixels=10, max_attempts=1024)   # synthesize.cpp:1590-1599; max_attempts is ours


# ---- what the two routes' wrappers check and allocate alike
def _pose_frames(label_2d, vertex_pred, extents, intrinsics=None, depth=None):
    """The checked frames of both routes; `depth` (uint16 [B,H,W] or [B,H,W,1]) only on the route that has one, `intrinsics`
    wherever the entry takes them. -> (label_2d, depth, vertex_pred, extents, intrinsics, B, H, W, C)."""
    label_2d = _dev(label_2d, "label_2d", torch.int32)
    if depth is not None:
        depth = _dev(depth, "depth", torch.uint16)
        if depth.dim() == 4 and depth.shape[3] == 1:
            depth = depth.reshape(depth.shape[:3])
    vertex_pred = _dev(vertex_pred, "vertex_pred", torch.float32)
    extents = _dev(extents, "extents", torch.float32)
    if intrinsics is not None:
        intrinsics = _dev(intrinsics, "intrinsics", torch.float32)
    if label_2d.dim() != 3:
        raise ValueError("label_2d must be [B,H,W] (got %s)" % (tuple(label_2d.shape),))
    B, H, W = label_2d.shape
    if depth is not None and tuple(depth.shape) != (B, H, W):
        raise ValueError("depth must be uint16 [%d,%d,%d] (got %s)" % (B, H, W, tuple(depth.shape)))
    if extents.dim() != 2 or extents.shape[1] != 3:
        raise ValueError("extents must be [C,3] (got %s)" % (tuple(extents.shape),))
    C = extents.shape[0]
    if tuple(vertex_pred.shape) != (B, H, W, 3 * C):
        raise ValueError("vertex_pred must be [%d,%d,%d,%d] (got %s)" % (B, H, W, 3 * C, tuple(vertex_pred.shape)))
    if intrinsics is not None and tuple(intrinsics.shape) != (B, 4):
        raise ValueError("intrinsics must be [B,4] rows (fx, fy, px, py) with B = %d (got %s)" % (B, tuple(intrinsics.shape)))
    return label_2d, depth, vertex_pred, extents, intrinsics, B, H, W, C


def _pose3d_streams(streams, B, device):
    if streams is None:
        return torch.zeros((B,), dtype=torch.int64, device=device)
    if not isinstance(streams, torch.Tensor):
        ids = [int(v) for v in streams]
        if any(not 0 <= v < 1 << 64 for v in ids):
            raise ValueError("streams must be in [0, 2^64)")
        streams = torch.from_numpy(np.array(ids, dtype=np.uint64).view(np.int64)).to(device)
    streams = _dev(streams, "streams", torch.int64)
    if tuple(streams.shape) != (B,):
        raise ValueError("streams must be one id per frame, [%d] (got %s)" % (B, tuple(streams.shape)))
    return streams


def _pose3d_seed(seed):
    seed = int(seed)
    if not 0 <= seed < 1 << 128:
        raise ValueError("seed must be in [0, 2^128)")
    return seed & (1 << 64) - 1, seed >> 64


def _pose_record_outputs(B, H, W, C, dev):
    """(records f32 [B,H*W,6], counts int32 [B,C], offsets int32 [B,C]) for a prepare entry to fill."""
    return (torch.empty((B, H * W, 6), dtype=torch.float32, device=dev), torch.empty((B, C), dtype=torch.int32, device=dev),
            torch.empty((B, C), dtype=torch.int32, device=dev))


def _pose3d_records(records, counts, offsets, H, W):
    records = _dev(records, "records", torch.float32)
    counts = _dev(counts, "counts", torch.int32)
    offsets = _dev(offsets, "offsets", torch.int32)
    if records.dim() != 3 or records.shape[1] != H * W or records.shape[2] != 6:
        raise ValueError("records must be [B,%d,6] (got %s)" % (H * W, tuple(records.shape)))
    B = records.shape[0]
    if counts.dim() != 2 or counts.shape[0] != B or counts.shape != offsets.shape:
        raise ValueError("counts and offsets must be [B,C] (got %s, %s)" % (tuple(counts.shape), tuple(offsets.shape)))
    return records, counts, offsets, B, counts.shape[1]


def _pose_sample_args(records, counts, offsets, extents, intrinsics, height, width, seed, streams, hypotheses, points):
    """Everything a sample entry takes in front of its thresholds, checked, and its four outputs, hyp_rec [B,n,points]:
    -> (the nine pointer / key arguments in the entry's order, (B, H, W, C, n), outputs)."""
    H, W = int(height), int(width)
    records, counts, offsets, B, C = _pose3d_records(records, counts, offsets, H, W)
    extents = _dev(extents, "extents", torch.float32)
    intrinsics = _dev(intrinsics, "intrinsics", torch.float32)
    if tuple(extents.shape) != (C, 3) or tuple(intrinsics.shape) != (B, 4):
        raise ValueError("extents must be [%d,3] and intrinsics [%d,4]" % (C, B))
    dev = records.device
    streams = _pose3d_streams(streams, B, dev)
    s0, s1 = _pose3d_seed(seed)
    n = int(hypotheses)
    outs = (torch.empty((B, max(n, 0), 3, 4), dtype=torch.float64, device=dev),
            torch.empty((B, max(n, 0)), dtype=torch.int32, device=dev),
            torch.empty((B, max(n, 0)), dtype=torch.int32, device=dev),
            torch.empty((B, max(n, 0), points), dtype=torch.int32, device=dev))
    return (_ptr(records), _ptr(counts), _ptr(offsets), _ptr(extents), _ptr(intrinsics), _ptr(streams), s0, s1), (B, H, W, C, n), outs


def _pose_round_outputs(hyp_pose, hyp_class, B):
    """The hypothesis-shape check of a round entry and its outputs: -> (n, (pose_out, class_out, inliers_out))."""
    if hyp_class.dim() != 2 or hyp_class.shape[0] != B or tuple(hyp_pose.shape) != tuple(hyp_class.shape) + (3, 4):
        raise ValueError("hyp_class must be [B,n] and hyp_pose [B,n,3,4] (got %s, %s)" % (tuple(hyp_class.shape), tuple(hyp_pose.shape)))
    n, dev = hyp_class.shape[1], hyp_pose.device
    return n, (torch.empty((B, n, 3, 4), dtype=torch.float64, device=dev), torch.empty((B, n), dtype=torch.int32, device=dev),
               torch.empty((B, n), dtype=torch.int32, device=dev))


def _pose_estimate_args(route, dims, dev, seed, streams, hypotheses, min_pixels, workspace, polished_max_pixels=None):
    """What an estimate entry takes besides its frames and thresholds, `route` "pose3d" | "pose2d", dims = (B, H, W, C):
    -> (streams, s0, s1, workspace buffer, its bytes, (poses64, poses, inliers, ref_steps, num_hyps)).
    polished_max_pixels (an int): the workspace of the route's polished driver instead, and the three polish outputs
    (energy f64 [B,C,2], evals, listed int32 [B,C]) behind the five."""
    B, H, W, C = dims
    streams = _pose3d_streams(streams, B, dev)
    s0, s1 = _pose3d_seed(seed)
    int(min_pixels)
    if polished_max_pixels is None:
        ws, nbytes = _workspace(dev, route, "pcnn_%s_workspace_bytes" % route, B, H, W, C, int(hypotheses), workspace=workspace)
    else:
        ws, nbytes = _workspace(dev, route + "_polished", "pcnn_%s_estimate_polished_workspace_bytes" % route, B, H, W, C,
                                int(hypotheses), int(polished_max_pixels), workspace=workspace)
    outs = (torch.empty((B, C, 3, 4), dtype=torch.float64, device=dev), torch.empty((B, C, 3, 4), dtype=torch.float32, device=dev),
            torch.empty((B, C), dtype=torch.int32, device=dev), torch.empty((B, C), dtype=torch.int32, device=dev),
            torch.empty((B, C), dtype=torch.int32, device=dev))
    if polished_max_pixels is not None:
        outs += _pose_polish_outputs(B, C, dev)
    return streams, s0, s1, ws, nbytes, outs


def _pose_polish_outputs(B, C, dev):
    """(energy f64 [B,C,2], evals int32 [B,C], listed int32 [B,C]) for a polish launch to fill."""
    return (torch.empty((B, C, 2), dtype=torch.float64, device=dev), torch.empty((B, C), dtype=torch.int32, device=dev),
            torch.empty((B, C), dtype=torch.int32, device=dev))


def _polish_evaluations(polish_evaluations):
    n = int(polish_evaluations)
    if n < 0:
        raise ValueError("polish_evaluations must not be negative (got %d)" % n)
    return n


# ---- the route with a depth frame
def pose3d_prepare(label_2d, depth, vertex_pred, extents, intrinsics, factor_depth):
    """The correspondence records of `estimate_poses_3d` (getEye, getLabels, getMode3D): -> (records f32 [B,H*W,6] rows
    (eye xyz, obj xyz), compacted per (frame, class) in raster order, counts int32 [B,C], offsets int32 [B,C]). Rows past a
    frame's total are not written."""
    label_2d, depth, vertex_pred, extents, intrinsics, B, H, W, C = _pose_frames(label_2d, vertex_pred, extents, intrinsics, depth)
    records, counts, offsets = _pose_record_outputs(B, H, W, C, label_2d.device)
    call("pcnn_pose3d_prepare_fwd", _ptr(label_2d), _ptr(depth), _ptr(vertex_pred), _ptr(extents), _ptr(intrinsics),
         float(factor_depth), B, H, W, C, _ptr(records), _ptr(counts), _ptr(offsets), _stream(records))
    return records, counts, offsets


def pose3d_sample(records, counts, offsets, extents, intrinsics, height, width, seed=0, streams=None, hypotheses=256,
                  max_attempts=1024, min_area=400, inlier_threshold=0.01, min_dist=0.01):
    """One 3-point hypothesis per (frame, h) from `pose3d_prepare`'s records: -> (hyp_pose f64 [B,hypotheses,3,4],
    hyp_class int32 [B,hypotheses] (0: none found), hyp_attempt int32 (the accepted attempt, -1), hyp_rec int32 [..,3]
    (the three records, indices inside their class))."""
    args, dims, outs = _pose_sample_args(records, counts, offsets, extents, intrinsics, height, width, seed, streams, hypotheses, 3)
    call("pcnn_pose3d_sample_fwd", *args, *dims, int(max_attempts), int(min_area), float(inlier_threshold), float(min_dist),
         *map(_ptr, outs), _stream(outs[0]))
    return outs


def pose3d_round(records, counts, offsets, hyp_pose, hyp_class, height, width, round, pixel_batch=1000, max_pixels=1000,
                 inlier_threshold=0.01):
    """ONE count -> rank -> halve -> refit round of the preemptive loop on the given hypotheses (hyp_class 0: empty slot):
    -> (pose_out f64 [B,n,3,4], class_out int32 [B,n] (0 where the slot was dropped), inliers_out int32 [B,n])."""
    H, W = int(height), int(width)
    records, counts, offsets, B, C = _pose3d_records(records, counts, offsets, H, W)
    hyp_pose = _dev(hyp_pose, "hyp_pose", torch.float64)
    hyp_class = _dev(hyp_class, "hyp_class", torch.int32)
    n, outs = _pose_round_outputs(hyp_pose, hyp_class, B)
    call("pcnn_pose3d_round_fwd", _ptr(records), _ptr(counts), _ptr(offsets), _ptr(hyp_pose), _ptr(hyp_class), B, H, W, C, n,
         int(round), int(pixel_batch), int(max_pixels), float(inlier_threshold), *map(_ptr, outs), _stream(records))
    return outs


def estimate_poses_3d(label_2d, depth, vertex_pred, extents, intrinsics, factor_depth, seed=0, streams=None, hypotheses=256,
                      pixel_batch=1000, max_pixels=1000, ref_it=8, min_area=400, inlier_threshold=0.01, min_dist=0.01,
                      min_pixels=10, max_attempts=1024, workspace=None, polish_evaluations=0):
    """`Synthesizer::estimatePose3D` (lib/synthesize/synthesize.cpp:1769-1966) for a batch, three launches and no
    synchronisation: label_2d int32 [B,H,W], depth uint16 [B,H,W], vertex_pred f32 [B,H,W,3C] (the `vertex_reg_3d` network's
    object coordinates, scaled into [0, 1] per extent), extents f32 [C,3], intrinsics f32 [B,4] rows (fx, fy, px, py).
    seed: the Philox key (< 2^128); streams: one uint64 id per frame (default 0), so that a frame's poses do not depend on
    its batch slot.
    Returns device tensors (poses f32 [B,C,3,4], poses64 f64 [B,C,3,4], inliers, ref_steps, num_hyps int32 [B,C]); a class
    without hypothesis is all zero (the reference's caller reads t_z > 0 as found).
    polish_evaluations > 0 (the reference's refinementIterations is 100; 7 at least): a fourth launch, the Nelder-Mead polish
    of `pose_polish` on every class with inliers > min_pixels (refineWithOpt, :1936-1944) — poses and poses64 are the
    polished ones and (energy f64 [B,C,2], evals, listed int32 [B,C]) follow num_hyps. At 0, the default, there is no
    polish and min_pixels is unused. Deviations from the reference: DESIGN.md 3.7b."""
    label_2d, depth, vertex_pred, extents, intrinsics, B, H, W, C = _pose_frames(label_2d, vertex_pred, extents, intrinsics, depth)
    if _polish_evaluations(polish_evaluations):
        streams, s0, s1, ws, nbytes, outs = _pose_estimate_args("pose3d", (B, H, W, C), label_2d.device, seed, streams, hypotheses,
                                                                min_pixels, workspace, polished_max_pixels=max_pixels)
        call("pcnn_pose3d_estimate_polished_fwd", _ptr(label_2d), _ptr(depth), _ptr(vertex_pred), _ptr(extents), _ptr(intrinsics),
             _ptr(streams), float(factor_depth), s0, s1, B, H, W, C, int(hypotheses), int(pixel_batch), int(max_pixels), int(ref_it),
             int(min_area), float(inlier_threshold), float(min_dist), int(max_attempts), int(min_pixels), int(polish_evaluations),
             *map(_ptr, outs), _ptr(ws), nbytes, _stream(outs[1]))
        poses64, poses, inliers, ref_steps, num_hyps, energy, evals, listed = outs
        return poses, poses64, inliers, ref_steps, num_hyps, energy, evals, listed
    streams, s0, s1, ws, nbytes, outs = _pose_estimate_args("pose3d", (B, H, W, C), label_2d.device, seed, streams, hypotheses,
                                                            min_pixels, workspace)
    call("pcnn_pose3d_estimate_fwd", _ptr(label_2d), _ptr(depth), _ptr(vertex_pred), _ptr(extents), _ptr(intrinsics), _ptr(streams),
         float(factor_depth), s0, s1, B, H, W, C, int(hypotheses), int(pixel_batch), int(max_pixels), int(ref_it), int(min_area),
         float(inlier_threshold), float(min_dist), int(max_attempts), *map(_ptr, outs), _ptr(ws), nbytes, _stream(outs[1]))
    poses64, poses, inliers, ref_steps, num_hyps = outs
    return poses, poses64, inliers, ref_steps, num_hyps


# ---- the route without depth: P3P hypotheses and a Gauss-Newton refit (include/posecnn_hip_pose2d.h)
def pose2d_prepare(label_2d, vertex_pred, extents):
    """The correspondence records of `estimate_poses_2d`: -> (records f32 [B,H*W,6] rows (pixel x, pixel y, 0, obj xyz),
    compacted per (frame, class) in raster order, counts int32 [B,C], offsets int32 [B,C]). Rows past a frame's total are
    not written."""
    label_2d, _, vertex_pred, extents, _, B, H, W, C = _pose_frames(label_2d, vertex_pred, extents)
    records, counts, offsets = _pose_record_outputs(B, H, W, C, label_2d.device)
    call("pcnn_pose2d_prepare_fwd", _ptr(label_2d), _ptr(vertex_pred), _ptr(extents), B, H, W, C, _ptr(records), _ptr(counts),
         _ptr(offsets), _stream(records))
    return records, counts, offsets


def pose2d_sample(records, counts, offsets, extents, intrinsics, height, width, seed=0, streams=None, hypotheses=256,
                  max_attempts=1024, min_area=400, inlier_threshold=10.0, min_dist2d=10.0, min_dist3d=0.01):
    """One 4-point hypothesis per (frame, h) from `pose2d_prepare`'s records — P3P on three pairs, the fourth chooses the
    root: -> (hyp_pose f64 [B,hypotheses,3,4], hyp_class int32 [B,hypotheses] (0: none found), hyp_attempt int32 (the
    accepted attempt, -1), hyp_rec int32 [..,4] (the four records, indices inside their class))."""
    args, dims, outs = _pose_sample_args(records, counts, offsets, extents, intrinsics, height, width, seed, streams, hypotheses, 4)
    call("pcnn_pose2d_sample_fwd", *args, *dims, int(max_attempts), int(min_area), float(inlier_threshold), float(min_dist2d),
         float(min_dist3d), *map(_ptr, outs), _stream(outs[0]))
    return outs


def pose2d_round(records, counts, offsets, intrinsics, hyp_pose, hyp_class, height, width, round, pixel_batch=1000,
                 max_pixels=1000, inlier_threshold=10.0):
    """ONE count -> rank -> halve -> Gauss-Newton refit round of the preemptive loop on the given hypotheses (hyp_class 0:
    empty slot): -> (pose_out f64 [B,n,3,4], class_out int32 [B,n] (0 where the slot was dropped), inliers_out int32 [B,n])."""
    H, W = int(height), int(width)
    records, counts, offsets, B, C = _pose3d_records(records, counts, offsets, H, W)
    intrinsics = _dev(intrinsics, "intrinsics", torch.float32)
    hyp_pose = _dev(hyp_pose, "hyp_pose", torch.float64)
    hyp_class = _dev(hyp_class, "hyp_class", torch.int32)
    if tuple(intrinsics.shape) != (B, 4):
        raise ValueError("intrinsics must be [%d,4] (got %s)" % (B, tuple(intrinsics.shape)))
    n, outs = _pose_round_outputs(hyp_pose, hyp_class, B)
    call("pcnn_pose2d_round_fwd", _ptr(records), _ptr(counts), _ptr(offsets), _ptr(intrinsics), _ptr(hyp_pose), _ptr(hyp_class), B,
         H, W, C, n, int(round), int(pixel_batch), int(max_pixels), float(inlier_threshold), *map(_ptr, outs), _stream(records))
    return outs


def estimate_poses_2d(label_2d, vertex_pred, extents, intrinsics, seed=0, streams=None, hypotheses=256, pixel_batch=1000,
                      max_pixels=1000, ref_it=8, min_area=400, inlier_threshold=10.0, min_dist2d=10.0, min_dist3d=0.01,
                      min_pixels=10, max_attempts=1024, workspace=None, polish_evaluations=0):
    """`Synthesizer::estimatePose2D` (lib/synthesize/synthesize.cpp:1571-1767) for a batch, three launches and no
    synchronisation, no depth frame: label_2d int32 [B,H,W], vertex_pred f32 [B,H,W,3C] (the `vertex_reg_3d` network's
    object coordinates, scaled into [0, 1] per extent), extents f32 [C,3], intrinsics f32 [B,4] rows (fx, fy, px, py).
    seed, streams and the return value as in `estimate_poses_3d`: device tensors (poses f32 [B,C,3,4], poses64 f64
    [B,C,3,4], inliers, ref_steps, num_hyps int32 [B,C]); a class without hypothesis is all zero. inlier_threshold and
    min_dist2d are in pixels, min_dist3d in metres. polish_evaluations > 0: the fourth launch of `estimate_poses_3d` with
    the reprojection energy (refineWithOpt, :1737-1745), gated by min_pixels, and (energy, evals, listed) behind num_hyps;
    at 0, the default, no polish and min_pixels is unused. Deviations from the reference: DESIGN.md 3.7c."""
    label_2d, _, vertex_pred, extents, intrinsics, B, H, W, C = _pose_frames(label_2d, vertex_pred, extents, intrinsics)
    if _polish_evaluations(polish_evaluations):
        streams, s0, s1, ws, nbytes, outs = _pose_estimate_args("pose2d", (B, H, W, C), label_2d.device, seed, streams, hypotheses,
                                                                min_pixels, workspace, polished_max_pixels=max_pixels)
        call("pcnn_pose2d_estimate_polished_fwd", _ptr(label_2d), _ptr(vertex_pred), _ptr(extents), _ptr(intrinsics), _ptr(streams),
             s0, s1, B, H, W, C, int(hypotheses), int(pixel_batch), int(max_pixels), int(ref_it), int(min_area),
             float(inlier_threshold), float(min_dist2d), float(min_dist3d), int(max_attempts), int(min_pixels),
             int(polish_evaluations), *map(_ptr, outs), _ptr(ws), nbytes, _stream(outs[1]))
        poses64, poses, inliers, ref_steps, num_hyps, energy, evals, listed = outs
        return poses, poses64, inliers, ref_steps, num_hyps, energy, evals, listed
    streams, s0, s1, ws, nbytes, outs = _pose_estimate_args("pose2d", (B, H, W, C), label_2d.device, seed, streams, hypotheses,
                                                            min_pixels, workspace)
    call("pcnn_pose2d_estimate_fwd", _ptr(label_2d), _ptr(vertex_pred), _ptr(extents), _ptr(intrinsics), _ptr(streams), s0, s1, B,
         H, W, C, int(hypotheses), int(pixel_batch), int(max_pixels), int(ref_it), int(min_area), float(inlier_threshold),
         float(min_dist2d), float(min_dist3d), int(max_attempts), *map(_ptr, outs), _ptr(ws), nbytes, _stream(outs[1]))
    poses64, poses, inliers, ref_steps, num_hyps = outs
    return poses, poses64, inliers, ref_steps, num_hyps


# ---- the polish that ends both routes (include/posecnn_hip/pose_polish.h)
POSE_POLISH_ROUTES = {0: 0, 1: 1, "depth": 0, "colour": 1, "color": 1}


def pose_polish(records, counts, offsets, poses64, gate, route, intrinsics=None, *, height, width, max_pixels=1000, min_pixels=10,
                evaluations=100, inlier_threshold=None, workspace=None):
    """`refineWithOpt` (lib/synthesize/synthesize.cpp:1510-1567) for a batch, one launch: the Nelder-Mead polish of the
    poses `poses64` f64 [B,C,3,4] on the records of `pose3d_prepare` (route 0 or "depth": mean point distance) or
    `pose2d_prepare` (route 1 or "colour": mean reprojection distance, needs intrinsics f32 [B,4]). A class is polished
    when gate[b][c] > min_pixels (gate int32 [B,C]: the `inliers` of an estimate) and the pose has an inlier among the
    class's records under inlier_threshold (default: the route's, 0.01 m / 10 pixels); the inliers, thinned to max_pixels,
    are the points of the energy. evaluations: exactly that many energy evaluations (7 at least; 0: nothing is polished).
    Returns device tensors (poses f32 [B,C,3,4], poses64 f64 [B,C,3,4], energy f64 [B,C,2] (before, after), evals int32
    [B,C], listed int32 [B,C] (the points used)); an unpolished class keeps its pose with energy, evals, listed 0. The
    unknowns, the box and the optimiser's rules: the header; deviation from the reference: DESIGN.md 3.7b (l)."""
    if route not in POSE_POLISH_ROUTES:
        raise ValueError("route must be 0 / 'depth' or 1 / 'colour' (got %r)" % (route,))
    route = POSE_POLISH_ROUTES[route]
    H, W = int(height), int(width)
    records, counts, offsets, B, C = _pose3d_records(records, counts, offsets, H, W)
    poses64 = _dev(poses64, "poses64", torch.float64)
    gate = _dev(gate, "gate", torch.int32)
    if tuple(poses64.shape) != (B, C, 3, 4) or tuple(gate.shape) != (B, C):
        raise ValueError("poses64 must be [%d,%d,3,4] and gate [%d,%d] (got %s, %s)" % (B, C, B, C, tuple(poses64.shape), tuple(gate.shape)))
    if route == 1 and intrinsics is None:
        raise ValueError("the colour route needs intrinsics")
    if intrinsics is not None:
        intrinsics = _dev(intrinsics, "intrinsics", torch.float32)
        if tuple(intrinsics.shape) != (B, 4):
            raise ValueError("intrinsics must be [%d,4] (got %s)" % (B, tuple(intrinsics.shape)))
    thr = (POSE3D_DEFAULTS, POSE2D_DEFAULTS)[route]["inlier_threshold"] if inlier_threshold is None else inlier_threshold
    dev = records.device
    ws, nbytes = _workspace(dev, "pose_polish", "pcnn_pose_polish_workspace_bytes", B, C, int(max_pixels), workspace=workspace)
    out64 = torch.empty((B, C, 3, 4), dtype=torch.float64, device=dev)
    out32 = torch.empty((B, C, 3, 4), dtype=torch.float32, device=dev)
    energy, evals, listed = _pose_polish_outputs(B, C, dev)
    call("pcnn_pose_polish_fwd", route, _ptr(records), _ptr(counts), _ptr(offsets), _ptr(intrinsics), _ptr(poses64), _ptr(gate), B, H,
         W, C, int(max_pixels), int(min_pixels), int(evaluations), float(thr), _ptr(out64), _ptr(out32), _ptr(energy), _ptr(evals),
         _ptr(listed), _ptr(ws), nbytes, _stream(out64))
    return out32, out64, energy, evals, listed
