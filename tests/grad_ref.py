"""Plain float64 restatement of the training side, differentiated by torch.autograd. TEST INFRASTRUCTURE ONLY.

The forward of every op here is pinned elsewhere (bit for bit against the C oracle, the dense kernels against
float64). What this module adds is an independent statement of the DERIVATIVES: each function below is the forward
written with differentiable torch ops only — no HIP, no oracle, no hand-written backward — so `torch.autograd`
supplies a reference gradient that shares nothing with the reading of the reference's backward code that the
kernels and oracle/pcnn_oracle.c were both written from.

  deconv_bilinear64, smooth_l1_vertex64, roi_pool64, average_distance64    the four ops with hand-written backwards
  training_loss64                                                          the whole vgg16_convs(is_train=True) graph
  vars_from_net / grads_of / rel_err / bound / rejected                    the comparison of tests/test_gpu_gradients.py

Every function computes in the dtype of its floating inputs, so the same code run on float32 tensors measures the
float32 floor of the comparison (tests/test_grad_ref_cpu.py).

A new training kernel drops in like this: write its forward here with torch ops, gradcheck it in
tests/test_grad_ref_cpu.py, compare the kernel's backward with `torch.autograd.grad` of it in
tests/test_gpu_gradients.py on inputs away from its kinks.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import exact

MUTATIONS = ("vertex_w_doubled", "pose_w_zero", "vertex_conv4_detached", "roi_pool8_detached", "sl1_sigma2_once_less")


# ---- the four ops ---------------------------------------------------------------------------------------------------
def deconv_bilinear64(x, k, s, add1=None, add2=None, bias=None, relu=False):
    """The fixed bilinear `deconv` layer (lib/networks/network.py:141-157,207-222): x [B,H,W,C] -> [B,H s,W s,C], a
    per-channel conv_transpose2d with outer(f, f), f = exact.deconv_filter_1d(k), 'SAME' = padding (k - s) / 2; then the
    optional addends, per-channel bias and ReLU of ops.deconv_bilinear."""
    C = x.shape[-1]
    f = torch.tensor(exact.deconv_filter_1d(k), dtype=x.dtype, device=x.device)
    w = torch.outer(f, f).expand(C, 1, k, k)
    y = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, None, stride=s, padding=(k - s) // 2, groups=C).permute(0, 2, 3, 1)
    for t in (add1, add2, bias):
        if t is not None:
            y = y + t
    return torch.relu(y) if relu else y


def smooth_l1_vertex64(pred, target, weight, sigma=1.0, _drop_sigma2_in_grad=False):
    """lib/fcn/train.py:564-573, line by line. `_drop_sigma2_in_grad` is the mutation of the comparator self-test: the
    value is unchanged, the quadratic branch's gradient loses one factor sigma^2."""
    sigma_2 = sigma ** 2
    vertex_diff = pred - target
    diff = weight * vertex_diff
    abs_diff = diff.abs()
    with torch.no_grad():                                   # tf.stop_gradient(tf.to_float(tf.less(...)))
        sign = (abs_diff < 1. / sigma_2).to(pred.dtype)
    quad = diff ** 2 * (sigma_2 / 2.)
    if _drop_sigma2_in_grad:
        g = diff ** 2 * 0.5
        quad = quad.detach() + (g - g.detach())
    in_loss = quad * sign + (abs_diff - (0.5 / sigma_2)) * (1. - sign)
    return in_loss.sum() / (weight.sum() + 1e-10)


def _c_round(x):
    """C roundf on a float32: half away from zero."""
    x = np.float32(x)
    return int(np.sign(x) * np.floor(np.abs(x) + np.float32(0.5)))


def roi_bins(roi, H, W, ph, pw, scale):
    """The integer bin edges [(hs, he, ws, we)] in (ph, pw) order of one ROI row (batch, cls, x1, y1, x2, y2, ...):
    lib/roi_pooling_layer/roi_pooling_op_gpu.cu.cc:40-72 in float32, one rounding per operation — the edges are
    discrete, so they are computed exactly as the op computes them, not in float64."""
    f = np.float32
    sw, sh = _c_round(f(roi[2]) * f(scale)), _c_round(f(roi[3]) * f(scale))
    ew, eh = _c_round(f(roi[4]) * f(scale)), _c_round(f(roi[5]) * f(scale))
    rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
    bh, bw = f(rh) / f(ph), f(rw) / f(pw)
    out = []
    for i in range(ph):
        hs = min(max(int(np.floor(f(i) * bh)) + sh, 0), H)
        he = min(max(int(np.ceil(f(i + 1) * bh)) + sh, 0), H)
        for j in range(pw):
            ws = min(max(int(np.floor(f(j) * bw)) + sw, 0), W)
            we = min(max(int(np.ceil(f(j + 1) * bw)) + sw, 0), W)
            out.append((hs, he, ws, we))
    return out


def roi_pool64(data, rois, ph, pw, scale):
    """ROI max pooling without channel pooling: data [B,H,W,C], rois [R,>=6] (numpy or tensor, no gradient) ->
    [R,ph,pw,C]. A bin is `amax` over its rectangle, an empty bin or a row with a batch index outside [0, B) is zero.
    torch's amax splits the gradient evenly among equal maxima while the op routes it to the first: feed data without
    ties inside a bin. Equal rectangles are pooled once (autograd sums their upstream gradients)."""
    B, H, W, C = data.shape
    rois = np.asarray(rois.detach().cpu() if isinstance(rois, torch.Tensor) else rois, dtype=np.float32)
    zero = torch.zeros((C,), dtype=data.dtype, device=data.device)
    seen = {}
    rows = []
    for r in rois:
        b = int(r[0])
        cells = []
        for hs, he, ws, we in roi_bins(r, H, W, ph, pw, scale):
            if b < 0 or b >= B or he <= hs or we <= ws:
                cells.append(zero)
                continue
            key = (b, hs, he, ws, we)
            if key not in seen:
                seen[key] = data[b, hs:he, ws:we, :].amax(dim=(0, 1))
            cells.append(seen[key])
        rows.append(torch.stack(cells).reshape(ph, pw, C))
    if not rows:
        return torch.zeros((0, ph, pw, C), dtype=data.dtype, device=data.device)
    return torch.stack(rows)


def quat_rot(q):
    """Rotation matrix of an (un-normalised) quaternion (s, u, v, w): the formula of tests/np_ref._rot."""
    s, u, v, w = q[0], q[1], q[2], q[3]
    return torch.stack([
        torch.stack([s * s + u * u - v * v - w * w, 2 * (u * v - s * w), 2 * (u * w + s * v)]),
        torch.stack([2 * (u * v + s * w), s * s - u * u + v * v - w * w, 2 * (v * w - s * u)]),
        torch.stack([2 * (u * w - s * v), 2 * (v * w + s * u), s * s - u * u - v * v + w * w])])


def average_distance_terms(pred, target, weight, points, symmetry):
    """Per row: None (no class: no weight[n, 4c] > 0) or (class, dist [P]), dist the SQUARED distance between the model
    points under the predicted and the target rotation — for a symmetric class to the nearest target point, its index
    taken without gradient (lib/average_distance_loss/average_distance_loss_op_gpu.cu.cc:35-120)."""
    C = points.shape[0]
    out = []
    for n in range(pred.shape[0]):
        live = torch.nonzero(weight[n].reshape(C, 4)[:, 0] > 0)
        if live.numel() == 0:
            out.append(None)
            continue
        c = int(live[0])
        pts = points[c].to(pred.dtype)
        x1 = pts @ quat_rot(pred[n, 4 * c:4 * c + 4]).t()
        x2 = pts @ quat_rot(target[n, 4 * c:4 * c + 4].to(pred.dtype)).t()
        if float(symmetry[c]) > 0:
            with torch.no_grad():
                idx = ((x1[:, None, :] - x2[None, :, :]) ** 2).sum(-1).argmin(dim=1)
            x2 = x2[idx]
        out.append((c, ((x1 - x2) ** 2).sum(-1)))
    return out


def average_distance64(pred, target, weight, points, symmetry, margin, num_rows=None):
    """The loss of the Averagedistance op: every point of every row with a class contributes
    (dist - margin) / (2 R P) where dist >= margin, else 0; R = the row count (`num_rows`: the true one of a capacity
    buffer, rows past it are ignored)."""
    R = pred.shape[0] if num_rows is None else int(num_rows)
    P = points.shape[1]
    total = pred.new_zeros(())
    for term in average_distance_terms(pred[:R], target[:R], weight[:R], points, symmetry):
        if term is None:
            continue
        dist = term[1]
        total = total + torch.where(dist >= margin, (dist - margin) / (2.0 * R * P), torch.zeros_like(dist)).sum()
    return total


# ---- the whole training graph ---------------------------------------------------------------------------------------
TRUNK = (("conv1_1", None), ("conv1_2", "pool1"), ("conv2_1", None), ("conv2_2", "pool2"),
         ("conv3_1", None), ("conv3_2", None), ("conv3_3", "pool3"),
         ("conv4_1", None), ("conv4_2", None), ("conv4_3", "pool4"),
         ("conv5_1", None), ("conv5_2", None), ("conv5_3", None))


def vars_from_net(net_vars, dtype=torch.float64, requires_grad=None):
    """THE place where weight layouts are decided: none is changed. `net.vars` keeps a convolution filter as
    [c_out, c_in, kh, kw] (the TF variable [kh, kw, c_in, c_out] permuted once, at load time) and an fc weight as the
    TF variable [in, out] over NHWC-flattened rows; `training_loss64` consumes exactly these, through F.conv2d on
    NCHW views and `x @ w`. A gradient computed here therefore has the layout of `net.vars[name].grad`, element for
    element. Returns detached CPU leaves in `dtype` that ask for gradients where the network's do (`requires_grad`
    None), or all / none of them (True / False)."""
    out = {}
    for k, v in net_vars.items():
        t = v.detach().to("cpu").contiguous().to(dtype)
        out[k] = t.requires_grad_(bool(v.requires_grad) if requires_grad is None else bool(requires_grad))
    return out


def _conv(x, v, name, relu=True, pad=0):
    y = F.conv2d(x, v[name + "/weights"], v[name + "/biases"], padding=pad)
    return torch.relu(y) if relu else y


def training_loss64(vars64, feed, consts, cfg, mutate=None):
    """loss = loss_cls + VERTEX_W smooth_l1 + POSE_W loss_pose + loss_regu (lib/fcn/train.py:488-519) of
    vgg16_convs("COLOR", C, U, ..., vertex_reg_2d=True, pose_reg=True, is_train=True) (lib/networks/vgg16_convs.py:36-212)
    as ONE plain function of the variables — no layer DSL, no Network subclass.

    vars64   {name: tensor} from `vars_from_net`; the dtype of the computation is theirs
    feed     data [B,H,W,3], vertex_targets / vertex_weights [B,H,W,3C], points [C,P,3], symmetry [C]; optional `planted`
             {add_score [B,H/8,W/8,U], add_score_vertex [B,H/8,W/8,128]}: constants added to the two head sums
             (vgg16_convs.run(feed, planted=...), the synthetic workload)
    consts   what the graph computes without a gradient, taken from the run under test: rois [R,7], poses_target and
             poses_weight [R,4C] (Hough voting: zero gradient registered), gt_label_weight [B,H,W,C] (hard labels: zero
             gradient registered). keep_prob is 1.
    cfg      VERTEX_W, POSE_W, WEIGHT_REG; optional VERTEX_SIGMA (the graph under test uses 1), POSE_MARGIN (0.01)
    mutate   one of MUTATIONS (the comparator self-test), or None
    Returns {"loss", "loss_cls", "loss_vertex", "loss_pose", "loss_regu"}."""
    assert mutate is None or mutate in MUTATIONS, mutate
    v = vars64
    dt = v["conv1_1/weights"].dtype
    t = lambda a: torch.as_tensor(np.asarray(a.detach().cpu()) if isinstance(a, torch.Tensor) else a).to(dt)
    x = t(feed["data"]).permute(0, 3, 1, 2)
    keep = {}
    for name, pool in TRUNK:
        x = _conv(x, v, name, pad=1)
        keep[name] = x
        if pool is not None:
            x = F.max_pool2d(x, 2, 2)
    conv4_3, conv5_3 = keep["conv4_3"], keep["conv5_3"]
    nhwc = lambda a: a.permute(0, 2, 3, 1)

    # label head: score_conv5 -> deconv 4/2, + score_conv4 -> deconv 16/8 -> 1x1 `score` with ReLU -> log_softmax
    s5 = _conv(conv5_3, v, "score_conv5")
    s4 = _conv(conv4_3, v, "score_conv4")
    planted = feed.get("planted") or {}
    add = nhwc(s4) + deconv_bilinear64(nhwc(s5), 4, 2)
    if "add_score" in planted:
        add = add + t(planted["add_score"])
    up = deconv_bilinear64(add, 16, 8)
    score = _conv(up.permute(0, 3, 1, 2), v, "score")
    prob = torch.log_softmax(nhwc(score), dim=-1)
    glw = t(consts["gt_label_weight"])
    loss_cls = -(glw * prob).sum(dim=3).sum() / (glw.sum() + 1e-10)

    # vertex head: the twin without ReLU
    s5v = _conv(conv5_3, v, "score_conv5_vertex", relu=False)
    s4v = _conv(conv4_3.detach() if mutate == "vertex_conv4_detached" else conv4_3, v, "score_conv4_vertex", relu=False)
    if mutate == "vertex_conv4_detached":
        s4v = s4v.detach()
    addv = nhwc(s4v) + deconv_bilinear64(nhwc(s5v), 4, 2)
    if "add_score_vertex" in planted:
        addv = addv + t(planted["add_score_vertex"])
    upv = deconv_bilinear64(addv, 16, 8)
    vertex_pred = nhwc(_conv(upv.permute(0, 3, 1, 2), v, "vertex_pred", relu=False))
    sigma = float(getattr(cfg, "VERTEX_SIGMA", 1.0))
    vertex_w = cfg.VERTEX_W * (2.0 if mutate == "vertex_w_doubled" else 1.0)
    loss_vertex = vertex_w * smooth_l1_vertex64(vertex_pred, t(feed["vertex_targets"]), t(feed["vertex_weights"]), sigma,
                                                _drop_sigma2_in_grad=(mutate == "sl1_sigma2_once_less"))

    # pose branch: ROI pools of conv5_3 at 1/16 and conv4_3 at 1/8, added; fc6, fc7 (ReLU), fc8, tanh
    rois = consts["rois"]
    pool5 = roi_pool64(nhwc(conv5_3), rois, 7, 7, 1.0 / 16.0)
    pool4 = roi_pool64(nhwc(conv4_3), rois, 7, 7, 1.0 / 8.0)
    if mutate == "roi_pool8_detached":
        pool4 = pool4.detach()
    h = (pool5 + pool4).reshape(pool5.shape[0], -1)                       # NHWC flatten (network.py:399-408)
    h = torch.relu(h @ v["fc6/weights"] + v["fc6/biases"])
    h = torch.relu(h @ v["fc7/weights"] + v["fc7/biases"])
    poses_tanh = torch.tanh(h @ v["fc8/weights"] + v["fc8/biases"])
    pw = t(consts["poses_weight"])
    mul = poses_tanh * pw
    poses_pred = mul * torch.rsqrt(torch.clamp((mul * mul).sum(dim=1, keepdim=True), min=1e-12))   # tf.nn.l2_normalize
    pose_w = 0.0 if mutate == "pose_w_zero" else cfg.POSE_W
    loss_pose = pose_w * average_distance64(poses_pred, t(consts["poses_target"]), pw, t(feed["points"]),
                                            t(feed["symmetry"]), float(getattr(cfg, "POSE_MARGIN", 0.01)))

    # tf.contrib.layers.l2_regularizer on every conv / fc variable, biases included (network.py:171,184,417); the fixed
    # `upscore*` filters are not variables of this graph
    loss_regu = None
    for k in sorted(v):
        if k.endswith(("/weights", "/biases")):
            term = (v[k] * v[k]).sum() * (0.5 * cfg.WEIGHT_REG)
            loss_regu = term if loss_regu is None else loss_regu + term
    loss = loss_cls + loss_regu + loss_vertex + loss_pose
    return {"loss": loss, "loss_cls": loss_cls, "loss_vertex": loss_vertex, "loss_pose": loss_pose, "loss_regu": loss_regu}


def grads_of(vars_, feed, consts, cfg, mutate=None):
    """({name: gradient of `loss`} for the variables that ask for one, {loss term: float})."""
    names = [k for k in sorted(vars_) if vars_[k].requires_grad]
    out = training_loss64(vars_, feed, consts, cfg, mutate)
    g = torch.autograd.grad(out["loss"], [vars_[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(vars_[k]) if gi is None else gi) for k, gi in zip(names, g)}
    return grads, {k: float(t_.detach()) for k, t_ in out.items()}


# ---- the comparison -------------------------------------------------------------------------------------------------
FLOOR_CAP = 1e-3       # the float32 restatement itself must stay this close to float64, per variable
MARGIN = 16.0          # a kernel's summation order may cost a few times the error of the plain float32 one
FLOOR_MIN = 2.0 ** -20


def rel_err(g, g64):
    """||g - g64||_2 / ||g64||_2 in float64 (0 when both vanish, inf when only the reference does)."""
    g, g64 = g.detach().to("cpu", torch.float64), g64.detach().to("cpu", torch.float64)
    num, den = float((g - g64).norm()), float(g64.norm())
    if den == 0.0:
        return 0.0 if num == 0.0 else math.inf
    return num / den


def bound(floor):
    return MARGIN * max(floor, FLOOR_MIN)


def rejected(grads, grads64, floors):
    """{name: (err, bound)} of the variables whose gradient the comparison of tests/test_gpu_gradients.py turns down."""
    out = {}
    for k, g64 in grads64.items():
        e = rel_err(grads[k], g64)
        if not e <= bound(floors[k]):
            out[k] = (e, bound(floors[k]))
    return out


# ---- the shared workload --------------------------------------------------------------------------------------------
GRAPH_SHAPE = (2, 96, 128)     # B, H, W of the whole-graph tests
# The scene seed. Of the seeds whose two frames each show three objects of >= 600 pixels, one of them of a symmetric class,
# this is the first whose float32 floor (tests/test_grad_ref_cpu.py) stays at rounding level, 5e-6: on seeds 3, 6, 17 and 25
# a pool / ReLU / hinge decision flips between float32 and float64 and the floor rises to 6e-4 .. 7e-3 (a looser bound,
# or over the cap). Chosen on the CPU, before any GPU run.
GRAPH_SEED = 52
NUM_CLASSES, NUM_UNITS = 22, 64


def graph_feed(seed=GRAPH_SEED, shape=GRAPH_SHAPE, n_obj=3):
    """numpy feed of the whole-graph tests, the project's synthetic training workload (synthetic workload):
    uniform random frames, the label map of a synthetic scene, the same scene planted at 1/8 resolution into the head
    features (`planted`: with random weights the heads would hand the Hough layer noise and no ROI would ever get a pose
    target), one ground-truth pose row per object at its planted centre and depth, and `vertex_objects` — the object table
    of the target-free vertex loss, with the weight 1 that dense `vertex_weights` carry."""
    from posecnn_amd import config, synth
    B, H, W = shape
    f32 = np.float32
    K = config.DEMO_INTRINSICS.copy()
    K[:2] *= W / 640.0
    label, _, frames = synth.make_batch(seed, B, H=H, W=W, C=NUM_CLASSES, n_obj=n_obj, K=K)
    planted, scenes = synth.make_planted_batch(seed, B, H=H, W=W, C=NUM_CLASSES, num_units=NUM_UNITS, n_obj=n_obj, K=K)
    assert all(f["objects"] == s["objects"] for f, s in zip(frames, scenes))      # one scene, drawn twice from one seed
    rng = np.random.default_rng(seed)
    data = (rng.integers(0, 256, (B, H, W, 3)).astype(f32) - config.PIXEL_MEANS).astype(f32)
    objects = np.zeros((B, n_obj, 6), f32)
    for n in range(B):
        for j, (cls, cx, cy, z) in enumerate(frames[n]["objects"]):
            objects[n, j] = (cls, 0, f32(cx), f32(cy), f32(np.log(z)), 1.0)
    meta = np.stack([config.make_meta_data(K)] * B).reshape(B, 1, 1, 48)
    return {"data": data, "gt_label_2d": label.astype(np.int32), "keep_prob": 1.0, "poses": synth.make_gt_poses(scenes, K),
            "extents": config.LOV_EXTENTS, "meta_data": meta, "points": synth.make_model_points(NUM_CLASSES, 64),
            "symmetry": config.LOV_SYMMETRY, "vertex_objects": objects, "planted": planted}


def dense_vertex_feed(feed):
    """+ vertex_targets / vertex_weights [B,H,W,3C] of the object table (tests/vertex_ref.py: the numpy restatement that is
    pinned to the reference's own outputs)."""
    import vertex_ref
    out = dict(feed)
    out["vertex_targets"], out["vertex_weights"] = vertex_ref.vertex_targets(feed["gt_label_2d"], feed["vertex_objects"], NUM_CLASSES)
    return out
