"""Every host-path route of `posecnn_amd/networks.py` and `fcn.im_segment_batch` (tests/network_routes.py has the table)
against a float64 restatement of the graph: the kernels the route launched (a), its layers bit for bit against the partner
route where the code claims equal bits (b), every layer within M e32 of float64 (c), the label map on every pixel whose
float64 margin pins it (d), and the pose path against the oracle-based CPU network on the route's own maps (e).
tests/ROUTES.md records the table as run, the measured ratios and the mutants."""
import numpy as np
import pytest
import torch

import network_routes as R
from posecnn_amd import config, synth

pytestmark = pytest.mark.gpu

_VARS, _RUNS, _POSE = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_what_the_module_shared():
    """The variables (fc6 among them) and every row's outputs live for this module only."""
    yield
    _VARS.clear(), _RUNS.clear(), _POSE.clear()
    torch.cuda.empty_cache()


def gpu_vars(gpu, fmt, C, U, fc=False):
    """One set of variables per (format, C, units) for the whole module, handed to every variant."""
    key = (fmt, C, U, fc)
    if key not in _VARS:
        _VARS[key] = {k: v.to(gpu) for k, v in R.vars_for(fmt, C, U, fc).items()}
    return _VARS[key]


def extents_for(C):
    e = np.asarray(config.LOV_EXTENTS, np.float32)
    return np.stack([e[c % len(e)] for c in range(C)])


def inputs_for(gpu, case, H, W, C, U):
    color, depth, (bc, bd) = R.frames_for(case.B, H, W)
    if getattr(case, "raw", False):
        data, data_p = torch.from_numpy(color).to(gpu), torch.from_numpy(depth).to(gpu)
    else:
        data, data_p = torch.from_numpy(bc).to(gpu), torch.from_numpy(bd).to(gpu)
    planted = None
    if getattr(case, "planted", True):
        planted = {k: torch.from_numpy(v).to(gpu) for k, v in R.planted_for(case.B, H, W, C, U)[0].items()}
    return data, (data_p if case.fmt == "RGBD" else None), planted


def profiled(fn):
    """fn() with the library's kernel profile on: (result, {kernel: calls})."""
    from posecnn_amd import _lib
    _lib.profile_enable(True)
    try:
        _lib.profile_report()
        out = fn()
        torch.cuda.synchronize()
        return out, R.kernel_calls(_lib.profile_report())
    finally:
        _lib.profile_enable(False)


def fetch(net, names):
    out = {}
    for n in names:
        if n in net.layers:
            t = net.get_output(n)
            if isinstance(t, torch.Tensor):
                out[n] = t.detach().cpu()
    return out


def layer_names(fmt, pose=False):
    trunk = [n for n in R.TRUNK_KEEP if not (pose and n == "pool4")]      # (the pose graph's `pool4` is the roi_pool of that name)
    if fmt == "RGBD":
        trunk += [n + "_p" for n in trunk]
    return trunk + list(R.HEAD_LAYERS) + ["label_2d"]


def run_case(gpu, case):
    """One row of the table, once per module: {layer: cpu tensor}, {kernel: calls}, the network."""
    if case.name in _RUNS:
        return _RUNS[case.name]
    from posecnn_amd import fcn
    from posecnn_amd.networks import vgg16_convs
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    a, kw = R.ctor_args(case.fmt, case.C, case.U, case.ctor, gpu)
    net = vgg16_convs(*a, **kw)
    shared = gpu_vars(gpu, case.fmt, case.C, case.U)
    net.vars = {k: v.clone() for k, v in shared.items()} if case.grad else dict(shared)   # (autograd flags its variables)
    for k, v in case.flags.items():
        assert hasattr(net, k), k
        setattr(net, k, v)
    data, data_p, planted = inputs_for(gpu, case, case.H, case.W, case.C, case.U)
    feed = fcn._feed(net, data, data_p, R.intrinsics(case.W), extents_for(case.C), np.zeros((case.C, 4, 3), np.float32),
                     np.zeros((case.C,), np.float32), case.C, gpu)

    def go():
        with (torch.enable_grad() if case.grad else torch.no_grad()):
            net.run(feed, planted=planted)
            return fetch(net, layer_names(case.fmt))
    layers, calls = profiled(go)
    _RUNS[case.name] = (layers, calls, net)
    return _RUNS[case.name]


def check_layers_present(case, net, layers, pose=False):
    want = set(layer_names(case.fmt, pose)) - {"score", "prob_normalized"}
    if net.want_prob:
        want.add("prob_normalized")
    if net.with_losses or not net.fused_heads:
        want.add("score")
    assert want <= set(layers), sorted(want - set(layers))


def check_against_float64(tag, layers, refs, family):
    """c. and d.: every layer within M e32 of ref64; the label map on the pixels that count. Prints each ratio first."""
    r64, r32, e32 = refs
    bad = []
    for name, t in sorted(layers.items()):
        if name == "label_2d":
            continue
        fam = R.family_of_layer(name, family)
        ratio = float((t.double() - r64[name]).abs().max()) / e32[name]
        print("RATIO %-30s %-20s %-7s %8.3f" % (tag, name, fam, ratio))
        if not ratio <= R.M[fam]:
            bad.append((name, fam, ratio, R.M[fam]))
    counted, wrong, left = R.label_check(layers["label_2d"], r64, e32)
    print("LABEL %-30s counted %d wrong %d left out %.4f" % (tag, counted, wrong, left))
    assert not bad, bad
    assert wrong == 0, "%d label pixels differ from the float64 argmax where its margin pins them" % wrong
    assert left <= R.LABEL_CAP


def check_equal_bits(case, layers, partner_layers):
    names = sorted(set(layers) & set(partner_layers)) if case.e_layers == R.ALL else [n for n in case.e_layers if n in layers]
    assert len(names) >= (9 if case.e_layers != R.ALL else min(len(layers), len(partner_layers))), names
    diff = [n for n in names if not torch.equal(layers[n], partner_layers[n])]
    assert not diff, "%s differs from %s in %s although: %s" % (case.name, case.partner, diff, R.CLAIMS[case.claim])


@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_route(gpu, case):
    layers, calls, net = run_case(gpu, case)
    print("CALLS %-30s %s" % (case.name, sorted(calls.items())))
    assert not R.route_errors(calls, case.present), (R.route_errors(calls, case.present), sorted(calls.items()))     # a.
    check_layers_present(case, net, layers)
    if case.partner is not None:                                                                                    # b.
        check_equal_bits(case, layers, run_case(gpu, next(c for c in R.TABLE if c.name == case.partner))[0])
    check_against_float64(case.name, layers, R.case_reference(case), case.family)                                   # c., d.


def test_lazily_initialised_network_first_and_second_run(gpu):
    """A COLOR network without variables: on its first run `_merged_head_convs` is off (the head variables do not exist yet:
    four row products, created in the reference's order), on the second it is on (two). The profile differs, the outputs
    must not, and both are the float64 graph of the variables the first run created."""
    from posecnn_amd import fcn
    from posecnn_amd.networks import vgg16_convs
    case = R.TABLE[0]
    a, kw = R.ctor_args("COLOR", case.C, case.U, {}, gpu)
    net = vgg16_convs(*a, **kw)
    assert not net.vars
    data, data_p, planted = inputs_for(gpu, case, case.H, case.W, case.C, case.U)
    feed = fcn._feed(net, data, None, R.intrinsics(case.W), extents_for(case.C), np.zeros((case.C, 4, 3), np.float32),
                     np.zeros((case.C,), np.float32), case.C, gpu)

    def go():
        with torch.no_grad():
            net.run(feed, planted=planted)
            return fetch(net, layer_names("COLOR"))
    first, calls1 = profiled(go)
    second, calls2 = profiled(go)
    print("CALLS lazy_first %s\nCALLS lazy_second %s" % (sorted(calls1.items()), sorted(calls2.items())))
    assert not R.route_errors(calls1, R.LAZY_FIRST), R.route_errors(calls1, R.LAZY_FIRST)
    assert not R.route_errors(calls2, R.LAZY_SECOND), R.route_errors(calls2, R.LAZY_SECOND)
    assert calls1 != calls2
    assert set(first) == set(second) and len(first) >= 12
    diff = [n for n in first if not torch.equal(first[n], second[n])]
    assert not diff, "second run differs in %s although: %s" % (diff, R.CLAIMS["merged"])
    refs = R.case_reference(case, variables=net.vars, vars_key="lazy")
    check_against_float64("lazy_first", first, refs, "F(4,3)")


# ---- pose path ----------------------------------------------------------------------------------------------------------

def run_pose(gpu, case):
    if case.name in _POSE:
        return _POSE[case.name]
    from posecnn_amd import fcn
    from posecnn_amd.networks import vgg16_convs
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    C, H, W = R.POSE_C, R.POSE_H, R.POSE_W
    a, kw = R.ctor_args(case.fmt, C, 64, {}, gpu)
    kw.update(vertex_reg_2d=True, vertex_reg_3d=False, pose_reg=True)
    kw.update(case.ctor)
    net = vgg16_convs(*a, **kw)
    net.vars = dict(gpu_vars(gpu, case.fmt, C, 64, True))
    for k, v in case.flags.items():
        assert hasattr(net, k), k
        setattr(net, k, v)
    data, data_p, planted = inputs_for(gpu, case, H, W, C, 64)
    K = R.intrinsics(W)
    pts = synth.make_model_points(C, 32)
    scenes = R.planted_for(case.B, H, W, C, 64)[1]
    gt = torch.from_numpy(synth.make_gt_poses(scenes, K, seed=3)).to(gpu) if case.kwargs.get("gt") else None
    res = {"gt": gt}

    def go():
        with torch.no_grad():
            if case.driver == "batch":
                det = fcn.im_segment_batch(net, data, K, config.LOV_EXTENTS, pts, config.LOV_SYMMETRY, data_p=data_p, planted=planted,
                                           with_losses=bool(case.kwargs.get("with_losses")), gt_poses=gt,
                                           frame_offset=case.kwargs.get("frame_offset"))
                res.update(rows=det.rows.cpu(), count=int(det.count.item()), packed=None if det.packed is None else det.packed.cpu(),
                           det=det)
            else:
                feed = fcn._feed(net, data, data_p, K, config.LOV_EXTENTS, pts, config.LOV_SYMMETRY, C, gpu)
                net.run(feed, planted=planted)
            out = fetch(net, layer_names(case.fmt, pose=True) + ["rois", "poses_init", "poses_tanh", "poses_target", "poses_weight",
                                                                 "pool_score", "poses_pred", "extents", "meta_data", "gt_label_weight"])
            return out
    layers, calls = profiled(go)
    _POSE[case.name] = (layers, calls, net, res)
    return _POSE[case.name]


@pytest.mark.parametrize("case", R.POSE_TABLE, ids=lambda c: c.name)
def test_pose_route(gpu, case):
    from cpu_reference import vgg16_convs_cpu
    from posecnn_amd import dist as pdist, ops
    layers, calls, net, res = run_pose(gpu, case)
    print("CALLS %-30s %s" % (case.name, sorted(calls.items())))
    assert not R.route_errors(calls, case.present), (R.route_errors(calls, case.present), sorted(calls.items()))
    graph = {k: v for k, v in layers.items() if k in layer_names(case.fmt, pose=True)}
    check_layers_present(case, net, graph, pose=True)
    check_against_float64(case.name, graph, R.case_reference(case), "F(4,3)")

    # e. the discrete part on identical inputs: the oracle-based CPU network on this route's own label_2d / vertex_pred
    C = R.POSE_C
    is_train = int(net.is_train)
    stride = 9 if is_train else 1
    cpu = vgg16_convs_cpu(*R.ctor_args(case.fmt, C, 64, {}, "cpu")[0], vertex_reg_2d=True, pose_reg=True, trainable=False,
                          is_train=bool(is_train), init="he")
    cpu.vars = R.vars_for(case.fmt, C, 64, True)
    src = dict(layers, poses=res["gt"])
    per_image = C - 1 if case.driver == "batch" else 0
    tail = R.pose_tail_cpu(cpu, src, is_train, per_image, dtype=None)
    n = tail["n"]
    print("POSE  %-30s rows %d" % (case.name, n))
    assert n >= case.B * stride, "the planted scene gave no detections"
    if case.driver == "batch":
        assert res["count"] * stride == n, (res["count"], stride, n)
        assert ops.hough_rows_capacity(case.B, is_train, C - 1) == layers["rois"].shape[0] == case.expect["capacity"]
    rois, init = layers["rois"][:n].numpy(), layers["poses_init"][:n].numpy()
    assert np.array_equal(rois, tail["rois"][:n]), np.abs(rois - tail["rois"][:n]).max(axis=0)      # image, class, box, votes
    assert np.array_equal(init, tail["poses_init"][:n]), np.abs(init - tail["poses_init"][:n]).max(axis=0)
    assert np.array_equal(layers["pool_score"][:n].numpy().reshape(n, -1), tail["pool_score"][:n].reshape(n, -1)), R.CLAIMS["pool2"]
    t64, t32 = tail["poses_tanh", torch.float64][:n], tail["poses_tanh", torch.float32][:n]
    e32 = float((t32.double() - t64).abs().max())
    ratio = float((layers["poses_tanh"][:n].double() - t64).abs().max()) / e32
    print("RATIO %-30s %-20s %-7s %8.3f" % (case.name, "poses_tanh", "fc", ratio))
    assert np.isfinite(e32) and e32 > 0
    assert ratio <= R.M["fc"], (ratio, e32)
    if is_train:
        assert np.array_equal(layers["poses_weight"][:n].numpy(), tail["poses_weight"][:n])
        assert np.array_equal(layers["poses_target"][:n].numpy(), tail["poses_target"][:n])
        assert tail["poses_weight"][:n].any()
    if case.driver == "batch":
        rows, cnt = res["rows"].numpy(), res["count"]
        pt = layers["poses_tanh"].numpy()
        assert not rows[cnt:].any(), "rows at or past the device-side count must be zero"
        for i in range(cnt):
            r = i * stride
            c = int(rois[r, 1])
            shift = case.kwargs.get("frame_offset") or 0     # (with an offset `rows` is a view of the packed block: global frames)
            assert rows[i, 0] == rois[r, 0] + shift and np.array_equal(rows[i, 1:7], rois[r, 1:])
            assert np.array_equal(rows[i, 7:11], pt[r, 4 * c:4 * c + 4])
            assert np.array_equal(rows[i, 11:], init[r, 4:])
        dead = [k for k in ("poses_tanh", "poses_pred") if k in layers and layers[k][n:].any()]
        assert not dead, "%s has rows at or past the count" % dead
        if case.kwargs.get("frame_offset") is not None:
            # (`rows` already carries the global frame numbers, checked above: the block is those rows + the count row)
            want = pdist.pack_detections(res["det"].rows, res["det"].count, 0).cpu()
            assert torch.equal(res["packed"], want)
        if case.kwargs.get("with_losses"):
            pred = layers["poses_pred"][:n].double()
            mul = layers["poses_tanh"][:n].double() * layers["poses_weight"][:n].double()
            want = mul * torch.rsqrt(torch.clamp((mul * mul).sum(dim=1, keepdim=True), min=1e-12))
            assert float((pred - want).abs().max()) < 3e-7      # (the bound test_gpu_round5.py holds the kernel to)
            hard = ops.hard_label(net.get_output("prob_normalized"), net.get_output("gt_label_2d"), net.threshold_label)
            assert torch.equal(net.get_output("gt_label_weight"), hard)
    else:
        # the DSL graph against the batch driver on the same frame: the same rows, pooled features bit for bit, and poses_tanh
        # of the framework's addmm within the fc margin of the same float64 tail (above)
        b_layers = run_pose(gpu, next(c for c in R.POSE_TABLE if c.name == "pose_b1_skinny"))[0]
        assert layers["rois"].shape[0] == n
        assert torch.equal(layers["rois"], b_layers["rois"][:n])
        assert torch.equal(layers["pool_score"], b_layers["pool_score"][:n]), R.CLAIMS["pool2"]
