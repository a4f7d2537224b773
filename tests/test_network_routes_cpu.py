"""The route table of tests/network_routes.py and its float64 reference, as far as they can be checked without a GPU: the
reference against the CPU restatement the end-to-end tests trust, the yardstick e32, the 1 % cap on label pixels that are
left out, the pure predicates at each row's shapes, and that every route flag has a row."""
import numpy as np
import pytest
import torch

import network_routes as R
from posecnn_amd import fcn, ops

ROWS = {c.name: c for c in R.TABLE}
REF_KEYS = {}
for _c in list(R.TABLE) + list(R.POSE_TABLE):
    REF_KEYS.setdefault((_c.fmt, _c.B, getattr(_c, "H", R.POSE_H), getattr(_c, "C", R.POSE_C), getattr(_c, "U", 64),
                         getattr(_c, "planted", True)), _c)


@pytest.mark.parametrize("name", ["color_default", "rgbd_grouped_b2", "color_c33", "color_u40", "color_unplanted"])
def test_reference_float32_agrees_with_the_cpu_restatement(name):
    """The new reference in float32 against `vgg16_convs_cpu` (framework convolutions + the C oracle) on the same variables at
    32 x 48. Both are float32 evaluations of the float64 graph in different summation orders. e32 is ONE sample of the largest
    error such an evaluation makes over a layer; another order's largest error is a second sample of the same tail and may
    well be twice the first, so the two evaluations can be (1 + 2) e32 apart, and 8 leaves the usual factor of two and a
    bit on top. A reference with a wrong tap, bias or transpose is thousands of e32 away."""
    from cpu_reference import vgg16_convs_cpu
    case = ROWS[name]
    r64, r32, e32 = R.case_reference(case)
    a, kw = R.ctor_args(case.fmt, case.C, case.U, {}, "cpu")
    cpu = vgg16_convs_cpu(*a, **kw)
    cpu.vars = dict(R.vars_for(case.fmt, case.C, case.U))
    color, depth, (bc, bd) = R.frames_for(case.B, case.H, case.W)
    K = R.intrinsics(case.W)
    feed = fcn._feed(cpu, torch.from_numpy(bc), torch.from_numpy(bd) if case.fmt == "RGBD" else None, K,
                     np.zeros((case.C, 3), np.float32), np.zeros((case.C, 1, 3), np.float32), np.zeros((case.C,), np.float32),
                     case.C, torch.device("cpu"))
    planted = R.planted_for(case.B, case.H, case.W, case.C, case.U)[0] if case.planted else None
    with torch.no_grad():
        cpu.run(feed, planted=None if planted is None else {k: torch.from_numpy(v) for k, v in planted.items()})
    seen = 0
    for layer in sorted(e32):
        if layer not in cpu.layers or layer == "score":
            continue
        got = cpu.get_output(layer)
        if got is None:
            continue
        d = float((got.double() - r32[layer].double()).abs().max())
        print("%-22s |cpu - ref32| = %.3g = %.2f e32" % (layer, d, d / e32[layer]))
        assert d <= 8 * e32[layer], (layer, d, e32[layer])
        seen += 1
    assert seen >= 11
    counted, wrong, left = R.label_check(cpu.get_output("label_2d"), r64, e32)
    assert wrong == 0 and left <= R.LABEL_CAP


@pytest.mark.parametrize("key", sorted(REF_KEYS, key=str), ids=lambda k: "-".join(map(str, k)))
def test_e32_is_a_yardstick_and_the_label_cap_holds(key):
    """e32[layer] = max|ref32 - ref64| is finite and non-zero for every layer of every distinct (format, batch, size, C, units,
    planted) of the two tables, and ref32's own argmax equals ref64's on every pixel that counts, with at most 1 % left out."""
    case = REF_KEYS[key]
    r64, r32, e32 = R.case_reference(case)
    want = set(R.TRUNK_KEEP) | set(R.HEAD_LAYERS)
    if case.fmt == "RGBD":
        want |= {n + "_p" for n in R.TRUNK_KEEP}
    assert set(e32) == want
    for layer, e in e32.items():
        assert np.isfinite(e) and e > 0, (layer, e)
        assert e < 1e-3 * max(1.0, float(r64[layer].abs().max())), (layer, e)     # (a float32 rounding error, not a disagreement)
    counted, wrong, left = R.label_check(r32["label_2d"], r64, e32)
    print("label pixels left out: %.3f %%, threshold %.3g" % (100 * left, 2 * R.M["1x1"] * e32["score"]))
    assert wrong == 0
    assert left <= R.LABEL_CAP, left


def test_pose_scene_yields_detections():
    """96 x 128 with two planted objects per frame: LABEL_THRESHOLD = 500 pixels still leaves detections in every frame of the
    float64 label map (checked before the scene was fixed)."""
    for B in (1, 2):
        case = next(c for c in R.POSE_TABLE if c.B == B and c.fmt == "COLOR")
        r64 = R.case_reference(case)[0]
        for b in range(B):
            lab = r64["label_2d"][b].numpy()
            big = [c for c in range(1, R.POSE_C) if (lab == c).sum() > ops.LABEL_THRESHOLD]
            assert len(big) >= 1, (B, b, np.bincount(lab.ravel()))


@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_predicates_take_the_side_the_row_expects(case):
    net = R.instance_for(case)
    if "conv12" in case.expect:
        assert net._conv12_fused_at(case.H, case.W) is case.expect["conv12"]
    if "mfma_label" in case.expect:
        assert net._mfma_head_ok(case.U, case.C) is case.expect["mfma_label"]
    if "mfma_vertex" in case.expect:
        assert net._mfma_head_ok(128, 3 * case.C) is case.expect["mfma_vertex"]
    # what the kernel counts of the row say about the same predicates
    if case.present.get("head_lowres_mfma_kernel") == 2:
        assert net._mfma_head_ok(case.U, case.C) and net._mfma_head_ok(128, 3 * case.C)
    if case.present.get("conv12_wino43_fused_kernel", 0) > 0:
        assert net._conv12_fused_at(case.H, case.W)


@pytest.mark.parametrize("case", R.POSE_TABLE, ids=lambda c: c.name)
def test_pose_predicates_take_the_side_the_row_expects(case):
    net = R.instance_for(case)
    is_train = bool(net.is_train)
    cap = ops.hough_rows_capacity(case.B, is_train, R.POSE_C - 1)
    if "capacity" in case.expect:
        assert cap == case.expect["capacity"]
    grad = False
    if "fc6" in case.expect:
        assert net._fc_route(True, cap, 7 * 7 * 512, 4096, grad, True) == case.expect["fc6"]
        assert net._fc_route(True, cap, 4096, 4096, grad, True) == case.expect["fc6"]
    if "fc8" in case.expect:
        assert net._fc_route(True, cap, 4096, 4 * R.POSE_C, grad, True, padded_width=True) == case.expect["fc8"]
    if "masks" in case.expect:
        with torch.no_grad():
            assert net.fc_masks_dead_rows("fc6", 7 * 7 * 512, 4096, rows=cap) is case.expect["masks"]
    if case.driver == "dsl":      # no device-side count: the framework, whatever the shapes
        assert net._fc_route(True, cap, 7 * 7 * 512, 4096, grad, False) == "addmm"


def test_every_route_flag_has_a_row_with_a_value_that_is_not_the_default():
    """Parses `Network.__init__` and `vgg16_convs.__init__`: every attribute they assign that a condition in networks.py or
    fcn.py reads, other than those network_routes.NOT_ROUTES explains away, differs from the default instance in some row."""
    flags, assigned, read = R.route_flags()
    for must in ("fused_conv12", "fused_first_conv", "fuse_first_conv_into_winograd", "winograd_mfma", "winograd_tile",
                 "winograd_min_channels", "defer_act", "dual_pool", "strict_numerics", "fused_heads", "want_prob", "with_losses",
                 "grouped_towers", "merge_head_convs", "mfma_heads", "head_gemm", "small_heads", "small_heads_max_pixels", "fc_skinny",
                 "num_units", "num_classes", "input_format", "is_train", "trainable"):
        assert must in flags, (must, flags)      # (the parse finds what the issue names)
    assert set(R.NOT_ROUTES) <= set(assigned), set(R.NOT_ROUTES) - set(assigned)
    default = R.instance_for(R.TABLE[0])
    instances = [R.instance_for(c) for c in list(R.TABLE) + list(R.POSE_TABLE)]
    missing = [f for f in flags if not any(getattr(i, f) != getattr(default, f) for i in instances)]
    assert not missing, "route flags no row sets: %s" % missing


def test_table_is_well_formed():
    names = [c.name for c in R.TABLE]
    assert len(set(names)) == len(names)
    for c in R.TABLE:
        assert c.family in R.M
        if c.partner is not None:
            p = ROWS[c.partner]
            assert (p.fmt, p.B, p.H, p.W, p.C, p.U, p.planted) == (c.fmt, c.B, c.H, c.W, c.C, c.U, c.planted), c.name
            assert c.claim in R.CLAIMS and c.e_layers, c.name
            assert names.index(c.partner) < names.index(c.name)
    assert all(1 <= m <= 16 for m in R.M.values())
