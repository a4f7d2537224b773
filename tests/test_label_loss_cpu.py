"""CPU-side checks of the training label head (include/posecnn_hip_loss.h, posecnn_amd/ops.label_head_loss): the float32
log of the softmax denominator against float64 over every argument it can meet, the C entries' host validation, and the float32 restatement the GPU test compares with (tests/label_loss_ref.py) against float64
autograd — with the five seeded defects that comparison has to turn down.

Measured here and recorded in DESIGN.md: log_sum_f32 over all 50 331 649 float32 in [1, 64] is within 1.97 ulp of the
float64 logarithm (worst at x = 1.0038618; ulp = the float32 spacing at the true value), 2.62e-7 in absolute terms."""
import ctypes
import os

import numpy as np
import pytest

import grad_ref
import label_loss_ref as R

F = np.float32


# ---- log_sum_f32 -------------------------------------------------------------------------------------------------------
def test_log_sum_f32_against_float64_over_every_float_in_range():
    lo, hi = int(F(1).view(np.int32)), int(F(64).view(np.int32))
    assert hi - lo + 1 == 6 * (1 << 23) + 1
    worst, worst_x, worst_abs = 0.0, None, 0.0
    step = 1 << 22
    for a in range(lo, hi + 1, step):
        x = np.arange(a, min(a + step, hi + 1), dtype=np.int32).view(F)
        got = R.log_sum_f32(x).astype(np.float64)
        ref = np.log(x.astype(np.float64))
        err = np.abs(got - ref)
        ulps = err / np.spacing(np.abs(ref).astype(F)).astype(np.float64)
        i = int(np.argmax(ulps))
        if ulps[i] > worst:
            worst, worst_x = float(ulps[i]), float(x[i])
        worst_abs = max(worst_abs, float(err.max()))
    print("log_sum_f32: worst error %.4f ulp at x = %.9g, worst absolute error %.4e" % (worst, worst_x, worst_abs))
    assert R.log_sum_f32(np.array([1.0], F))[0] == 0.0
    assert 1.96 < worst <= 1.97 and worst_abs <= 2.62e-7          # the recorded figures (module docstring)
    nan = R.log_sum_f32(np.array([np.nan], F))
    assert nan[0] != nan[0]


# ---- the C boundary ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from posecnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_cpu_tensors_are_refused():
    import torch
    from posecnn_amd import ops
    z, b, gt = torch.zeros(1, 1, 1, 5), torch.zeros(5), torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.label_head_loss(z, b, gt, 0.5, 4, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.label_head_loss_grad(z, b, gt, 0.5, 4, 2)


def test_argument_validation_happens_on_the_host(L):
    """Every call here returns before anything is launched: the device pointers are host addresses that are never read."""
    from posecnn_amd._lib import PCNN_EINVAL, PCNN_ENULL, PCNN_EWORKSPACE, PCNN_OK
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 8)
    n = ctypes.c_size_t(77)
    # one workgroup per 128-pixel run of an output row, C doubles each
    assert L.pcnn_label_head_loss_workspace_bytes(2, 3, 17, 22, 16, 8, ctypes.byref(n)) == PCNN_OK and n.value == 2 * 24 * 2 * 22 * 8
    assert L.pcnn_label_head_loss_workspace_bytes(1, 1, 3, 5, 4, 2, ctypes.byref(n)) == PCNN_OK and n.value == 2 * 5 * 8
    need = n.value
    assert L.pcnn_label_head_loss_workspace_bytes(1, 1, 3, 5, 4, 2, None) == PCNN_ENULL
    assert b"bytes" in L.pcnn_last_error_string()

    base = dict(z=p, bias=p, gt=p, sums=p, up=None, B=1, H=1, W=3, C=5, k=4, s=2, relu=1, thr=0.5, loss=p, label=p, terms=None,
                dscore=p, dbias=p, ws=p, ws_bytes=need)

    def fwd(**kw):
        a = dict(base, **kw)
        return L.pcnn_label_head_loss_fwd(a["z"], a["bias"], a["gt"], a["B"], a["H"], a["W"], a["C"], a["k"], a["s"], a["relu"],
                                          a["thr"], a["loss"], a["sums"], a["label"], a["terms"], a["ws"], a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(base, **kw)
        return L.pcnn_label_head_loss_bwd(a["z"], a["bias"], a["gt"], a["sums"], a["up"], a["B"], a["H"], a["W"], a["C"], a["k"],
                                          a["s"], a["relu"], a["thr"], a["dscore"], a["dbias"], a["ws"], a["ws_bytes"], None)

    def refused(call, status, word, **kw):
        assert call(**kw) == status, kw
        msg = L.pcnn_last_error_string().decode()
        assert word in msg, (kw, msg)

    for call, outputs in ((fwd, ("loss", "label")), (bwd, ("dscore", "dbias"))):
        for name, word in (("z", "z"), ("bias", "bias"), ("gt", "gt_label"), ("sums", "sums")) + tuple((o, o) for o in outputs):
            refused(call, PCNN_ENULL, "NULL " + word, **{name: None})
        refused(call, PCNN_EINVAL, "num_classes", C=1)
        refused(call, PCNN_EINVAL, "num_classes", C=65)
        refused(call, PCNN_EINVAL, "threshold", thr=0.0)
        refused(call, PCNN_EINVAL, "threshold", thr=-1.0)
        for k, s in ((3, 2), (2, 4), (10, 2), (4, 0), (66, 22)):              # odd difference, k < s, k > 4 s, s < 1, k > 64
            refused(call, PCNN_EINVAL, "kernel", k=k, s=s)
        refused(call, PCNN_EINVAL, "batch", B=0)
        refused(call, PCNN_EINVAL, "2^31", B=1 << 14, H=1 << 8, W=1 << 8, s=2, k=4)
        refused(call, PCNN_EINVAL, "sums must be 16-byte aligned", sums=odd)
        refused(call, PCNN_EINVAL, "workspace must be 16-byte aligned", ws=odd)
        refused(call, PCNN_EWORKSPACE, "workspace", ws=None)
        refused(call, PCNN_EWORKSPACE, "workspace", ws_bytes=need - 1)
    refused(lambda **kw: L.pcnn_label_head_loss_workspace_bytes(1, 1, 3, kw["C"], 4, 2, ctypes.byref(n)), PCNN_EINVAL,
            "num_classes", C=1)


# ---- the restatement against float64 ----------------------------------------------------------------------------------
UPSTREAM = 0.37
# The criterion of tests/grad_ref.py with the floor at its minimum: 16 x 2^-20 = 1.5e-5. A pixel takes ~40 float32
# operations from z to dscore (2.4e-6 at 6e-8 each) and the sums of the reference are float64.
BOUND = grad_ref.bound(0.0)


def _errors(c, mutate=None):
    shape, C, (k, s) = c
    z, bias, gt = R.case(shape, C, (k, s))
    r = R.reference(shape, C, (k, s), upstream=UPSTREAM)
    loss64, dz64, db64 = R.loss64(z, bias, gt, R.THRESHOLD, k, s, mutate=mutate)
    import torch
    t = torch.from_numpy
    return {"loss": abs(float(r["loss"]) - loss64) / abs(loss64),
            "dz": grad_ref.rel_err(t(r["dz"].copy()), t(dz64 * UPSTREAM)),
            "dbias": grad_ref.rel_err(t(r["dbias64"].copy()), t(db64 * UPSTREAM))}


@pytest.mark.parametrize("c", R.cases(), ids=R.case_id)
def test_cases_hold_what_the_gpu_test_needs(c):
    """-1, ground-truth 0 with prob[0] clearly on either side of the threshold, foreground, a label >= C, gated and live
    ReLUs; the all-ignored map counts nothing and has zero gradients."""
    shape, C, ks = c
    _, _, gt = R.case(shape, C, ks)
    r = R.reference(shape, C, ks, upstream=UPSTREAM)
    p0 = r["prob"][..., 0][gt == 0]
    assert (p0 < R.THRESHOLD - 1e-3).any() and (p0 > R.THRESHOLD + 1e-3).any() and (np.abs(p0 - R.THRESHOLD) > 1e-3).all()
    assert (gt == -1).any() and (gt >= C).any() and ((gt > 0) & (gt < C)).any()
    assert not r["hot"][(gt < 0) | (gt >= C)].any() and r["hot"][(gt > 0) & (gt < C)].all()
    assert (r["score"] == 0).any() and (r["score"] > 0).any()
    assert 0 < r["count"] < gt.size and np.isfinite(r["loss"]) and r["loss"] > 0
    if shape[0] > 1:
        assert not r["hot"][-1].any() and not r["dscore"][-1].any()
    e = R.reference(shape, C, ks, "ignored")
    assert e["count"] == 0 and e["loss"] == 0 and not e["dscore"].any() and not e["dz"].any() and not e["terms"].any()
    assert np.array_equal(e["label"], r["label"])


@pytest.mark.parametrize("c", R.cases(), ids=R.case_id)
def test_restatement_is_within_the_criterion_of_float64(c):
    err = _errors(c)
    print(R.case_id(c), {k: "%.2e" % v for k, v in err.items()}, "bound %.2e" % BOUND)
    assert all(v <= BOUND for v in err.values()), err


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_seeded_defects_are_rejected(mutate):
    """Each defect must push the loss or a gradient over the bound on every case it can show on (all but the ReLU gate's
    defect change the result wherever a pixel is hot)."""
    for c in R.cases():
        err = _errors(c, mutate)
        assert any(not v <= BOUND for v in err.values()), (mutate, R.case_id(c), err)
