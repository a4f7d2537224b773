"""CPU-side checks of the training vertex head (include/posecnn_hip_vertex_loss.h, posecnn_amd/ops.vertex_head_loss): the
C entries' host validation, and the two numpy statements the GPU test compares with
(tests/vertex_head_ref.py) against each other and against float64 autograd.

The central claim of the fused backward — a pixel whose matched class does not own a channel would add +-0 to a sum that
is never -0, so skipping it changes no bit — is proven here: `restate` skips, `reference` is the dense composition, and the
two are bit-equal on every case and kind."""
import ctypes
import os

import numpy as np
import pytest

import grad_ref
import vertex_head_ref as R

F = np.float32
IDS = ["%s-%s" % nk for nk in R.case_ids()]


@pytest.fixture(scope="module")
def L():
    from posecnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the C boundary ------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    import torch
    from posecnn_amd import ops
    z, b = torch.zeros(1, 1, 1, 6), torch.zeros(6)
    gt, obj = torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(1, 1, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vertex_head_loss(z, b, gt, obj, 4, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vertex_head_loss_grad(z, b, gt, obj, 4, 2)


def test_argument_validation_happens_on_the_host(L):
    """Every call here returns before anything is launched: the device pointers are host addresses that are never read."""
    from posecnn_amd._lib import PCNN_EINVAL, PCNN_ENULL, PCNN_EWORKSPACE, PCNN_OK
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 8)
    n = ctypes.c_size_t(77)
    # backward: one f64 per channel and tile of 4 x 8 cells; the forward's 2 x 1024 f32 partials when that is more
    assert L.pcnn_vertex_head_loss_workspace_bytes(16, 60, 80, 22, 16, 8, ctypes.byref(n)) == PCNN_OK
    assert n.value == 16 * 15 * 10 * 66 * 8
    assert L.pcnn_vertex_head_loss_workspace_bytes(1, 1, 3, 5, 4, 2, ctypes.byref(n)) == PCNN_OK and n.value == 2 * 1024 * 4
    need = n.value
    assert L.pcnn_vertex_head_loss_workspace_bytes(1, 1, 3, 5, 4, 2, None) == PCNN_ENULL
    assert b"bytes" in L.pcnn_last_error_string()

    base = dict(z=p, bias=p, label=p, inst=None, obj=p, out=p, up=None, B=1, H=1, W=3, C=5, M=2, k=4, s=2, sigma=1.0, dz=p,
                dbias=p, ws=p, ws_bytes=need)

    def fwd(**kw):
        a = dict(base, **kw)
        return L.pcnn_vertex_head_loss_fwd(a["z"], a["bias"], a["label"], a["inst"], a["obj"], a["B"], a["H"], a["W"], a["C"],
                                           a["M"], a["k"], a["s"], a["sigma"], a["out"], a["ws"], a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(base, **kw)
        return L.pcnn_vertex_head_loss_bwd(a["z"], a["bias"], a["label"], a["inst"], a["obj"], a["out"], a["up"], a["B"], a["H"],
                                           a["W"], a["C"], a["M"], a["k"], a["s"], a["sigma"], a["dz"], a["dbias"], a["ws"],
                                           a["ws_bytes"], None)

    def refused(call, status, word, **kw):
        assert call(**kw) == status, kw
        msg = L.pcnn_last_error_string().decode()
        assert word in msg, (kw, msg)

    for call, outputs in ((fwd, ()), (bwd, ("dz", "dbias"))):
        for name, word in (("z", "z"), ("bias", "bias"), ("label", "label"), ("obj", "objects"), ("out", "out")) + tuple(
                (o, o) for o in outputs):
            refused(call, PCNN_ENULL, "NULL " + word, **{name: None})
        refused(call, PCNN_EINVAL, "num_classes", C=1)
        refused(call, PCNN_EINVAL, "num_classes", C=65)
        refused(call, PCNN_EINVAL, "num_objects", M=65)
        refused(call, PCNN_EINVAL, "num_objects", M=-1)
        refused(call, PCNN_EINVAL, "sigma", sigma=0.0)
        refused(call, PCNN_EINVAL, "sigma", sigma=-1.0)
        for k, s in ((3, 2), (2, 4), (6, 2), (4, 0), (66, 64)):               # odd difference, k < s, k > 2 s, s < 1, k > 64
            refused(call, PCNN_EINVAL, "kernel", k=k, s=s)
        refused(call, PCNN_EINVAL, "negative", B=-1)
        refused(call, PCNN_EINVAL, "65535", B=65536)
        refused(call, PCNN_EINVAL, "2^30", B=1 << 10, H=1 << 10, W=1 << 10, s=2, k=4)
        refused(call, PCNN_EINVAL, "workspace must be 16-byte aligned", ws=odd)
        refused(call, PCNN_EWORKSPACE, "workspace", ws=None)
        refused(call, PCNN_EWORKSPACE, "workspace", ws_bytes=need - 1)
    refused(bwd, PCNN_EINVAL, "dz must be 16-byte aligned", dz=odd)
    assert fwd(obj=None, M=0, ws=None) == PCNN_EWORKSPACE           # a NULL table is allowed with no rows: the next check speaks
    refused(lambda **kw: L.pcnn_vertex_head_loss_workspace_bytes(1, 1, 3, kw["C"], 4, 2, ctypes.byref(n)), PCNN_EINVAL,
            "num_classes", C=1)


# ---- the two statements against each other -----------------------------------------------------------------------------
@pytest.mark.parametrize("nk", R.case_ids(), ids=IDS)
def test_restatement_equals_the_unfused_composition_bit_for_bit(nk):
    c = R.case(*nk)
    r, q = R.reference(c), R.restate(c)
    assert R.same_bits(q["out"], r["out"]), (q["out"], r["out"])
    assert np.array_equal(q["dz"], r["dz"])                           # by value: the +-0 claim ...
    assert R.same_bits(q["dz"], r["dz"])                              # ... and in fact bit for bit: neither sum can be -0
    tol = 2.0 ** -24 * np.abs(r["dbias64"]) + 2.0 ** -30 * r["dbias_abs"]
    got = q["dbias"].astype(np.float64)
    assert np.isfinite(got).all() and (np.abs(got - r["dbias64"]) <= tol).all(), (got, r["dbias64"], tol)
    kind = nk[1]
    if kind == "empty":
        assert q["n_matched"] == 0 and not r["out"].any() and not r["dz"].any() and not q["dbias"].any()
        assert np.isfinite(r["out"]).all()
    else:
        assert q["n_matched"] > 0 and r["out"][0] > 0 and r["dz"].any()
    if kind == "full":
        assert q["n_matched"] == c["label"].size
    if kind.startswith("branches"):
        assert r["n_quadratic"] > 0 and r["n_linear"] > 0


def test_cases_hold_what_they_claim():
    for name in R.CASES:
        c = R.case(name, "mixed")
        lab, C = c["label"], c["C"]
        rows = c["objects"][0]
        assert (lab == -1).any() and (lab == C).any() and (lab == 0).any()
        assert rows[0, 0] == rows[1, 0] and rows[0, 1] == 0 and rows[1, 1] == R.INSTANCE_ID       # two rows of one class, one masked
        assert (c["instance"][lab == rows[0, 0]] == R.INSTANCE_ID).any() and (c["instance"][lab == rows[0, 0]] != R.INSTANCE_ID).any()
        assert not (lab == rows[2, 0]).any()                                                      # a row whose class never appears
        fg = set(np.unique(lab[(lab > 0) & (lab < C)]).tolist())
        assert fg - set(rows[:, 0].astype(int).tolist())                                          # a class with no row
        assert 10.0 in rows[:, 5]
        w = R.reference(c)["weights"]
        assert (w == 10).any() and (w == 1).any()
    B, H, W, k, s, C, M = R.CASES["C"]
    assert B * H * s * W * s * 3 * C == 2433024 > 8 * 262144 and (B * H * s * W * s * 3 * C) % 262144 != 0
    assert R.tile_shape(16, 8) == (4, 8) and R.tile_shape(4, 2) == (4, 8) and R.tile_shape(64, 64) == (1, 1)
    assert R.CASES["A"][1] % 4 and R.CASES["A"][2] % 8 and R.CASES["A"][1] > 4 and R.CASES["A"][2] > 8   # ragged second tiles


# ---- against float64 autograd ------------------------------------------------------------------------------------------
def _autograd(c, dtype):
    import torch
    r = R.reference(c)
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    z, b = t(c["z"]).requires_grad_(True), t(c["bias"]).requires_grad_(True)
    pred = grad_ref.deconv_bilinear64(z, c["k"], c["s"], bias=b)
    loss = grad_ref.smooth_l1_vertex64(pred, t(r["targets"]), t(r["weights"]), c["sigma"])
    dz, db = torch.autograd.grad(loss, [z, b])
    return float(loss.detach()), dz, db


@pytest.mark.parametrize("nk", [nk for nk in R.case_ids() if nk[1] != "empty"], ids=[i for i in IDS if "empty" not in i])
def test_reference_is_within_the_criterion_of_float64(nk):
    import torch
    c = R.case(*nk)
    r = R.reference(c)
    l64, dz64, db64 = _autograd(c, torch.float64)
    l32, dz32, db32 = _autograd(c, torch.float32)
    t = lambda a: torch.from_numpy(np.array(a))
    floor = {"loss": abs(l32 - l64) / abs(l64), "dz": grad_ref.rel_err(dz32, dz64), "dbias": grad_ref.rel_err(db32, db64)}
    err = {"loss": abs(float(r["out"][0]) - l64) / abs(l64), "dz": grad_ref.rel_err(t(r["dz"]), dz64),
           "dbias": grad_ref.rel_err(t(r["dbias64"]), db64)}
    print(nk, {k: "%.2e (floor %.2e, bound %.2e)" % (err[k], floor[k], grad_ref.bound(floor[k])) for k in err})
    for k in err:
        assert floor[k] <= grad_ref.FLOOR_CAP and err[k] <= grad_ref.bound(floor[k]), (k, err[k], floor[k])


# ---- seeded defects ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_seeded_defects_are_rejected(mutate):
    """Bias dropped, row priority reversed, and the taps of rows and columns swapped (case A: 6 x 11 cells, not square):
    each must change the loss or dz against the reference on case A, `mixed`."""
    c = R.case("A", "mixed")
    r, q = R.reference(c), R.restate(c, mutate=mutate)
    assert not R.same_bits(q["out"], r["out"]) and not np.array_equal(q["dz"], r["dz"])
