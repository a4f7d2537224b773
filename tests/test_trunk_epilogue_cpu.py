"""tests/trunk_epilogue_ref.py — the numpy restatement the GPU kernels of csrc/trunk_epilogue.hip are pinned to — against
autograd of the framework composition on the CPU: max_pool2d(relu(x + b), 2) and relu(x + b).

  dy      exact on tie-free inputs (float64 autograd; every biased value of trunk_epilogue_ref.tie_free is exact in f32);
          within 1 ulp in the dual form, whose one extra f32 add float64 does not round
  dbias   |dbias - S64| <= 2^-24 |S64| + 2^-30 sum |dy|: a float64 accumulation in any order, then one rounding to f32 (the
          bound of the label head's dbias, tests/test_gpu_label_loss.py)
  pooled, act   the bits of the existing forward kernels as csrc/upscore.hip states them

On inputs WITH ties the routing is a convention — the first maximum of the biased f32 values, a gate of > 0 — which the
framework's float32 composition shares; three seeded departures from it must be rejected there.
"""
import numpy as np
import pytest
import torch

import trunk_epilogue_ref as R

F = np.float32
SHAPES = ((1, 2, 2, 4), (1, 2, 2, 3), (2, 4, 6, 5), (2, 6, 4, 64), (1, 2, 258, 4), (1, 130, 512, 2))


def composition(y, bias, relu, dpooled, dact=None, dtype=torch.float64):
    """autograd of the framework composition -> (pooled, act, dy, dbias) as numpy arrays of `dtype`"""
    x = torch.from_numpy(y).to(dtype).requires_grad_(True)
    b = torch.from_numpy(bias).to(dtype).requires_grad_(True)
    a = x + b
    a = torch.relu(a) if relu else a
    p = torch.nn.functional.max_pool2d(a.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    loss = (p * torch.from_numpy(dpooled).to(dtype)).sum()
    if dact is not None:
        loss = loss + (a * torch.from_numpy(dact).to(dtype)).sum()
    loss.backward()
    return p.detach().numpy(), a.detach().numpy(), x.grad.numpy(), b.grad.numpy()


def check_dbias(dbias, dy):
    s, tol = R.dbias_bound(dy)
    assert np.isfinite(dbias).all() and (np.abs(dbias.astype(np.float64) - s) <= tol).all(), (dbias, s, tol)


@pytest.mark.parametrize("relu", (1, 0))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_pooled_form_equals_float64_autograd_on_tie_free_inputs(shape, relu):
    y, bias = R.tie_free(shape, 11)
    dpooled, dact = R.grads(shape, 11)
    pooled, sel, act = R.pool_forward(y, bias, relu)
    p64, a64, dy64, db64 = composition(y, bias, relu, dpooled)
    assert np.array_equal(pooled, p64.astype(F)) and np.array_equal(pooled.astype(np.float64), p64)
    assert np.array_equal(act.astype(np.float64), a64)
    assert sel.dtype == np.uint8 and sel.max() <= (4 if relu else 3)
    if relu:
        assert ((sel == 4) == (pooled == 0)).all()
    dy, dbias = R.pool_backward(dpooled, sel)
    assert np.array_equal(dy.astype(np.float64), dy64)
    check_dbias(dbias, dy)
    assert np.abs(dbias - db64).max() <= np.abs(R.dbias_bound(dy)[1]).max()
    if relu:   # the dual form: one f32 add more than float64 rounds
        _, _, dy64, _ = composition(y, bias, relu, dpooled, dact)
        dy, dbias = R.pool_backward(dpooled, sel, dact, act)
        assert (np.abs(dy.astype(np.float64) - dy64) <= np.spacing(np.abs(dy64).astype(F))).all()
        check_dbias(dbias, dy)


@pytest.mark.parametrize("relu", (1, 0))
@pytest.mark.parametrize("rows", (1, 127, 128, 129, 32769))
def test_unpooled_form_equals_float64_autograd(rows, relu):
    rng = np.random.default_rng(rows)
    y = (rng.integers(-8, 9, (rows, 6)) / 4.0).astype(F)
    bias = ((2 * rng.integers(-3, 4, 6) + 1) / 16.0).astype(F)
    da = rng.standard_normal((rows, 6)).astype(F)
    a = R.bias_act(y, bias, relu)
    x = torch.from_numpy(y).double().requires_grad_(True)
    b = torch.from_numpy(bias).double().requires_grad_(True)
    out = torch.relu(x + b) if relu else x + b
    (out * torch.from_numpy(da).double()).sum().backward()
    assert np.array_equal(a.astype(np.float64), out.detach().numpy())
    dy, dbias = R.backward(da, a, relu)
    assert np.array_equal(dy.astype(np.float64), x.grad.numpy())
    check_dbias(dbias, dy)
    assert (np.abs(dbias - b.grad.numpy()) <= R.dbias_bound(dy)[1]).all()


@pytest.mark.parametrize("relu", (1, 0))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_has_the_bits_of_the_existing_kernels(shape, relu):
    y, bias = R.edge_input(shape, 5)
    pooled, sel, act = R.pool_forward(y, bias, relu)
    assert np.array_equal(pooled.view(np.uint32), R.existing_pool(y, bias, relu).view(np.uint32))
    assert np.array_equal(act.view(np.uint32), R.bias_act(y, bias, relu).view(np.uint32))
    # and of the framework's float32 composition, ties included
    p32, a32, _, _ = composition(y, bias, relu, R.grads(shape, 5)[0], dtype=torch.float32)
    assert np.array_equal(pooled, p32) and np.array_equal(act, a32)


def test_the_dbias_order_is_the_headers():
    """A single value comes through wherever it sits (no pixel, run or finishing thread is dropped or counted twice), and two
    cancellations come out as the stated order has them, not as an ascending or a pairwise sum would."""
    v = np.zeros((300 * 128, 1, 1), F)
    for p in (0, 15, 16, 127, 128, 255 * 128 + 5, 256 * 128, 300 * 128 - 1):
        w = v.copy()
        w[p] = 3.0
        assert R.dbias_sum(w)[0] == 3.0
    w = v[:128].copy()
    w[0], w[16], w[1], w[2] = 2.0 ** 60, 1.0, -2.0 ** 60, 1.0
    # slot 0 = 2^60 + 1 = 2^60 (pixels 0 and 16); tree: slot 0 + slot 2 = 2^60 + 1 = 2^60, then + slot 1 = 0. Exactly: 2.
    assert R.dbias_sum(w)[0] == 0.0
    w = v[:128].copy()
    w[0], w[1], w[8] = 2.0 ** 60, 1.0, -2.0 ** 60
    # slots 0 and 8 meet in the tree's first level and cancel; the 1 of slot 1 survives. Ascending: (2^60 + 1) - 2^60 = 0.
    assert R.dbias_sum(w)[0] == 1.0
    w = np.zeros((257 * 128, 1, 1), F)
    w[0], w[128], w[256 * 128] = 2.0 ** 60, 1.0, -2.0 ** 60
    # finishing pass: thread 0 takes runs 0 and 256 in that order and cancels them; run 1 (thread 1) survives
    assert R.dbias_sum(w)[0] == 1.0


# ---- the three seeded defects ------------------------------------------------------------------------------------------------
def _rejected(y, bias, dpooled, dact, defect):
    """Does the float32 framework composition reject the restatement with `defect`? (dy only: bit for bit)"""
    pooled, sel, act = R.pool_forward(y, bias, 1, defect)
    dy = R.pool_backward(dpooled, sel, dact, act if dact is not None else None, defect)[0]
    want = composition(y, bias, 1, dpooled, dact, dtype=torch.float32)[2]
    return not np.array_equal(dy, want)


def _defect_cases():
    shape = (2, 6, 4, 8)
    y, bias = R.edge_input(shape, 3)
    dpooled, dact = R.grads(shape, 3)
    dpooled = np.where(dpooled == 0, F(1), dpooled)
    return y, bias, dpooled, dact


def test_the_restatement_itself_is_accepted_with_ties():
    y, bias, dpooled, dact = _defect_cases()
    assert not _rejected(y, bias, dpooled, None, None)
    assert not _rejected(y, bias, dpooled, dact, None)
    pooled, sel, act = R.pool_forward(y, bias, 1)
    assert sel[0, 0, 0, 0] == 0 and pooled[0, 0, 0, 0] == 1025.0          # the bias-induced tie: position 0
    assert sel[0, -1, -1, 0] == 4 and pooled[0, -1, -1, 0] == 0.0         # best == 0: closed
    assert (sel == 4).sum() > 10 and all((sel == k).any() for k in range(4))


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_are_rejected(defect):
    y, bias, dpooled, dact = _defect_cases()
    assert _rejected(y, bias, dpooled, dact if defect == "relu_ge" else None, defect), defect


def test_raw_argmax_is_rejected_by_the_bias_induced_tie_alone():
    y = np.array([1.0, 1.0 + 2.0 ** -23, 0.5, -1.0], F).reshape(1, 2, 2, 1)
    bias = np.array([1024.0], F)
    dpooled = np.ones((1, 1, 1, 1), F)
    assert (y[0, 0, 1, 0] > y[0, 0, 0, 0]) and F(y[0, 0, 1, 0] + bias[0]) == F(y[0, 0, 0, 0] + bias[0])
    assert not _rejected(y, bias, dpooled, None, None) and R.pool_forward(y, bias, 1)[1].item() == 0
    assert _rejected(y, bias, dpooled, None, "raw_argmax") and R.pool_forward(y, bias, 1, "raw_argmax")[1].item() == 1


def test_relu_ge_is_rejected_by_the_unpooled_backward():
    a = np.array([[0.0, 1.0, 0.0, 2.0]], F)
    da = np.ones((1, 4), F)
    assert np.array_equal(R.backward(da, a, 1)[0], [[0, 1, 0, 1]])
    assert not np.array_equal(R.backward(da, a, 1, "relu_ge")[0], R.backward(da, a, 1)[0])
    x = torch.zeros(1, 4, requires_grad=True)
    torch.relu(x).sum().backward()
    assert not x.grad.any()                                                 # the framework's gate at 0 is closed too
