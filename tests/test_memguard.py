"""CPU checks of the memory-contract harness (tests/memguard.py): it catches each kind of breach on fake ops built on the
proxy with CPU tensors, passes a clean one, and the case table of tests/test_gpu_memory_contract.py reaches every entry
of include/posecnn_hip.h that launches work."""
import ctypes
import os
import re

import numpy as np
import pytest

import memguard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _raw(ptr, n, ctype=ctypes.c_float):
    """n elements at a raw address: what a kernel sees of a pointer argument."""
    return np.ctypeslib.as_array((ctype * n).from_address(ptr))


def clean_op(g, x):
    """y[i] = 2 x[i] + 1 with a workspace of exactly what it asks for."""
    import torch
    ws = g.empty(4 * x.numel(), dtype=torch.uint8)
    _raw(ws.data_ptr(), x.numel())[:] = x.numpy() * 2
    y = g.empty_like(x)
    _raw(y.data_ptr(), x.numel())[:] = _raw(ws.data_ptr(), x.numel()) + 1
    return {"y": y}


def store_past_end(g, x):
    y = clean_op(g, x)["y"]
    _raw(y.data_ptr(), x.numel() + 1)[x.numel()] = 0.0
    return {"y": y}


def store_before_start(g, x):
    y = clean_op(g, x)["y"]
    _raw(y.data_ptr() - 4, 1)[0] = 0.0
    return {"y": y}


def reads_uninitialised(g, x):
    import torch
    y = g.empty_like(x)
    acc = g.zeros(1, dtype=torch.float32)
    _raw(y.data_ptr(), x.numel() - 1)[:] = x.numpy()[:-1]      # the last element is never written
    _raw(acc.data_ptr(), 1)[0] = _raw(y.data_ptr(), x.numel()).sum()
    return {"y_head": y[:-1].clone(), "sum": acc}


def writes_input(g, x):
    out = clean_op(g, x)
    _raw(x.data_ptr(), 1)[0] += 1.0
    return out


def workspace_overrun(g, x):
    import torch
    ws = g.empty(64, dtype=torch.uint8)
    _raw(ws.data_ptr(), 68, ctypes.c_uint8)[:] = 7
    return clean_op(g, x)


def run_fake(op):
    x_np = np.arange(-7, 30, dtype=F) * F(0.25)
    runs = {}
    for p in memguard.PATTERNS:
        g = memguard.GuardedTorch(p, devices=("cpu",))
        x = g.embed(x_np, "cpu")
        out = op(g, x)
        g.check()
        runs[p] = {k: memguard.to_numpy(v) for k, v in out.items()}
    memguard.compare_patterns(runs)
    return runs["P1"], x_np


def test_clean_fake_op_passes():
    out, x = run_fake(clean_op)
    assert np.array_equal(out["y"], x * 2 + 1)


@pytest.mark.parametrize("op,match", [(store_past_end, "AFTER the body hit, first store at byte 0 past its end"),
                                      (store_before_start, "BEFORE the body hit, farthest store 4 bytes before its start"),
                                      (reads_uninitialised, "depends on the memory's previous contents"),
                                      (writes_input, "input .* modified, first changed byte at body offset \\d+"),
                                      (workspace_overrun, "empty \\(64,\\) uint8 from test_memguard.py:\\d+ \\(workspace_overrun\\): guard AFTER")])
def test_breaches_are_caught(op, match):
    with pytest.raises(memguard.GuardError, match=match):
        run_fake(op)


def test_layout_alignment_and_poison():
    import torch
    for p, off in (("P1", 0), ("P2", 16)):
        g = memguard.GuardedTorch(p, devices=("cpu",))
        for dt in (torch.float32, torch.float64, torch.int32, torch.uint8):
            t = g.empty((3, 5), dtype=dt)
            assert t.data_ptr() % 256 == off and t.is_contiguous() and t.shape == (3, 5)
            raw = memguard.to_numpy(t).reshape(-1).view(np.uint8).reshape(15, -1)
            assert (raw == memguard.poison_bytes(p, memguard.to_numpy(t).dtype)).all()
        assert memguard.to_numpy(g.zeros(7, dtype=torch.int32)).tolist() == [0] * 7
        assert g.empty(0, 7, dtype=torch.float32).shape == (0, 7)
        g.check()
    assert np.isnan(memguard.to_numpy(memguard.GuardedTorch("P1", ("cpu",)).empty(2))).all()
    assert (memguard.to_numpy(memguard.GuardedTorch("P2", ("cpu",)).empty(2)) == np.finfo(F).max).all()
    # allocations on other devices pass through unguarded
    g = memguard.GuardedTorch("P1", devices=("cuda",))
    g.empty(4)
    assert not g.arenas


def test_untouched_and_zero_regions():
    runs = {p: {"out": np.concatenate([np.ones(3, F), np.frombuffer(memguard.poison_bytes(p, F).tobytes() * 2, F)])}
            for p in memguard.PATTERNS}
    memguard.compare_patterns(runs, keep={"out": np.s_[3:]})
    with pytest.raises(memguard.GuardError, match="depends on the memory"):
        memguard.compare_patterns(runs)
    runs = {p: {"out": np.array([1, 2, 0, 0], F)} for p in memguard.PATTERNS}
    memguard.compare_patterns(runs, zero={"out": np.s_[2:]})
    with pytest.raises(memguard.GuardError, match="zero region"):
        memguard.compare_patterns(runs, zero={"out": np.s_[1:]})


# ---- coverage of the C-ABI --------------------------------------------------------------------------------------------
HOST_ONLY = {"pcnn_abi_version", "pcnn_status_string", "pcnn_last_error_string", "pcnn_crc32c", "pcnn_hough_voting_debug_layout"}


def launching_exports():
    with open(os.path.join(ROOT, "include", "posecnn_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    names = set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][A-Za-z_0-9]*\s*\**\s+\**(pcnn_[A-Za-z_0-9]+)\s*\(", text, flags=re.M))
    assert len(names) > 40, names
    return {n for n in names if not n.endswith("_workspace_bytes") and not n.startswith("pcnn_profile_") and n not in HOST_ONLY}


def test_every_launching_export_has_a_memory_contract_case():
    import test_gpu_memory_contract as contract
    covered = set()
    for case in contract.CASES:
        covered |= set(case.covers)
    exports = launching_exports()
    assert "pcnn_fc_skinny_fwd" in exports and "pcnn_icp_polish_fwd" in exports
    assert not exports - covered, "exports without a memory-contract case: %s" % sorted(exports - covered)
    assert not covered - exports, "cases cover names the header does not export: %s" % sorted(covered - exports)
