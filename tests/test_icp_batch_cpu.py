"""The batched pose refinement on the CPU: the restatement `icp.refine_batch` is held to (tests/icp_batch_ref.py) against the
per-object flow on the checker (tests/icp_scene.solve_icp_reference), the status of every row kind, the regime each case of
tests/icp_batch_cases.py claims, the explicit-order compose against numpy's, the capacity rule, and the new names."""
import os

import numpy as np
import pytest

import icp_batch_cases as C
import icp_batch_ref as ref
import icp_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_status_of_every_row(name):
    info = C.reference(name)[2]
    assert info[:, 0].tolist() == C.STATUS[name]
    pn, pi = C.reference(name)[:2]
    for r, st in enumerate(info[:, 0]):
        if st != ref.REFINED:
            assert not pn[r].any() and not pi[r].any() and not info[r, 1:].any(), r
        else:
            assert np.isfinite(pn[r]).all() and np.isfinite(pi[r]).all(), r


def test_each_case_is_in_the_regime_it_claims():
    b, (pn, pi, info, _) = C.small(), C.reference("small")
    assert b["labels"].shape == (2, 100, 131) and (100 * 131) % 256 != 0 and not np.array_equal(b["intrinsics"][0], b["intrinsics"][1])
    row = lambda kind: C.KINDS[kind][1]
    cls = lambda r: int(b["rois"][r, 1])
    frm = lambda r: int(b["rois"][r, 0])
    # two live objects of different classes in one frame; one class live in both frames; a duplicate of frame and class
    assert frm(row("live")) == frm(row("other class, same frame")) and cls(row("live")) != cls(row("other class, same frame"))
    assert cls(row("live")) == cls(row("same class, other frame")) and frm(row("live")) != frm(row("same class, other frame"))
    assert (frm(row("duplicate")), cls(row("duplicate"))) == (frm(row("live")), cls(row("live")))
    assert not np.array_equal(b["poses"][row("duplicate")], b["poses"][row("live")])
    for kind in ("live", "other class, same frame", "same class, other frame", "duplicate"):
        assert info[row(kind), 1] > 0 and info[row(kind), 2] > 0, kind                     # agree, pairs
    r = row("under min_pixels")
    assert 0 < (b["labels"][frm(r)] == cls(r)).sum() < b["min_pixels"]
    assert cls(row("beyond the bank")) > len(C.meshes()) and cls(row("background")) == 0
    r = row("agree == 0")
    assert info[r, 1] == 0 and info[r, 2] > 0 and (info[r, 4:] >= 0).all()
    r = row("pairs == 0")
    assert info[r, 2] == 0 and info[r, 3] == 0 and (info[r, 4:] == -1).all()
    r = row("t_z == 0")
    assert b["poses"][r, 6] == 0 and info[r, 0] == ref.REFINED
    dead = b["rois"][b["count"]:]
    assert len(dead) == 2 and np.isnan(dead[:, 2:]).all() and (dead[:, 1] > 2 ** 31).all() and np.isnan(b["poses"][b["count"]:]).all()
    big = C.large()
    assert big["labels"].shape == (1, 240, 320) and big["min_pixels"] == 400
    assert 0 < (big["labels"][0] == 3).sum() < 400 <= min((big["labels"][0] == 1).sum(), (big["labels"][0] == 2).sum())


@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_restatement_equals_the_per_object_flow(name):
    """Discrete diagnostics equal; rotation-matrix and translation entries within 1e-6 (tests/test_gpu_icp_render.py's bound)."""
    b, (pn, pi, info, _) = C.BATCHES[name](), C.reference(name)
    refined = [r for r in range(len(info)) if info[r, 0] == ref.REFINED]
    assert refined
    for r in refined:
        fr, cls = int(b["rois"][r, 0]), int(b["rois"][r, 1])
        q_t = b["poses"][r].astype(np.float64)
        T_in = S.pose(S.quat2mat(q_t[:4]), q_t[4:])
        k = b["intrinsics"][fr].astype(np.float64)
        K = np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]])
        want = S.solve_icp_reference(b["labels"][fr], b["depth"][fr], K, b["factor"], cls, T_in, C.meshes()[cls - 1], q_t=q_t)
        assert (info[r, 1], info[r, 2], info[r, 3]) == (want["agree"], want["pairs"], want["choose"]), r
        assert info[r, 4:].tolist() == ([-1] * 8 if want["hits"] is None else want["hits"].tolist()), r
        for got, T in ((pn[r], want["T_new"]), (pi[r], want["T_icp"])):
            assert np.abs(S.quat2mat(got[:4].astype(np.float64)) - T[:, :3]).max() < 1e-6 and np.abs(got[4:] - T[:, 3]).max() < 1e-6, r


def test_explicit_order_compose_against_numpy():
    """Each entry is a 3-term dot product (plus one addend): both evaluation orders lie within gamma_3 of the exact value,
    so |difference| <= 8 * 2^-53 * sum |products| (2 gamma_3 ~ 6 * 2^-53, a third of margin)."""
    rng = np.random.default_rng(5)
    pairs = [(S.pose(S.rot(rng.standard_normal(3), rng.uniform(-3, 3)), rng.uniform(-1, 1, 3)),
              S.pose(S.rot(rng.standard_normal(3), rng.uniform(-3, 3)), rng.uniform(-1, 1, 3))) for _ in range(200)]
    extras = C.reference("small")[3]
    pairs += [(S.pose(S.rot([0, 0, 1], 1e-3), [1e-3, 0, 0]), e["T_new"]) for e in extras.values()]
    for U, T in pairs:
        got = np.array(ref.compose(list(U.reshape(12)), list(T.reshape(12)))).reshape(3, 4)
        want = S.compose(U, T)
        u = 2.0 ** -53
        prod = np.abs(U[:, :3]) @ np.abs(T)                      # sum |products| of every entry's 3-term dot product
        assert (np.abs(got[:, :3] - want[:, :3]) <= 8 * u * prod[:, :3]).all()
        # the translation adds U's own: 4 terms, 2 gamma_4 = 8 u, held with a quarter of margin
        assert (np.abs(got[:, 3] - want[:, 3]) <= 10 * u * (prod[:, 3] + np.abs(U[:, 3]))).all()


def test_capacity_takes_the_first_refinable_rows():
    full, capped = C.reference("small"), C.reference("small", max_jobs=1)
    assert capped[2][:, 0].tolist() == [1, 5, 5, 5, 2, 3, 4, 5, 5, 5, 0, 0]
    for a, b in zip(full[:3], capped[:3]):
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))          # the first refinable row: the same bits
    assert not capped[0][1:].any() and not capped[1][1:].any() and not capped[2][1:, 1:].any()


def test_new_names_are_exported():
    from posecnn_amd import fcn, icp, ops
    assert "icp_refine_batch" in ops.__all__ and callable(ops.icp_refine_batch)
    assert "refine_detections" in fcn.__all__ and callable(fcn.refine_detections)
    for name in ("MeshBank", "RefinedBatch", "refine_batch"):
        assert callable(getattr(icp, name)), name
    assert callable(icp.Synthesizer.icp_batch)
    assert (icp.STATUS_DEAD, icp.STATUS_REFINED, icp.STATUS_BACKGROUND, icp.STATUS_FEW_PIXELS, icp.STATUS_NO_MODEL,
            icp.STATUS_CAPACITY) == (ref.DEAD, ref.REFINED, ref.BACKGROUND, ref.FEW_PIXELS, ref.NO_MODEL, ref.CAPACITY)
    assert icp.INFO_COLUMNS == ref.INFO_COLUMNS and icp.HYPOTHESIS_DZ == ref.HYPOTHESIS_DZ


def test_prototypes_are_in_the_main_header():
    from ctypes import POINTER, c_float, c_int, c_size_t, c_void_p
    from posecnn_amd import _lib
    text = open(os.path.join(ROOT, "include", "posecnn_hip.h")).read()
    table = _lib.parse_header("posecnn_hip.h", text)
    assert table["pcnn_icp_batch_workspace_bytes"] == (c_int, [c_int, c_int, c_int, POINTER(c_size_t)])
    res, args = table["pcnn_icp_batch_fwd"]
    P = c_void_p
    assert res is c_int and args == ([P, P, P, c_int, c_int, c_int, c_float, P, c_int, P, P, c_int, P, P, P, P, P, c_int, c_int, c_int,
                                      c_float, c_int, c_int, c_int, c_float, c_float, c_float, P, P, P, P, c_size_t, P])
    assert _lib.header_abi_version() == 2
