"""`icp.refine_batch` on the GPU: bit for bit the CPU restatement (tests/icp_batch_ref.py, computed once per process in
tests/icp_batch_cases.py), the per-frame `Synthesizer.icp_python` within the project's bound, row independence, capacity and
status rows, the memory contract, bad arguments, graph capture (the proof that nothing synchronises) and `fcn.refine_detections`."""
import ctypes

import numpy as np
import pytest

import icp_batch_cases as C
import icp_batch_ref as ref

import test_gpu_memory_contract as contract

pytestmark = pytest.mark.gpu
F = np.float32

# The memory-contract case of pcnn_icp_batch_fwd, in the case table that holds one for every launching entry of
# include/posecnn_hip.h (tests/test_memguard.py reads the table); test_memory_contract below runs it. The table is rebound
# to a longer list, not appended to: that module's own parametrisation keeps the list (and the ids) it was made with.
CONTRACT_CASE = contract.Case("icp_batch_100x131", ("pcnn_icp_batch_fwd",), C.contract_make, C.contract_run, C.contract_check)
if CONTRACT_CASE.name not in {c.name for c in contract.CASES}:
    contract.CASES = contract.CASES + [CONTRACT_CASE]


@pytest.fixture(scope="module")
def bank(gpu):
    return C.bank(gpu)


def bits(out):
    return [a.cpu().numpy().view(np.uint32) for a in (out.poses_new, out.poses_icp, out.info)]


def same_bits(got, want, what=""):
    for name, g, w in zip(("poses_new", "poses_icp", "info"), got, want):
        assert np.array_equal(g, np.ascontiguousarray(w).view(np.uint32)), "%s %s differs:\n%s\n%s" % (what, name, g, w)


@pytest.fixture(scope="module")
def small_out(gpu, bank):
    return bits(C.run(C.small(), gpu, bank))


@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_bit_for_bit_the_restatement(gpu, bank, name):
    got = bits(C.run(C.BATCHES[name](), gpu, bank))
    same_bits(got, C.reference(name)[:3], name)
    assert got[2].view(np.int32)[:, 0].tolist() == C.STATUS[name]


@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_against_icp_python_frame_by_frame(gpu, bank, name):
    """`last` diagnostics equal, rows within 1e-6 (rotation-matrix and translation entries); the number of entries that are
    not bit-equal is printed, not asserted."""
    from posecnn_amd import icp
    from posecnn_amd.pose_error import quat2mat
    b = C.BATCHES[name]()
    pn, pi, info = (a.view(t) for a, t in zip(bits(C.run(b, gpu, bank)), (F, F, np.int32)))
    syn = icp.Synthesizer(meshes=[icp.Mesh(m[0], m[2], m[1], device=gpu) for m in C.meshes()], device=gpu)
    n, rois, poses = b["count"], b["rois"], b["poses"]
    unequal = total = 0
    for fr in range(b["labels"].shape[0]):
        rows = [r for r in range(n) if rois[r, 0] == fr and rois[r, 1] <= len(C.meshes())]       # (icp_python raises past the bank)
        H, W = b["labels"].shape[1:]
        syn.setup(W, H)
        new, best = np.zeros((len(rows), 7), F), np.zeros((len(rows), 7), F)
        k = b["intrinsics"][fr]
        syn.icp_python(b["labels"][fr], b["depth"][fr], np.array([k[0], k[1], k[2], k[3], 0.25, 6.0, b["factor"]], F), H, W, len(rows), 7,
                       rois[rows], poses[rows], new, best, 0.01, min_pixels=b["min_pixels"])
        refined = [r for r in rows if info[r, 0] == ref.REFINED]
        assert [rows[d["roi"]] for d in syn.last] == refined
        for d in syn.last:
            r = rows[d["roi"]]
            assert (d["agree"], d["pairs"], d["choose"]) == tuple(info[r, 1:4]), r
            assert info[r, 4:].tolist() == ([-1] * 8 if d["hits"] is None else d["hits"].tolist()), r
            for got, want in ((pn[r], new[d["roi"]]), (pi[r], best[d["roi"]])):
                assert np.abs(quat2mat(got[:4].astype(np.float64)) - quat2mat(want[:4].astype(np.float64))).max() < 1e-6, r
                assert np.abs(got[4:] - want[4:]).max() < 1e-6, r
                unequal += int((got.view(np.uint32) != want.view(np.uint32)).sum())
                total += 7
    print("%s: %d of %d output entries differ in bits from icp_python" % (name, unequal, total))


def test_rows_are_independent(gpu, bank, small_out):
    b = C.small()
    n = b["count"]
    # a permutation of the live rows permutes the outputs (capacity = all rows, so the slot order does not matter)
    perm = np.concatenate([np.random.default_rng(3).permutation(n), np.arange(n, len(b["rois"]))])
    p = dict(b, rois=b["rois"][perm], poses=b["poses"][perm])
    same_bits(bits(C.run(p, gpu, bank)), [a[perm] for a in small_out], "permuted")
    # other garbage in the dead rows changes nothing, and they stay zero
    g = dict(b, rois=b["rois"].copy(), poses=b["poses"].copy())
    g["rois"][n:] = [[0, 1, -np.inf, 5, 1e30, 2, 3], [1, 2, 0, 0, 0, 0, 0]]
    g["poses"][n:] = [b["poses"][0], [np.inf, 0, 0, 1, -1e30, 0, 0.5]]
    got = bits(C.run(g, gpu, bank))
    same_bits(got, small_out, "garbage")
    assert not any(a[n:].any() for a in got)
    # a frame refined alone (B = 1) gives the bits it gives inside the batch
    for fr in range(2):
        rows = [r for r in range(n) if b["rois"][r, 0] == fr]
        one = dict(b, labels=b["labels"][fr:fr + 1], depth=b["depth"][fr:fr + 1], intrinsics=b["intrinsics"][fr:fr + 1],
                   rois=b["rois"][rows].copy(), poses=b["poses"][rows], count=len(rows))
        one["rois"][:, 0] = 0
        same_bits(bits(C.run(one, gpu, bank)), [a[rows] for a in small_out], "frame %d alone" % fr)
    # count = None: every row is live (here: all of them refinable or not on their own merits)
    live = dict(b, rois=b["rois"][:n], poses=b["poses"][:n])
    from posecnn_amd import icp
    args = C.device_args(live, gpu)
    out = icp.refine_batch(*args[:6], None, bank, min_pixels=b["min_pixels"], **C.OPTIONS)
    same_bits(bits(out), [a[:n] for a in small_out], "count None")


def test_capacity_and_status_rows(gpu, bank, small_out):
    b = C.small()
    same_bits(bits(C.run(b, gpu, bank, max_jobs=1)), C.reference("small", max_jobs=1)[:3], "max_jobs = 1")
    got = bits(C.run(b, gpu, bank, max_jobs=0))
    assert got[2].view(np.int32)[:, 0].tolist() == [5, 5, 5, 5, 2, 3, 4, 5, 5, 5, 0, 0] and not got[0].any() and not got[1].any()
    # more slots than rows: the same bits
    same_bits(bits(C.run(b, gpu, bank, max_jobs=20)), small_out, "max_jobs = 20")
    assert small_out[2].view(np.int32)[C.KINDS["beyond the bank"][1], 0] == ref.NO_MODEL
    # more rows than the largest capacity, max_jobs left to its default (clamped to icp.MAX_JOBS): 8 x 8 frames keep it small
    import torch
    from posecnn_amd import icp
    R = icp.MAX_JOBS + 9
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=gpu)
    out = icp.refine_batch(z(1, 8, 8, dt=torch.int32), z(1, 8, 8, dt=torch.int16).view(torch.uint16), torch.ones((1, 4), device=gpu), 1000.0,
                           z(R, 7), z(R, 7), None, bank)
    assert bool((out.info[:, 0] == ref.BACKGROUND).all()) and not bool(out.poses_new.any()) and not bool(out.info[:, 1:].any())


def test_memory_contract(gpu):
    """The case under both poison patterns: guard bands around the outputs, the workspace (exactly
    pcnn_icp_batch_workspace_bytes) and the inputs (the mesh bank, with a class id beyond it among the rows) stay intact, the
    two runs agree bit for bit, the entry is reached, and the outputs are the restatement's."""
    contract.execute(CONTRACT_CASE)


def test_short_workspace_is_refused_without_a_launch(gpu, bank):
    import torch
    from posecnn_amd import _lib, ops
    b = C.small()
    labels, depth, intr, factor, rois, poses, count = C.device_args(b, gpu)
    R, (B, H, W) = rois.shape[0], labels.shape
    need = ctypes.c_size_t()
    L = _lib.lib()
    assert L.pcnn_icp_batch_workspace_bytes(R, H, W, ctypes.byref(need)) == 0
    P, nb, nw = H * W, -(-H * W // 256), -(-H * W // 32)
    up = lambda x: -(-x // 256) * 256
    parts = [64 * R * P, 16 * R * P, 16 * R * P, 12 * R * P, 12 * R * P, R * P, 128 * R * P, 128 * R * P, 4 * 8 * R * nb * 29, 4 * 8 * R * nw,
             96 * R, 128 * R, 768 * R, 768 * R, 384 * R, 32 * R, 32 * R, 16 * R]
    assert need.value == sum(up(x) for x in parts)                                          # the documented function of (max_jobs, H, W)
    ws = torch.zeros(need.value, dtype=torch.uint8, device=gpu)
    outs = [torch.full((R, 7), 7.0, device=gpu), torch.full((R, 7), 7.0, device=gpu), torch.full((R, 12), 7, dtype=torch.int32, device=gpu)]
    p = ops._ptr
    st = L.pcnn_icp_batch_fwd(p(labels), p(depth), p(intr), B, H, W, factor, p(rois), 7, p(poses), p(count), R, p(bank.vertices),
                              p(bank.normals), p(bank.faces), p(bank.vertex_offsets), p(bank.face_offsets), bank.num_classes,
                              bank.max_faces, R, 0.01, 8, 50, b["min_pixels"], 0.01, 0.25, 6.0, p(outs[0]), p(outs[1]), p(outs[2]), p(ws),
                              need.value - 1, ops._stream(labels))
    torch.cuda.synchronize()
    assert st == _lib.PCNN_EWORKSPACE
    assert all(bool((o == 7).all()) for o in outs) and not bool(ws.any())                  # nothing was launched


def test_bad_arguments_raise_before_any_launch(gpu, bank):
    import torch
    from posecnn_amd import icp
    b = C.small()
    good = list(C.device_args(b, gpu))
    ok = dict(C.OPTIONS, min_pixels=b["min_pixels"])

    def bad(i, value, **kw):
        args = list(good)
        if i is not None:
            args[i] = value
        with pytest.raises(ValueError):
            icp.refine_batch(*args, bank, **dict(ok, **kw))

    bad(0, good[0][0])                                      # labels [H,W]
    bad(0, good[0].to(torch.int64))
    bad(1, good[1][:, :50])                                 # depth of another size
    bad(1, good[1].view(torch.int16))
    bad(2, good[2][:, :3])                                  # intrinsics [B,3]
    bad(2, good[2][:1])
    bad(4, good[4][:, :1])                                  # rois with one column
    bad(4, good[4].double())
    bad(5, good[5][:, :6])                                  # poses [R,6]
    bad(5, good[5][:-1])
    bad(6, good[6].to(torch.int64))
    bad(6, good[6].cpu())
    bad(0, good[0].cpu())
    bad(None, None, iterations=-1)
    for n in (1, 7, -1):
        bad(None, None, polish_evaluations=n)
    bad(None, None, max_jobs=-1)
    bad(None, None, max_jobs=icp.MAX_JOBS + 1)
    bad(3, 0.0)                                             # factor_depth
    with pytest.raises(ValueError):
        icp.refine_batch(*good, object(), **ok)
    torch.cuda.synchronize()


def test_graph_capture_and_replay(gpu, bank, small_out):
    """A host synchronisation inside the call would make the capture fail: one stream, no parallel branches."""
    import torch
    from posecnn_amd import icp
    b = C.small()
    n = b["count"]
    swapped = dict(b, rois=b["rois"].copy(), poses=b["poses"].copy())
    swapped["rois"][[0, 1]] = b["rois"][[1, 0]]
    swapped["poses"][[0, 1]] = b["poses"][[1, 0]]
    want_swapped = bits(C.run(swapped, gpu, bank))
    opts = dict(C.OPTIONS, min_pixels=b["min_pixels"])
    static = list(C.device_args(b, gpu))
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        icp.refine_batch(*static, bank, **opts)                                            # warm-up on the capture stream
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = icp.refine_batch(*static, bank, **opts)
    for inputs, want in ((swapped, want_swapped), (b, small_out)):
        fresh = C.device_args(inputs, gpu)
        for dst, src in zip(static, fresh):
            if isinstance(dst, torch.Tensor):
                dst.copy_(src)
        for t in out:
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        same_bits(bits(out), want, "replay")
    assert n == 10


def test_refine_detections_equals_refine_batch(gpu, bank, small_out):
    import torch
    from posecnn_amd import fcn, icp
    b = C.small()
    labels, depth, intr, factor, rois, poses, count = C.device_args(b, gpu)
    det = fcn.Detections(torch.cat([rois, poses], dim=1), count, labels)
    syn = icp.Synthesizer(meshes=[icp.Mesh(m[0], m[2], m[1], device=gpu) for m in C.meshes()], device=gpu)
    out = fcn.refine_detections(det, depth, intr, factor, syn, min_pixels=b["min_pixels"])
    same_bits(bits(out), small_out, "refine_detections")
    assert isinstance(out, icp.RefinedBatch) and syn._icp_bank.num_classes == 3
    with pytest.raises(ValueError):
        fcn.refine_detections(fcn.Detections(det.rows, count), depth, intr, factor, syn)
