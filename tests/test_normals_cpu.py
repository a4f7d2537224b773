"""CPU checks of the input front end (include/posecnn_hip_frontend.h): the numpy restatement (tests/normals_ref.py)
against recorded outputs of the reference's own normal-map kernels (tests/golden/normals.npz, written by
tests/golden/make_normals_golden.py), the bilateral filter's weight tables, and the host-side
argument checks of its entries (nothing is launched)."""
import ctypes
import os

import numpy as np
import pytest

import normals_ref

F = np.float32


# ---- the reference pin ---------------------------------------------------------------------------------------------
def test_golden_covers_the_cases_it_is_there_for():
    cases = normals_ref.golden_cases()
    assert [c["depth"].shape for c in cases] == [(12, 20), (19, 37)]
    for c in cases:
        d, n = c["depth"], c["nmap"]
        assert d.dtype == F and n.dtype == F and n.shape == d.shape + (3,)
        assert (d == 0).any() and (d >= c["cutoff"]).any() and np.isnan(d).any()
        nan = np.isnan(n)
        assert (nan.all(-1) == nan.any(-1)).all()                              # a pixel is NaN in all three or in none
        assert nan[-1].all() and nan[:, -1].all() and nan[:-1, :-1].any() and not nan[:-1, :-1].all()
        assert (n.view(np.uint32)[nan] == 0x7fffffff).all()
        norm = np.sqrt((n[~nan.any(-1)].astype(np.float64) ** 2).sum(-1))
        assert np.abs(norm - 1).max() < 1e-6


@pytest.mark.parametrize("case", normals_ref.golden_cases(), ids=lambda c: c["name"])
def test_restatement_equals_the_reference_bit_for_bit(case):
    n = normals_ref.depth_normals(case["depth"][None], case["intrinsics"][None], case["cutoff"])
    assert normals_ref.same_bits(n[0], case["nmap"])                          # NaN positions and payloads included


def test_quantise_and_the_uint16_division():
    n = np.array([[-1.0, 0.0, 1.0], [np.nan, 0.5, -0.5], [1.0 / 255, -1e-9, 0.999]], F)
    q = normals_ref.quantise(n)
    assert q.dtype == np.uint8 and q.tolist() == [[255, 127, 0], [63, 191, 0], [254, 127, 128]]
    d = np.array([[[0, 1, 9999, 10000, 65535]]], np.uint16)
    assert normals_ref.same_bits(normals_ref.metres(d, 10000.0), d.astype(np.float32) / float(10000.0))


def test_restated_filter_on_images_with_a_known_answer():
    rng = np.random.default_rng(4)
    const = np.broadcast_to(rng.integers(0, 256, (2, 1, 1, 3)).astype(np.uint8), (2, 7, 9, 3))
    assert np.array_equal(normals_ref.bilateral(const, 9), const) and np.array_equal(normals_ref.bilateral(const, 3), const)
    # two colours 765 apart in the index: the other side's weight is exp(-765^2 / (2 * 75^2)) ~ 3e-23, nothing crosses
    step = np.zeros((1, 10, 12, 3), np.uint8)
    step[:, :, 6:] = 255
    assert np.array_equal(normals_ref.bilateral(step, 9), step)
    # a wide sigma_color turns it into a blur: the edge pixels move towards each other
    soft = normals_ref.bilateral(step, 9, 1000.0, 75.0)
    assert 0 < soft[0, 5, 5, 0] < soft[0, 5, 6, 0] < 255


# ---- the weight tables ---------------------------------------------------------------------------------------------
def test_bilateral_tables():
    from posecnn_amd import ops
    color, space, offsets = ops.bilateral_tables(9, 75, 75)
    assert color.dtype == F and color.shape == (768,) and space.dtype == F and space.shape == (49,) and offsets.shape == (49, 2)
    want = [(i, j) for i in range(-4, 5) for j in range(-4, 5) if i * i + j * j <= 16]    # i outer, j inner
    assert len(want) == 49 and [tuple(o) for o in offsets.tolist()] == want
    assert color[0] == 1 and (np.diff(color) <= 0).all() and (np.diff(color[:300]) < 0).all() and color[767] >= 0
    centre = want.index((0, 0))
    assert space[centre] == 1 and (np.delete(space, centre) < 1).all()
    order = np.argsort((offsets.astype(np.int64) ** 2).sum(1), kind="stable")
    assert (np.diff(space[order]) <= 0).all()                                           # decreasing in the distance
    assert color[75] == F(np.exp(-0.5)) and space[want.index((0, 3))] == F(np.exp(-0.5 * 9 / 75.0 ** 2))
    # the restatement builds the same tables on its own
    rc, rs, ro = normals_ref.tables(9, 75.0, 75.0)
    assert normals_ref.same_bits(color, rc) and normals_ref.same_bits(space, rs) and ro == want
    assert ops.bilateral_tables(9, 75, 75)[0] is color                                  # cached
    assert len(ops.bilateral_tables(3, 10, 10)[1]) == 5 and len(ops.bilateral_tables(15, 10, 10)[1]) == 149
    for bad in (0, 1, 4, 17):
        with pytest.raises(ValueError):
            ops.bilateral_tables(bad, 75, 75)


# ---- the C boundary ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from posecnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_argument_validation_happens_on_the_host(L):
    """Every call here returns before anything is launched: the pointers are host addresses that are never read."""
    from posecnn_amd import _lib
    buf = ctypes.create_string_buffer(1 << 14)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    q = ctypes.c_void_p(p.value + 4096)
    EINVAL, ENULL = _lib.PCNN_EINVAL, _lib.PCNN_ENULL
    err = L.pcnn_last_error_string
    nm = lambda f32, u16, B=1, H=8, W=8, factor=1000.0: L.pcnn_depth_normals_fwd(f32, u16, factor, p, B, H, W, 20.0, q, None)
    bl = lambda d, taps, B=1, H=8, W=8: L.pcnn_bilateral_u8c3_fwd(p, B, H, W, d, p, p, taps, q, None)
    im = lambda f32, u16, d=9, taps=49, B=1, H=8, W=8: L.pcnn_normal_image_fwd(f32, u16, 1000.0, p, B, H, W, 20.0, d, p, p, taps, q, None)
    # both or neither depth pointer
    for call in (nm, im):
        assert call(p, p) == EINVAL and b"exactly one" in err()
        assert call(None, None) == EINVAL and b"exactly one" in err()
        # bad shapes: H < 5, W < 5, no frame, a negative size
        assert call(p, None, H=4) == EINVAL and b"at least 5" in err()
        assert call(None, p, W=4) == EINVAL
        assert call(p, None, B=0) == EINVAL and b"batch" in err()
        assert call(p, None, B=-1) == EINVAL
        assert call(p, None, H=-8) == EINVAL
        assert call(p, None, B=1 << 12, H=1 << 10, W=1 << 10) == EINVAL and b"2^30" in err()
        assert call(p, None, H=65535 * 32 + 1, W=5) == EINVAL and b"height" in err()          # more grid rows than a launch takes
    assert nm(None, p, factor=0.0) == EINVAL and b"factor_depth" in err()
    assert bl(9, 49, H=4) == EINVAL and bl(9, 49, W=3) == EINVAL and bl(9, 49, B=0) == EINVAL
    # d: even, too small, too large; a tap count that is not d's
    for d in (8, 2, 1, 0, -3, 17):
        assert bl(d, 49) == EINVAL and b"odd" in err(), d
    for d in (8, 2, 1, -3, 17):
        assert im(p, None, d=d) == EINVAL and b"odd" in err(), d
    assert bl(9, 48) == EINVAL and b"49 taps" in err()
    assert im(p, None, d=3, taps=49) == EINVAL and b"5 taps" in err()
    # NULL pointers are reported, not dereferenced
    assert L.pcnn_depth_normals_fwd(p, None, 0.0, None, 1, 8, 8, 20.0, q, None) == ENULL
    assert L.pcnn_depth_normals_fwd(p, None, 0.0, p, 1, 8, 8, 20.0, None, None) == ENULL
    assert L.pcnn_bilateral_u8c3_fwd(None, 1, 8, 8, 9, p, p, 49, q, None) == ENULL
    assert L.pcnn_bilateral_u8c3_fwd(p, 1, 8, 8, 9, None, p, 49, q, None) == ENULL
    assert L.pcnn_bilateral_u8c3_fwd(p, 1, 8, 8, 9, p, None, 49, q, None) == ENULL
    assert L.pcnn_bilateral_u8c3_fwd(p, 1, 8, 8, 9, p, p, 49, None, None) == ENULL
    assert L.pcnn_bilateral_u8c3_fwd(p, 1, 8, 8, 9, p, p, 49, p, None) == EINVAL and b"alias" in err()
    assert L.pcnn_normal_image_fwd(p, None, 0.0, p, 1, 8, 8, 20.0, 9, None, p, 49, q, None) == ENULL
    assert L.pcnn_normal_image_fwd(p, None, 0.0, p, 1, 8, 8, 20.0, 0, None, None, 0, None, None) == ENULL    # d = 0: no tables, but an image


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from posecnn_amd import ops
    for name in ("depth_normals", "bilateral_filter_u8", "normal_image", "bilateral_tables"):
        assert name in ops.__all__
    k = torch.zeros(1, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.depth_normals(torch.zeros(1, 8, 8), k)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.depth_normals(torch.zeros(1, 8, 8, dtype=torch.uint16), k, factor_depth=10000.0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.normal_image(torch.zeros(1, 8, 8), k)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.bilateral_filter_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        ops.normal_image(np.zeros((1, 8, 8), F), k)


def test_single_frame_depth_input_refuses_a_frame_that_is_not_uint16():
    """Before anything touches a device: a float frame in metres or an int32 frame would otherwise be cast silently."""
    from posecnn_amd import fcn
    for bad in (np.zeros((8, 8), F), np.zeros((8, 8), np.int32), np.zeros((8, 8, 1), np.uint16)):
        for fmt in ("DEPTH", "NORMAL"):
            with pytest.raises(TypeError, match="uint16"):
                fcn._depth_frame_input(fmt, bad, {}, "cpu")
