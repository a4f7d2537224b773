"""The input front end (include/posecnn_hip_frontend.h) on the GPU:

  * `ops.depth_normals` against the recorded outputs of the reference's kernels (tests/golden/normals.npz) and the numpy
    restatement (tests/normals_ref.py), bit for bit;
  * `ops.bilateral_filter_u8` against the restatement, byte for byte;
  * `ops.normal_image` (the fused kernel) against the restatement and against the unfused composition, byte for byte, on
    synthetic frames, a demo depth frame, and the shapes around the kernel's 32 x 32 tile;
  * the memory contract of the three entries (tests/memguard.py through the harness of test_gpu_memory_contract.py);
  * `fcn.im_segment_single_frame` with `input_format` 'NORMAL' and 'DEPTH' against the same network fed the host-built
    float32 blob, bit for bit.
"""
import functools
import os

import numpy as np
import pytest

import normals_ref as R
from normals_ref import same_bits
from posecnn_amd import config, synth
from test_gpu_memory_contract import Case, execute

pytestmark = pytest.mark.gpu
F = np.float32
TILE = 32                                    # csrc/normals.hip: NT
SHAPES = [(5, 5), (19, 37), (33, 70)]        # 3 W % 4 = 3, 3, 2: no row of any of them ends on a dword boundary
DEMO_DEPTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo_images", "000001-depth.png")
FACTOR = 10000.0
CUTOFF = 2.0


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def intrinsics(B, H, W):
    """A different camera per frame; principal point inside the frame."""
    return np.array([[500.0 + 37.5 * b, 510.0 - 21.25 * b, 0.5 * H + 0.3 * b, 0.45 * W - 0.7 * b] for b in range(B)], F)


@functools.lru_cache(maxsize=None)
def depth_frames(H, W, raw):
    """B = 3: a rippled slope with zero holes and values at / above the cutoff; random depths (+ a NaN, float only); a
    constant-depth plane with holes. raw: uint16 over FACTOR, else float32 metres."""
    rng = np.random.default_rng(1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    a = 0.9 + 0.004 * xx + 0.007 * yy + 0.03 * np.sin(0.8 * xx) * np.cos(0.6 * yy)
    a[rng.random((H, W)) < 0.08] = 0
    a[H // 2, W // 2] = CUTOFF
    a[H // 2, W // 2 - 1] = CUTOFF + 0.5
    b = rng.uniform(0.3, 2.4, (H, W))                        # some above the cutoff
    b[rng.random((H, W)) < 0.1] = 0
    c = np.full((H, W), 1.25)
    c[1, 1] = c[H - 2, W - 2] = 0
    d = np.stack([a, b, c])
    if raw:
        return np.round(d * FACTOR).astype(np.uint16)
    d = d.astype(F)
    d[1, H // 3, W // 3] = np.nan
    d[1, 0, 0] = np.nan
    return d


def frames_case(H, W, raw):
    depth = depth_frames(H, W, raw)
    K = intrinsics(3, H, W)
    m = R.metres(depth, FACTOR) if raw else depth
    assert (m == 0).any() and (m >= CUTOFF).any() and (raw or np.isnan(m).any())
    return depth, K, m


def run_normals(gpu, depth, K, cutoff, raw):
    from posecnn_amd import ops
    n = ops.depth_normals(_t(depth, gpu), _t(K, gpu), cutoff, FACTOR if raw else None)
    return _np(n)


def run_image(gpu, depth, K, cutoff, raw, d):
    from posecnn_amd import ops
    im = ops.normal_image(_t(depth, gpu), _t(K, gpu), factor_depth=FACTOR if raw else None, depth_cutoff=cutoff, d=d)
    assert im.dtype.is_floating_point is False and tuple(im.shape) == depth.shape + (3,)
    return _np(im)


def first_difference(got, want):
    bad = np.argwhere((got != want).reshape(got.shape[:3] + (-1,)).any(-1))
    return "%d pixels differ, first at %s: got %s want %s" % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]) if len(bad) else ""


# ---- the normal map ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.golden_cases(), ids=lambda c: c["name"])
def test_depth_normals_equal_the_reference_outputs(gpu, case):
    n = run_normals(gpu, case["depth"][None], case["intrinsics"][None], case["cutoff"], False)
    assert n.dtype == F and same_bits(n[0].view(np.uint32), case["nmap"].view(np.uint32))


@pytest.mark.parametrize("raw", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_depth_normals_equal_the_restatement(gpu, shape, raw):
    depth, K, m = frames_case(*shape, raw)
    want = R.depth_normals(m, K, CUTOFF)
    nan = np.isnan(want).any(-1)
    assert nan[:, -1].all() and nan[:, :, -1].all() and not nan.all() and nan[:, :-1, :-1].any()
    plane = want[2][~nan[2]]
    assert len(plane) and (plane == np.array([0, 0, 1], F)).all()             # constant depth: the normal is the optical axis
    got = run_normals(gpu, depth, K, CUTOFF, raw)
    assert same_bits(got.view(np.uint32), want.view(np.uint32)), first_difference(got.view(np.uint32), want.view(np.uint32))


# ---- the bilateral filter ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def images(H, W):
    """B = 5: uniform noise; a smooth ramp with small noise (every tap carries weight); a two-colour step edge; a
    constant image; 0 / 255 in a checker pattern."""
    rng = np.random.default_rng(7 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    noise = rng.integers(0, 256, (H, W, 3))
    ramp = np.clip(np.stack([3 * xx + yy, 200 - 2 * yy + xx, 90 + xx - yy], -1) + rng.integers(-6, 7, (H, W, 3)), 0, 255)
    step = np.where((xx > W // 2)[..., None], (200, 40, 90), (30, 180, 60))
    const = np.broadcast_to((17, 250, 101), (H, W, 3))
    checker = np.broadcast_to((((xx + yy) & 1) * 255)[..., None], (H, W, 3))
    return np.stack([noise, ramp, step, const, checker]).astype(np.uint8)


@pytest.mark.parametrize("d", [3, 9])
@pytest.mark.parametrize("shape", SHAPES + [(34, 33)], ids=lambda s: "%dx%d" % s)
def test_bilateral_filter_equals_the_restatement(gpu, shape, d):
    from posecnn_amd import ops
    src = images(*shape)
    assert 3 * shape[1] % 4 != 0
    want = R.bilateral(src, d)
    assert np.array_equal(want[3], src[3]) and not np.array_equal(want[1], src[1])
    got = _np(ops.bilateral_filter_u8(_t(src, gpu), d))
    assert got.dtype == np.uint8 and np.array_equal(got, want), first_difference(got, want)
    assert np.array_equal(got[3], src[3])                                    # a constant image returns itself
    # other sigmas reach the kernel through the tables
    want = R.bilateral(src[:2], d, 20.0, 3.0)
    got = _np(ops.bilateral_filter_u8(_t(src[:2], gpu), d, 20.0, 3.0))
    assert np.array_equal(got, want), first_difference(got, want)


def test_bilateral_filter_diameters_of_the_generic_loop(gpu):
    from posecnn_amd import ops
    src = images(19, 37)[:2]
    for d in (5, 15):
        want = R.bilateral(src, d, 60.0, 4.0)
        got = _np(ops.bilateral_filter_u8(_t(src, gpu), d, 60.0, 4.0))
        assert np.array_equal(got, want), (d, first_difference(got, want))
    with pytest.raises(ValueError):
        ops.bilateral_filter_u8(_t(src, gpu)[:, :4], 9)                      # H < 5: the library's check
    with pytest.raises(ValueError):
        ops.bilateral_filter_u8(_t(src, gpu)[..., :2], 9)


# ---- the fused kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [0, 9])
@pytest.mark.parametrize("raw", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_normal_image_equals_the_restatement_and_the_unfused_composition(gpu, shape, raw, d):
    from posecnn_amd import ops
    depth, K, m = frames_case(*shape, raw)
    want = R.normal_image(m, K, CUTOFF, d)
    assert len(np.unique(want)) > 3
    got = run_image(gpu, depth, K, CUTOFF, raw, d)
    assert np.array_equal(got, want), first_difference(got, want)
    q = _t(R.quantise(run_normals(gpu, depth, K, CUTOFF, raw)), gpu)
    unfused = _np(q) if d == 0 else _np(ops.bilateral_filter_u8(q, d))
    assert np.array_equal(got, unfused), first_difference(got, unfused)


@functools.lru_cache(maxsize=None)
def demo_frame():
    """(depth uint16 [480,640], intrinsics [1,4], quantised image, filtered image) of a recorded YCB-Video frame."""
    from PIL import Image
    depth = np.array(Image.open(DEMO_DEPTH)).astype(np.uint16)
    assert depth.shape == (480, 640) and (depth == 0).any()
    Kd = config.DEMO_INTRINSICS.astype(F)
    K = np.array([[Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2]]], F)
    q = R.quantise(R.depth_normals(R.metres(depth[None], FACTOR), K, 20.0))
    return depth, K, q, R.bilateral(q, 9)


@pytest.mark.parametrize("d", [0, 9])
def test_normal_image_of_a_demo_frame(gpu, d):
    depth, K, q, filtered = demo_frame()
    want = q if d == 0 else filtered
    assert len(np.unique(want)) > 100 and (q != filtered).mean() > 0.2
    got = run_image(gpu, depth[None], K, 20.0, True, d)
    assert np.array_equal(got, want), first_difference(got, want)
    # a 48 x 64 crop is a frame of its own: new borders, a shifted principal point
    y0, x0 = 200, 300
    crop = np.ascontiguousarray(depth[None, y0:y0 + 48, x0:x0 + 64])
    Kc = K - np.array([[0, 0, y0, x0]], F)                                   # cx goes with the row, cy with the column
    want = R.normal_image(R.metres(crop, FACTOR), Kc, 20.0, d)
    assert len(np.unique(want)) > 30
    got = run_image(gpu, crop, Kc, 20.0, True, d)
    assert np.array_equal(got, want), first_difference(got, want)


@pytest.mark.parametrize("W", [TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("H", [TILE - 1, TILE, TILE + 1])
def test_normal_image_at_the_tile_boundaries(gpu, H, W):
    depth, K, m = frames_case(H, W, True)
    want = R.normal_image(m, K, CUTOFF, 9)
    got = run_image(gpu, depth, K, CUTOFF, True, 9)
    assert np.array_equal(got, want), first_difference(got, want)


def test_normal_image_errors(gpu):
    from posecnn_amd import ops
    depth, K, _ = frames_case(19, 37, True)
    d, k = _t(depth, gpu), _t(K, gpu)
    with pytest.raises(ValueError):
        ops.normal_image(d, k)                                               # uint16 without its factor
    with pytest.raises(ValueError):
        ops.normal_image(_t(R.metres(depth, FACTOR), gpu), k, factor_depth=FACTOR)   # float32 with one
    with pytest.raises(ValueError):
        ops.normal_image(d, k[:2], factor_depth=FACTOR)                      # one camera per frame
    with pytest.raises(ValueError):
        ops.normal_image(d, k, factor_depth=FACTOR, d=4)
    with pytest.raises(ValueError):
        ops.normal_image(_t(depth[:, :4], gpu), k, factor_depth=FACTOR)      # H < 5: the library's check
    with pytest.raises(ValueError):
        ops.depth_normals(d, k, factor_depth=0.0)


# ---- memory contract -----------------------------------------------------------------------------------------------
def _normals_case(name, H, W, raw):
    def make():
        depth, K, m = frames_case(H, W, raw)
        return dict(depth=depth, K=K, want=R.depth_normals(m, K, CUTOFF))

    def run(c):
        from posecnn_amd import ops
        return dict(nmap=ops.depth_normals(c.e("depth"), c.e("K"), CUTOFF, FACTOR if raw else None))

    def check(d, o):
        assert same_bits(o["nmap"].view(np.uint32), d["want"].view(np.uint32))
    return Case(name, ("pcnn_depth_normals_fwd",), make, run, check)


def _bilateral_case(name, H, W, d):
    def make():
        src = images(H, W)
        return dict(src=src, want=R.bilateral(src, d))

    def run(c):
        from posecnn_amd import ops
        return dict(dst=ops.bilateral_filter_u8(c.e("src"), d))

    def check(dd, o):
        assert np.array_equal(o["dst"], dd["want"])
    return Case(name, ("pcnn_bilateral_u8c3_fwd",), make, run, check)


def _image_case(name, H, W, raw, d):
    def make():
        depth, K, m = frames_case(H, W, raw)
        return dict(depth=depth, K=K, want=R.normal_image(m, K, CUTOFF, d))

    def run(c):
        from posecnn_amd import ops
        return dict(image=ops.normal_image(c.e("depth"), c.e("K"), factor_depth=FACTOR if raw else None, depth_cutoff=CUTOFF, d=d))

    def check(dd, o):
        assert np.array_equal(o["image"], dd["want"])
    return Case(name, ("pcnn_normal_image_fwd",), make, run, check)


CONTRACT = [_normals_case("depth_normals_f32_3x19x37", 19, 37, False), _normals_case("depth_normals_u16_3x33x70", 33, 70, True),
            _bilateral_case("bilateral_5x19x37_d9", 19, 37, 9), _bilateral_case("bilateral_5x5x5_d3", 5, 5, 3),
            _image_case("normal_image_u16_3x33x70_d9", 33, 70, True, 9), _image_case("normal_image_f32_3x19x37_d0", 19, 37, False, 0),
            _image_case("normal_image_f32_3x5x5_d9", 5, 5, False, 9)]


@pytest.mark.parametrize("case", CONTRACT, ids=[c.name for c in CONTRACT])
def test_memory_contract_of_the_frontend_entries(gpu, case):
    """Guard bands around every output and input, both poison patterns of uninitialised memory: identical results (so
    every output byte is written), guards and inputs intact, every entry reached."""
    execute(case)


# ---- end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["NORMAL", "DEPTH"])
def test_single_frame_input_modes_equal_the_host_built_blob(gpu, fmt, monkeypatch):
    """`im_segment_single_frame` of a 'NORMAL' / 'DEPTH' network: the device-side input (ops.normal_image / the raw uint16
    frame, the blob formed in the first kernel) gives the outputs of the same network fed the float32 blob built on the
    host as lib/fcn/test.py:70-74, :89-96 builds it, bit for bit."""
    import torch
    from posecnn_amd import fcn
    from posecnn_amd.networks import vgg16_convs
    H = W = 64
    depth = np.ascontiguousarray(demo_frame()[0][200:200 + H, 300:300 + W])
    Kmat = config.DEMO_INTRINSICS.copy()
    Kmat[0, 2], Kmat[1, 2] = 31.5, 30.25
    meta = {"intrinsic_matrix": Kmat, "factor_depth": np.array([[FACTOR]])}
    if fmt == "NORMAL":
        K32 = Kmat.astype(F)
        img = R.normal_image(R.metres(depth[None], FACTOR), np.array([[K32[0, 0], K32[1, 1], K32[0, 2], K32[1, 2]]], F), 20.0, 9)
        assert len(np.unique(img)) > 30
        blob = img.astype(F)
        blob -= config.PIXEL_MEANS
    else:
        blob = fcn._get_image_blob(np.zeros((H, W, 3), np.uint8), depth)[1]
    assert blob.shape == (1, H, W, 3) and blob.dtype == F
    net = vgg16_convs(fmt, 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=False, is_train=False,
                      device=gpu, seed=3, init="he")
    synth.init_calibrated(net)
    pts = synth.make_model_points(22, 128)
    call = lambda: fcn.im_segment_single_frame(net, None, depth, meta, config.LOV_EXTENTS, pts, config.LOV_SYMMETRY, 22, device=gpu)
    with torch.no_grad():
        got = call()
        fed = net.get_output("data")
        assert fed.dtype == (torch.uint8 if fmt == "NORMAL" else torch.uint16)
        monkeypatch.setattr(fcn, "_depth_frame_input", lambda *a: blob)
        want = call()
        assert net.get_output("data").dtype == torch.float32
    assert got[0].shape == (H, W) and got[1].shape == (H, W, 22) and got[2].shape == (H, W, 66) and np.isfinite(got[1]).all()
    for name, g, w in zip(("labels", "probs", "vertex_pred", "rois", "poses"), got, want):
        assert same_bits(g, w), name
