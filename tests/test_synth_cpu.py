"""Synthetic training scenes, the part that needs no GPU: the numpy restatement of csrc/synth_scene.hip (tests/synth_ref.py)
against the pinned CPU checker of the refinement renderer and against hand-derived lighting answers; the scene sampler's
invariants; the host-built training tables against datasets.training_blobs; the OBJ reader; the C-ABI's host-side
argument validation."""
import ctypes
import os

import numpy as np
import pytest

import icp_scene as S
import oracle
import synth_cases as C
import synth_ref as R
from posecnn_amd import config

F = np.float32


# ---- geometry: tied to the pinned checker of render.hip ------------------------------------------------------------
@pytest.mark.parametrize("size", C.SIZES, ids=["%dx%d" % s for s in C.SIZES])
@pytest.mark.parametrize("mesh", ["box", "icosphere"])
def test_single_instance_geometry_equals_the_refinement_renderer(mesh, size):
    """Hit mask, winning camera depth and object-frame point of a one-object scene = oracle.render_mesh, bit for bit."""
    H, W = size
    K = C.intrinsics(H, W)
    v, n, f = S.box_mesh((0.06, 0.04, 0.05)) if mesh == "box" else S.icosphere(0.05, 2, (1.0, 0.8, 1.2))
    T = S.pose(S.rot((1, 2, 0.5), 0.7), (0.02, -0.01, 0.45))
    got = R.render_scenes([dict(vertices=v, normals=n, faces=f)], [[(0, 3, T, 40)]], [[0, 0, 0, 1]], C.K4(K), H, W, C.Z_NEAR,
                          C.Z_FAR, 1000.0, 1)
    want = oracle.render_mesh(v, n, f, T[None], K, H, W, (C.Z_NEAR, C.Z_FAR), model_index=0, want=("vertices", "canonical"))
    hit = np.isfinite(want["vertices"][0, :, :, 2])
    assert hit.sum() > 500 and np.array_equal(got["label"][0] == 3, hit)
    assert np.array_equal(got["camz"][0][hit].view(np.uint32), want["vertices"][0, :, :, 2][hit].view(np.uint32))
    assert np.array_equal(got["vertmap"][0][hit], want["canonical"][0][hit])
    assert not got["vertmap"][0][~hit].any() and not got["depth"][0][~hit].any()
    assert np.array_equal(got["depth"][0][hit], np.minimum(F(65535), F(1000.0) * got["camz"][0][hit]).astype(np.uint16))
    assert got["pixel_counts"].tolist() == [int(hit.sum())] and got["valid"].tolist() == [1]


# ---- lighting: hand-derived answers ---------------------------------------------------------------------------------
def _shade(pos, n, col, light, sh):
    return R.shade(np.asarray([pos], F), np.asarray([n], F), np.asarray([col], F), np.asarray(light, F), np.asarray([sh]))[0]


def test_surface_facing_the_light_at_a_known_distance():
    """Light at the camera, surface 2 m in front facing it: L = V = r = -z, diffuse = specular = 1, attenuation
    1 / (1 + 0.01 * 4); ambient 0.5 c I."""
    col = (0.5, 0.25, 0.125)
    for sh in (1, 64):
        got = _shade((0, 0, 2), (0, 0, -1), col, (0, 0, 0, 1.0), sh)
        att = F(1) / (F(1) + F(0.01) * F(4))
        want = [F(0.5) * F(c) + att * (F(c) + F(1)) for c in col]
        assert got.tolist() == [float(w) for w in want]
    got = _shade((0, 0, 2), (0, 0, -1), col, (0, 0, 0, 0.5), 40)       # the intensity scales every term
    assert got.tolist() == [float((F(0.5) * F(c)) * F(0.5) + att * (F(c) * F(0.5) + F(0.5))) for c in col]


def test_zero_diffuse_kills_the_specular_term():
    """Normal perpendicular to (or facing away from) the light: only the ambient term is left, whatever the shininess."""
    for n in ((1, 0, 0), (0, 0, 1)):
        for sh in (1, 64):
            got = _shade((0, 0, 2), n, (0.5, 0.25, 1.0), (0, 0, 0, 2.0), sh)
            assert got.tolist() == [0.5, 0.25, 1.0]                      # (0.5 c) * 2


def test_integer_shininess_is_binary_powering():
    x = np.asarray([0.5, 0.9, 0.999], F)
    assert np.array_equal(R.powi(x, 1), x)
    assert R.powi(x, 64)[0] == F(2.0) ** -64                             # six squarings of a power of two are exact
    x2 = x * x; x4 = x2 * x2; x5 = x4 * x; x10 = x5 * x5; x20 = x10 * x10; x40 = x20 * x20   # 40 = 101000b
    assert np.array_equal(R.powi(x, 40), x40)
    # through the shader: normal tilted by t off the light / view axis: V.r = cos 2t
    t = np.radians(30.0)
    n = (np.sin(t), 0.0, -np.cos(t))
    a, b = _shade((0, 0, 1), n, (0, 0, 0), (0, 0, 0, 1.0), 1), _shade((0, 0, 1), n, (0, 0, 0), (0, 0, 0, 1.0), 64)
    att = 1.0 / 1.01
    assert abs(a[0] - att * np.cos(2 * t)) < 1e-6 and abs(b[0] - att * np.cos(2 * t) ** 64) < 1e-6


def test_quantisation_truncates_and_saturates():
    lin = np.asarray([-0.1, 0.0, 0.999 / 255, 1.0 / 255, 0.5, 254.999 / 255, 1.0, 3.7], F)
    assert R.to_byte(lin).tolist() == [0, 0, 0, 1, 127, 254, 255, 255]
    got = _shade((0, 0, 2), (0, 0, -1), (1.0, 1.0, 1.0), (0, 0, 0, 2.0), 40)     # 1 + (2 + 2) / 1.04 > 1
    assert R.to_byte(got).tolist() == [255, 255, 255]


def test_texture_fetch_by_hand():
    tex = np.asarray([[[0, 0, 0], [255, 255, 255]], [[51, 51, 51], [102, 102, 102]]], np.uint8)    # 2 x 2
    uv = np.asarray([[0.25, 0.75], [0.75, 0.75], [0.25, 0.25], [0.5, 0.75], [-3.0, 9.0], [7.0, -2.0], [0.5, 0.5]], F)
    got = R.texture_sample(tex, uv)[:, 0]
    # texel centres, v flipped: (u, v) = (.25, .75) is the first row's first texel; outside: clamped to the edge
    assert got[:3].tolist() == [0.0, 1.0, float(F(51) / F(255))] and got[3] == F(0.5)
    assert got[4] == 0.0 and got[5] == F(102) / F(255)
    assert abs(got[6] - (0 + 255 + 51 + 102) / 4 / 255) < 1e-6


def test_depth_ties_go_to_the_lower_slot_then_the_lower_face():
    o = C.main_reference(*C.SIZES[0])
    assert o["pixel_counts"][2] > 500 and o["pixel_counts"][3] == 0     # scene 1: slots 0 and 1 are one mesh at one pose
    assert o["pixel_counts"][5] == 0                                    # the box past z_far
    assert o["valid"].tolist() == [1, 0, 1]                             # an empty scene is valid


@pytest.mark.parametrize("first_is_red", [True, False])
def test_coplanar_faces_tie_and_the_lower_face_wins(first_is_red):
    """Two faces over the same three positions: every covered pixel carries two equal depths; the colour is face 0's."""
    H, W = C.SIZES[0]
    K = C.intrinsics(H, W)
    o = R.render_scenes([C.coplanar_mesh(K, first_is_red)], [[(0, 1, S.pose(np.eye(3), (0, 0, 0)), 40)]], [[0, 0, 0, 1]], C.K4(K), H, W)
    hit = o["label"][0] == 1
    bgr = o["color"][0][hit][:, :3]
    assert hit.sum() > 20 and (bgr[:, 1] == 0).all()
    won, lost = (2, 0) if first_is_red else (0, 2)                      # BGR
    assert (bgr[:, won] > 0).all() and (bgr[:, lost] == 0).all()


@pytest.mark.parametrize("size", C.SIZES, ids=["%dx%d" % s for s in C.SIZES])
def test_the_two_triangles_at_the_small_box_threshold(size):
    K, stats = C.intrinsics(*size), {}
    o = R.render_scenes([C.box_pixels_mesh(K)], [[(0, 1, S.pose(np.eye(3), (0, 0, 0)), 40)]], [[0, 0, 0, 1]], C.K4(K), *size, stats=stats)
    assert sorted(stats["boxes"]) == [64, 65] and o["pixel_counts"][0] > 40


# ---- the sampler ----------------------------------------------------------------------------------------------------
def test_sampler_invariants():
    from posecnn_amd.synthesize import SceneSampler
    a, b = SceneSampler(21, seed=7, tnear=0.5, tfar=1.5), SceneSampler(21, seed=7, tnear=0.5, tfar=1.5)
    seen = set()
    for _ in range(60):
        sc, sc2 = a.sample(), b.sample()
        n = len(sc.instances)
        seen.add(n)
        assert 5 <= n <= 7 and len({m for m, _, _ in sc.instances}) == n
        assert all(0 <= m < 21 for m, _, _ in sc.instances)
        t = np.stack([T[:, 3] for _, T, _ in sc.instances])
        d = np.linalg.norm(t[:, None] - t[None], axis=2) + np.eye(n)
        assert d.min() >= 0.2
        assert (np.abs(t[:, :2]) <= 0.1).all() and (t[:, 2] >= 0.5).all() and (t[:, 2] <= 1.5).all()
        for _, T, sh in sc.instances:
            assert np.allclose(T[:, :3] @ T[:, :3].T, np.eye(3), atol=1e-12) and np.linalg.det(T[:, :3]) > 0
            assert isinstance(sh, int) and 40 <= sh <= 120
        assert abs(sc.light[0]) <= 2 and abs(sc.light[1]) <= 2 and sc.light[2] == 0 and 0.5 <= sc.light[3] <= 2
        assert np.array_equal(sc.light, sc2.light)
        assert all(m == m2 and sh == sh2 and np.array_equal(T, T2) for (m, T, sh), (m2, T2, sh2) in zip(sc.instances, sc2.instances))
    assert seen == {5, 6, 7}
    assert not np.array_equal(SceneSampler(21, seed=8).sample().light, SceneSampler(21, seed=7).sample().light)
    every = SceneSampler(4, seed=1, is_sampling=False, tnear=0.6, tfar=2.0).sample()
    assert [m for m, _, _ in every.instances] == [0, 1, 2, 3]


def test_sampler_pose_table_branch():
    from posecnn_amd.synthesize import SceneSampler
    table = [np.asarray([[1, 0, 0, 0, 0.3 * c - 1.0, 0.0, 1.0], [0, 1, 0, 0, 0.3 * c - 1.0, 0.4, 1.2]]) for c in range(8)]
    s = SceneSampler(8, seed=3, is_sampling_pose=True, pose_table=table)
    for _ in range(20):
        for m, T, _ in s.sample().instances:
            d = np.abs(T[:, 3][None] - np.stack([r[4:] for r in table[m]]))
            assert (d <= 0.1 + 1e-12).all(axis=1).any()                 # +-0.1 around one of the model's table rows
            assert np.allclose(T[:, :3] @ T[:, :3].T, np.eye(3), atol=1e-9)


def test_pose_table_is_the_reference_format(tmp_path):
    """Synthesizer::loadPoses: a list of per-model files, rows of 7 floats; relative names resolve next to the list."""
    from posecnn_amd.synthesize import SceneSampler
    _, pose_file, tables = C.write_model_and_pose_files(str(tmp_path), textured=False)
    got = SceneSampler.load_pose_table(pose_file)
    assert len(got) == 3 and [t.shape for t in got] == [(2, 7), (1, 7), (3, 7)]
    for g, w in zip(got, tables):
        assert np.allclose(g, w, rtol=0, atol=1e-8)
    s = SceneSampler(3, seed=5, is_sampling=False, is_sampling_pose=True, pose_table=got)
    assert [m for m, _, _ in s.sample().instances] == [0, 1, 2]
    (tmp_path / "poses1.txt").write_text("1 0 0 0 0.1 0.2\n")           # six numbers
    with pytest.raises(ValueError, match="rows of 7"):
        SceneSampler.load_pose_table(pose_file)


def test_online_minibatches_needs_the_reference_switches():
    from posecnn_amd import synthesize as syn, train
    assert train.TrainConfig.SYN_ONLINE is False and (train.TrainConfig.SYN_TNEAR, train.TrainConfig.SYN_TFAR) == (0.5, 2.0)
    with pytest.raises(ValueError, match="SYN_ONLINE"):
        syn.online_minibatches(train.TrainConfig, None, None, 2, None, None, None)


# ---- the training tables --------------------------------------------------------------------------------------------
def _cpu_batch(H, W):
    """A SceneBatch whose frames come from the restatement (CPU tensors): what render_scenes returns, without a GPU."""
    import torch
    from posecnn_amd import synthesize as syn
    K = C.intrinsics(H, W)
    bank = syn.MeshBank(C.bank_meshes(K), C.CLASSES, device="cpu")
    scenes, lights = C.main_scenes()
    scenes = [[inst for i, inst in enumerate(sc) if not (si == 1 and i == 1)] for si, sc in enumerate(scenes)][:2]   # no repeated class
    ref = R.render_scenes(C.bank_meshes(K), C.ref_instances(scenes), lights[:2], C.K4(K), H, W, C.Z_NEAR, C.Z_FAR, 1000.0, 100)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    batch = syn.SceneBatch(bank, [syn.Scene(sc, l) for sc, l in zip(scenes, lights)], K, H, W, 1000.0, t(ref["color"]),
                           t(ref["depth"].view(np.int16)).view(torch.uint16), t(ref["label"]), t(ref["vertmap"]),
                           t(ref["pixel_counts"]), t(ref["valid"]))
    return batch, ref


def test_feed_tables_equal_training_blobs_of_the_downloaded_frames():
    from posecnn_amd import datasets, synth
    batch, ref = _cpu_batch(112, 160)
    frames = batch.frames()
    assert np.array_equal(frames[1]["color"], ref["color"][1, :, :, :3]) and np.array_equal(frames[0]["depth"], ref["depth"][0])
    want = datasets.training_blobs(frames, 22)
    feed = batch.feed(config.LOV_EXTENTS, synth.make_model_points(22, 16), config.LOV_SYMMETRY, rgbd=True)
    assert want["vertex_objects"].shape == (2, 5, 6) and want["poses"].shape == (7, 13)
    for k in ("gt_label_2d", "vertex_objects", "poses", "meta_data"):
        g = feed[k].numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape and g.tobytes() == want[k].tobytes(), k
    assert feed["gt_label_2d"] is batch.label and feed["data_p"] is batch.depth
    assert feed["data"].dtype.is_floating_point is False and tuple(feed["data"].shape) == (2, 112, 160, 3)
    meta = frames[0]["meta"]
    assert meta["factor_depth"] == 1000.0 and meta["poses"].shape == (3, 4, 2) and meta["box"].shape == (2, 4)
    # the box holds the label pixels of an object that is wholly inside the image and the depth range
    ys, xs = np.nonzero(ref["label"][0] == meta["cls_indexes"][0])
    b = meta["box"][0]
    assert b[0] <= xs.min() and xs.max() <= b[2] and b[1] <= ys.min() and ys.max() <= b[3]
    c = meta["center"][0]
    assert b[0] < c[0] < b[2] and b[1] < c[1] < b[3]
    with pytest.raises(ValueError):
        _cpu_batch(101, 131)[0].feed(config.LOV_EXTENTS, synth.make_model_points(22, 16), config.LOV_SYMMETRY)


# ---- the OBJ reader -------------------------------------------------------------------------------------------------
OBJ = """mtllib quad.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 0.5 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt 0.5 0.5
vt 0.25 0.25
usemtl m
f 1/1 2/2 3/3 4/4
f 1/6 2/2 5/5
"""


def test_textured_obj_reader(tmp_path):
    from posecnn_amd.icp import Mesh
    from posecnn_amd.synthesize import TexturedMesh
    (tmp_path / "quad.obj").write_text(OBJ)
    (tmp_path / "quad.mtl").write_text("newmtl m\nKd 1 1 1\nmap_Kd quad.png\n")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    tex = np.arange(4 * 6 * 3, dtype=np.uint8).reshape(4, 6, 3)
    if Image is not None:
        Image.fromarray(tex).save(str(tmp_path / "quad.png"))
        m = TexturedMesh.load_obj(str(tmp_path / "quad.obj"))
        assert np.array_equal(m.texture, tex)
    else:
        with pytest.raises(RuntimeError, match="PIL"):
            TexturedMesh.load_obj(str(tmp_path / "quad.obj"))
        (tmp_path / "quad.mtl").write_text("newmtl m\nKd 1 1 1\n")
        m = TexturedMesh.load_obj(str(tmp_path / "quad.obj"))
        assert m.texture is None
    # vertex 1 is used with two texture coordinates: split; the polygon is fanned
    assert m.vertices.shape == (6, 3) and m.uvs.shape == (6, 2) and m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [4, 1, 5]]
    assert np.array_equal(m.vertices[4], m.vertices[0]) and m.uvs[4].tolist() == [0.25, 0.25] and m.uvs[0].tolist() == [0.0, 0.0]
    # the normals are smooth over POSITIONS: both copies of vertex 1 carry the same one
    pos = np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]], F)
    sm = Mesh.smooth_normals(pos, np.asarray([[0, 1, 2], [0, 2, 3], [0, 1, 4]], np.int32))
    assert np.array_equal(m.normals[0], sm[0]) and np.array_equal(m.normals[4], sm[0]) and np.array_equal(m.normals[5], sm[4])


# ---- the C-ABI ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from posecnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_argument_validation_happens_on_the_host(L):
    """Every call here returns before anything is launched: the device pointers are host addresses that are never read."""
    from posecnn_amd._lib import PCNN_EINVAL, PCNN_ENULL, PCNN_EWORKSPACE, PCNN_OK
    buf = ctypes.create_string_buffer(1 << 14)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    n = ctypes.c_size_t(0)
    assert L.pcnn_synth_scene_workspace_bytes(2, 8, 8, ctypes.byref(n)) == PCNN_OK
    assert n.value >= 8 * 2 * 64 + 2 * 32 * 96 and n.value % 16 == 0
    assert L.pcnn_synth_scene_workspace_bytes(2, 8, 8, None) == PCNN_ENULL
    assert L.pcnn_synth_scene_workspace_bytes(-1, 8, 8, ctypes.byref(n)) == PCNN_EINVAL
    assert L.pcnn_synth_scene_workspace_bytes(1, 0, 8, ctypes.byref(n)) == PCNN_EINVAL
    L.pcnn_synth_scene_workspace_bytes(2, 8, 8, ctypes.byref(n))

    base = dict(mesh=np.asarray([[0, 30, 0, 40], [30, 10, 40, 20]], np.int32), tex=None,
                ids=np.asarray([[0, 0, 1], [0, 1, 2], [1, 1, 5]], np.int32),
                prm=np.tile(np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 40], F), (3, 1)), lights=np.zeros((2, 4), F),
                nv=40, nf=60, S=2, H=8, W=8, znear=0.25, zfar=6.0, factor=1000.0, ws=n.value, texbytes=0, uvs=None, textures=None,
                color=p, label=p, valid=p, counts=p, vertices=p)

    def call(**kw):
        a = dict(base, **kw)
        hp = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
        ids, prm = a["ids"], a["prm"]
        return L.pcnn_synth_scene_fwd(a["vertices"], p, None, a["uvs"], p, a["nv"], a["nf"], hp(a["mesh"]), len(a["mesh"]), a["textures"],
                                      a["texbytes"], hp(a["tex"]), hp(ids), hp(prm), len(ids), hp(a["lights"]), None, a["S"], a["H"], a["W"],
                                      100.0, 100.0, 4.0, 4.0, a["znear"], a["zfar"], a["factor"], 10, a["color"], p, a["label"], None,
                                      a["counts"], a["valid"], p, a["ws"], None)

    E = PCNN_EINVAL
    assert call(S=-1) == E and call(H=0) == E and call(nv=-1) == E
    assert call(znear=0.0) == E and call(zfar=0.1) == E and call(factor=0.0) == E
    assert call(ids=base["ids"][[2, 0, 1]]) == E                                        # not sorted by scene
    assert call(ids=np.asarray([[0, 0, 1], [2, 1, 2]], np.int32), prm=base["prm"][:2]) == E   # scene out of range
    assert call(ids=np.asarray([[0, 2, 1]], np.int32), prm=base["prm"][:1]) == E         # mesh out of range
    assert call(ids=np.asarray([[0, 0, 0]], np.int32), prm=base["prm"][:1]) == E         # class 0 is the background
    assert call(ids=np.asarray([[0, 0, 64]], np.int32), prm=base["prm"][:1]) == E
    assert call(mesh=np.asarray([[0, 30, 0, 40], [30, 11, 40, 20]], np.int32)) == E      # vertices past the pool
    assert call(mesh=np.asarray([[0, 30, 0, 40], [30, 10, 41, 20]], np.int32)) == E      # faces past the pool
    assert call(mesh=np.asarray([[0, 30, 0, (1 << 27) + 1], [30, 10, 40, 20]], np.int32), nf=1 << 28) == E
    for bad in (0.0, 256.0, 40.5, -3.0, float("nan")):
        prm = base["prm"].copy()
        prm[1, 12] = bad
        assert call(prm=prm) == E, bad
    many = np.zeros((33, 3), np.int32); many[:, 2] = 1
    assert call(ids=many, prm=np.tile(base["prm"][:1], (33, 1))) == E                    # 33 instances in scene 0
    tex = np.asarray([[0, 2, 2], [16, 4, 4]], np.int32)
    assert call(tex=tex, texbytes=63, uvs=p, textures=p) == E                            # 16 + 48 > 63
    assert call(tex=tex, texbytes=64, uvs=None, textures=p) == PCNN_ENULL                # textured without uvs
    assert call(color=None) == PCNN_ENULL and call(label=None) == PCNN_ENULL and call(valid=None) == PCNN_ENULL
    assert call(counts=None) == PCNN_ENULL and call(lights=None) == PCNN_ENULL
    assert call(vertices=None) == PCNN_ENULL
    assert call(ws=n.value - 1) == PCNN_EWORKSPACE
    assert call(S=0, ids=base["ids"][:0], prm=base["prm"][:0]) == PCNN_OK                # nothing to do, nothing launched
