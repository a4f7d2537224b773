"""pcnn_synth_scene_fwd on the GPU: every output byte — label, depth, colour, vertex map, pixel counts, valid flags — equals
the numpy restatement tests/synth_ref.py; the memory contract of the two entries; and one training step fed from a rendered
batch without a download."""
import contextlib
import functools

import numpy as np
import pytest

import icp_scene as S
import memguard
import synth_cases as C
import synth_ref as R
from posecnn_amd import config, synth

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ("color", "depth", "label", "vertmap", "pixel_counts", "valid")


def _scenes(scenes, lights):
    from posecnn_amd import synthesize as syn
    return [syn.Scene(sc, l) for sc, l in zip(scenes, lights)]


@functools.lru_cache(maxsize=None)
def _bank(H, W, gpu):
    from posecnn_amd import synthesize as syn
    return syn.MeshBank(C.bank_meshes(C.intrinsics(H, W)), C.CLASSES, device=gpu)


def _numpy(batch):
    out = {k: getattr(batch, k) for k in NAMES}
    return {k: memguard.to_numpy(v) for k, v in out.items() if v is not None}


def render(gpu, bank, scenes, lights, K, H, W, background=None, min_pixels=100, want_vertmap=True, z_far=C.Z_FAR):
    import torch
    from posecnn_amd import synthesize as syn
    bg = None if background is None else torch.from_numpy(background).to(gpu)
    batch = syn.render_scenes(bank, _scenes(scenes, lights), K, H, W, bg, (C.Z_NEAR, z_far), 1000.0, min_pixels, want_vertmap)
    torch.cuda.synchronize()
    return batch


def first_difference(name, g, w):
    bad = np.argwhere(g != w)
    return "%s: %d of %d elements differ, first at %s: %r vs %r" % (name, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


def assert_same(got, want, names=NAMES):
    for k in names:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), first_difference(k, g, w)


# ---- the main scenes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_background", [True, False], ids=["background", "black"])
@pytest.mark.parametrize("size", C.SIZES, ids=["%dx%d" % s for s in C.SIZES])
def test_three_scenes_equal_the_restatement(gpu, size, with_background):
    """S = 3 scenes with 2, 6 and 0 instances: a box walked by the workgroup, mutual occlusion, two copies of one mesh at
    one pose, objects half outside the image, past z_far and across z_near, a 64 x 32 and a 1 x 1 texture with uvs outside
    [0, 1], vertex colours, no colours."""
    H, W = size
    want = C.main_reference(H, W, with_background)
    assert max(want["stats"]["boxes"]) > 1000 and want["pixel_counts"][3] == 0 and want["pixel_counts"][2] > 300
    assert (want["label"] > 0).sum() > 0.25 * H * W and len(np.unique(want["label"])) == 6
    scenes, lights = C.main_scenes()
    bg = C.backgrounds(3, H, W) if with_background else None
    got = _numpy(render(gpu, _bank(H, W, gpu), scenes, lights, C.intrinsics(H, W), H, W, bg))
    assert_same(got, want)
    miss = want["label"] == 0
    assert not got["color"][miss][:, 3].any() and (got["color"][~miss][:, 3] == 255).all()
    if with_background:
        assert np.array_equal(got["color"][miss][:, :3], bg[miss])


def test_vertmap_may_be_null(gpu):
    H, W = C.SIZES[1]
    scenes, lights = C.main_scenes()
    batch = render(gpu, _bank(H, W, gpu), scenes, lights, C.intrinsics(H, W), H, W, C.backgrounds(3, H, W), want_vertmap=False)
    assert batch.vertmap is None
    assert_same(_numpy(batch), C.main_reference(H, W, True), [n for n in NAMES if n != "vertmap"])


@pytest.mark.parametrize("size", C.SIZES, ids=["%dx%d" % s for s in C.SIZES])
def test_bounding_boxes_of_64_and_65_pixels(gpu, size):
    """The last triangle walked by its own thread and the first one queued for the workgroup."""
    H, W = size
    K, stats = C.intrinsics(H, W), {}
    scenes, lights = [[(5, S.pose(np.eye(3), (0, 0, 0)), 40)]], np.asarray([[0.3, 0.2, 0, 1.5]], F)
    want = R.render_scenes(C.bank_meshes(K), C.ref_instances(scenes), lights, C.K4(K), H, W, C.Z_NEAR, C.Z_FAR, 1000.0, 10, None, stats)
    assert sorted(stats["boxes"]) == [64, 65] and want["valid"].tolist() == [1]
    assert_same(_numpy(render(gpu, _bank(H, W, gpu), scenes, lights, K, H, W, min_pixels=10)), want)


def test_icosphere_of_20480_faces(gpu):
    """80 chunks of one instance next to the 1-chunk box: the flat (instance, chunk) work list."""
    from posecnn_amd import synthesize as syn
    H, W = C.SIZES[1]
    K = C.intrinsics(H, W)
    v, n, f = S.icosphere(0.07, 5, (1.0, 1.1, 0.9))
    assert len(f) == 20480
    rng = np.random.default_rng(3)
    meshes = [dict(vertices=v, normals=n, faces=f, colors=rng.uniform(0, 1, v.shape).astype(F)), C.meshes()[0]]
    scenes = [[(1, S.pose(S.rot((1, 1, 0), 0.5), (0.03, 0.0, 0.5)), 90), (0, S.pose(S.rot((0, 1, 0), 0.8), (-0.07, 0.01, 0.42)), 60)]]
    lights = np.asarray([[1.0, 1.0, 0, 1.0]], F)
    want = R.render_scenes(meshes, [[(m, m + 7, T, sh) for m, T, sh in scenes[0]]], lights, C.K4(K), H, W, C.Z_NEAR, C.Z_FAR, 1000.0, 100)
    assert (want["pixel_counts"] > 1000).all()
    bank = syn.MeshBank(meshes, (7, 8), device=gpu)
    assert_same(_numpy(render(gpu, bank, scenes, lights, K, H, W)), want)


def test_min_pixels_at_and_one_above_an_instance_count(gpu):
    H, W = C.SIZES[0]
    scenes, lights = C.main_scenes()
    counts = C.main_reference(H, W)["pixel_counts"]
    c = int(counts[:2].min())                    # scene 0: the smaller of its two instances
    assert c > 0
    for mp, ok in ((c, 1), (c + 1, 0)):
        batch = render(gpu, _bank(H, W, gpu), scenes[:1], lights[:1], C.intrinsics(H, W), H, W, min_pixels=mp)
        assert batch.valid.cpu().tolist() == [ok] and batch.pixel_counts.cpu().tolist() == counts[:2].tolist()


def test_no_scenes_and_no_instances(gpu):
    H, W = C.SIZES[1]
    K = C.intrinsics(H, W)
    batch = render(gpu, _bank(H, W, gpu), [], np.zeros((0, 4), F), K, H, W)
    assert tuple(batch.color.shape) == (0, H, W, 4) and tuple(batch.valid.shape) == (0,)
    bg = C.backgrounds(2, H, W)
    got = _numpy(render(gpu, _bank(H, W, gpu), [[], []], np.ones((2, 4), F), K, H, W, bg))
    assert np.array_equal(got["color"][..., :3], bg) and not got["color"][..., 3].any()
    assert not got["label"].any() and not got["depth"].any() and not got["vertmap"].any()
    assert got["valid"].tolist() == [1, 1] and got["pixel_counts"].shape == (0,)


def test_side_stream_gives_the_same_bytes(gpu):
    import torch
    H, W = C.SIZES[0]
    scenes, lights = C.main_scenes()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        batch = render(gpu, _bank(H, W, gpu), scenes, lights, C.intrinsics(H, W), H, W, C.backgrounds(3, H, W))
    side.synchronize()
    assert_same(_numpy(batch), C.main_reference(H, W, True))


# ---- memory contract ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def guarded(pattern):
    from posecnn_amd import _lib, ops, synthesize
    g = memguard.GuardedTorch(pattern, devices=("cuda",))
    rec = memguard.Recorder(_lib.lib())
    with pytest.MonkeyPatch.context() as mp:
        for mod in (ops, synthesize):
            mp.setattr(mod, "torch", g)
            mp.setattr(mod, "lib", lambda: rec)
        mp.setattr(ops, "_default_ws", {})
        yield g, rec


@pytest.mark.parametrize("want_vertmap", [True, False], ids=["vertmap", "no_vertmap"])
def test_memory_contract_of_the_synth_entries(gpu, want_vertmap):
    """Guard bands around every output, the workspace (exactly pcnn_synth_scene_workspace_bytes) and every device input,
    both poison patterns of uninitialised memory: identical results (so every output byte is written), guards and inputs
    intact, both entries reached."""
    import torch
    from posecnn_amd import synthesize as syn
    H, W = C.SIZES[1]
    K = C.intrinsics(H, W)
    scenes, lights = C.main_scenes()
    bg = C.backgrounds(3, H, W)
    runs, calls = {}, set()
    for p in memguard.PATTERNS:
        with guarded(p) as (g, rec):
            bank = syn.MeshBank(C.bank_meshes(K), C.CLASSES, device=gpu)
            for name in ("vertices", "normals", "colors", "uvs", "faces", "textures"):
                setattr(bank, name, g.embed(getattr(bank, name), "cuda"))
            batch = syn.render_scenes(bank, _scenes(scenes, lights), K, H, W, g.embed(bg, "cuda"), (C.Z_NEAR, C.Z_FAR), 1000.0, 100,
                                      want_vertmap)
            torch.cuda.synchronize()
            g.check()
            assert sum(a.kind == "empty" for a in g.arenas) == (7 if want_vertmap else 6)      # outputs + workspace
            runs[p] = _numpy(batch)
            calls |= set(rec.calls)
    memguard.compare_patterns(runs)
    assert {"pcnn_synth_scene_workspace_bytes", "pcnn_synth_scene_fwd"} <= calls
    assert_same(runs["P1"], C.main_reference(H, W, True), [n for n in NAMES if want_vertmap or n != "vertmap"])


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_training_step_fed_from_a_rendered_batch(gpu):
    """Two scenes at 160 x 208 -> SceneBatch.feed -> SolverWrapper.train_step: the label map, the frames and the tables
    never leave the device; the tables equal datasets.training_blobs of the downloaded frames bit for bit."""
    import torch
    from posecnn_amd import datasets, train
    from posecnn_amd.networks import vgg16_convs
    H, W = 160, 208
    K = C.intrinsics(H, W)
    P = S.pose
    scenes = [[(0, P(S.rot((1, 2, 0.5), 0.7), (-0.08, -0.02, 0.5)), 50), (1, P(S.rot((0, 1, 0), 0.3), (0.09, 0.03, 0.55)), 100)],
              [(4, P(S.rot((1, 0, 1), 0.4), (0.1, -0.05, 0.6)), 40), (3, P(S.rot((0, 1, 1), 0.9), (-0.07, 0.04, 0.45)), 80),
               (2, P(S.rot((1, 1, 0), 2.0), (0.0, 0.09, 0.5)), 120)]]
    lights = np.asarray([[0.5, -1.0, 0.0, 1.2], [-1.5, 0.7, 0.0, 0.9]], F)
    bg = C.backgrounds(2, H, W)
    want = R.render_scenes(C.bank_meshes(K), C.ref_instances(scenes), lights, C.K4(K), H, W, C.Z_NEAR, C.Z_FAR, 1000.0, 500, bg)
    assert want["valid"].tolist() == [1, 1] and (want["pixel_counts"] >= 500).all()
    batch = render(gpu, _bank(H, W, gpu), scenes, lights, K, H, W, bg, min_pixels=500)
    assert_same(_numpy(batch), want)

    points = synth.make_model_points(22, 64)
    feed = batch.feed(config.LOV_EXTENTS, points, config.LOV_SYMMETRY)
    assert feed["gt_label_2d"] is batch.label and feed["data"].dtype == torch.uint8
    blobs = datasets.training_blobs(batch.frames(points), 22)
    for k in ("gt_label_2d", "vertex_objects", "poses", "meta_data"):
        g = feed[k].cpu().numpy()
        assert g.dtype == blobs[k].dtype and g.shape == blobs[k].shape and g.tobytes() == blobs[k].tobytes(), k

    torch.manual_seed(0)
    net = vgg16_convs("COLOR", 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=True, is_train=True,
                      device=gpu, seed=3, init="he")

    class Cfg(train.TrainConfig):
        LEARNING_RATE = 1e-6

    solver = train.SolverWrapper(net, Cfg)
    losses = solver.train_step(feed)
    for k in ("loss", "loss_cls", "loss_vertex", "loss_pose", "loss_regu"):
        assert np.isfinite(losses[k]), (k, losses)
    assert losses["loss_vertex"] > 0
    assert net.get_output("rois").shape[0] >= 5      # is_train: at least one ROI per object of the two scenes
    # the same step from the host-built blobs of the downloaded frames reads the same label / table bits
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    again = solver.train_step(dict(feed, **{k: t(blobs[k]) for k in ("gt_label_2d", "vertex_objects", "poses", "meta_data")}))
    assert all(np.isfinite(v) for v in again.values())
    for k in ("gt_label_2d", "vertex_objects", "poses", "meta_data"):
        assert torch.equal(net.get_output(k), feed[k]), k


# ---- depth ties inside one mesh -------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_is_red", [True, False])
def test_coplanar_faces_go_to_the_lower_face(gpu, first_is_red):
    from posecnn_amd import synthesize as syn
    H, W = C.SIZES[0]
    K = C.intrinsics(H, W)
    mesh = C.coplanar_mesh(K, first_is_red)
    scenes, lights = [[(0, S.pose(np.eye(3), (0, 0, 0)), 40)]], np.asarray([[0, 0, 0, 1]], F)
    want = R.render_scenes([mesh], [[(0, 1, scenes[0][0][1], 40)]], lights, C.K4(K), H, W, C.Z_NEAR, C.Z_FAR, 1000.0, 10)
    got = _numpy(render(gpu, syn.MeshBank([mesh], (1,), device=gpu), scenes, lights, K, H, W, min_pixels=10))
    assert_same(got, want)
    bgr = got["color"][0][got["label"][0] == 1][:, :3]
    assert len(bgr) > 20 and (bgr[:, 2 if first_is_red else 0] > 0).all() and (bgr[:, 0 if first_is_red else 2] == 0).all()


# ---- the SYN_ONLINE iterator ----------------------------------------------------------------------------------------
class _ScriptedSampler:
    def __init__(self, scenes):
        self.scenes, self.drawn = list(scenes), 0

    def sample(self):
        self.drawn += 1
        return self.scenes.pop(0)


def test_synthetic_minibatches_redraws_only_the_invalid_scene(gpu):
    """Scene 1 of the first draw has an object outside the image (0 pixels < min_pixels): it alone is drawn and rendered
    again, over its own background; the batch that comes out is the render of [scene 0, the re-drawn scene]."""
    import torch
    from posecnn_amd import synthesize as syn
    H, W = 112, 160
    K = C.intrinsics(H, W)
    P = S.pose
    a = ([(0, P(S.rot((1, 2, 0.5), 0.7), (-0.05, -0.01, 0.5)), 50), (1, P(S.rot((0, 1, 0), 0.3), (0.08, 0.02, 0.55)), 100)], [0.5, -1.0, 0.0, 1.2])
    b = ([(4, P(S.rot((1, 0, 1), 0.4), (0.0, 0.0, 0.6)), 40), (3, P(np.eye(3), (2.0, 0.0, 0.6)), 80)], [0.0, 0.0, 0.0, 1.0])
    c = ([(4, P(S.rot((1, 0, 1), 0.4), (0.05, 0.0, 0.6)), 40), (3, P(S.rot((0, 1, 1), 0.9), (-0.07, 0.02, 0.45)), 80),
          (2, P(S.rot((1, 1, 0), 2.0), (0.0, -0.06, 0.5)), 120)], [-1.5, 0.7, 0.0, 0.9])
    sampler = _ScriptedSampler(syn.Scene(*x) for x in (a, b, c))
    bg = C.backgrounds(2, H, W)
    bg_t = torch.from_numpy(bg).to(gpu)
    calls = []
    real = syn.render_scenes

    def counting(bank, scenes, *args, **kw):
        calls.append(len(scenes))
        return real(bank, scenes, *args, **kw)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(syn, "render_scenes", counting)
        it = syn.synthetic_minibatches(_bank(H, W, gpu), sampler, K, H, W, 2, config.LOV_EXTENTS, synth.make_model_points(22, 16),
                                       config.LOV_SYMMETRY, backgrounds=lambda n: bg_t, rgbd=True, min_pixels=100, depth_range=(C.Z_NEAR, C.Z_FAR))
        feed, batch = next(it)
    torch.cuda.synchronize()
    assert calls == [2, 1] and sampler.drawn == 3 and batch.redraws == 1
    want = R.render_scenes(C.bank_meshes(K), C.ref_instances([a[0], c[0]]), np.asarray([a[1], c[1]], F), C.K4(K), H, W, C.Z_NEAR, C.Z_FAR,
                           1000.0, 100, bg)
    assert want["valid"].tolist() == [1, 1]
    assert_same(_numpy(batch), want, [n for n in NAMES if n != "vertmap"])
    assert feed["gt_label_2d"] is batch.label and feed["data_p"] is batch.depth
    assert np.array_equal(feed["data"].cpu().numpy(), want["color"][..., :3])
    assert tuple(feed["vertex_objects"].shape) == (2, 3, 6) and tuple(feed["poses"].shape) == (5, 13)
    assert feed["poses"][:, 1].cpu().tolist() == [1, 2, 5, 4, 3]


# ---- the reference's call -------------------------------------------------------------------------------------------
def test_render_python_binds_the_reference_training_script(gpu, tmp_path):
    """Synthesizer(model_file, pose_file).render_python with the arrays of tools/train_net.py:176-196, then the script's
    own conversions (:198-232): they give back the rendered bytes, the uint16 depth, the label and the vertex map."""
    from posecnn_amd import icp, synthesize as syn
    try:
        import PIL  # noqa: F401
        textured = True
    except ImportError:
        textured = False
    model_file, pose_file, _ = C.write_model_and_pose_files(str(tmp_path), textured)
    H, W = C.SIZES[0]
    K = C.intrinsics(H, W)
    znear, zfar, factor_depth, num_classes = 0.25, 6.0, 1000.0, 3
    parameters = np.asarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2], znear, zfar, 0.5, 2.0], F)
    synthesizer = icp.Synthesizer(model_file, pose_file, device=gpu)
    synthesizer.synthesis_seed = 9
    synthesizer.setup(W, H)
    im_syn, depth_syn, vertmap_syn = np.zeros((H, W, 4), F), np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
    class_indexes, poses, centers = -1 * np.ones((num_classes,), F), np.zeros((num_classes, 7), F), np.zeros((num_classes, 2), F)
    synthesizer.render_python(W, H, parameters, im_syn, depth_syn, vertmap_syn, class_indexes, poses, centers, False, True)

    # the script, verbatim in what it computes
    im = np.clip(255 * im_syn, 0, 255).astype(np.uint8)
    d = depth_syn[:, :, 0]
    im_depth_raw = factor_depth * 2 * zfar * znear / (zfar + znear - (zfar - znear) * (2 * d - 1))
    im_depth_raw[d == 1] = 0
    label = np.round(vertmap_syn[:, :, 0]) + 1
    label[np.isnan(label)] = 0
    vm = vertmap_syn.copy()
    vm[:, :, 0] = vm[:, :, 0] - np.round(vm[:, :, 0])
    vm[np.isnan(vm)] = 0

    # the same scene from an identically seeded sampler, on the restatement, with the models as the OBJ reader gives them
    models = [syn.TexturedMesh.load_obj("%s/model%d.obj" % (tmp_path, i)) for i in range(3)]
    assert (models[1].texture is not None) == textured and models[0].colors is not None
    scene = syn.SceneSampler(3, 9, 0.5, 2.0, False, True, syn.SceneSampler.load_pose_table(pose_file)).sample()
    ref_meshes = [{k: getattr(m, k) for k in ("vertices", "normals", "faces", "colors", "uvs", "texture") if getattr(m, k) is not None}
                  for m in models]
    want = R.render_scenes(ref_meshes, [[(m, m + 1, T, sh) for m, T, sh in scene.instances]], [scene.light], C.K4(K), H, W, znear, zfar,
                           factor_depth, 1)
    assert (want["pixel_counts"] > 100).all()
    assert np.array_equal(im, want["color"][0])
    assert np.array_equal(im_depth_raw.astype(np.uint16), want["depth"][0])
    assert np.array_equal(label.astype(np.int32), want["label"][0])
    # y, z exactly; x passed through `x + class index` in float32, as in the reference's shader: half an ulp of [2, 4)
    assert np.array_equal(vm[:, :, 1:], want["vertmap"][0][:, :, 1:])
    assert np.abs(vm[:, :, 0] - want["vertmap"][0][:, :, 0]).max() <= 2.0 ** -23
    assert class_indexes.tolist() == [0, 1, 2]
    for i, (m, T, _) in enumerate(scene.instances):
        assert np.allclose(poses[i, 4:], T[:, 3], atol=1e-6) and abs(np.linalg.norm(poses[i, :4]) - 1) < 1e-6
        assert np.allclose(centers[m], (K[0, 0] * T[0, 3] / T[2, 3] + K[0, 2], K[1, 1] * T[1, 3] / T[2, 3] + K[1, 2]), atol=1e-3)
