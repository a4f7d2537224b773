"""Synthetic training scenes on the device (cfg.TRAIN.SYN_ONLINE of the reference): the render thread of
tools/train_net.py:155-258 — `Synthesizer::render` (lib/synthesize/synthesize.cpp:345-609, OpenGL) followed by the
background paste of lib/gt_synthesize_layer/minibatch.py:113-154 — as one library call per minibatch:

    bank    = MeshBank(meshes, classes)                          models resident on the GPU
    sampler = SceneSampler(num_classes, seed)                    synthesize.cpp:359-482,498 on a numpy Generator
    batch   = render_scenes(bank, [sampler.sample() ...], K, H, W, background)     pcnn_synth_scene_fwd
    feed    = batch.feed(extents, points, symmetry)              label map, frames and tables stay on the device
    for feed, batch in synthetic_minibatches(...): solver.train_step(feed)

The kernel's arithmetic (posecnn_amd/csrc/synth_scene.hip) is this library's own: GL's rasteriser, texture filter and `pow`
have no reproducible bits. `chromatic_transform` and `add_noise` of minibatch.py:170-175 run on the device as well
(`feed(..., augment=AugmentSampler(...))`, posecnn_amd/augment.py, one `ops.augment_frames` call). Only the random flip of
minibatch.py:177-178 is absent: the followed configuration, experiments/cfgs/lov_color_2d.yml:19-21, sets USE_FLIPPED: False,
so the reference never trains on a flipped frame.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import ops
from ._lib import check, lib
from .config import make_meta_data
from .datasets import MAX_VERTEX_OBJECTS, mat2quat
from .pose_error import quat2mat


def call(name, *args):
    """`_lib.call` with the handle taken from this module's `lib` (see ops.call)."""
    check(name, getattr(lib(), name)(*args))


MAX_INSTANCES = 32                 # PCNN_SYNTH_MAX_INSTANCES
Z_NEAR, Z_FAR = 0.25, 6.0          # tools/train_net.py:166-167
FACTOR_DEPTH = 1000.0              # tools/train_net.py:170
MIN_PIXELS = 800                   # tools/train_net.py:224


def _np(mesh, name):
    """An attribute of an `icp.Mesh`, a `TexturedMesh` or a dict as a numpy array (None when absent)."""
    if isinstance(mesh, dict):
        v = mesh.get(name)
    else:
        v = getattr(mesh, name + "_np", None)
        if v is None:
            v = getattr(mesh, name, None)
    if v is None:
        return None
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


class TexturedMesh:
    """A model with per-vertex texture coordinates and its `map_Kd` image, or vertex colours (host arrays)."""

    def __init__(self, vertices, faces, normals, uvs=None, texture=None, colors=None):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        self.uvs = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 2)
        self.colors = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(-1, 3)
        self.texture = None if texture is None else np.ascontiguousarray(texture, dtype=np.uint8)

    @classmethod
    def load_obj(cls, path):
        """Wavefront OBJ with `v` (optionally `v x y z r g b`), `vt`, `vn`, `f` and `mtllib` records. Smooth normals are
        generated on the POSITIONS first (aiProcess_GenSmoothNormals, synthesize.cpp:199) unless every corner's normal
        index equals its position index; then the corners whose (v, vt) pairs differ are split into vertices of their
        own. The material's `map_Kd` image is loaded through PIL."""
        from .icp import Mesh
        vs, cols, vts, vns, corners, nidx_ok, mtllib = [], [], [], [], [], True, None
        with open(path) as fh:
            for line in fh:
                t = line.split()
                if not t:
                    continue
                if t[0] == "v":
                    vs.append([float(x) for x in t[1:4]])
                    if len(t) >= 7:
                        cols.append([float(x) for x in t[4:7]])
                elif t[0] == "vt":
                    vts.append([float(x) for x in t[1:3]])
                elif t[0] == "vn":
                    vns.append([float(x) for x in t[1:4]])
                elif t[0] == "mtllib":
                    mtllib = line.split(None, 1)[1].strip()
                elif t[0] == "f":
                    idx = []
                    for c in t[1:]:
                        parts = c.split("/")
                        vi = int(parts[0])
                        vi = vi - 1 if vi > 0 else len(vs) + vi
                        ti = -1
                        if len(parts) >= 2 and parts[1]:
                            ti = int(parts[1])
                            ti = ti - 1 if ti > 0 else len(vts) + ti
                        if len(parts) >= 3 and parts[2]:
                            ni = int(parts[2])
                            ni = ni - 1 if ni > 0 else len(vns) + ni
                            nidx_ok = nidx_ok and ni == vi
                        else:
                            nidx_ok = False
                        idx.append((vi, ti))
                    for k in range(1, len(idx) - 1):
                        corners.append([idx[0], idx[k], idx[k + 1]])
        v = np.asarray(vs, dtype=np.float32).reshape(-1, 3)
        pos_faces = np.asarray([[c[0] for c in tri] for tri in corners], dtype=np.int32).reshape(-1, 3)
        if pos_faces.size and (pos_faces.min() < 0 or pos_faces.max() >= len(v)):
            raise ValueError("%s: face index out of range" % path)
        n = np.asarray(vns, dtype=np.float32) if (nidx_ok and vns and len(vns) == len(vs)) else Mesh.smooth_normals(v, pos_faces)
        colors = np.asarray(cols, dtype=np.float32) if cols and len(cols) == len(vs) else None
        has_uv = bool(vts) and all(c[1] >= 0 for tri in corners for c in tri)
        if not has_uv:
            return cls(v, pos_faces, n, None, None, colors)
        remap, src, uv, faces = {}, [], [], []
        for tri in corners:
            row = []
            for key in tri:
                if key not in remap:
                    remap[key] = len(src)
                    src.append(key[0])
                    uv.append(vts[key[1]])
                row.append(remap[key])
            faces.append(row)
        src = np.asarray(src, dtype=np.int64)
        texture = None
        if mtllib is not None:
            texture = cls._load_map_kd(os.path.join(os.path.dirname(path), mtllib))
        return cls(v[src], faces, n[src], uv, texture, None if colors is None else colors[src])

    @staticmethod
    def _load_map_kd(mtl_path):
        name = None
        with open(mtl_path) as fh:
            for line in fh:
                t = line.split(None, 1)
                if len(t) == 2 and t[0] == "map_Kd":
                    name = t[1].strip()
        if name is None:
            return None
        try:
            from PIL import Image
        except ImportError:
            raise RuntimeError("TexturedMesh.load_obj: %s names the texture %r and PIL (Pillow) is not installed" % (mtl_path, name))
        with Image.open(os.path.join(os.path.dirname(mtl_path), name)) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


class MeshBank:
    """The models of a training run pooled into the arrays `pcnn_synth_scene_fwd` reads (include/posecnn_hip_synth.h).
    meshes: `icp.Mesh`, `TexturedMesh` or dicts (vertices, normals, faces; optional colors, uvs, texture);
    classes: the class id (1..C-1) of each mesh, default 1, 2, ..."""

    def __init__(self, meshes, classes=None, device="cuda"):
        self.device = torch.device(device)
        self.classes = [int(c) for c in (classes if classes is not None else range(1, len(meshes) + 1))]
        if len(self.classes) != len(meshes):
            raise ValueError("MeshBank: one class id per mesh")
        V, Nn, Cc, U, Fc, tex = [], [], [], [], [], []
        self.meshes_np = []
        table, ttable = np.zeros((len(meshes), 4), np.int32), np.zeros((len(meshes), 3), np.int32)
        nv = nf = nt = 0
        any_col = any(_np(m, "colors") is not None for m in meshes)
        for i, m in enumerate(meshes):
            v = np.ascontiguousarray(_np(m, "vertices"), dtype=np.float32).reshape(-1, 3)
            f = np.ascontiguousarray(_np(m, "faces"), dtype=np.int32).reshape(-1, 3)
            n = np.ascontiguousarray(_np(m, "normals"), dtype=np.float32).reshape(-1, 3)
            if n.shape != v.shape:
                raise ValueError("MeshBank: mesh %d needs one normal per vertex" % i)
            if f.size and (f.min() < 0 or f.max() >= len(v)):
                raise ValueError("MeshBank: mesh %d has a face index out of range" % i)
            c, uv, t = _np(m, "colors"), _np(m, "uvs"), _np(m, "texture")
            d = {"vertices": v, "normals": n, "faces": f}
            if t is not None and uv is not None:
                t = np.ascontiguousarray(t, dtype=np.uint8)
                if t.ndim != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                    raise ValueError("MeshBank: mesh %d: texture must be uint8 [h,w,3]" % i)
                uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
                if len(uv) != len(v):
                    raise ValueError("MeshBank: mesh %d needs one uv per vertex" % i)
                ttable[i] = (nt, t.shape[0], t.shape[1])
                tex.append(t.reshape(-1))
                nt += t.size + (-t.size) % 16
                tex.append(np.zeros((-t.size) % 16, np.uint8))
                d["uvs"], d["texture"] = uv, t
            else:
                uv = np.zeros((len(v), 2), np.float32)
                if c is not None:
                    d["colors"] = np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3)
            c = np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3) if c is not None else np.ones((len(v), 3), np.float32)
            if len(c) != len(v):
                raise ValueError("MeshBank: mesh %d needs one colour per vertex" % i)
            table[i] = (nv, len(v), nf, len(f))
            V.append(v); Nn.append(n); Cc.append(c); U.append(uv); Fc.append(f)
            nv += len(v); nf += len(f)
            self.meshes_np.append(d)
        cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dt)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.num_vertices, self.num_faces, self.texture_bytes = nv, nf, nt
        self.vertices, self.normals = up(cat(V, (0, 3), np.float32)), up(cat(Nn, (0, 3), np.float32))
        self.faces = up(cat(Fc, (0, 3), np.int32))
        self.colors = up(cat(Cc, (0, 3), np.float32)) if any_col else None
        self.uvs = up(cat(U, (0, 2), np.float32)) if nt else None
        self.textures = up(np.concatenate(tex)) if nt else None
        self.mesh_table, self.texture_table = table, (ttable if nt else None)

    def __len__(self):
        return len(self.classes)


class Scene:
    """One scene: instances = [(mesh index, pose 3x4 camera <- object, integer shininess)], light = (x, y, z, intensity)."""

    def __init__(self, instances, light):
        self.instances = [(int(m), np.asarray(T, dtype=np.float64).reshape(3, 4), int(s)) for m, T, s in instances]
        self.light = np.asarray(light, dtype=np.float32).reshape(4)


def euler_rotation(roll, pitch, yaw):
    """AngleAxis(roll, X) * AngleAxis(pitch, Y) * AngleAxis(yaw, Z) (synthesize.cpp:429-431), angles in degrees."""
    a, b, c = (math.radians(x) for x in (roll, pitch, yaw))
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


class SceneSampler:
    """The sampling of synthesize.cpp:359-482,498 — the distribution, not the reference's random stream — on a seeded
    numpy Generator. `num_classes` counts the MODELS (mesh indices 0..num_classes-1, as `pose_nums_.size()`).
    pose_table: per model an array [k,7] of (quaternion wxyz, translation) rows (`load_pose_table`), for `is_sampling_pose`."""

    def __init__(self, num_classes, seed=0, tnear=0.5, tfar=2.0, is_sampling=True, is_sampling_pose=False, pose_table=None,
                 threshold=0.2):
        self.num_classes, self.rng = int(num_classes), np.random.default_rng(seed)
        self.tnear, self.tfar, self.threshold = float(tnear), float(tfar), float(threshold)
        self.is_sampling, self.is_sampling_pose, self.pose_table = bool(is_sampling), bool(is_sampling_pose), pose_table
        if self.is_sampling_pose and pose_table is None:
            raise ValueError("SceneSampler: is_sampling_pose needs pose_table")
        if self.is_sampling and self.num_classes < 7:
            raise ValueError("SceneSampler: sampling 5..7 distinct classes needs at least 7 models")

    @staticmethod
    def load_pose_table(path):
        """`Synthesizer::loadPoses` (synthesize.cpp:84-126): `path` lists one pose file per model, a line each (a relative
        name is taken from the list's own directory when it does not exist as given); every pose file holds rows of 7
        floats, quaternion (w, x, y, z) and translation. -> list of float64 [k,7] arrays, one per model."""
        base = os.path.dirname(os.path.abspath(path))
        with open(path) as fh:
            names = [line.strip() for line in fh if line.strip()]
        table = []
        for name in names:
            if not os.path.exists(name) and not os.path.isabs(name):
                name = os.path.join(base, name)
            with open(name) as fh:
                values = np.asarray(fh.read().split(), dtype=np.float64)
            if values.size == 0 or values.size % 7:
                raise ValueError("load_pose_table: %s holds %d numbers, not rows of 7" % (name, values.size))
            table.append(values.reshape(-1, 7))
        return table

    def _pose(self, mesh):
        rng = self.rng
        if self.is_sampling_pose:
            tab = np.asarray(self.pose_table[mesh], dtype=np.float64).reshape(-1, 7)
            row = tab[int(rng.integers(0, len(tab)))]
            q = row[:4] + rng.uniform(-0.2, 0.2, 4)
            t = row[4:] + rng.uniform(-0.1, 0.1, 3)
            return quat2mat(q / np.linalg.norm(q)), t          # Sophus normalises the quaternion
        R = euler_rotation(*rng.uniform(0, 360, 3))
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(self.tnear, self.tfar)])
        return R, t

    def sample(self):
        rng = self.rng
        if self.is_sampling:
            num = int(rng.integers(5, 8))                       # irand(5, 8) = 5..7
            ids = [int(c) for c in rng.choice(self.num_classes, size=num, replace=False)]
        else:
            ids = list(range(self.num_classes))
        placed, instances = [], []
        for m in ids:
            while True:
                R, t = self._pose(m)
                if all(np.linalg.norm(p - t) >= self.threshold for p in placed):
                    break
            placed.append(t)
            instances.append([m, np.concatenate([R, t[:, None]], axis=1)])
        intensity = rng.uniform(0.5, 2.0)
        light = (rng.uniform(-2, 2), rng.uniform(-2, 2), 0.0, intensity)
        return Scene([(m, T, int(rng.integers(40, 121))) for m, T in instances], light)


class SceneBatch:
    """The device tensors of one `render_scenes` call and the few host rows they were rendered from."""

    def __init__(self, bank, scenes, K, height, width, factor_depth, color, depth, label, vertmap, pixel_counts, valid):
        self.bank, self.scenes, self.K = bank, scenes, np.asarray(K, dtype=np.float64)
        self.height, self.width, self.factor_depth = height, width, float(factor_depth)
        self.color, self.depth, self.label, self.vertmap = color, depth, label, vertmap
        self.pixel_counts, self.valid = pixel_counts, valid

    def _rows_meta(self, scene):
        """train_net.py:206-214, synthesize.cpp:552-563: class ids, poses [3,4,n] float32, float32 centres"""
        n = len(scene.instances)
        K = self.K
        poses = np.zeros((3, 4, n), dtype=np.float32)
        center = np.zeros((n, 2), dtype=np.float32)
        cls = np.zeros((n,), dtype=np.float32)
        for j, (m, T, _) in enumerate(scene.instances):
            poses[:, :, j] = T
            t = T[:, 3].astype(np.float32)
            center[j] = (np.float32(K[0, 0]) * (t[0] / t[2]) + np.float32(K[0, 2]), np.float32(K[1, 1]) * (t[1] / t[2]) + np.float32(K[1, 2]))
            cls[j] = self.bank.classes[m]
        return {"cls_indexes": cls, "poses": poses, "center": center}

    def _meta(self, scene, points=None):
        """The frame's meta dict (train_net.py:234-255): the rows above + box, intrinsic_matrix, factor_depth"""
        meta = self._rows_meta(scene)
        K = self.K
        box = np.zeros((len(scene.instances), 4), dtype=np.float32)
        for j, (m, T, _) in enumerate(scene.instances):
            pts = self.bank.meshes_np[m]["vertices"] if points is None else np.asarray(points[self.bank.classes[m]], dtype=np.float32)
            x3d = np.ones((4, len(pts)), dtype=np.float32)
            x3d[:3] = pts.T
            x2d = np.matmul(K, np.matmul(meta["poses"][:, :, j], x3d))
            if x2d.shape[1]:
                box[j] = ((x2d[0] / x2d[2]).min(), (x2d[1] / x2d[2]).min(), (x2d[0] / x2d[2]).max(), (x2d[1] / x2d[2]).max())
        meta.update(box=box, intrinsic_matrix=K.copy(), factor_depth=self.factor_depth)
        return meta

    def frames(self, points=None):
        """Download: the frame dicts `datasets.training_blobs` takes (color BGR uint8, depth uint16, label int32, meta);
        `box` from `points[cls]` (train_net.py:234-250) or, without `points`, from the mesh's own vertices."""
        color = self.color.cpu().numpy()
        depth = self.depth.view(torch.int16).cpu().numpy().view(np.uint16)
        label = self.label.cpu().numpy()
        return [{"index": "syn/%06d" % i, "color": np.ascontiguousarray(color[i, :, :, :3]), "depth": depth[i], "label": label[i],
                 "meta": self._meta(sc, points)} for i, sc in enumerate(self.scenes)]

    def tables(self, w_inside=10.0):
        """`vertex_objects`, `poses`, `meta_data` of `datasets.training_blobs(self.frames(), C)` from the sampler's rows
        alone (numpy; nothing is downloaded)."""
        tabs, rows = [], []
        for i, sc in enumerate(self.scenes):
            meta = self._rows_meta(sc)
            n = len(meta["cls_indexes"])
            if n > MAX_VERTEX_OBJECTS:
                raise ValueError("SceneBatch: scene %d has %d objects (at most %d)" % (i, n, MAX_VERTEX_OBJECTS))
            if len(np.unique(meta["cls_indexes"])) < n:
                raise ValueError("SceneBatch: scene %d repeats a class" % i)
            tab = np.zeros((n, 6), dtype=np.float32)
            qt = np.zeros((n, 13), dtype=np.float32)
            poses = meta["poses"].astype(np.float64)
            center = meta["center"].astype(np.float64)
            for j in range(n):
                c = (1.0 * center[j]).astype(np.float32)
                tab[j] = (meta["cls_indexes"][j], 0, c[0], c[1], np.float32(math.log(poses[2, 3, j])), w_inside)
                qt[j, 0], qt[j, 1] = i, meta["cls_indexes"][j]
                qt[j, 6:10] = mat2quat(poses[:, :3, j])
                qt[j, 10:] = poses[:, 3, j]
            tabs.append(tab)
            rows.append(qt)
        B = len(self.scenes)
        M = max([t.shape[0] for t in tabs] + [0])
        objects = np.zeros((B, M, 6), dtype=np.float32)
        for i, t in enumerate(tabs):
            objects[i, :t.shape[0]] = t
        meta_data = np.stack([make_meta_data(self.K, 1.0) for _ in range(B)]).reshape(B, 1, 1, 48) if B else np.zeros((0, 1, 1, 48), np.float32)
        return {"vertex_objects": objects, "poses": np.concatenate(rows, axis=0) if rows else np.zeros((0, 13), np.float32),
                "meta_data": meta_data}

    def replace(self, indices, other):
        """Scene indices[k] of this batch becomes scene k of `other` (same size, same bank): frames copied on the device,
        `pixel_counts` spliced by instance."""
        dev = self.label.device
        index = torch.as_tensor(np.asarray(indices, dtype=np.int64), device=dev)
        for name in ("color", "depth", "label", "vertmap", "valid"):
            mine, theirs = getattr(self, name), getattr(other, name)
            if mine is not None:
                if mine.dtype == torch.uint16:
                    mine, theirs = mine.view(torch.int16), theirs.view(torch.int16)
                mine[index] = theirs
        first = np.concatenate([[0], np.cumsum([len(sc.instances) for sc in self.scenes])])
        ofirst = np.concatenate([[0], np.cumsum([len(sc.instances) for sc in other.scenes])])
        where = {int(i): k for k, i in enumerate(indices)}
        parts = []
        for i in range(len(self.scenes)):
            k = where.get(i)
            parts.append(self.pixel_counts[first[i]:first[i + 1]] if k is None else other.pixel_counts[ofirst[k]:ofirst[k + 1]])
            if k is not None:
                self.scenes[i] = other.scenes[k]
        self.pixel_counts = torch.cat(parts) if parts else self.pixel_counts

    def feed(self, extents, points, symmetry, rgbd=False, keep_prob=1.0, w_inside=10.0, augment=None):
        """The training feed without a download: `gt_label_2d` is the label tensor itself, `data` the BGR bytes of the
        colour frame (a raw uint8 frame: the first-layers kernel forms the blob), `data_p` the uint16 depth frame in the
        RGB-D mode; the object table, the pose rows and the camera rows are built on the host and uploaded.
        augment: an `augment.AugmentSampler`; `data` (and `data_p`) are then the f32 blobs of `ops.augment_frames` on the
        BGRA frame as it is (minibatch.py:170-201: chromatic, noise, minus PIXEL_MEANS; depth over its own maximum), drawn
        with the rows kept in `self.augment_rows`."""
        if self.height % 16 or self.width % 16:
            raise ValueError("SceneBatch.feed: render at a height and width that are multiples of 16 (got %dx%d)" % (self.height, self.width))
        dev = self.label.device
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        tabs = self.tables(w_inside)
        if augment is None:
            data, data_p = self.color[..., :3].contiguous(), self.depth
        else:
            self.augment_rows = augment.sample(len(self.scenes))
            data, data_p = ops.augment_frames(self.color, self.depth if rgbd else None, self.augment_rows, augment.seed)
        feed = {"data": data, "gt_label_2d": self.label, "keep_prob": keep_prob,
                "vertex_objects": t(tabs["vertex_objects"]), "poses": t(tabs["poses"]), "meta_data": t(tabs["meta_data"]),
                "extents": t(extents), "points": t(points), "symmetry": t(symmetry)}
        if rgbd:
            feed["data_p"] = data_p
        return feed


def render_scenes(bank, scenes, K, height, width, background=None, depth_range=(Z_NEAR, Z_FAR), factor_depth=FACTOR_DEPTH,
                  min_pixels=MIN_PIXELS, want_vertmap=True):
    """One `pcnn_synth_scene_fwd`: every scene of the minibatch rendered, lit, composited over `background`
    (uint8 [S,H,W,3] BGR on the device, or None) -> SceneBatch of device tensors. Enqueued on the current stream."""
    dev = bank.device
    S = len(scenes)
    ids, params, lights = [], [], np.zeros((S, 4), np.float32)
    for s, sc in enumerate(scenes):
        lights[s] = sc.light
        for m, T, shin in sc.instances:
            if not 0 <= m < len(bank):
                raise ValueError("render_scenes: scene %d names mesh %d of %d" % (s, m, len(bank)))
            ids.append((s, m, bank.classes[m]))
            params.append(np.concatenate([T.reshape(12), [shin]]))
    N = len(ids)
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(N, 3))
    params = np.ascontiguousarray(np.asarray(params, dtype=np.float32).reshape(N, 13))
    bg = None
    if background is not None:
        bg = ops._dev(background, "background", torch.uint8)
        if tuple(bg.shape) != (S, height, width, 3):
            raise ValueError("background must be uint8 [%d,%d,%d,3]" % (S, height, width))
    color = torch.empty((S, height, width, 4), dtype=torch.uint8, device=dev)
    depth = torch.empty((S, height, width), dtype=torch.uint16, device=dev)
    label = torch.empty((S, height, width), dtype=torch.int32, device=dev)
    vertmap = torch.empty((S, height, width, 3), dtype=torch.float32, device=dev) if want_vertmap else None
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    valid = torch.empty((S,), dtype=torch.int32, device=dev)
    ws, nbytes = ops._workspace(dev, "synth_scene", "pcnn_synth_scene_workspace_bytes", S, height, width)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else ctypes.c_void_p(0)
    K = np.asarray(K, dtype=np.float64)
    call("pcnn_synth_scene_fwd", ops._ptr(bank.vertices), ops._ptr(bank.normals), ops._ptr(bank.colors), ops._ptr(bank.uvs),
         ops._ptr(bank.faces), bank.num_vertices, bank.num_faces, hp(bank.mesh_table), len(bank), ops._ptr(bank.textures),
         bank.texture_bytes, hp(bank.texture_table), hp(ids), hp(params), N, hp(lights), ops._ptr(bg), S, height, width,
         float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), float(depth_range[0]), float(depth_range[1]),
         float(factor_depth), int(min_pixels), ops._ptr(color), ops._ptr(depth), ops._ptr(label), ops._ptr(vertmap),
         ops._ptr(counts), ops._ptr(valid), ops._ptr(ws), nbytes, ops._stream(bank.vertices))
    return SceneBatch(bank, list(scenes), K, height, width, factor_depth, color, depth, label, vertmap, counts, valid)


def synthetic_minibatches(bank, sampler, K, height, width, batch_size, extents, points, symmetry, backgrounds=None, rgbd=False,
                          min_pixels=MIN_PIXELS, depth_range=(Z_NEAR, Z_FAR), factor_depth=FACTOR_DEPTH, max_redraws=100,
                          augment=None):
    """The SYN_ONLINE data path: yields (feed, batch) forever. A scene whose `valid` flag is 0 — an object owns fewer
    than `min_pixels` label pixels — is drawn again, the reference's `continue` (train_net.py:220-228). Cost: one
    read of the `valid` flags per render call (the only host synchronisation of the feed), and only the re-drawn
    scenes are rendered again, over their own backgrounds; their frames replace the invalid ones inside the batch's
    tensors. backgrounds: callable(batch_size) -> uint8 [B,H,W,3] BGR device tensor, or None. `batch.redraws` counts the
    scenes that were drawn again. augment: an `augment.AugmentSampler` for `SceneBatch.feed`, or None (clean renders)."""
    while True:
        scenes = [sampler.sample() for _ in range(batch_size)]
        bg = backgrounds(batch_size) if backgrounds is not None else None
        batch = render_scenes(bank, scenes, K, height, width, bg, depth_range, factor_depth, min_pixels, want_vertmap=False)
        batch.redraws = 0
        for _ in range(max_redraws):
            bad = np.nonzero(batch.valid.cpu().numpy() == 0)[0]
            if not len(bad):
                break
            index = torch.as_tensor(bad, device=batch.label.device)
            fresh = [sampler.sample() for _ in bad]
            part = render_scenes(bank, fresh, K, height, width, bg[index] if bg is not None else None, depth_range, factor_depth,
                                 min_pixels, want_vertmap=False)
            batch.replace(bad, part)
            batch.redraws += len(bad)
        else:
            raise RuntimeError("synthetic_minibatches: no valid batch after %d draws (min_pixels = %d)" % (max_redraws, min_pixels))
        yield batch.feed(extents, points, symmetry, rgbd=rgbd, augment=augment), batch


def online_minibatches(cfg, bank, K, batch_size, extents, points, symmetry, seed=0, pose_table=None, augment_seed=None, **kw):
    """How a trainer selects the path: the reference's switches, `cfg.SYNTHESIZE and cfg.SYN_ONLINE`
    (tools/train_net.py:302), and its `cfg.SYN_*` settings (lib/fcn/config.py:74-88; `train.TrainConfig` carries them)
    -> `synthetic_minibatches` at cfg.SYN_HEIGHT x cfg.SYN_WIDTH. Raises when the switches are off. augment_seed: when given,
    the frames are augmented by `AugmentSampler(augment_seed, cfg.CHROMATIC, cfg.ADD_NOISE)` (lib/fcn/config.py:112-113)."""
    if not (getattr(cfg, "SYNTHESIZE", False) and getattr(cfg, "SYN_ONLINE", False)):
        raise ValueError("online_minibatches: cfg.SYNTHESIZE and cfg.SYN_ONLINE are not both set")
    sampler = SceneSampler(len(bank), seed, cfg.SYN_TNEAR, cfg.SYN_TFAR, cfg.SYN_SAMPLE_OBJECT, cfg.SYN_SAMPLE_POSE, pose_table)
    if augment_seed is not None:
        from .augment import AugmentSampler
        kw["augment"] = AugmentSampler(augment_seed, getattr(cfg, "CHROMATIC", True), getattr(cfg, "ADD_NOISE", False))
    return synthetic_minibatches(bank, sampler, K, cfg.SYN_HEIGHT, cfg.SYN_WIDTH, batch_size, extents, points, symmetry, **kw)
