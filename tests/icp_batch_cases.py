"""Scenes for the batched pose refinement (TEST INFRASTRUCTURE): two batches built from tests/icp_scene.py meshes through the CPU
checker's renderer, their rows covering every row kind `icp.refine_batch` distinguishes, and the CPU restatement of each
(tests/icp_batch_ref.py), computed once per process.

  "small": B = 2 frames of 100 x 131 (odd width, 13 100 pixels: not a multiple of the 256-pixel reduction block), each frame
           with its own intrinsics, min_pixels lowered to 150 to fit the frame.
  "large": B = 1 frame of 240 x 320 under the reference's min_pixels = 400 (frame sizes do not mix within a batch).
KINDS maps a row kind to (batch, row)."""
import functools

import numpy as np

import icp_batch_ref as ref
import icp_scene as S
from posecnn_amd import config

F = np.float32
FACTOR = 10000.0
OPTIONS = dict(max_error=0.01, iterations=8, polish_evaluations=50, radius=0.01, depth_range=(0.25, 6.0))


@functools.lru_cache(maxsize=None)
def meshes():
    """class 1: ellipsoid, class 2: box, class 3: small sphere — (vertices, normals, faces) each"""
    return (S.icosphere(0.05, 2, scale=(1.0, 0.7, 1.3)), S.box_mesh((0.05, 0.04, 0.03)), S.icosphere(0.03, 2))


def intrinsics(W, fscale=1.0, shift=(0.0, 0.0)):
    K = config.DEMO_INTRINSICS.copy()
    K[:2] *= W / 640.0
    return np.array([K[0, 0] * fscale, K[1, 1] * fscale, K[0, 2] + shift[0], K[1, 2] + shift[1]], F)


def _K(intr):
    return np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float64)


def frame(intr, H, W, placed):
    """depth uint16 / label int32 of the objects `placed` = [(class id, T_true)], later ones in front"""
    import oracle
    depth, label = np.zeros((H, W), np.uint16), np.zeros((H, W), np.int32)
    K = _K(intr)
    for cls, T in placed:
        v, n, f = meshes()[cls - 1]
        d, l = S.depth_scene_from_mesh(lambda P: oracle.render_mesh(v, n, f, P, K, H, W, want=("vertices",))["vertices"], T, K, H, W,
                                       factor=FACTOR, obj_id=cls)
        depth = np.where(l > 0, d, depth).astype(np.uint16)
        label = np.where(l > 0, l, label).astype(np.int32)
    return depth, label


def pose_row(T):
    from posecnn_amd import icp
    return np.concatenate([icp.mat2quat(T[:, :3]), T[:, 3]]).astype(F)


def estimate(T, axis, angle, dz):
    """the network's pose for a truth T: a small rotation off and dz further along the viewing ray"""
    return S.pose(S.rot(axis, angle) @ T[:, :3], T[:, 3] * (1 + dz / T[2, 3]))


def _rows(entries, dead=2):
    """entries: [(frame, class id, pose row or None)] -> rois f32 [R,7], poses f32 [R,7], count; `dead` rows of NaN and huge
    class ids follow the live ones"""
    R = len(entries) + dead
    rois, poses = np.zeros((R, 7), F), np.zeros((R, 7), F)
    for r, (fr, cls, row) in enumerate(entries):
        rois[r, 0], rois[r, 1] = fr, cls
        rois[r, 2:6] = (1, 2, 30, 40)
        if row is not None:
            poses[r] = row
    rois[len(entries):] = np.nan
    rois[len(entries):, 1] = 3e9
    rois[len(entries):, 0] = 1e9
    poses[len(entries):] = np.nan
    return rois, poses, len(entries)


@functools.lru_cache(maxsize=None)
def small():
    H, W = 100, 131
    intr = np.stack([intrinsics(W), intrinsics(W, 1.03, (1.5, -1.0))])
    t = {  # truths
        (0, 1): S.pose(S.rot([0.3, 1, 0.2], 0.7), [-0.07, 0.01, 0.7]),
        (0, 2): S.pose(S.rot([1, 0.4, 0.1], 1.0), [0.08, -0.02, 0.8]),
        (1, 1): S.pose(S.rot([0.1, 1, 0.5], -0.4), [0.07, -0.03, 0.75]),
        (1, 2): S.pose(S.rot([1, 0.2, 0.3], 0.8), [-0.07, 0.0, 0.7]),
        (1, 3): S.pose(np.eye(3), [0.0, 0.2, 1.5]),
    }
    frames = [frame(intr[0], H, W, [(1, t[0, 1]), (2, t[0, 2])]), frame(intr[1], H, W, [(1, t[1, 1]), (2, t[1, 2]), (3, t[1, 3])])]
    far = t[1, 2].copy()
    far[:, 3] *= 1 + 0.3 / 0.7                      # 30 cm behind the depth along the ray: overlaps the label, agrees nowhere
    aside = t[1, 2].copy()
    aside[0, 3] += 0.25                             # rendered off to the side: no pixel shared with the label
    at_zero = pose_row(t[0, 1])
    at_zero[4:] = 0                                 # t_z == 0: nothing is rendered in front of z_near
    entries = [
        (0, 1, pose_row(estimate(t[0, 1], [0, 1, 0], 0.02, 0.02))),       # 0 live
        (0, 2, pose_row(estimate(t[0, 2], [1, 0, 0], -0.03, 0.03))),      # 1 live, another class of the same frame
        (1, 1, pose_row(estimate(t[1, 1], [0, 0, 1], 0.02, -0.015))),     # 2 the class of row 0, live in the other frame
        (0, 1, pose_row(estimate(t[0, 1], [1, 1, 0], -0.02, 0.01))),      # 3 duplicate of row 0's frame and class
        (0, 0, None),                                                      # 4 background
        (1, 3, pose_row(t[1, 3])),                                         # 5 under min_pixels
        (1, 7, pose_row(t[1, 1])),                                         # 6 class id beyond the bank
        (1, 2, pose_row(far)),                                             # 7 agree == 0, pairs > 0
        (1, 2, pose_row(aside)),                                           # 8 pairs == 0
        (0, 1, at_zero),                                                   # 9 t_z == 0
    ]
    rois, poses, count = _rows(entries)
    return dict(labels=np.stack([f[1] for f in frames]), depth=np.stack([f[0] for f in frames]), intrinsics=intr, factor=FACTOR,
                rois=rois, poses=poses, count=count, min_pixels=150, truths=t)


@functools.lru_cache(maxsize=None)
def large():
    H, W = 240, 320
    intr = intrinsics(W)[None]
    t = {(0, 1): S.pose(S.rot([0.3, 1, 0.2], 0.7), [-0.08, 0.015, 0.7]), (0, 2): S.pose(S.rot([1, 0.4, 0.1], 1.0), [0.09, -0.02, 0.8]),
         (0, 3): S.pose(np.eye(3), [0.0, 0.11, 1.5])}
    depth, label = frame(intr[0], H, W, [(1, t[0, 1]), (2, t[0, 2]), (3, t[0, 3])])
    entries = [(0, 1, pose_row(estimate(t[0, 1], [0, 1, 0], 0.02, 0.02))), (0, 2, pose_row(estimate(t[0, 2], [1, 0, 0], -0.03, 0.03))),
               (0, 3, pose_row(t[0, 3])), (0, 0, None)]
    rois, poses, count = _rows(entries, dead=1)
    return dict(labels=label[None], depth=depth[None], intrinsics=intr, factor=FACTOR, rois=rois, poses=poses, count=count,
                min_pixels=400, truths=t)


BATCHES = {"small": small, "large": large}
KINDS = {
    "live": ("small", 0), "other class, same frame": ("small", 1), "same class, other frame": ("small", 2),
    "duplicate": ("small", 3), "background": ("small", 4), "under min_pixels": ("small", 5), "beyond the bank": ("small", 6),
    "agree == 0": ("small", 7), "pairs == 0": ("small", 8), "t_z == 0": ("small", 9), "dead": ("small", 10),
    "live at 400": ("large", 0), "under 400": ("large", 2),
}
STATUS = {"small": [1, 1, 1, 1, 2, 3, 4, 1, 1, 1, 0, 0], "large": [1, 1, 3, 2, 0]}


@functools.lru_cache(maxsize=None)
def reference(name, max_jobs=None):
    """(poses_new, poses_icp, info, extras) of tests/icp_batch_ref.py for a batch: computed once, never modified"""
    b = BATCHES[name]()
    out = ref.refine_batch(b["labels"], b["depth"], b["intrinsics"], b["factor"], b["rois"], b["poses"], b["count"], meshes(),
                           min_pixels=b["min_pixels"], max_jobs=max_jobs, **OPTIONS)
    for a in out[:3]:
        a.setflags(write=False)
    return out


# ---- on the device ----------------------------------------------------------------------------------------------------------
def bank(device):
    from posecnn_amd import icp
    return icp.MeshBank([icp.Mesh(m[0], m[2], m[1], device=device) for m in meshes()], device)


def device_args(b, device, put=None):
    """(labels, depth, intrinsics, factor, rois, poses, count) of a batch as device tensors (`put(array)`: another way in)"""
    import torch
    put = put or (lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).to(device))
    depth = put(b["depth"])
    if depth.dtype == torch.int16:
        depth = depth.view(torch.uint16)
    return (put(b["labels"]), depth, put(b["intrinsics"]), b["factor"], put(b["rois"]), put(b["poses"]),
            put(np.array([b["count"]], np.int32)))


def run(b, device, bank_, **overrides):
    from posecnn_amd import icp
    opts = dict(OPTIONS, min_pixels=b["min_pixels"])
    opts.update(overrides)
    return icp.refine_batch(*device_args(b, device), bank_, **opts)


# ---- the memory-contract case of pcnn_icp_batch_fwd (run under guard bands by tests/test_gpu_icp_batch.py) -------------------------
def contract_make():
    return dict(small())


def contract_run(c):
    from posecnn_amd import icp
    b = c.d
    m = meshes()
    bk = icp.MeshBank([icp.Mesh(x[0], x[2], x[1], device="cpu") for x in m], "cpu")
    for key in ("vertices", "normals", "faces", "vertex_offsets", "face_offsets"):
        setattr(bk, key, c.e(getattr(bk, key).numpy()))
    bk.device = bk.vertices.device
    out = icp.refine_batch(c.e(b["labels"]), c.e(b["depth"]), c.e(b["intrinsics"]), b["factor"], c.e(b["rois"]), c.e(b["poses"]),
                           c.e(np.array([b["count"]], np.int32)), bk, min_pixels=b["min_pixels"], **OPTIONS)
    return dict(poses_new=out.poses_new, poses_icp=out.poses_icp, info=out.info)


def contract_check(d, o):
    want = reference("small")
    for key, w in zip(("poses_new", "poses_icp", "info"), want):
        assert np.array_equal(o[key].view(np.uint32), w.view(np.uint32)), key
