"""Meshes and scenes shared by tests/test_synth_cpu.py and tests/test_gpu_synth.py (TEST INFRASTRUCTURE). Everything is
seeded and built once per process; nobody modifies what these functions return."""
import functools

import numpy as np

import icp_scene as S
import synth_ref as R
from posecnn_amd import config

F = np.float32
Z_NEAR, Z_FAR = 0.25, 2.0
SIZES = ((120, 160), (101, 131))


def intrinsics(H, W):
    K = config.DEMO_INTRINSICS.copy()
    K[:2] *= W / 640.0
    K[1, 2] = (H - 1) / 2.0 + 0.75
    return K


def K4(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def _sphere_uv(v):
    """longitude / latitude coordinates stretched beyond [0, 1] so that the clamp-to-edge branch is taken"""
    p = v / np.linalg.norm(v, axis=1, keepdims=True)
    u = np.arctan2(p[:, 1], p[:, 0]) / (2 * np.pi) + 0.5
    w = np.arcsin(np.clip(p[:, 2], -1, 1)) / np.pi + 0.5
    return np.stack([u * 1.5 - 0.25, w * 1.4 - 0.2], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def meshes():
    """0 box with vertex colours; 1 icosphere, 1 280 faces, 64 x 32 texture; 2 icosphere, 320 faces, 1 x 1 texture;
    3 box without colours (white); 4 icosphere, 1 280 faces, vertex colours; 5 two triangles whose bounding boxes at the
    identity pose of `box_pixels_scene` are 64 and 65 pixels"""
    rng = np.random.default_rng(11)
    out = []
    v, n, f = S.box_mesh((0.06, 0.04, 0.05))
    out.append(dict(vertices=v, normals=n, faces=f, colors=rng.uniform(0, 1, v.shape).astype(F)))
    v, n, f = S.icosphere(0.05, 3, (1.0, 0.8, 1.2))
    out.append(dict(vertices=v, normals=n, faces=f, uvs=_sphere_uv(v), texture=rng.integers(0, 256, (32, 64, 3)).astype(np.uint8)))
    v, n, f = S.icosphere(0.04, 2)
    out.append(dict(vertices=v, normals=n, faces=f, uvs=_sphere_uv(v), texture=np.array([[[200, 90, 30]]], np.uint8)))
    v, n, f = S.box_mesh((0.03, 0.05, 0.03))
    out.append(dict(vertices=v, normals=n, faces=f))
    v, n, f = S.icosphere(0.05, 3)
    out.append(dict(vertices=v, normals=n, faces=f, colors=rng.uniform(0, 1, v.shape).astype(F)))
    out.append(None)      # filled per size by box_pixels_mesh (it depends on the intrinsics)
    return out


def box_pixels_mesh(K):
    """Two triangles at z = 1 (identity pose) covering columns 10..17 x rows 20..27 (64 pixels) and columns 40..52 x rows
    20..24 (65): the corners sit on half-pixel coordinates, far from a rounding boundary."""
    def tri(u0, u1, v0, v1):
        pts = [(u0, v0), (u1, v0), (u0, v1)]
        return [[(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], 1.0] for u, v in pts]
    v = np.asarray(tri(9.5, 17.5, 19.5, 27.5) + tri(39.5, 52.5, 19.5, 24.5), F)
    n = np.tile(np.asarray([[0, 0, -1]], F), (6, 1))
    return dict(vertices=v, normals=n, faces=np.asarray([[0, 1, 2], [3, 5, 4]], np.int32),
                colors=np.linspace(0.1, 0.9, 18).reshape(6, 3).astype(F))


def bank_meshes(K):
    m = list(meshes())
    m[5] = box_pixels_mesh(K)
    return m


CLASSES = (1, 2, 3, 4, 5, 6)


def main_scenes():
    """S = 3 scenes with 2, 6 and 0 instances: (mesh, pose, shininess) lists and the lights.
    scene 0: a box close to the camera (its 12 triangles are walked by the workgroup) in front of, and partly hiding, a
             textured ellipsoid that in turn pokes through it (mutual occlusion);
    scene 1: two copies of mesh 4 at one pose in slots 0 and 1; a textured sphere half outside the image; a box past z_far;
             a sphere straddling z_near; a white box behind the first sphere."""
    P = S.pose
    s0 = [(0, P(S.rot((1, 2, 0.5), 0.7), (0.01, -0.01, 0.36)), 40),
          (1, P(S.rot((0, 1, 0), 0.3), (0.05, 0.0, 0.40)), 64)]
    T = P(S.rot((1, 0, 1), 0.4), (-0.08, -0.05, 0.7))
    s1 = [(4, T, 120), (4, T, 40),
          (1, P(S.rot((0, 0, 1), 1.1), (0.235, 0.05, 0.8)), 1),
          (0, P(np.eye(3), (0.0, 0.0, 2.5)), 50),
          (2, P(S.rot((1, 1, 0), 2.0), (0.06, 0.07, 0.27)), 255),
          (3, P(S.rot((0, 1, 1), 0.9), (-0.06, -0.03, 0.9)), 77)]
    lights = np.asarray([[0.5, -1.0, 0.0, 1.2], [-1.5, 0.7, 0.0, 2.0], [0.0, 0.0, 0.0, 1.0]], F)
    return [s0, s1, []], lights


def ref_instances(scenes):
    """(mesh, pose, shininess) -> the (mesh, class, pose, shininess) tuples of synth_ref.render_scenes"""
    return [[(m, CLASSES[m], T, sh) for m, T, sh in sc] for sc in scenes]


def backgrounds(n, H, W, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def main_reference(H, W, with_background=True, min_pixels=100):
    K = intrinsics(H, W)
    scenes, lights = main_scenes()
    stats = {}
    out = R.render_scenes(bank_meshes(K), ref_instances(scenes), lights, K4(K), H, W, Z_NEAR, Z_FAR, 1000.0, min_pixels,
                          backgrounds(3, H, W) if with_background else None, stats)
    out["stats"] = stats
    return out


# ---- model and pose files as the reference's Synthesizer(model_file, pose_file) reads them --------------------------
def write_obj(path, v, f, colors=None, uvs=None, texture=None):
    """Wavefront OBJ with optional per-vertex colours (`v x y z r g b`) or uvs + an .mtl naming a PNG written with PIL."""
    lines = []
    if texture is not None:
        from PIL import Image
        stem = path[:-4]
        Image.fromarray(texture).save(stem + ".png")
        with open(stem + ".mtl", "w") as fh:
            fh.write("newmtl m\nKd 1 1 1\nmap_Kd %s\n" % (stem.rsplit("/", 1)[-1] + ".png"))
        lines.append("mtllib %s" % (stem.rsplit("/", 1)[-1] + ".mtl"))
    for i, p in enumerate(v):
        c = "" if colors is None else " %r %r %r" % tuple(float(x) for x in colors[i])
        lines.append("v %r %r %r%s" % (float(p[0]), float(p[1]), float(p[2]), c))
    if uvs is not None:
        lines += ["vt %r %r" % (float(a), float(b)) for a, b in uvs]
    for a, b, c in f:
        lines.append("f %d/%d %d/%d %d/%d" % ((a + 1,) * 2 + (b + 1,) * 2 + (c + 1,) * 2) if uvs is not None else "f %d %d %d" % (a + 1, b + 1, c + 1))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def write_model_and_pose_files(tmp, textured):
    """Three small models (vertex colours; the second textured when `textured`) and the reference's two list files: one
    model path per line, one pose file per line holding rows of 7 floats. -> (model_file, pose_file, pose tables)"""
    rng = np.random.default_rng(21)
    m = meshes()
    models, poses = [], []
    tables = [np.asarray([[1, 0, 0, 0, -0.16, -0.02, 0.62], [0.9, 0.1, 0.3, 0.2, -0.15, 0.0, 0.6]]),
              np.asarray([[0.7, 0.0, 0.7, 0.1, 0.17, 0.02, 0.72]]),
              np.asarray([[0.5, 0.5, 0.5, 0.5, 0.0, 0.12, 1.0], [0.2, 0.9, 0.1, 0.3, 0.02, 0.1, 1.05], [1, 0, 0, 1, 0.0, 0.1, 0.95]])]
    for i, src in enumerate((m[0], m[2], m[3])):
        path = "%s/model%d.obj" % (tmp, i)
        v, f = src["vertices"], src["faces"]
        if i == 1 and textured:
            write_obj(path, v, f, uvs=np.clip(_sphere_uv(v), 0, 1), texture=rng.integers(0, 256, (8, 16, 3)).astype(np.uint8))
        else:
            write_obj(path, v, f, colors=rng.uniform(0, 1, v.shape).astype(F))
        models.append(path)
        np.savetxt("%s/poses%d.txt" % (tmp, i), tables[i], fmt="%.9g")
        poses.append("poses%d.txt" % i)              # relative to the list file
    with open("%s/models.txt" % tmp, "w") as fh:
        fh.write("\n".join(models) + "\n")
    with open("%s/poses.txt" % tmp, "w") as fh:
        fh.write("\n".join(poses) + "\n")
    return "%s/models.txt" % tmp, "%s/poses.txt" % tmp, tables


def coplanar_mesh(K, first_is_red):
    """Two triangles with the SAME three positions (the 64-pixel triangle of box_pixels_mesh) and vertex indices 0..2 and
    3..5: every pixel ties bit for bit, the lower face must win. Colours tell the faces apart."""
    src = box_pixels_mesh(K)
    v = np.concatenate([src["vertices"][:3], src["vertices"][:3]])
    red, blue = np.tile([[1.0, 0.0, 0.0]], (3, 1)), np.tile([[0.0, 0.0, 1.0]], (3, 1))
    return dict(vertices=v, normals=src["normals"], faces=np.asarray([[0, 1, 2], [3, 4, 5]], np.int32),
                colors=np.concatenate([red, blue] if first_is_red else [blue, red]).astype(F))
