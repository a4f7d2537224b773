"""Writes tests/golden/vertex_targets.npz: inputs and outputs of the reference's own `_generate_vertex_targets`
(lib/gt_synthesize_layer/minibatch.py:543-602), the pin of tests/vertex_ref.py and of the device-side generator.

    python tests/golden/make_vertex_targets_golden.py <root of the PoseCNN reference tree>

The function is lifted out of the reference file when this runs (nothing of it is kept here): the module is Python 2 and
imports OpenCV, so the text of that one `def` is cut out, parsed with `ast` and executed with `xrange = range` and a
stub `cfg` (VERTEX_REG_2D on, VERTEX_REG_3D off, VERTEX_W_INSIDE 10). Arrays only; frames of at most 96 x 128."""
import ast
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "_generate_vertex_targets"
W_INSIDE = 10.0


def lift(reference_root):
    path = os.path.join(reference_root, "lib", "gt_synthesize_layer", "minibatch.py")
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("def %s(" % NAME))
    end = next(i for i in range(start + 1, len(lines)) if lines[i][:1] not in ("", " ", "\t", "#", ")"))
    tree = ast.parse("\n".join(lines[start:end]))
    assert len(tree.body) == 1 and isinstance(tree.body[0], ast.FunctionDef) and tree.body[0].name == NAME
    cfg = types.SimpleNamespace(TRAIN=types.SimpleNamespace(VERTEX_REG_2D=True, VERTEX_REG_3D=False, VERTEX_W_INSIDE=W_INSIDE))
    env = {"np": np, "math": math, "xrange": range, "cfg": cfg}
    exec(compile(tree, path, "exec"), env)
    return env[NAME]


def blobs(rng, H, W, objs, paint=None):
    """objs: [(cls, cx, cy, z, radius)] -> label map with one disc per object (later discs on top), meta arrays."""
    label = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for k, (cls, cx, cy, z, rad) in enumerate(objs):
        if paint is None or paint[k]:
            label[(xx - cx) ** 2 + (yy - cy) ** 2 <= rad * rad] = cls
    poses = np.zeros((3, 4, len(objs)))
    for k, o in enumerate(objs):
        poses[:, :3, k] = np.eye(3)
        poses[:, 3, k] = (rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), o[3])
    return label, np.array([o[0] for o in objs], np.float64), np.array([[o[1], o[2]] for o in objs], np.float64), poses


def cases():
    rng = np.random.default_rng(543602)
    out = []

    def single(name, H, W, C, objs, paint=None, extra_label=None, im_scale=1.0):
        label, cls_indexes, center, poses = blobs(rng, H, W, objs, paint)
        if extra_label is not None:
            (y0, y1, x0, x1), cls = extra_label
            label[y0:y1, x0:x1] = cls
        out.append(dict(name=name, label=label, cls_indexes=cls_indexes, center=center, poses=poses, num_classes=C,
                        im_scale=im_scale, multi=0, mask=np.zeros((0, 0), np.int32), cls_indexes_old=np.zeros(0, np.int64)))

    # several classes, fractional centres
    single("several_classes", 96, 128, 22, [(3, 30.25, 40.5, 0.9, 14), (7, 90.75, 50.125, 1.1, 18), (21, 60.5, 20.75, 0.7, 10),
                                             (1, 100.3, 80.9, 1.3, 9)])
    # a class in the label but not in cls_indexes (class 4 painted by hand)
    single("label_without_object", 64, 80, 6, [(2, 20.5, 30.5, 1.0, 10), (5, 60.25, 20.0, 0.8, 8)], extra_label=((40, 60, 50, 70), 4))
    # a class in cls_indexes but not in the label
    single("object_without_label", 64, 80, 6, [(2, 20.5, 30.5, 1.0, 10), (3, 50.0, 40.0, 0.9, 12)], paint=[True, False])
    # a centre outside the image, on both sides
    single("centre_outside", 48, 64, 5, [(1, -15.5, 20.25, 1.2, 30), (4, 70.75, 60.5, 0.6, 28)])
    # pixels exactly on their (integer) centre
    single("pixel_on_centre", 48, 64, 5, [(2, 20.0, 17.0, 1.0, 6), (3, 50.0, 30.0, 2.0, 1)])
    # im_scale * center is what the function is handed
    single("scaled_centres", 48, 64, 5, [(1, 21.3, 13.7, 1.05, 9), (2, 45.1, 33.3, 0.95, 11)], im_scale=0.75)
    # two-class training, three instances of the kept class among five objects (minibatch.py:356-367, :426-431)
    H, W = 64, 96
    objs = [(6, 20.5, 20.5, 1.0, 9), (9, 48.25, 30.0, 0.8, 8), (6, 70.0, 40.75, 1.2, 10), (2, 30.0, 50.0, 0.9, 7), (6, 85.5, 12.5, 1.4, 6)]
    label, cls_indexes, center, poses = blobs(rng, H, W, objs)
    mask = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for k, (cls, cx, cy, z, rad) in enumerate(objs):
        mask[(xx - cx) ** 2 + (yy - cy) ** 2 <= rad * rad] = k + 1
    ind = np.where(cls_indexes == 6)[0]
    out.append(dict(name="two_class_multi_instance", label=(label == 6).astype(np.int32), cls_indexes=np.ones(len(ind), np.float32),
                    center=center[ind], poses=poses[:, :, ind], num_classes=2, im_scale=1.0, multi=1, mask=mask, cls_indexes_old=ind))
    return out


def main(reference_root):
    fn = lift(reference_root)
    arrays = {}
    names = []
    for c in cases():
        H, W = c["label"].shape
        assert H <= 96 and W <= 128
        C = c["num_classes"]
        targets = np.zeros((H, W, 3 * C), np.float32)
        weights = np.zeros((H, W, 3 * C), np.float32)
        targets, weights = fn(c["label"], c["cls_indexes"], c["im_scale"] * c["center"], c["poses"], C, [], None, c["mask"],
                              c["multi"], c["cls_indexes_old"], targets, weights)
        assert weights.any()
        names.append(c["name"])
        for k in ("label", "cls_indexes", "center", "poses", "mask", "cls_indexes_old"):
            arrays["%s/%s" % (c["name"], k)] = c[k]
        arrays["%s/num_classes" % c["name"]] = np.int32(C)
        arrays["%s/im_scale" % c["name"]] = np.float64(c["im_scale"])
        arrays["%s/multi" % c["name"]] = np.int32(c["multi"])
        arrays["%s/targets" % c["name"]] = targets
        arrays["%s/weights" % c["name"]] = weights
    arrays["names"] = np.array(names)
    arrays["w_inside"] = np.float64(W_INSIDE)
    path = os.path.join(HERE, "vertex_targets.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d cases, %d bytes" % (path, len(names), os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
