"""numpy restatement of the vertex-target arithmetic of include/posecnn_hip_train.h — the checker of the device-side
generator and of `datasets.training_blobs`. It is itself pinned, bit for bit, to outputs of the reference's
`_generate_vertex_targets` (tests/golden/vertex_targets.npz, tests/test_vertex_targets_cpu.py)."""
import math
import os

import numpy as np

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vertex_targets.npz")


def object_table(cls_indexes, center, poses, w_inside=10.0, im_scale=1.0, mask_ids=None):
    """Rows (cls, mask_id, cx, cy, log_z, w) from the arrays of a -meta.mat as minibatch.py:420-437 hands them on:
    cx, cy = float32(im_scale * center) (the reference's `c` is a float32 array), log_z = float32(math.log(z))."""
    n = len(cls_indexes)
    tab = np.zeros((n, 6), F)
    for j in range(n):
        c = (im_scale * np.asarray(center[j], np.float64)).astype(F)
        tab[j] = (cls_indexes[j], 0 if mask_ids is None else mask_ids[j], c[0], c[1], F(math.log(float(poses[2, 3, j]))), w_inside)
    return tab


def vertex_targets(label, objects, num_classes, instance=None):
    """label int [B,H,W], objects f32 [B,M,6], instance int [B,H,W] | None -> (targets, weights) f32 [B,H,W,3C].
    Rows are applied in ascending order, so the highest matching row wins; float64 with one rounding per operation."""
    label = np.asarray(label)
    objects = np.asarray(objects, F)
    B, H, W = label.shape
    C = int(num_classes)
    targets = np.zeros((B, H, W, 3 * C), F)
    weights = np.zeros((B, H, W, 3 * C), F)
    for b in range(B):
        inst = np.zeros((H, W), F) if instance is None else np.asarray(instance[b]).astype(F)
        live = (label[b] > 0) & (label[b] < C)
        for cls, mask_id, cx, cy, log_z, w in objects[b]:
            sel = live & (label[b].astype(F) == cls)
            if mask_id != 0:
                sel &= inst == mask_id
            y, x = np.where(sel)            # int64: the float32 centre minus it is float64
            if len(x) == 0:
                continue
            dx, dy = np.float64(cx) - x, np.float64(cy) - y
            n = np.sqrt(dx * dx + dy * dy) + 1e-10
            l3 = 3 * int(cls)
            targets[b, y, x, l3 + 0] = dx / n
            targets[b, y, x, l3 + 1] = dy / n
            targets[b, y, x, l3 + 2] = log_z
            weights[b, y, x, l3:l3 + 3] = w
    return targets, weights


def golden_cases():
    """-> [dict(name, label [H,W], cls_indexes, center, poses, mask, cls_indexes_old, num_classes, im_scale, multi,
    targets, weights)] of the reference pin, plus `objects` / `instance`: the same inputs as the object table."""
    z = np.load(GOLDEN)
    w_inside = float(z["w_inside"])
    out = []
    for name in z["names"]:
        c = {k: z["%s/%s" % (name, k)] for k in ("label", "cls_indexes", "center", "poses", "mask", "cls_indexes_old", "targets", "weights")}
        c.update(name=str(name), num_classes=int(z["%s/num_classes" % name]), im_scale=float(z["%s/im_scale" % name]),
                 multi=int(z["%s/multi" % name]))
        mask_ids = c["cls_indexes_old"] + 1.0 if c["multi"] else None    # minibatch.py:553: mask == cls_indexes_old[i] + 1
        c["objects"] = object_table(c["cls_indexes"], c["center"], c["poses"], w_inside, c["im_scale"], mask_ids)
        c["instance"] = c["mask"] if c["multi"] else None
        out.append(c)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == F and np.array_equal(a.view(np.uint32), b.view(np.uint32))
