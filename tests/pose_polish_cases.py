"""Cases for the pose polish (TEST INFRASTRUCTURE), shared by tests/test_pose_polish_cpu.py — which proves what each case
exercises — and tests/test_gpu_pose_polish.py, which runs them on the GPU. Everything is built from the planted 64 x 96
scenes of tests/pose3d_cases.py (route 0, depth) and tests/pose2d_cases.py (route 1, colour): their prepared records, and
their planted poses moved inside the polish's box.

BATCH of four frames per route (C = 7):
  frames 0 .. 2   the scenes of seeds 1, 2, 3 with their own intrinsics. Classes 1, 2, 3: the planted pose perturbed by
                  PERTURB (2 degrees about a random axis, 5 mm along a random direction), gate 100. Class 4 (400 records): the
                  same, with gate == MIN_PIXELS in frame 0 (not polished: the test is `>`), MIN_PIXELS + 1 in frame 1
                  (polished) and 0 in frame 2. Class 5 (depth: every record a hole, so the list is empty behind an open gate;
                  colour: every object point the origin), gate 100. Class 6: no record, gate 100. Class 0: a pose that is not
                  a rotation and an open gate: copied.
  frame 3         hand-counted classes cut from the planted inliers of frame 0's class 1, all under that class's perturbed
                  pose and frame 0's intrinsics: 63, 64, 65, 5, 0 and 129 records (LENGTHS) — with THRESHOLD every one of
                  them is listed, so the list lengths are those numbers: below, at and above one and two turns of the 64 lanes.
NEAR (colour only, one frame, C = 2): 40 object points in a 0.2 m cube whose near face is 0.5 mm in front of the camera, the
four corners of that face among them: a rotation of a third of a degree about x or y puts one of them behind the camera
(energy +inf): two vertices of the initial simplex and later reflections are +inf and are never taken.
EDGE (both routes, one frame): frame 0 of the batch with every gate but class 2's closed and that class's planted pose moved
by 12 cm along -x: the best update lies outside the box (|tau_x| <= 0.1), trial points are clamped onto the bound. The
inlier threshold is wide enough (EDGE_THRESHOLD) to list the class under so distant a start.
SHRINK (colour only): frame 2 of the batch with every gate but class 5's closed. That class's object points are all the
origin, so its energy does not depend on the rotation; its simplex is the one of all these cases that shrinks within 300
evaluations (evaluations 290 .. 295): a budget of 292 ends inside the shrink, one of 300 goes through it. The simplex code
is one template for both routes (the route only changes the distance), so the depth route runs the same instructions."""
import functools

import numpy as np

import pose2d_cases as C2
import pose2d_ref as R2
import pose3d_cases as C3
import pose3d_ref as R3
import pose_polish_ref as PR

F, D = np.float32, np.float64
H, W, C = C3.H, C3.W, C3.C
SEEDS = (1, 2, 3)
POSED = C3.POSED
THRESHOLD = {0: 0.025, 1: 6.0}          # metres / pixels: above what PERTURB moves a planted inlier, below the planted outliers
MIN_PIXELS = 10
PERTURB = (0.035, 0.005)                # radians (2 degrees), metres
LENGTHS = (0, 63, 64, 65, 5, 0, 129)
CASES = {0: C3, 1: C2}


def planted12(frame, c):
    Rm, t = frame["poses"][c]
    return np.concatenate([Rm, t[:, None]], axis=1).reshape(12)


def perturb(P, seed, rot=PERTURB[0], tr=PERTURB[1]):
    """P(x) for an x of the given rotation and translation lengths in seeded random directions"""
    rng = np.random.RandomState(seed)
    w, t = rng.normal(size=3), rng.normal(size=3)
    return PR.pose_of(P, np.concatenate([w * (rot / np.linalg.norm(w)), t * (tr / np.linalg.norm(t))]))


@functools.lru_cache(maxsize=None)
def frames(route):
    """the three scene frames of a route: [(frame dict, records, counts, offsets)]"""
    out = []
    for seed, K in zip(SEEDS, C3.INTRINSICS):
        f = CASES[route].make_frame(seed, K)
        if route == 0:
            prep = R3.prepare(f["label"], f["depth"], f["vertex_pred"], f["extents"], f["K"], C3.FACTOR)
        else:
            prep = R2.prepare(f["label"], f["vertex_pred"], f["extents"])
        out.append((f,) + tuple(prep))
    return out


@functools.lru_cache(maxsize=None)
def batch(route):
    """-> dict(records f32 [4,H W,6], counts, offsets, gate int32 [4,C], poses f64 [4,C,12], K f32 [4,4], planted: {(b, c): the
    planted (R, t)}, extents)"""
    fr = frames(route)
    records = np.zeros((4, H * W, 6), F)
    counts, offsets, gate = np.zeros((4, C), np.int32), np.zeros((4, C), np.int32), np.zeros((4, C), np.int32)
    poses = np.zeros((4, C, 12), D)
    K = np.array([f["K"] for f, _, _, _ in fr] + [fr[0][0]["K"]], dtype=F)
    planted = {}
    for b, (f, rec, cnt, off) in enumerate(fr):
        records[b, :len(rec)], counts[b], offsets[b] = rec, cnt, off
        poses[b, 0] = np.arange(12) * 0.25 - 1.0
        gate[b] = 100
        for c in range(1, C):
            if c in f["poses"]:
                poses[b, c] = perturb(planted12(f, c), 100 * SEEDS[b] + c)
                planted[(b, c)] = f["poses"][c]
        gate[b, 4] = (MIN_PIXELS, MIN_PIXELS + 1, 0)[b]
    f, rec, cnt, off = fr[0]
    inl = rec[off[1]:off[1] + cnt[1]][f["inlier"][1]]
    assert len(inl) >= sum(LENGTHS)
    records[3, :sum(LENGTHS)] = inl[:sum(LENGTHS)]
    counts[3] = LENGTHS
    offsets[3] = np.concatenate([[0], np.cumsum(LENGTHS)[:-1]])
    poses[3, :] = poses[0, 1]
    gate[3] = 100
    return dict(records=records, counts=counts, offsets=offsets, gate=gate, poses=poses, K=K, planted=planted, extents=f["extents"])


# every (max_pixels, evaluations) the GPU test runs the batch at: 7 = the initial simplex alone, 8 = one reflection,
# 100 = the reference's budget; 37 thins the small scene, 1000 is the default, 1025 and 2000 put the list into the workspace
# (PCNN_POSE_POLISH_LDS_RECORDS = 1024), thinned and not
RUNS = ((1000, 7), (1000, 8), (1000, 100), (37, 100), (1025, 100), (2000, 100), (1000, 0))


@functools.lru_cache(maxsize=None)
def reference(route, max_pixels, evaluations, trace=False):
    """the restatement on the batch, computed once per run: [per frame dict of pose_polish_ref.polish] (and the traces)"""
    bt = batch(route)
    out, traces = [], []
    for b in range(4):
        tr = {} if trace else None
        out.append(PR.polish(route, bt["records"][b], bt["counts"][b], bt["offsets"][b], bt["poses"][b], bt["gate"][b],
                             K=tuple(bt["K"][b]), max_pixels=max_pixels, min_pixels=MIN_PIXELS, evaluations=evaluations,
                             inlier_threshold=THRESHOLD[route], trace=tr))
        traces.append(tr)
    return (out, traces) if trace else out


# ---- the colour case that meets +inf ------------------------------------------------------------------------------------------
NEAR_K = (120.0, 118.0, 48.0, 32.0)
NEAR_POSE = np.array([1.0, 0, 0, 0.01, 0, 1.0, 0, -0.02, 0, 0, 1.0, 0.1005])
NEAR_THRESHOLD = 40.0


@functools.lru_cache(maxsize=None)
def near():
    """-> dict(records f32 [1,H W,6], counts, offsets, gate int32 [1,2], poses f64 [1,2,12], K f32 [1,4]): pixels are the
    projections under NEAR_POSE moved by up to 2 pixels"""
    rng = np.random.RandomState(7)
    obj = rng.uniform(-0.1, 0.1, size=(40, 3)).astype(F)
    obj[:4] = [[0.1, 0.1, -0.1], [-0.1, 0.1, -0.1], [0.1, -0.1, -0.1], [-0.1, -0.1, -0.1]]
    pix = C2.project(NEAR_POSE.reshape(3, 4)[:, :3], NEAR_POSE.reshape(3, 4)[:, 3], obj.astype(D), NEAR_K) + rng.uniform(-2, 2, size=(40, 2))
    records = np.zeros((1, H * W, 6), F)
    records[0, :40, :2], records[0, :40, 3:] = pix.astype(F), obj
    poses = np.zeros((1, 2, 12), D)
    poses[0, 1] = NEAR_POSE
    return dict(records=records, counts=np.array([[0, 40]], np.int32), offsets=np.array([[0, 0]], np.int32),
                gate=np.array([[0, 40]], np.int32), poses=poses, K=np.array([NEAR_K], dtype=F))


NEAR_RUNS = (100,)


@functools.lru_cache(maxsize=None)
def near_reference(evaluations, trace=False):
    n = near()
    tr = {} if trace else None
    out = PR.polish(1, n["records"][0], n["counts"][0], n["offsets"][0], n["poses"][0], n["gate"][0], K=NEAR_K, max_pixels=1000,
                    min_pixels=MIN_PIXELS, evaluations=evaluations, inlier_threshold=NEAR_THRESHOLD, trace=tr)
    return (out, tr) if trace else out


# ---- the simplex that shrinks ---------------------------------------------------------------------------------------------------
SHRINK_RUNS = (292, 300)


@functools.lru_cache(maxsize=None)
def shrink():
    """-> the dict of `near` (C = 7): frame 2 of the colour batch, only class 5 behind an open gate"""
    bt = batch(1)
    gate = np.zeros((1, C), np.int32)
    gate[0, 5] = 100
    return dict(records=bt["records"][2:3], counts=bt["counts"][2:3], offsets=bt["offsets"][2:3], gate=gate, poses=bt["poses"][2:3],
                K=bt["K"][2:3])


@functools.lru_cache(maxsize=None)
def shrink_reference(evaluations, trace=False):
    n = shrink()
    tr = {} if trace else None
    out = PR.polish(1, n["records"][0], n["counts"][0], n["offsets"][0], n["poses"][0], n["gate"][0], K=tuple(n["K"][0]),
                    max_pixels=1000, min_pixels=MIN_PIXELS, evaluations=evaluations, inlier_threshold=THRESHOLD[1], trace=tr)
    return (out, tr) if trace else out


# ---- a start whose best update lies outside the box --------------------------------------------------------------------------
EDGE_THRESHOLD = {0: 0.3, 1: 40.0}
EDGE_SHIFT = (0.0, 0.0, 0.0, -0.12, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def edge(route):
    """-> the dict of `near` (C = 7)"""
    bt = batch(route)
    gate = np.zeros((1, C), np.int32)
    gate[0, 2] = 100
    poses = bt["poses"][0:1].copy()
    poses[0, 2] = PR.pose_of(planted12(frames(route)[0][0], 2), EDGE_SHIFT)
    return dict(records=bt["records"][0:1], counts=bt["counts"][0:1], offsets=bt["offsets"][0:1], gate=gate, poses=poses, K=bt["K"][0:1])


@functools.lru_cache(maxsize=None)
def edge_reference(route, evaluations=100, trace=False, defect=None):
    n = edge(route)
    tr = {} if trace else None
    out = PR.polish(route, n["records"][0], n["counts"][0], n["offsets"][0], n["poses"][0], n["gate"][0], K=tuple(n["K"][0]),
                    max_pixels=1000, min_pixels=MIN_PIXELS, evaluations=evaluations, inlier_threshold=EDGE_THRESHOLD[route], trace=tr,
                    defect=defect)
    return (out, tr) if trace else out
