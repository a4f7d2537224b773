"""The staged paths of the custom-op kernels: which compile-time constant separates which regimes, and the GPU cases that
sit just below, at and just above each of them. Shared by tests/test_thresholds_cpu.py (the audit: needs no GPU) and
tests/test_gpu_thresholds.py (the parity runs).

  ROWS    plain data: kernel, source file, the constants restated with their values, the quantity compared with them and the
          regimes they separate. A regime's `key` is what a classifier below returns; `side` places it against the constant.
  CASES   plain data: the op, its parameters, the regimes the case claims per row, and where it comes from ("new": run by
          tests/test_gpu_thresholds.py; otherwise the id of the existing GPU test that runs these very inputs).
  build / reference / classify   the inputs of a case, the oracle's outputs for them, and the regimes the case reaches —
          computed from those two alone, never from the library.

The classifiers restate, in a few lines each, the loop structure a constant controls (how many rounds, where a flush falls);
they take the per-record facts that loop consumes from the oracle's outputs (e.g. a cell's voters from the emitted row).
"""
import functools
import math
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "posecnn_amd", "csrc")


# =====================================================================================================================
# the table
def _r(key, side, what):
    return dict(key=key, side=side, what=what)


ROWS = [
    dict(id="adl_sum_tile", kernel="adl_sum_kernel", file="average_distance.hip",
         constants={"ADL_SUM_TILE_MAX": 3072, "ADL_SUM_THREADS": 256, "ADL_SUM_PAD": 36},
         quantity="P, the terms of one row (model points)",
         regimes=[_r("one partial round", "below", "P < 3072: the whole row staged once"),
                  _r("one full round, float4", "at", "P = 3072"),
                  _r("second round of one term, scalar", "above", "P = 3073"),
                  _r("scalar staging in every round", "above", "P % 4 != 0 and a last round of more than one term"),
                  _r("second round under one trip, float4", "above", "P % 4 = 0, last round of fewer than 16 terms"),
                  _r("two exact rounds", "above", "P = 6144"),
                  _r("third ragged round with a full trip", "above", "three rounds, the last of 16..31 terms, float4")]),
    dict(id="adl_qtile", kernel="adl_terms_kernel (symmetric scan)", file="average_distance.hip",
         constants={"ADL_QTILE": 1024, "ADL_THREADS": 256},
         quantity="P on a row of a symmetric class: candidate tiles of the nearest-neighbour scan and the `q0 + ADL_QTILE < P` prefetch",
         regimes=[_r("P = t - 1", "below", "one ragged tile, no prefetch"),
                  _r("P = t", "at", "one full tile, no prefetch"),
                  _r("P = t + 1", "above", "a second tile of one candidate"),
                  _r("P = 2t", "above", "two full tiles, one prefetch"),
                  _r("P = 2t + 1", "above", "a third tile of one candidate")]),
    dict(id="adl_rows", kernel="adl_order_kernel / adl_total_kernel", file="average_distance.hip",
         constants={"ADL_ORDER_THREADS": 1024},
         quantity="R, the op's row count (host-side, and device-side inside a larger capacity): passes of 1024 rows / chunks of 1024 losses",
         regimes=[_r("R = t - 1", "below", "one partial pass"),
                  _r("R = t", "at", "exactly one pass"),
                  _r("R = t + 1", "above", "a second pass of one row")]),
    dict(id="adl_row_slots", kernel="adl_terms_kernel (grid.y)", file="average_distance.hip",
         constants={"ADL_ROW_SLOTS": 512},
         quantity="rows with a pose target (the list adl_terms strides over grid.y = min(R, 512))",
         regimes=[_r("targets = t - 1", "below", "the last slot's workgroups find no row"),
                  _r("targets = t", "at", "one row per slot"),
                  _r("targets = t + 1", "above", "slot 0 takes a second row")]),
    dict(id="hough_wcd", kernel="wave_cell_data (hv_localmax_kernel, vote_threshold > 0)", file="hough_voting.hip",
         constants={"WCD_CAP": 1024},
         quantity="voters of a non-first maximum's cell; the strip is flushed when fill > WCD_CAP - 64 after a batch of 64 records",
         regimes=[_r("no flush, far below", "below", "a few hundred voters"),
                  _r("no flush, fill = WCD_CAP - 64", "at", "960 voters"),
                  _r("one flush, fill = WCD_CAP - 63", "above", "961 voters"),
                  _r("one flush, strip full", "above", "1024 voters: fill = WCD_CAP"),
                  _r("two flushes", "above", "more than 1920 voters")]),
    dict(id="hough_select", kernel="hv_select_kernel", file="hough_voting.hip",
         constants={"HV_SEL_NT": 1024, "SEL_CAP": 4096},
         quantity="voters of the winning cell against SEL_CAP - HV_SEL_NT = 3072, in trips of 1024 of the class' m = ceil(pixels / skip) records",
         regimes=[_r("one trip", "below", "m <= 1024"),
                  _r("fill = t, no capacity flush", "at", "3072 voters in three trips"),
                  _r("capacity flush on the last trip", "above", "fill = SEL_CAP = 4096 when the records end"),
                  _r("capacity flush with records to come", "above", "m > 4096, more than 3072 voters")]),
    dict(id="hough_rchunk", kernel="hv_vote_kernel", file="hough_voting.hip", constants={"HV_RCHUNK": 256},
         quantity="records of a class (staged 256 per round)",
         regimes=[_r("m = t - 1", "below", ""), _r("m = t", "at", ""), _r("m = t + 1", "above", "")]),
    dict(id="hough_chunk", kernel="hv_hist_kernel / hv_scatter_kernel", file="hough_voting.hip", constants={"HV_CHUNK": 2048},
         quantity="label pixels of an image, H * W",
         regimes=[_r("HW = t - 1", "below", ""), _r("HW = t", "at", ""), _r("HW = t + 1", "above", "")]),
    dict(id="hough_lm_chunk", kernel="hv_localmax_kernel / hv_gather_kernel", file="hough_voting.hip", constants={"LM_CHUNK": 1024},
         quantity="Hough cells of an image, slots * H * W (vote_threshold > 0)",
         regimes=[_r("cells = t - 1", "below", ""), _r("cells = t", "at", ""), _r("cells = t + 1", "above", "")]),
    dict(id="roi_lds", kernel="roi_pool_fwd_staged", file="roi_pool.hip", constants={"RP_LDS_WORDS": 4096, "RP_CHUNK": 32},
         quantity="ncols * cc * per_col of one (roi, bin row, channel chunk) workgroup; per_col = 2 with an argmax output",
         regimes=[_r("argmax: words = t - one column", "below", "63 columns x 32 channels x 2"),
                  _r("argmax: words = t", "at", "64 columns: staged"),
                  _r("argmax: words = t + one column", "above", "65 columns: unstaged"),
                  _r("no argmax: words = t - one column", "below", "127 columns x 32 channels"),
                  _r("no argmax: words = t", "at", "128 columns: staged"),
                  _r("no argmax: words = t + one column", "above", "129 columns: unstaged")]),
    dict(id="roi_bwd_list", kernel="roi_pool_bwd_binned", file="roi_pool.hip", constants={"RB_LIST": 512, "RB_TILE_W": 8},
         quantity="ROIs hitting one 8-column tile; rounds of 64 are collected while count <= RB_LIST - 64",
         regimes=[dict(key="one short pass", side="below", what="far fewer than 448", passes=None),
                  dict(key="passes [448]", side="at", what="count = RB_LIST - 64 as the table ends", passes=[448]),
                  dict(key="passes [449]", side="above", what="count = RB_LIST - 64 with one ROI left: an eighth round", passes=[449]),
                  dict(key="passes [512]", side="at", what="the list exactly full", passes=[512]),
                  dict(key="passes [512, 1]", side="above", what="a second pass of one ROI", passes=[512, 1])]),
    dict(id="render_small", kernel="render_raster_kernel", file="render.hip", constants={"RD_SMALL": 64},
         quantity="pixels of a triangle's clipped bounding box (the nearest areas a box of integer sides has)",
         regimes=[_r("%s, box = %s" % (w, b), s, "%d pixels" % n) for w in ("ccw", "cw")
                  for b, s, n in (("t - 1", "below", 63), ("t", "at", 64), ("t + 1", "above", 65), ("t + 2", "above", 66))]),
    dict(id="backproject_tile", kernel="backproject_window_range_kernel", file="backproject.hip", constants={"TW": 64, "TH": 16, "KMAX": 3},
         quantity="the window-range table (W + 2k) x (H + 2k) against the 64 x 16 tile, at a threshold the table's skip test decides",
         regimes=[_r("table = tile - 1", "below", "63 x 15"), _r("table = tile", "at", "64 x 16"),
                  _r("table = tile + 1", "above", "65 x 17")]),
    dict(id="backproject_list", kernel="backproject_fused_kernel", file="backproject.hip", constants={"LIST": 56, "KMAX": 3},
         quantity="hits of one voxel: at most (2 KMAX + 1)^2 = 49 of the 56 slots", sides=("below",),
         regimes=[_r("49 hits", "below", "every pixel of a full 7 x 7 window matches")]),
    dict(id="vertex_objects", kernel="pcnn_vertex_targets_fwd", file="vertex_targets.hip", constants={"VT_MAX_OBJECTS": 64},
         quantity="M, rows of the object table",
         regimes=[_r("M = t - 1", "below", ""), _r("M = t", "at", ""), _r("M = t + 1: PCNN_EINVAL", "above", "rejected, nothing launched")]),
]
ROW = {r["id"]: r for r in ROWS}


def parse_constants(path):
    """{NAME: value} of the `constexpr int NAME = value[, NAME = value]...;` statements of one source file; a value may
    be an integer expression over names defined earlier in the file."""
    with open(path) as fh:
        text = fh.read()
    out = {}
    for stmt in re.findall(r"constexpr\s+int\s+([^;]+);", text):
        for part in stmt.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*([\w\s+\-*/()]+?)\s*(?://.*)?", part, re.S)
            if not m:
                continue
            try:
                out[m.group(1)] = int(eval(m.group(2).replace("/", "//"), {"__builtins__": {}}, dict(out)))
            except Exception:
                pass
    return out


# =====================================================================================================================
# the cases
def _adl(name, claims, R, P, margin, pattern, C=6, sym=(2,), targets=None, cap=None, origin="new", **kw):
    return dict(id=name, op="adl", claims=claims, origin=origin, R=R, C=C, P=P, margin=margin, pattern=pattern, sym=sym,
                targets=targets, cap=cap if cap is not None else R + 3, **kw)


# rows: class 1, the symmetric class 2, a row without a target, the last class, class 3
_MIX = (1, 2, 0, 5, 3)
_SYM = (2, 1, 2)
_MANY = (1, 2, 3, 4, 5, 0, 5, 4, 3, 1)


def _hough(name, claims, H, W, blobs, vote_thr, origin="new", skip=1, label_thr=100):
    C = 1 + max(b[0] for b in blobs)
    return dict(id=name, op="hough", claims=claims, origin=origin, H=H, W=W, C=C, blobs=blobs, vote_thr=vote_thr, skip=skip,
                label_thr=label_thr)


def _wcd(n):   # class 1: the first maximum (287 voters); class 2: the cell under test
    return [(1, 0, 287, (48, 1)), (2, 8, n, (48, 13))]


def _roi(name, claims, ncols, argmax):
    return dict(id=name, op="roi_fwd", claims=claims, origin="new", ncols=ncols, argmax=argmax)


def _tri(name, key, bw, bh, cw):
    return dict(id=name, op="render", claims={"render_small": [key]}, origin="new", bw=bw, bh=bh, cw=cw)


CASES = [
    # ---- average distance loss
    _adl("adl_P2620_existing", {"adl_sum_tile": ["one partial round"]}, 7, 2620, 0.01, None, C=22,
         origin="tests/test_gpu_ops.py::test_average_distance_forward[7-22-2620-0.01]", seed=17, sym=(16, 21)),
    _adl("adl_P3072", {"adl_sum_tile": ["one full round, float4"]}, 5, 3072, 0.0, _MIX),
    _adl("adl_P3073", {"adl_sum_tile": ["second round of one term, scalar"]}, 5, 3073, 0.01, _MIX),
    _adl("adl_P3075", {"adl_sum_tile": ["scalar staging in every round"]}, 5, 3075, 0.0, _MIX),
    _adl("adl_P3076", {"adl_sum_tile": ["second round under one trip, float4"]}, 5, 3076, 0.01, _MIX),
    _adl("adl_P6144", {"adl_sum_tile": ["two exact rounds"]}, 5, 6144, 0.01, _MIX),
    _adl("adl_P6164", {"adl_sum_tile": ["third ragged round with a full trip"]}, 6, 6164, 0.0, _MIX),
    _adl("adl_P1023", {"adl_qtile": ["P = t - 1"]}, 3, 1023, 0.01, _SYM),
    _adl("adl_P1024", {"adl_qtile": ["P = t"]}, 3, 1024, 0.0, _SYM),
    _adl("adl_P1025_existing", {"adl_qtile": ["P = t + 1"]}, 12, 1025, 0.01, None, C=5,
         origin="tests/test_gpu_ops.py::test_average_distance_forward[12-5-1025-0.01]", seed=17),
    _adl("adl_P2048", {"adl_qtile": ["P = 2t"]}, 3, 2048, 0.01, _SYM),
    _adl("adl_P2049", {"adl_qtile": ["P = 2t + 1"]}, 3, 2049, 0.0, _SYM),
    _adl("adl_R1023", {"adl_rows": ["R = t - 1"]}, 1023, 64, 0.01, _MANY, cap=1100),
    _adl("adl_R1024", {"adl_rows": ["R = t"]}, 1024, 64, 0.01, _MANY, cap=1100),
    _adl("adl_R1025", {"adl_rows": ["R = t + 1"]}, 1025, 64, 0.0, _MANY, cap=1100),
    _adl("adl_T511", {"adl_row_slots": ["targets = t - 1"]}, 600, 64, 0.01, _MANY[:5], targets=511, cap=640),
    _adl("adl_T512", {"adl_row_slots": ["targets = t"]}, 600, 64, 0.01, _MANY[:5], targets=512, cap=640),
    _adl("adl_T513", {"adl_row_slots": ["targets = t + 1"]}, 600, 64, 0.0, _MANY[:5], targets=513, cap=640),
    # ---- Hough voting: blobs whose pixels all point at one cell, skip_pixels = 1
    _hough("hough_wcd_960", {"hough_wcd": ["no flush, far below", "no flush, fill = WCD_CAP - 64"]}, 64, 96, _wcd(960), 250.0),
    _hough("hough_wcd_961", {"hough_wcd": ["no flush, far below", "one flush, fill = WCD_CAP - 63"]}, 64, 96, _wcd(961), 250.0),
    _hough("hough_wcd_1024", {"hough_wcd": ["no flush, far below", "one flush, strip full"]}, 64, 96, _wcd(1024), 250.0),
    _hough("hough_wcd_2000", {"hough_wcd": ["no flush, far below", "two flushes"]}, 64, 96, _wcd(2000), 250.0),
    _hough("hough_sel_1000", {"hough_select": ["one trip"]}, 64, 96, [(1, 2, 1000, (48, 7))], -1.0),
    _hough("hough_sel_3072", {"hough_select": ["fill = t, no capacity flush"]}, 64, 96, [(1, 2, 3072, (48, 18))], -1.0),
    _hough("hough_sel_4096", {"hough_select": ["capacity flush on the last trip"]}, 64, 96, [(1, 2, 4096, (48, 23))], -1.0),
    _hough("hough_sel_5000", {"hough_select": ["capacity flush with records to come"]}, 64, 96, [(1, 2, 5000, (48, 28))], -1.0),
    _hough("hough_m255", {"hough_rchunk": ["m = t - 1"]}, 24, 40, [(1, 2, 255, (20, 5))], -1.0),
    _hough("hough_m256", {"hough_rchunk": ["m = t"]}, 24, 40, [(1, 2, 256, (20, 5))], -1.0),
    _hough("hough_m257", {"hough_rchunk": ["m = t + 1"]}, 24, 40, [(1, 2, 257, (20, 5))], -1.0),
    _hough("hough_hw2047", {"hough_chunk": ["HW = t - 1"]}, 23, 89, [(1, 4, 400, (44, 6))], -1.0),
    _hough("hough_hw2048", {"hough_chunk": ["HW = t"]}, 32, 64, [(1, 4, 400, (32, 7))], -1.0),
    _hough("hough_hw2049", {"hough_chunk": ["HW = t + 1"]}, 3, 683, [(1, 0, 1500, (341, 1))], -1.0),
    _hough("hough_cells1023", {"hough_lm_chunk": ["cells = t - 1"]}, 11, 93, [(1, 2, 400, (46, 4))], 100.0),
    _hough("hough_cells1024", {"hough_lm_chunk": ["cells = t"]}, 32, 32, [(1, 4, 400, (16, 10))], 100.0),
    _hough("hough_cells1025", {"hough_lm_chunk": ["cells = t + 1"]}, 25, 41, [(1, 4, 400, (20, 8))], 100.0),
    # ---- ROI pooling
    _roi("roi_argmax_63", {"roi_lds": ["argmax: words = t - one column"]}, 63, True),
    _roi("roi_argmax_64", {"roi_lds": ["argmax: words = t"]}, 64, True),
    _roi("roi_argmax_65", {"roi_lds": ["argmax: words = t + one column"]}, 65, True),
    _roi("roi_plain_127", {"roi_lds": ["no argmax: words = t - one column"]}, 127, False),
    _roi("roi_plain_128", {"roi_lds": ["no argmax: words = t"]}, 128, False),
    _roi("roi_plain_129", {"roi_lds": ["no argmax: words = t + one column"]}, 129, False),
    dict(id="roi_bwd_existing", op="roi_bwd", claims={"roi_bwd_list": ["one short pass"]}, R=9,
         origin="tests/test_gpu_ops.py::test_roi_pool_backward"),
    dict(id="roi_bwd_448", op="roi_bwd", claims={"roi_bwd_list": ["passes [448]"]}, origin="new", R=448),
    dict(id="roi_bwd_449", op="roi_bwd", claims={"roi_bwd_list": ["passes [449]"]}, origin="new", R=449),
    dict(id="roi_bwd_512", op="roi_bwd", claims={"roi_bwd_list": ["passes [512]"]}, origin="new", R=512),
    dict(id="roi_bwd_513", op="roi_bwd", claims={"roi_bwd_list": ["passes [512, 1]"]}, origin="new", R=513),
    # ---- renderer: one triangle whose bounding box has bw x bh pixels, both windings
    _tri("render_63_ccw", "ccw, box = t - 1", 7, 9, False), _tri("render_64_ccw", "ccw, box = t", 8, 8, False),
    _tri("render_65_ccw", "ccw, box = t + 1", 5, 13, False), _tri("render_66_ccw", "ccw, box = t + 2", 6, 11, False),
    _tri("render_63_cw", "cw, box = t - 1", 9, 7, True), _tri("render_64_cw", "cw, box = t", 8, 8, True),
    _tri("render_65_cw", "cw, box = t + 1", 13, 5, True), _tri("render_66_cw", "cw, box = t + 2", 11, 6, True),
    # ---- backproject, k = 3: the table sizes at the threshold of test_backproject_forward (some voxels hit, most miss, and
    # the skip test decides both kinds in the table's last column and row); one case at a threshold every depth passes
    dict(id="backproject_9x57", op="backproject", claims={"backproject_tile": ["table = tile - 1"]}, origin="new", H=9, W=57, thr=0.05),
    dict(id="backproject_10x58", op="backproject", claims={"backproject_tile": ["table = tile"]}, origin="new", H=10, W=58, thr=0.05),
    dict(id="backproject_11x59", op="backproject", claims={"backproject_tile": ["table = tile + 1"]}, origin="new", H=11, W=59, thr=0.05),
    dict(id="backproject_full_windows", op="backproject", claims={"backproject_list": ["49 hits"]}, origin="new", H=12, W=40, thr=50.0),
    # ---- vertex targets
    dict(id="vertex_M63", op="vertex", claims={"vertex_objects": ["M = t - 1"]}, origin="new", M=63),
    dict(id="vertex_M64", op="vertex", claims={"vertex_objects": ["M = t"]}, origin="new", M=64),
    dict(id="vertex_M65", op="vertex", claims={"vertex_objects": ["M = t + 1: PCNN_EINVAL"]}, origin="new", M=65),
]
CASE = {c["id"]: c for c in CASES}
assert len(CASE) == len(CASES)


def new_cases(op=None):
    return [c for c in CASES if c["origin"] == "new" and (op is None or c["op"] == op)]


# =====================================================================================================================
# inputs
def _build_adl(c):
    from posecnn_amd import synth
    R, C, P, cap = c["R"], c["C"], c["P"], c["cap"]
    if c["pattern"] is None:      # the inputs of the existing test, made the way it makes them
        from test_gpu_ops import adl_case
        pred, tgt, wgt, pts, sym = adl_case(np.random.default_rng(c["seed"]), R, C, P, sym_classes=c["sym"] if C == 22 else (2,))
        return dict(pred=pred, tgt=tgt, wgt=wgt, pts=pts, sym=sym, R=R, margin=c["margin"])
    rng = np.random.default_rng(1000 + P + R)
    pts = synth.make_model_points(C, P)
    sym = np.zeros(C, F)
    sym[list(c["sym"])] = 1
    pred, tgt, wgt = (np.zeros((cap, 4 * C), F) for _ in range(3))
    T = c["targets"]
    for n in range(cap):
        cls = c["pattern"][n % len(c["pattern"])]
        if T is not None and n < R:      # exactly T of the R rows have a target, spread evenly
            cls = (cls or 1) if (n * T) // R != ((n + 1) * T) // R else 0
        if cls == 0:
            continue
        pred[n, 4 * cls:4 * cls + 4] = np.tanh(rng.standard_normal(4)).astype(F)
        tgt[n, 4 * cls:4 * cls + 4] = synth.random_unit_quats(rng, 1)[0]
        wgt[n, 4 * cls:4 * cls + 4] = 1
    return dict(pred=pred, tgt=tgt, wgt=wgt, pts=pts, sym=sym, R=R, margin=c["margin"])


def blob_pixels(W, start_row, n, centre):
    """The first n raster positions from (start_row, 0), the centre cell left out."""
    cx, cy = centre
    idx = np.arange(start_row * W, start_row * W + n + 1)
    idx = idx[idx != cy * W + cx][:n]
    return idx // W, idx % W


def _build_hough(c):
    from posecnn_amd import config
    H, W, C = c["H"], c["W"], c["C"]
    label = np.zeros((1, H, W), np.int32)
    vertex = np.zeros((1, H, W, 3 * C), F)
    rng = np.random.default_rng(30 + H * W + sum(b[2] for b in c["blobs"]))
    for cls, row0, n, (cx, cy) in c["blobs"]:
        y, x = blob_pixels(W, row0, n, (cx, cy))
        assert y.max() < H and (label[0, y, x] == 0).all(), c["id"]
        dx, dy = (cx - x).astype(np.float64), (cy - y).astype(np.float64)
        norm = np.sqrt(dx * dx + dy * dy)
        label[0, y, x] = cls
        vertex[0, y, x, 3 * cls] = dx / norm
        vertex[0, y, x, 3 * cls + 1] = dy / norm
        # a log-depth of its own per voter: the f32 sum of the voters' depths then depends on their order, on the slot
        # each one lands in and on where a flush falls. Depths in (0.8, 1]: the vote box of every pixel stays wider than
        # the frame for these extents, so all of a blob's records still vote for its centre.
        vertex[0, y, x, 3 * cls + 2] = rng.uniform(-0.2, 0.0, len(y)).astype(F)
    ext = np.full((C, 3), 0.2, F)
    meta = config.make_meta_data(config.DEMO_INTRINSICS)[None]
    return dict(label=label, vertex=vertex, ext=ext, meta=meta)


ROI_MAP = (1, 6, 136, 32)      # B, H, W, C of the forward cases: one channel chunk of 32
ROI_PH, ROI_PW = 2, 4


def _build_roi_fwd(c):
    rng = np.random.default_rng(40 + c["ncols"])
    data = rng.integers(-2, 3, ROI_MAP).astype(F)           # ties: the first maximum must win
    x1 = 3
    rois = np.array([[0, 1, x1, 0, x1 + c["ncols"] - 1, 5, 0],
                     [0, 2, 10, 1, 30, 4, 0],
                     [0, 3, 100, 2, 140, 9, 0]], F)
    return dict(data=data, rois=rois, PH=ROI_PH, PW=ROI_PW, scale=1.0, argmax=c["argmax"])


def _build_roi_bwd(c):
    R = c["R"]
    if c["origin"] != "new":
        from test_gpu_ops import random_rois
        rng = np.random.default_rng(14)
        data = rng.standard_normal((2, 10, 12, 8)).astype(F)
        return dict(data=data, rois=random_rois(rng, 9, 2, 8, 12 * 8, 10 * 8), PH=3, PW=3, scale=0.125)
    rng = np.random.default_rng(50 + R)
    data = rng.integers(-2, 3, (1, 4, 16, 8)).astype(F)
    i = np.arange(R)
    rois = np.zeros((R, 7), F)
    rois[:, 1] = i % 8
    rois[:, 2], rois[:, 3], rois[:, 4], rois[:, 5] = i % 3, 0, 15 - i % 2, 3          # every ROI meets both column tiles of every row
    g = (rng.integers(-3, 4, (R, 2, 2, 8)) * 0.37).astype(F)
    return dict(data=data, rois=rois, PH=2, PW=2, scale=1.0, grad=g)


RENDER_HW = (24, 24)
RENDER_K = np.array([[64.0, 0, 0], [0, 64.0, 0], [0, 0, 1]])


def _build_render(c):
    a, b = 3, 4                                   # first column / row of the box
    x0, x1, y0, y1 = a - 0.5, a + c["bw"] - 1 + 0.5, b - 0.5, b + c["bh"] - 1 + 0.5     # pixel units: box = ceil .. floor
    v = np.array([[x0, y0, 0], [x1, y0, 0], [x0, y1, 0]], np.float64) / 64.0
    v[:, 2] = [0.0, 0.25, -0.125]                 # a tilted triangle: perspective-correct weights do some work
    v[:, :2] *= (1.0 + v[:, 2:3])                 # keep the projections where they were: u = x / z * 64
    faces = np.array([[0, 2, 1]] if c["cw"] else [[0, 1, 2]], np.int32)
    pose = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.0]]], F)
    return dict(vertices=v.astype(F), faces=faces, pose=pose, K=RENDER_K, H=RENDER_HW[0], W=RENDER_HW[1])


def _build_backproject(c):
    from test_gpu_ops import backproject_case
    G = 16
    data, label, depth, meta, label3d = backproject_case(np.random.default_rng(60 + c["W"]), 1, c["H"], c["W"], 4, 3, G)
    return dict(data=data, label=label, depth=depth, meta=meta, label3d=label3d, G=G, k=3, thr=c["thr"])


VT_SHAPE = (2, 9, 11, 64)      # B, H, W, C (the entry takes at most 64 classes)


def _build_vertex(c):
    B, H, W, C = VT_SHAPE
    M = c["M"]
    rng = np.random.default_rng(70 + M)
    label = rng.integers(-1, C + 1, (B, H, W)).astype(np.int32)
    inst = rng.integers(0, 3, (B, H, W)).astype(np.int32)
    obj = np.zeros((B, M, 6), F)
    obj[..., 0] = 1 + (np.arange(M) * 7) % (C - 1)
    obj[..., 1] = rng.integers(0, 3, (B, M))
    obj[..., 2] = rng.uniform(-W, 2 * W, (B, M))
    obj[..., 3] = rng.uniform(-H, 2 * H, (B, M))
    obj[..., 4:] = rng.uniform(-1, 1, (B, M, 2))
    return dict(label=label, inst=inst, obj=obj, C=C)


_BUILD = {"adl": _build_adl, "hough": _build_hough, "roi_fwd": _build_roi_fwd, "roi_bwd": _build_roi_bwd,
          "render": _build_render, "backproject": _build_backproject, "vertex": _build_vertex}


@functools.lru_cache(maxsize=None)
def build(case_id):
    return _BUILD[CASE[case_id]["op"]](CASE[case_id])


# =====================================================================================================================
# the oracle's outputs (computed once per case; callers must not modify them)
HOUGH_PER_THR = 0.0


@functools.lru_cache(maxsize=None)
def reference(case_id):
    import oracle
    c, d = CASE[case_id], build(case_id)
    op = c["op"]
    if op == "adl":
        R = d["R"]
        loss, diff = oracle.average_distance(d["pred"][:R], d["tgt"][:R], d["wgt"][:R], d["pts"], d["sym"], d["margin"])
        return dict(loss=loss, diff=diff)
    if op == "hough":
        out = oracle.hough_voting(d["label"], d["vertex"], d["ext"], d["meta"], None, 0, c["vote_thr"], HOUGH_PER_THR, c["skip"],
                                  label_thr=c["label_thr"], padded=True)
        return dict(zip(("top_box", "top_pose", "top_target", "top_weight", "top_domain", "num_rois"), out))
    if op == "roi_fwd":
        top, arg = oracle.roi_pool(d["data"], d["rois"], d["PH"], d["PW"], d["scale"], 0)
        return dict(top=top, argmax=arg)
    if op == "roi_bwd":
        top, arg = oracle.roi_pool(d["data"], d["rois"], d["PH"], d["PW"], d["scale"], 0)
        out = dict(top=top, argmax=arg)
        if "grad" in d:
            B, H, W, C = d["data"].shape
            out["bottom_diff"] = oracle.roi_pool_bwd(d["grad"], d["rois"], arg, B, H, W, C, d["PH"], d["PW"], d["scale"], 0)
        return out
    if op == "render":
        return oracle.render_mesh(d["vertices"], smooth_normals(d["vertices"], d["faces"]), d["faces"], d["pose"], d["K"], d["H"], d["W"],
                                  want=("vertices", "normals", "canonical"))
    if op == "backproject":
        td, tl, tf = oracle.backproject(d["data"], d["label"], d["depth"], d["meta"], d["label3d"], d["G"], d["k"], d["thr"])
        return dict(top_data=td, top_label=tl, top_flag=tf)
    if op == "vertex":
        import vertex_ref
        if c["M"] > 64:
            return {}
        t, w = vertex_ref.vertex_targets(d["label"], d["obj"], d["C"], d["inst"])
        return dict(targets=t, weights=w)
    raise KeyError(op)


def smooth_normals(v, f):
    """posecnn_amd.icp.Mesh.smooth_normals restated (that module needs torch; the audit does not)."""
    v = np.asarray(v, np.float64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    return (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)).astype(F)


# =====================================================================================================================
# RoiGeom / bin_span of csrc/roi_pool.hip restated (beside np_ref.roi_pool, which uses the same expressions inline)
def roi_geom(roi, scale, PH, PW):
    from np_ref import c_round
    sw, sh, ew, eh = (c_round(F(roi[k]) * F(scale)) for k in (2, 3, 4, 5))
    return dict(batch=int(roi[0]), cls=int(roi[1]), sw=sw, sh=sh, ew=ew, eh=eh,
                bin_h=F(max(eh - sh + 1, 1)) / F(PH), bin_w=F(max(ew - sw + 1, 1)) / F(PW))


def bin_span(bin_, p, start, limit):
    lo = min(max(int(np.floor(F(p) * bin_)) + start, 0), limit)
    hi = min(max(int(np.ceil(F(p + 1) * bin_)) + start, 0), limit)
    return lo, hi


def roi_staged_words(d, chunk=32):
    """ncols * cc * per_col of every (roi, bin row, channel chunk) workgroup of roi_pool_fwd_staged that has work."""
    B, H, W, C = d["data"].shape
    per_col = 2 if d["argmax"] else 1
    words = []
    for roi in d["rois"]:
        g = roi_geom(roi, d["scale"], d["PH"], d["PW"])
        w0, _ = bin_span(g["bin_w"], 0, g["sw"], W)
        _, w1 = bin_span(g["bin_w"], d["PW"] - 1, g["sw"], W)
        for ph in range(d["PH"]):
            hlo, hhi = bin_span(g["bin_h"], ph, g["sh"], H)
            if not (0 <= g["batch"] < B) or hhi <= hlo:
                continue
            for c0 in range(0, C, chunk):
                words.append(max(w1 - w0, 0) * min(chunk, C - c0) * per_col)
    return words


def roi_bwd_passes(d, list_cap, tile_w=8):
    """The compaction passes of roi_pool_bwd_binned for the (image, row, tile) that the most ROIs hit: counts per pass."""
    B, H, W, C = d["data"].shape
    geo = [roi_geom(r, d["scale"], d["PH"], d["PW"]) for r in d["rois"]]
    best = []
    for n in range(B):
        for h in range(H):
            for w_lo in range(0, W, tile_w):
                w_hi = min(W, w_lo + tile_w)
                hit = np.array([g["batch"] == n and g["sh"] <= h <= max(g["eh"], g["sh"]) and w_lo <= max(g["ew"], g["sw"])
                                and w_hi - 1 >= g["sw"] for g in geo])
                passes, cursor = [], 0
                while cursor < len(geo):
                    count, r = 0, cursor
                    while r < len(geo) and count <= list_cap - 64:
                        count += int(hit[r:r + 64].sum())
                        r += 64
                    passes.append(count)
                    cursor = r
                if sum(passes) > sum(best):
                    best = passes
    return best


# =====================================================================================================================
# classifiers: case -> {row id: set of regime keys reached}
def _adl_facts(d):
    R = d["R"]
    C = d["sym"].shape[0]
    w = d["wgt"][:R].reshape(R, C, 4)[:, :, 0] > 0
    cls = np.where(w.any(1), w.argmax(1), -1)                 # the first positive weight names the class
    with_target = cls >= 0
    symmetric = with_target & (d["sym"][np.maximum(cls, 0)] > 0)
    return dict(R=R, P=d["pts"].shape[1], targets=int(with_target.sum()), symmetric=int(symmetric.sum()), cls=cls, C=C)


def _rel(v, t, name):
    return {t - 1: "%s = t - 1", t: "%s = t", t + 1: "%s = t + 1", 2 * t: "%s = 2t", 2 * t + 1: "%s = 2t + 1"}.get(v, "%s far from t") % name


def _classify_adl(c, d, ref):
    f = _adl_facts(d)
    P, out = f["P"], {}
    if f["targets"]:
        t = ROW["adl_sum_tile"]["constants"]["ADL_SUM_TILE_MAX"]
        rounds, last, vec = -(-P // t), P - (-(-P // t) - 1) * t, P % 4 == 0       # (the workspace is 256-byte aligned)
        if rounds == 1:
            key = "one full round, float4" if (P == t and vec) else "one partial round"
        elif P == t + 1:
            key = "second round of one term, scalar"
        elif not vec:
            key = "scalar staging in every round"
        elif rounds == 2 and last < 16:
            key = "second round under one trip, float4"
        elif rounds == 2 and last == t:
            key = "two exact rounds"
        elif rounds == 3 and 16 <= last < 32:
            key = "third ragged round with a full trip"
        else:
            key = "%d rounds, last of %d" % (rounds, last)
        out["adl_sum_tile"] = {key}
    if f["symmetric"]:
        out["adl_qtile"] = {_rel(P, ROW["adl_qtile"]["constants"]["ADL_QTILE"], "P")}
    out["adl_rows"] = {_rel(f["R"], ROW["adl_rows"]["constants"]["ADL_ORDER_THREADS"], "R")}
    out["adl_row_slots"] = {_rel(f["targets"], ROW["adl_row_slots"]["constants"]["ADL_ROW_SLOTS"], "targets")}
    return out


def hough_facts(c, d, ref):
    """Per class: pixels, records m, and the oracle's rows for it; every blob of these cases must vote for its centre as one
    (the emitted row of the centre cell carries exactly m votes), so the voter flags of its records are all ones."""
    label = d["label"][0]
    H, W = label.shape
    n = int(ref["num_rois"][1])
    rows = ref["top_box"][:n]
    facts = {}
    for cls, row0, npix, (cx, cy) in c["blobs"]:
        pixels = int((label == cls).sum())
        m = -(-pixels // c["skip"])
        at = [i for i in range(n) if int(rows[i, 1]) == cls and abs((rows[i, 2] + rows[i, 4]) / 2 - cx) < 0.01
              and abs((rows[i, 3] + rows[i, 5]) / 2 - cy) < 0.01]
        if c["id"].startswith(("hough_wcd", "hough_sel")):
            assert len(at) == 1, "%s: class %d: no row (or several) for the cell (%d, %d): %s" % (c["id"], cls, cx, cy, rows[:, :7])
        facts[cls] = dict(pixels=pixels, m=m, row=at[0] if at else None, votes=float(rows[at[0], 6]) if at else None)
    slots = sum(1 for k in range(1, c["C"]) if int((label == k).sum()) > c["label_thr"])
    return dict(H=H, W=W, classes=facts, slots=slots)


def wcd_flushes(flags, cap):
    """wave_cell_data's strip: flags in record order, batches of 64; -> (flushes inside the loop, fill at each flush, fill left)."""
    fill, at = 0, []
    for b0 in range(0, len(flags), 64):
        fill += int(np.sum(flags[b0:b0 + 64]))
        if fill > cap - 64:
            at.append(fill)
            fill = 0
    return at, fill


def select_flushes(flags, nt, cap):
    """hv_select_kernel's compaction: trips of nt records; -> [(fill, capacity flush?, last trip?)] per flush."""
    fill, out = 0, []
    for b0 in range(0, len(flags), nt):
        fill += int(np.sum(flags[b0:b0 + nt]))
        last = b0 + nt >= len(flags)
        if fill > cap - nt or last:
            out.append((fill, fill > cap - nt, last))
            fill = 0
    return out


def _classify_hough(c, d, ref):
    f = hough_facts(c, d, ref)
    out = {}
    tw = ROW["hough_wcd"]["constants"]["WCD_CAP"]
    cons = ROW["hough_select"]["constants"]
    keys_w, keys_s, keys_m = set(), set(), set()
    for cls, k in f["classes"].items():
        if c["id"].startswith(("hough_wcd", "hough_sel")):
            assert k["votes"] == k["m"], "%s: class %d: %g votes of %d records" % (c["id"], cls, k["votes"], k["m"])
        flags = np.ones(k["m"], bool) if k["votes"] == k["m"] else None
        keys_m.add(_rel(k["m"], ROW["hough_rchunk"]["constants"]["HV_RCHUNK"], "m"))
        if flags is None:
            continue
        if c["vote_thr"] > 0:
            at, left = wcd_flushes(flags, tw)
            if not at:
                key = "no flush, fill = WCD_CAP - 64" if left == tw - 64 else ("no flush, far below" if left < tw // 2 else "no flush")
            elif len(at) == 1:
                key = {tw - 63: "one flush, fill = WCD_CAP - 63", tw: "one flush, strip full"}.get(at[0], "one flush")
            else:
                key = {2: "two flushes"}.get(len(at), "%d flushes" % len(at))
            if k["row"] == 0 and key != "no flush, far below":
                key += " (first maximum)"
            keys_w.add(key)
        else:
            fl = select_flushes(flags, cons["HV_SEL_NT"], cons["SEL_CAP"])
            cap_fl = [x for x in fl if x[1]]
            if k["m"] <= cons["HV_SEL_NT"]:
                key = "one trip"
            elif not cap_fl:
                key = "fill = t, no capacity flush" if fl[-1][0] == cons["SEL_CAP"] - cons["HV_SEL_NT"] else "several trips, no capacity flush"
            elif cap_fl[0][2]:
                key = "capacity flush on the last trip"
            else:
                key = "capacity flush with records to come"
            keys_s.add(key)
    out["hough_rchunk"] = keys_m
    if keys_w:
        out["hough_wcd"] = keys_w
    if keys_s:
        out["hough_select"] = keys_s
    out["hough_chunk"] = {_rel(f["H"] * f["W"], ROW["hough_chunk"]["constants"]["HV_CHUNK"], "HW")}
    if c["vote_thr"] > 0:
        out["hough_lm_chunk"] = {_rel(f["slots"] * f["H"] * f["W"], ROW["hough_lm_chunk"]["constants"]["LM_CHUNK"], "cells")}
    return out


def _classify_roi_fwd(c, d, ref):
    cons = ROW["roi_lds"]["constants"]
    t, col = cons["RP_LDS_WORDS"], cons["RP_CHUNK"] * (2 if d["argmax"] else 1)
    pre = "argmax" if d["argmax"] else "no argmax"
    keys = set()
    for w in roi_staged_words(d, cons["RP_CHUNK"]):
        name = {t - col: "words = t - one column", t: "words = t", t + col: "words = t + one column"}.get(w)
        if name:
            keys.add("%s: %s" % (pre, name))
    return {"roi_lds": keys}


def _classify_roi_bwd(c, d, ref):
    cons = ROW["roi_bwd_list"]["constants"]
    passes = roi_bwd_passes(d, cons["RB_LIST"], cons["RB_TILE_W"])
    for r in ROW["roi_bwd_list"]["regimes"]:
        if r["passes"] == passes:
            return {"roi_bwd_list": {r["key"]}}
    short = len(passes) == 1 and passes[0] < (cons["RB_LIST"] - 64) // 2
    return {"roi_bwd_list": {"one short pass" if short else "passes %s" % passes}}


def render_box(d):
    """rd_setup of csrc/render.hip restated in float32 for the first face: (box pixels, signed doubled area)."""
    T = d["pose"].reshape(-1, 12)[0].astype(F)
    K = d["K"]
    fx, fy, px, py = (F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2]))
    u, v = [], []
    for i in d["faces"][0]:
        x, y, z = d["vertices"][i].astype(F)
        cx = F(F(F(T[0] * x) + F(T[1] * y)) + F(T[2] * z)) + T[3]
        cy = F(F(F(T[4] * x) + F(T[5] * y)) + F(T[6] * z)) + T[7]
        cz = F(F(F(T[8] * x) + F(T[9] * y)) + F(T[10] * z)) + T[11]
        u.append(F(F(cx / cz) * fx) + px)
        v.append(F(F(cy / cz) * fy) + py)
    x0, x1 = max(0, math.ceil(min(u))), min(d["W"] - 1, math.floor(max(u)))
    y0, y1 = max(0, math.ceil(min(v))), min(d["H"] - 1, math.floor(max(v)))
    area = float(u[1] - u[0]) * float(v[2] - v[0]) - float(v[1] - v[0]) * float(u[2] - u[0])
    return (x1 - x0 + 1) * (y1 - y0 + 1), area


def _classify_render(c, d, ref):
    box, area = render_box(d)
    t = ROW["render_small"]["constants"]["RD_SMALL"]
    covered = int(np.isfinite(ref["vertices"][0, :, :, 0]).sum())
    assert covered > box // 4, "%s: the triangle covers %d pixels of a box of %d" % (c["id"], covered, box)
    rel = {t - 1: "t - 1", t: "t", t + 1: "t + 1", t + 2: "t + 2"}.get(box, "far from t")
    return {"render_small": {"%s, box = %s" % ("ccw" if area > 0 else "cw", rel)}}


PASS_ALL = 50.0     # a backproject threshold every depth of these cases passes


def backproject_windows(d):
    """Per voxel whose window meets the image, from the oracle alone: at a threshold every depth passes, a voxel's outputs
    are means over its whole clipped window, and the means of x and x^2 give that window's centre and width (likewise y):
    var = (n^2 - 1) / 12. -> (voxel mask, pixels in the window, table column and row of the window's centre)."""
    import oracle
    B, H, W, _ = d["data"].shape
    k = d["k"]
    assert np.isfinite(d["depth"]).all() and float(np.abs(d["depth"]).max()) + 10 < PASS_ALL
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    probe = np.stack([xx, xx * xx, yy, yy * yy], -1)[None].astype(F)
    td, _, tf = oracle.backproject(probe, d["label"], d["depth"], d["meta"], d["label3d"], d["G"], k, PASS_ALL)
    mask = tf.reshape(-1, 4)[:, 0] > 0
    m = td.reshape(-1, 4).astype(np.float64)[mask]
    nx = np.rint(np.sqrt(12 * (m[:, 1] - m[:, 0] ** 2) + 1))
    ny = np.rint(np.sqrt(12 * (m[:, 3] - m[:, 2] ** 2) + 1))
    x0, x1 = m[:, 0] - (nx - 1) / 2, m[:, 0] + (nx - 1) / 2
    y0, y1 = m[:, 2] - (ny - 1) / 2, m[:, 2] + (ny - 1) / 2
    col = np.rint(np.where(x0 < 0.5, x1 - k, x0 + k) + k).astype(int)      # a window clipped on the left ends at its centre + k
    row = np.rint(np.where(y0 < 0.5, y1 - k, y0 + k) + k).astype(int)
    return mask, (nx * ny).astype(int), col, row


def _classify_backproject(c, d, ref):
    cons = ROW["backproject_tile"]["constants"]
    B, H, W, _ = d["data"].shape
    k = d["k"]
    assert k == cons["KMAX"]
    mask, pixels, col, row = backproject_windows(d)
    hit = ref["top_flag"].reshape(-1, ref["top_flag"].shape[-1])[:, 0][mask] > 0
    out = {}
    if d["thr"] >= PASS_ALL:
        assert hit.all() and pixels.max() <= ROW["backproject_list"]["constants"]["LIST"]
        out["backproject_list"] = {"%d hits" % pixels.max()}
        return out
    Wc, Hc = W + 2 * k, H + 2 * k
    dw, dh = Wc - cons["TW"], Hc - cons["TH"]
    key = {(-1, -1): "table = tile - 1", (0, 0): "table = tile", (1, 1): "table = tile + 1"}.get((dw, dh), "table = tile %+d x %+d" % (dw, dh))
    # the skip test must decide something there: voxels that hit and voxels that miss, both with their table entry in
    # the table's last column, and hits in its last row (for tile + 1 those entries are the second tiles')
    decided = (hit.any() and (~hit).any() and (col[hit] == Wc - 1).any() and (col[~hit] == Wc - 1).any() and (row[hit] == Hc - 1).any())
    out["backproject_tile"] = {key if decided else key + " (its edge entries decide nothing)"}
    return out


def _classify_vertex(c, d, ref):
    M = d["obj"].shape[1]
    key = _rel(M, ROW["vertex_objects"]["constants"]["VT_MAX_OBJECTS"], "M")
    return {"vertex_objects": {key + ": PCNN_EINVAL" if M > 64 else key}}


_CLASSIFY = {"adl": _classify_adl, "hough": _classify_hough, "roi_fwd": _classify_roi_fwd, "roi_bwd": _classify_roi_bwd,
             "render": _classify_render, "backproject": _classify_backproject, "vertex": _classify_vertex}


def classify(case_id):
    c = CASE[case_id]
    return _CLASSIFY[c["op"]](c, build(case_id), reference(case_id))


def coverage(cases=None):
    """{row id: {regime key: [case ids]}} over the regimes the cases CLAIM (the audit checks each claim against classify())."""
    cases = CASES if cases is None else cases
    cov = {r["id"]: {g["key"]: [] for g in r["regimes"]} for r in ROWS}
    for c in cases:
        for row, keys in c["claims"].items():
            for k in keys:
                cov[row][k].append(c["id"])
    return cov


def uncovered(cases=None):
    """The (row, what) pairs the cases leave open: a regime without a case, or a side of the constant without one."""
    cov = coverage(cases)
    missing = []
    for r in ROWS:
        sides = set()
        for g in r["regimes"]:
            if cov[r["id"]][g["key"]]:
                sides.add(g["side"])
            else:
                missing.append((r["id"], "regime '%s' (%s the threshold)" % (g["key"], g["side"])))
        for s in r.get("sides", ("below", "at", "above")):
            if s not in sides:
                missing.append((r["id"], "no case %s the threshold" % s))
    return missing
