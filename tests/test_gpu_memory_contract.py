"""The memory contract of include/posecnn_hip.h ("Conventions") for every entry that launches work: the library touches only
the caller's outputs and a workspace of exactly `pcnn_*_workspace_bytes`, never writes its inputs, and its results do not
depend on what the memory held before the call.

Every case runs twice through the public call, once under each poison pattern of tests/memguard.py (P1: 0xFF bytes, body
at 0 mod 256; P2: the largest finite value / zero bytes, body at 16 mod 256), with every allocation of posecnn_amd.ops and
posecnn_amd.icp inside a 1 MiB guard on each side, fresh workspace and ticket caches (each workspace exactly the size the
library asked for) and a recording stand-in for the library handle. Both runs must leave every guard and every input
intact and the fc_skinny tickets at zero, agree bit for bit, reach the `covers` entries, and match the reference (and
tolerance) of the op's existing test. Then the stale-state checks: a workspace reused after a larger call, the fc_skinny
exchange on a NaN-poisoned workspace, and graph replays with new inputs."""
import contextlib

import numpy as np
import pytest

import icp_scene as S
import memguard
import oracle
from posecnn_amd import config, synth
from test_gpu_hough import NAMES as HOUGH_NAMES, frames, lowres_case
from test_gpu_ops import (adl_case, backproject_case, np_wino43_input, np_wino43_output, np_wino_input, np_wino_output,
                          random_rois, same)

pytestmark = pytest.mark.gpu
F = np.float32


class Case:
    """make() -> inputs (seeded; numpy arrays or tensors); run(c) -> {name: tensor} through the public call under the guard;
    check(d, out) compares the numpy outputs with the reference. keep / zero: regions left untouched / written as zeros
    by contract."""

    def __init__(self, name, covers, make, run, check, keep=None, zero=None):
        self.name, self.covers, self.make, self.run, self.check = name, tuple(covers), make, run, check
        self.keep, self.zero = keep or {}, zero or {}


CASES = []


def add(name, covers, make, run, check, keep=None, zero=None):
    assert name not in {c.name for c in CASES}, name
    CASES.append(Case(name, covers, make, run, check, keep, zero))


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda:0")


def G(seed):
    """A seeded CPU generator (inputs are made on the host and embedded byte for byte)."""
    return _torch().Generator(device="cpu").manual_seed(seed)


class Ctx:
    def __init__(self, g, rec, data):
        self.g, self.rec, self.d = g, rec, data

    def e(self, key, mutable=False):
        v = self.d[key] if isinstance(key, str) else key
        return None if v is None else self.g.embed(v, "cuda", mutable=mutable)


@contextlib.contextmanager
def guarded(pattern):
    from posecnn_amd import _lib, icp, ops
    g = memguard.GuardedTorch(pattern, devices=("cuda",))
    rec = memguard.Recorder(_lib.lib())
    with pytest.MonkeyPatch.context() as mp:
        for mod in (ops, icp):
            mp.setattr(mod, "torch", g)
            mp.setattr(mod, "lib", lambda: rec)
        mp.setattr(ops, "_default_ws", {})
        mp.setattr(ops, "_tickets", {})
        yield g, rec


def _finish(g):
    from posecnn_amd import ops
    torch = _torch()
    torch.cuda.synchronize()
    g.check()
    for buf in ops._tickets.values():
        assert int(buf.abs().max()) == 0, "fc_skinny tickets not back at zero"


def _numpy(out):
    return {k: memguard.to_numpy(v) for k, v in out.items()}


def execute(case):
    data = case.make()
    runs, calls = {}, set()
    for p in memguard.PATTERNS:
        with guarded(p) as (g, rec):
            out = case.run(Ctx(g, rec, data))
            _finish(g)
            runs[p] = _numpy(out)
            calls |= set(rec.calls)
    memguard.compare_patterns(runs, keep=case.keep, zero=case.zero)
    missing = set(case.covers) - calls
    assert not missing, "%s never reached %s (called: %s)" % (case.name, sorted(missing), sorted(calls))
    case.check(data, runs["P1"])
    return data, runs["P1"]


def _ptr(t):
    from posecnn_amd import ops
    return ops._ptr(t)


def _rel_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) if ref.size else 0.0


# =====================================================================================================================
# Hough voting (tests/test_gpu_hough.py: oracle.hough_voting, bit-exact)
def _hough(name, first, B, H, W, C, n_obj, lt, vote=-1.0, per=0.02, train=0, rpi=0, with_gt=False):
    def make():
        label, vertex, meta, fr = frames(first, B, H=H, W=W, C=C, n_obj=n_obj)
        gt = None
        if with_gt:
            rng = np.random.default_rng(0)
            gts = []
            for n in range(B):
                for (cls, cx, cy, z) in fr[n]["objects"]:
                    q = synth.random_unit_quats(rng, 1)[0]
                    K = fr[n]["K"]
                    gts.append([n, cls, 0, 0, 0, 0, q[0], q[1], q[2], q[3], (cx - K[0, 2]) / K[0, 0] * z, (cy - K[1, 2]) / K[1, 1] * z, z])
            gt = np.array(gts, F)
        return dict(label=label, vertex=vertex, ext=np.ascontiguousarray(config.LOV_EXTENTS[:C]), meta=meta, gt=gt)

    def run(c):
        from posecnn_amd import ops
        out = ops.hough_voting_gpu_padded(c.e("label"), c.e("vertex"), c.e("ext"), c.e("meta"), c.e("gt"), train, vote, per, 10,
                                          label_threshold=lt, rois_per_image=rpi)
        return dict(zip(HOUGH_NAMES, out))

    def check(d, o):
        want = oracle.hough_voting(d["label"], d["vertex"], d["ext"], d["meta"], d["gt"], train, vote, per, 10, label_thr=lt,
                                   padded=True, rois_per_image=rpi)
        for n, w in zip(HOUGH_NAMES, want):
            same(o[n], w, n)
        assert int(o["num_rois"][0]) >= 1
    add(name, ("pcnn_hough_voting_fwd",), make, run, check)


_hough("hough_17x19", 31, 1, 17, 19, 22, 2, 5)
_hough("hough_33x2049", 32, 1, 33, 2049, 22, 3, 20)
_hough("hough_b16_cap8", 40, 16, 240, 320, 22, 9, 150)
_hough("hough_threshold", 60, 1, 120, 160, 22, 3, 60, vote=4.0)
_hough("hough_train", 100, 2, 240, 320, 22, 4, 150, train=1, with_gt=True)
_hough("hough_rois_per_image", 41, 3, 96, 128, 22, 4, 40, rpi=2)


def _hough_lowres(name, B, H, W, C, n_obj, k, s, lt):
    def make():
        label, z, bias, meta = lowres_case(500 + H, B, H, W, C, n_obj, s)
        return dict(label=label, z=z, bias=bias, ext=np.ascontiguousarray(config.LOV_EXTENTS[:C]), meta=meta)

    def run(c):
        from posecnn_amd import ops
        out = ops.hough_voting_gpu_lowres_padded(c.e("label"), c.e("z"), c.e("bias"), k, s, c.e("ext"), c.e("meta"), None, 0, -1.0,
                                                 0.02, 10, label_threshold=lt)
        return dict(zip(HOUGH_NAMES, out))

    def check(d, o):
        want = oracle.hough_voting(d["label"], oracle.deconv_bilinear(d["z"], k, s, None, None, d["bias"], False), d["ext"], d["meta"],
                                   None, 0, -1.0, 0.02, 10, label_thr=lt, padded=True)
        for n, w in zip(HOUGH_NAMES, want):
            same(o[n], w, n)
    add(name, ("pcnn_hough_voting_lowres_fwd",), make, run, check)


def _hough_threshold_case(name, case_id):
    """A case of tests/thresholds.py: wave_cell_data flushes its LDS strip twice for the second maximum."""
    import thresholds as TH
    case = TH.CASE[case_id]

    def run(c):
        from posecnn_amd import ops
        out = ops.hough_voting_gpu_padded(c.e("label"), c.e("vertex"), c.e("ext"), c.e("meta"), None, 0, case["vote_thr"],
                                          TH.HOUGH_PER_THR, case["skip"], label_threshold=case["label_thr"])
        return dict(zip(HOUGH_NAMES, out))

    def check(d, o):
        want = TH.reference(case_id)
        for n in HOUGH_NAMES:
            same(o[n], want[n], n)
        assert int(o["num_rois"][1]) >= 2
    add(name, ("pcnn_hough_voting_fwd",), lambda: dict(TH.build(case_id)), run, check)


_hough_threshold_case("hough_strip_flushes", "hough_wcd_2000")
_hough_lowres("hough_lowres_k4s2", 3, 120, 160, 8, 3, 4, 2, 60)
_hough_lowres("hough_lowres_k16s8", 1, 96, 136, 6, 2, 16, 8, 40)


def _hough_bwd_make():
    rng = np.random.default_rng(2)
    return dict(label=np.zeros((2, 17, 19), np.int32), vertex=rng.standard_normal((2, 17, 19, 15)).astype(F))


def _hough_bwd_run(c):
    from posecnn_amd import ops
    gl, gv = ops.hough_voting_grad(c.e("label"), c.e("vertex"))
    return dict(grad_label=gl, grad_vertex=gv)


def _hough_bwd_check(d, o):
    assert o["grad_label"].shape == (2, 17, 19) and o["grad_vertex"].shape == (2, 17, 19, 15)


add("hough_bwd", ("pcnn_hough_voting_bwd",), _hough_bwd_make, _hough_bwd_run, _hough_bwd_check,
    zero={"grad_label": np.s_[:], "grad_vertex": np.s_[:]})


# =====================================================================================================================
# ROI pooling (tests/test_gpu_ops.py, test_gpu_round4.py: oracle.roi_pool / roi_pool_bwd, bit-exact)
def _roi_make():
    rng = np.random.default_rng(12)
    data = rng.standard_normal((2, 12, 17, 22)).astype(F)
    rois = random_rois(rng, 31, 2, 22, 17 * 4, 12 * 4)
    rois[5, 0] = 9                                   # invalid batch index
    rois[6, 0] = -1
    rois[7, 2:6] = [400, 300, 500, 420]              # entirely outside the image
    rois[8, 2:6] = [-90, -80, -40, -30]
    g = {(pc, ph, pw): rng.standard_normal((31, ph, pw, 1 if pc else 22)).astype(F) for pc in (0, 1) for (ph, pw) in ((7, 7), (3, 5))}
    return dict(data=data, rois=rois, grads=g)


def _roi_run(c):
    torch = _torch()
    from posecnn_amd import ops
    out = {}
    rois = c.e("rois")
    for (pc, ph, pw), gr in c.d["grads"].items():
        d = c.e("data").requires_grad_(True)
        top, arg = ops.roi_pool(d, rois, ph, pw, 0.25, pc)
        (gd,) = torch.autograd.grad(top, d, grad_outputs=c.e(gr))
        tag = "pc%d_%dx%d" % (pc, ph, pw)
        out["top_" + tag], out["argmax_" + tag], out["grad_" + tag] = top.detach(), arg, gd
    top0, arg0 = ops.roi_pool(c.e("data"), c.e(c.d["rois"][:0]), 7, 7, 0.25, 0)
    out["top_empty"], out["argmax_empty"] = top0, arg0
    return out


def _roi_check(d, o):
    B, H, W, C = d["data"].shape
    for (pc, ph, pw), gr in d["grads"].items():
        tag = "pc%d_%dx%d" % (pc, ph, pw)
        wt, wa = oracle.roi_pool(d["data"], d["rois"], ph, pw, 0.25, pc)
        same(o["top_" + tag], wt, "top " + tag)
        same(o["argmax_" + tag], wa, "argmax " + tag)
        same(o["grad_" + tag], oracle.roi_pool_bwd(gr, d["rois"], wa, B, H, W, C, ph, pw, 0.25, pc), "bottom_diff " + tag)
    assert o["top_empty"].shape == (0, 7, 7, 22)


add("roi_pool_fwd_bwd", ("pcnn_roi_pool_fwd", "pcnn_roi_pool_bwd"), _roi_make, _roi_run, _roi_check)


def _roi_add2(name, R, cap, C):
    def make():
        rng = np.random.default_rng(13)
        a = rng.standard_normal((2, 15, 20, C)).astype(F)
        b = rng.standard_normal((2, 30, 40, C)).astype(F)
        rois = random_rois(rng, cap, 2, 22, 320, 240)
        rois[cap // 2:, 0] = np.where(np.arange(cap - cap // 2) % 5 == 4, 7, rois[cap // 2:, 0])   # invalid batch indices
        if cap > 3:
            rois[3, 2:6] = [900, 700, 990, 800]                                                  # outside the image
        return dict(a=a, b=b, rois=rois, count=np.array([R], np.int32))

    def run(c):
        from posecnn_amd import ops
        a, b, rois, cnt = c.e("a"), c.e("b"), c.e("rois"), c.e("count")
        zero = ops.roi_pool_add2(a, 1 / 16.0, b, 1 / 8.0, rois, num_rows=cnt)
        keep = c.g.empty((cap, 7, 7, C), dtype=_torch().float32, device=_dev())
        ops.roi_pool_add2(a, 1 / 16.0, b, 1 / 8.0, rois, num_rows=cnt, dead_rows="keep", out=keep)
        full = ops.roi_pool_add2(a, 1 / 16.0, b, 1 / 8.0, rois)
        return dict(zero_out=zero, keep_out=keep, all_rows=full)

    def check(d, o):
        for n, rows in (("zero_out", R), ("keep_out", R), ("all_rows", cap)):
            wa, _ = oracle.roi_pool(d["a"], d["rois"][:rows], 7, 7, 1 / 16.0, 0)
            wb, _ = oracle.roi_pool(d["b"], d["rois"][:rows], 7, 7, 1 / 8.0, 0)
            same(o[n][:rows], wa + wb, n)
    add(name, ("pcnn_roi_pool_add2_fwd", "pcnn_roi_pool_add2_live_fwd"), make, run, check,
        keep={"keep_out": np.s_[R:]}, zero={"zero_out": np.s_[R:]})


_roi_add2("roi_pool_add2_9_of_24", 9, 24, 512)
_roi_add2("roi_pool_add2_count0", 0, 5, 512)
_roi_add2("roi_pool_add2_count_cap", 33, 33, 64)
_roi_add2("roi_pool_add2_c20", 5, 40, 20)


# =====================================================================================================================
# Hard label (tests/test_gpu_ops.py, test_gpu_round2.py: oracle.hard_label bit-exact; the gradient entry writes zeros)
def _hard_label(name, shape):
    def make():
        rng = np.random.default_rng(15)
        prob = rng.random(shape).astype(F)
        gt = rng.integers(-1, shape[3], shape[:3]).astype(np.int32)
        k = min(3, gt.size)
        gt.ravel()[:k] = [-5, shape[3] + 2, -1][:k]
        return dict(prob=prob, gt=gt)

    def run(c):
        from posecnn_amd import ops
        p, gt = c.e("prob"), c.e("gt")
        gp, gg = ops.hard_label_grad(p, gt)
        return dict(out_03=ops.hard_label(p, gt, 0.3), out_10=ops.hard_label(p, gt, 1.0), grad_prob=gp, grad_gt=gg)

    def check(d, o):
        same(o["out_03"], oracle.hard_label(d["prob"], d["gt"], 0.3), "hard_label 0.3")
        same(o["out_10"], oracle.hard_label(d["prob"], d["gt"], 1.0), "hard_label 1.0")
    add(name, ("pcnn_hard_label_fwd", "pcnn_hard_label_bwd"), make, run, check,
        zero={"grad_prob": np.s_[:], "grad_gt": np.s_[:]})


_hard_label("hard_label_2x33x47x22", (2, 33, 47, 22))
_hard_label("hard_label_1x1x1x16", (1, 1, 1, 16))
_hard_label("hard_label_1x5x7x3", (1, 5, 7, 3))


# =====================================================================================================================
# Average distance loss (tests/test_gpu_ops.py, test_gpu_round2.py: oracle bit-exact, rows past the count zero)
def _adl(name, R, cap, C, P, margin, backward=False):
    def make():
        rng = np.random.default_rng(23)
        pred, tgt, wgt, pts, sym = adl_case(rng, cap, C, P)
        return dict(pred=pred, tgt=tgt, wgt=wgt, pts=pts, sym=sym, count=np.array([R], np.int32))

    def run(c):
        torch = _torch()
        from posecnn_amd import ops
        p = c.e("pred")
        if backward:
            p.requires_grad_(True)
        loss, diff = ops.average_distance_loss(p, c.e("tgt"), c.e("wgt"), c.e("pts"), c.e("sym"), margin,
                                               num_rows=None if R == cap else c.e("count"))
        out = dict(loss=loss.detach(), diff=diff)
        if backward:
            (gp,) = torch.autograd.grad((loss * 3.0).sum(), p)
            out["grad"] = gp
        return out

    def check(d, o):
        wl, wd = oracle.average_distance(d["pred"][:R], d["tgt"][:R], d["wgt"][:R], d["pts"], d["sym"], margin)
        same(o["loss"], wl, "loss")
        same(o["diff"][:R], wd, "bottom_diff")
        if backward:
            same(o["grad"], oracle.average_distance_bwd(np.array([3.0], F), o["diff"]), "grad")
    covers = ("pcnn_average_distance_fwd",) + (("pcnn_average_distance_bwd",) if backward else ())
    add(name, covers, make, run, check, zero={"diff": np.s_[R:]})


_adl("adl_count0", 0, 4, 22, 700, 0.01)
_adl("adl_count_cap", 16, 16, 22, 700, 0.01, backward=True)
_adl("adl_7_of_16", 7, 16, 22, 2620, 0.0)
_adl("adl_second_sum_round", 5, 8, 22, 3073, 0.0)       # P > ADL_SUM_TILE_MAX: a second staged round of one term; margin 0 keeps it live


# =====================================================================================================================
# smooth_l1_loss_vertex (tests/test_gpu_training.py: oracle bit-exact, forward and backward)
def _smooth_l1(name, n, sigma):
    def make():
        rng = np.random.default_rng(52)
        p = (rng.standard_normal(n) * 2).astype(F)
        t = (rng.standard_normal(n) * 2).astype(F)
        w = (rng.random(n) < 0.3).astype(F)
        if n == 1:
            w[:] = 1
        return dict(p=p, t=t, w=w)

    def run(c):
        torch = _torch()
        from posecnn_amd import ops
        p = c.e("p").requires_grad_(True)
        loss = ops.smooth_l1_loss_vertex(p, c.e("t"), c.e("w"), sigma)
        (gp,) = torch.autograd.grad(loss * 5.0, p)
        return dict(loss=loss.detach().reshape(1), grad=gp)

    def check(d, o):
        out, grad = oracle.smooth_l1_vertex(d["p"], d["t"], d["w"], sigma)
        same(o["loss"], out[:1], "loss")
        same(o["grad"], (grad * F(5.0)).astype(F), "grad")
    add(name, ("pcnn_smooth_l1_vertex_fwd", "pcnn_smooth_l1_vertex_bwd"), make, run, check)


_smooth_l1("smooth_l1_n1", 1, 1.0)
_smooth_l1("smooth_l1_n300001", 300001, 3.0)


# =====================================================================================================================
# Backprojecting (tests/test_gpu_ops.py, test_gpu_round6.py: oracle bit-exact)
def _backproject(name, B, H, W, Cd, Cl, G_, k, direct=False, backward=False):
    def make():
        rng = np.random.default_rng(19)
        data, label, depth, meta, label3d = backproject_case(rng, B, H, W, Cd, Cl, G_)
        g = rng.standard_normal((B, G_, G_, G_, Cd)).astype(F)
        return dict(data=data, label=label, depth=depth, meta=meta, m4=meta.reshape(B, 1, 1, 48), label3d=label3d, g=g)

    def run(c):
        torch = _torch()
        from posecnn_amd import ops
        d = c.e("data")
        if backward:
            d.requires_grad_(True)
        lab, dep, m4, l3 = c.e("label"), c.e("depth"), c.e("m4"), c.e("label3d")
        td, tl, tf = ops.backproject(d, lab, dep, m4, l3, G_, k, 0.05)
        out = dict(top_data=td.detach(), top_label=tl, top_flag=tf)
        if backward:
            (gd,) = torch.autograd.grad(td, d, grad_outputs=c.e("g"))
            out["grad"] = gd
        if direct:   # the workspace-less entry, straight through the C-ABI
            f32 = torch.float32
            pd = c.g.empty((B, G_, G_, G_, Cd), dtype=f32, device=_dev())
            pl = c.g.empty((B, G_, G_, G_, Cl), dtype=f32, device=_dev())
            pf = c.g.empty((B, G_, G_, G_, Cd), dtype=f32, device=_dev())
            from posecnn_amd import _lib
            rc = c.rec.pcnn_backproject_fwd(_ptr(d), _ptr(lab), _ptr(dep), _ptr(m4), _ptr(l3), B, H, W, Cd, Cl, 48, G_, k, 0.05,
                                            _ptr(pd), _ptr(pl), _ptr(pf), ops._stream(pd))
            _lib.check("pcnn_backproject_fwd", rc)
            out.update(direct_data=pd, direct_label=pl, direct_flag=pf)
        return out

    def check(d, o):
        wd, wl, wf = oracle.backproject(d["data"], d["label"], d["depth"], d["meta"], d["label3d"], G_, k, 0.05)
        same(o["top_data"], wd, "top_data"); same(o["top_flag"], wf, "top_flag"); same(o["top_label"], wl, "top_label")
        if direct:
            same(o["direct_data"], wd, "direct top_data"); same(o["direct_flag"], wf, "direct top_flag")
            same(o["direct_label"], wl, "direct top_label")
        if backward:
            want = oracle.backproject_bwd(d["g"], d["depth"], d["meta"], B, H, W, Cd, G_)
            same(o["grad"], want, "bottom_diff")
    covers = ("pcnn_backproject_ws_fwd",) + (("pcnn_backproject_fwd",) if direct else ()) + (("pcnn_backproject_bwd",) if backward else ())
    add(name, covers, make, run, check)


_backproject("backproject_ws_k3", 1, 20, 24, 4, 3, 5, 3, direct=True, backward=True)
_backproject("backproject_no_ws_k4", 1, 24, 32, 64, 22, 10, 4, direct=True)
_backproject("backproject_cl257_k0", 1, 16, 20, 4, 257, 6, 0, direct=True)
_backproject("backproject_big_k2", 2, 24, 32, 32, 22, 9, 2)


# =====================================================================================================================
# Label head epilogues (tests/test_gpu_ops.py, test_gpu_round3.py, test_gpu_round5.py: oracle bit-exact)
def _softmax(name, shape):
    def make():
        rng = np.random.default_rng(16)
        score = np.maximum(rng.standard_normal(shape) * 4, 0).astype(F)
        score.reshape(-1, shape[3])[0] = 0
        score.reshape(-1, shape[3])[1] = 200
        return dict(score=score)

    def run(c):
        from posecnn_amd import ops
        s = c.e("score")
        prob, lab = ops.softmax_argmax(s)
        _, lab2 = ops.softmax_argmax(s, want_prob=False)
        return dict(prob=prob, label=lab, label_only=lab2)

    def check(d, o):
        wp, wl = oracle.softmax_argmax(d["score"])
        same(o["prob"], wp, "prob"); same(o["label"], wl, "label"); same(o["label_only"], wl, "label only")
    add(name, ("pcnn_softmax_argmax_fwd",), make, run, check)


_softmax("softmax_2x17x31x22", (2, 17, 31, 22))
_softmax("softmax_3x4x4x2", (3, 4, 4, 2))
_softmax("softmax_1x9x9x40", (1, 9, 9, 40))


def _deconv(name, shape, k, s):
    B, H, W, C = shape

    def make():
        rng = np.random.default_rng(22)
        return dict(x=rng.standard_normal(shape).astype(F), a1=rng.standard_normal((B, H * s, W * s, C)).astype(F),
                    a2=rng.standard_normal((B, H * s, W * s, C)).astype(F), bias=rng.standard_normal(C).astype(F),
                    g=rng.standard_normal((B, H * s, W * s, C)).astype(F))

    def run(c):
        from posecnn_amd import ops
        x = c.e("x")
        return dict(out=ops.deconv_bilinear(x, k, s),
                    fused=ops.deconv_bilinear(x, k, s, add1=c.e("a1"), add2=c.e("a2"), bias=c.e("bias"), relu=True),
                    grad_in=ops.deconv_bilinear_grad(c.e("g"), k, s))

    def check(d, o):
        same(o["out"], oracle.deconv_bilinear(d["x"], k, s), "deconv")
        same(o["fused"], oracle.deconv_bilinear(d["x"], k, s, d["a1"], d["a2"], d["bias"], True), "deconv + adds + bias + relu")
        same(o["grad_in"], oracle.deconv_bilinear_bwd(d["g"], k, s), "deconv bwd")
    add(name, ("pcnn_deconv_bilinear_fwd", "pcnn_deconv_bilinear_bwd"), make, run, check)


_deconv("deconv_2x7x9x66_k16s8", (2, 7, 9, 66), 16, 8)
_deconv("deconv_1x3x4x5_k2s2", (1, 3, 4, 5), 2, 2)
_deconv("deconv_1x5x6x22_k4s2", (1, 5, 6, 22), 4, 2)


def _upscore(name, shape, k, s, thr=0.5):
    B, H, W, C = shape

    def make():
        rng = np.random.default_rng(C)
        z = (rng.standard_normal(shape) * 4).astype(F)
        z[0, 0, 0, :] = 0.0
        z[0, -1, :, 1 % C] = 95.0
        gt = rng.integers(-1, C, (B, H * s, W * s)).astype(np.int32)
        gt[rng.random(gt.shape) < 0.4] = 0
        gt[0, 0, :3] = [C, C + 5, -7]
        return dict(z=z, bias=rng.standard_normal(C).astype(F), gt=gt)

    def run(c):
        from posecnn_amd import ops
        z, b = c.e("z"), c.e("bias")
        s0, p0, l0 = ops.upscore_softmax_argmax(z, b, k, s, relu=True, want_score=True)
        s1, p1, l1 = ops.upscore_softmax_argmax(z, b, k, s, relu=False, want_score=False, want_prob=False)
        _, p2, l2, h2 = ops.upscore_softmax_argmax(z, b, k, s, relu=True, want_score=False, hard_gt=c.e("gt"), hard_threshold=thr)
        return dict(score=s0, prob=p0, label=l0, label_norelu=l1, hard_prob=p2, hard_label=l2, hard=h2)

    def check(d, o):
        ws, wp, wl = oracle.upscore_softmax_argmax(d["z"], d["bias"], k, s, True)
        same(o["score"], ws, "score"); same(o["prob"], wp, "prob"); same(o["label"], wl, "label")
        same(o["label_norelu"], oracle.upscore_softmax_argmax(d["z"], d["bias"], k, s, False)[2], "label (no ReLU)")
        same(o["hard_prob"], wp, "prob (hard launch)"); same(o["hard_label"], wl, "label (hard launch)")
        same(o["hard"], oracle.hard_label(wp, d["gt"], thr), "hard label")
    add(name, ("pcnn_upscore_softmax_argmax_fwd", "pcnn_upscore_softmax_argmax_hard_fwd"), make, run, check)


_upscore("upscore_c14", (2, 5, 7, 14), 16, 8)
_upscore("upscore_c16", (1, 7, 9, 16), 16, 8)
_upscore("upscore_c22", (1, 7, 9, 22), 16, 8)
_upscore("upscore_c40_generic", (1, 5, 21, 40), 16, 8)
_upscore("upscore_c3_k4s2", (1, 9, 5, 3), 4, 2)


# =====================================================================================================================
# Trunk pieces (tests/test_gpu_ops.py: numpy restatements bit-exact, float64 within the existing tolerances)
def _bias_act(name, shape):
    def make():
        rng = np.random.default_rng(24)
        return dict(x=rng.standard_normal(shape).astype(F), b=rng.standard_normal(shape[-1]).astype(F))

    def run(c):
        from posecnn_amd import ops
        b = c.e("b")
        return dict(relu=ops.bias_act_(c.e("x", mutable=True), b, True), linear=ops.bias_act_(c.e("x", mutable=True), b, False))

    def check(d, o):
        same(o["relu"], np.maximum(d["x"] + d["b"], 0).astype(F), "bias_act relu")
        same(o["linear"], (d["x"] + d["b"]).astype(F), "bias_act")
    add(name, ("pcnn_bias_act_fwd",), make, run, check)


_bias_act("bias_act_1x7x9x22", (1, 7, 9, 22))
_bias_act("bias_act_3x5x5x64", (3, 5, 5, 64))


def _bias_relu_pool2(name, shape):
    B, H, W, C = shape

    def make():
        rng = np.random.default_rng(31)
        return dict(x=(rng.standard_normal(shape) * 3).astype(F), b=rng.standard_normal(C).astype(F))

    def run(c):
        from posecnn_amd import ops
        x, b = c.e("x"), c.e("b")
        return dict(relu=ops.bias_relu_pool2(x, b, True), linear=ops.bias_relu_pool2(x, b, False))

    def check(d, o):
        act = d["x"] + d["b"]
        same(o["linear"], act.reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4)).astype(F), "pool")
        same(o["relu"], np.maximum(act, 0).reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4)).astype(F), "relu pool")
    add(name, ("pcnn_bias_relu_pool2_fwd",), make, run, check)


_bias_relu_pool2("bias_relu_pool2_1x6x10x3", (1, 6, 10, 3))
_bias_relu_pool2("bias_relu_pool2_3x2x2x128", (3, 2, 2, 128))


def _conv_c3(name, B, H, W, cout):
    def make():
        rng = np.random.default_rng(41)
        return dict(x=(rng.standard_normal((B, H, W, 3)) * 50).astype(F), w=(rng.standard_normal((3, 3, 3, cout)) * 0.3).astype(F),
                    b=rng.standard_normal(cout).astype(F))

    def run(c):
        from posecnn_amd import ops
        x, w, b = c.e("x"), c.e("w"), c.e("b")
        return dict(relu=ops.conv3x3_c3(x, w, b, True), linear=ops.conv3x3_c3(x, w, b, False))

    def check(d, o):
        x, w = d["x"], d["w"]
        xp = np.zeros((B, H + 2, W + 2, 3), np.float64); xp[:, 1:-1, 1:-1] = x
        want = np.zeros((B, H, W, cout), np.float64)
        for ky in range(3):
            for kx in range(3):
                want += np.einsum("bhwc,oc->bhwo", xp[:, ky:ky + H, kx:kx + W], w[ky, kx].T.astype(np.float64))
        want += d["b"]
        assert np.abs(o["linear"] - want).max() <= 2e-5 * np.abs(want).max()
        assert np.abs(o["relu"] - np.maximum(want, 0)).max() <= 2e-5 * np.abs(want).max()
    add(name, ("pcnn_conv3x3_c3_fwd",), make, run, check)


_conv_c3("conv3x3_c3_1x1x1", 1, 1, 1, 64)
_conv_c3("conv3x3_c3_1x5x131", 1, 5, 131, 64)
_conv_c3("conv3x3_c3_1x33x7", 1, 33, 7, 128)


def _conv_c3_wino(name, B, H, W, cout, groups):
    def make():
        rng = np.random.default_rng(71)
        return dict(x=(rng.standard_normal((B, H, W, 3)) * 50).astype(F),
                    w=(rng.standard_normal((groups, 3, 3, 3, cout)) * 0.1).astype(F), b=rng.standard_normal((groups, cout)).astype(F))

    def run(c):
        from posecnn_amd import ops
        x, w, b = c.e("x"), c.e("w"), c.e("b")
        return dict(relu=ops.conv3x3_c3_winograd43(x, w, b, True, groups=groups), linear=ops.conv3x3_c3_winograd43(x, w, b, False, groups=groups))

    def check(d, o):   # the existing test's reference: winograd_input(conv3x3_c3(x)) per filter set, bit for bit
        torch = _torch()
        from posecnn_amd import ops
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
        per = B // groups
        for relu in (True, False):
            want = torch.cat([ops.winograd_input(ops.conv3x3_c3(t(d["x"][k * per:(k + 1) * per]), t(d["w"][k]), t(d["b"][k]), relu), tile=4)
                              for k in range(groups)], dim=1)
            same(o["relu" if relu else "linear"], want.cpu().numpy(), "V relu=%s" % relu)
    add(name, ("pcnn_conv3x3_c3_winograd43_fwd",), make, run, check)


_conv_c3_wino("conv3x3_c3_wino43_1x5x7", 1, 5, 7, 128, 1)
_conv_c3_wino("conv3x3_c3_wino43_2x16x32_g2", 2, 16, 32, 64, 2)
_conv_c3_wino("conv3x3_c3_wino43_1x1x1", 1, 1, 1, 64, 1)


def _raw_make(B, H, W):
    rng = np.random.default_rng(H)
    im8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    d16 = rng.integers(0, 3000, (B, H, W)).astype(np.uint16)
    d16[0, :3, :5] = 65535
    d16[-1, -2:, :] = 0
    return im8, d16


def _conv_c3_wino_raw_make():
    im8, d16 = _raw_make(2, 50, 70)
    rng = np.random.default_rng(5)
    return dict(im8=im8, d16=d16, w=(rng.standard_normal((2, 3, 3, 3, 64)) * 0.1).astype(F), b=rng.standard_normal((2, 64)).astype(F))


def _conv_c3_wino_raw_run(c):
    from posecnn_amd import ops
    t8, t16, w, b = c.e("im8"), c.e("d16"), c.e("w"), c.e("b")
    return dict(both=ops.conv3x3_c3_winograd43_raw(t8, t16, w, b, True),
                colour=ops.conv3x3_c3_winograd43_raw(t8, None, c.e(c.d["w"][:1]), c.e(c.d["b"][:1]), True),
                depth=ops.conv3x3_c3_winograd43_raw(None, t16, c.e(c.d["w"][1:]), c.e(c.d["b"][1:]), False))


def _conv_c3_wino_raw_check(d, o):   # tests/test_gpu_round3.py: the blob path on host-built blobs, bit for bit
    torch = _torch()
    from posecnn_amd import fcn, ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    blobs = [fcn._get_image_blob(d["im8"][i], d["d16"][i]) for i in range(2)]
    data = np.concatenate([b[0] for b in blobs]).astype(F)
    data_p = np.concatenate([b[1] for b in blobs]).astype(F)
    same(o["both"], ops.conv3x3_c3_winograd43(t(np.concatenate([data, data_p])), t(d["w"]), t(d["b"]), True, groups=2).cpu().numpy(), "both")
    same(o["colour"], ops.conv3x3_c3_winograd43(t(data), t(d["w"][:1]), t(d["b"][:1]), True).cpu().numpy(), "colour")
    same(o["depth"], ops.conv3x3_c3_winograd43(t(data_p), t(d["w"][1:]), t(d["b"][1:]), False).cpu().numpy(), "depth")


add("conv3x3_c3_wino43_raw_50x70", ("pcnn_conv3x3_c3_winograd43_raw_fwd",), _conv_c3_wino_raw_make, _conv_c3_wino_raw_run,
    _conv_c3_wino_raw_check)


def _conv12(name, B, H, W, groups, raw):
    def make():
        torch = _torch()
        from posecnn_amd import ops
        g = G(100 + B * H)
        w1 = torch.randn((groups, 3, 3, 3, 64), generator=g) * 0.02
        b1 = torch.randn((groups, 64), generator=g) * 0.1
        w2 = torch.randn((groups, 64, 64, 3, 3), generator=g) * (2.0 / 576) ** 0.5
        b2 = torch.randn((groups, 64), generator=g) * 0.1
        ut2 = torch.stack([ops.winograd_filter(w2[k], 4).transpose(1, 2) for k in range(groups)]).contiguous()
        d = dict(w1=w1, b1=b1, ut2=ut2, ut2f=ops.conv12_fragment_major(ut2), b2=b2)
        if raw:
            nc = B if groups == 1 else B // 2
            d["im8"] = torch.randint(0, 256, (nc, H, W, 3), generator=g, dtype=torch.uint8)
            d["d16"] = np.random.default_rng(3).integers(0, 3000, (B - nc, H, W)).astype(np.uint16) if groups == 2 else None
        else:
            d["x"] = torch.randint(0, 256, (B, H, W, 3), generator=g).float() - 100.0
        return d

    def run(c):
        from posecnn_amd import ops
        w1, b1, ut2, ut2f, b2 = (c.e(k) for k in ("w1", "b1", "ut2", "ut2f", "b2"))
        if raw:
            im8, d16 = c.e("im8"), c.e("d16")
            return dict(y=ops.conv1_1_conv1_2_fused_raw(im8, d16, w1, b1, ut2, b2),
                        y_frag=ops.conv1_1_conv1_2_fused_raw(im8, d16, w1, b1, ut2f, b2, ut2_layout=1))
        x = c.e("x")
        return dict(y=ops.conv1_1_conv1_2_fused(x, w1, b1, ut2, b2, groups=groups),
                    y_frag=ops.conv1_1_conv1_2_fused(x, w1, b1, ut2f, b2, groups=groups, ut2_layout=1))

    def check(d, o):   # tests/test_gpu_round4.py: the unfused pair bit for bit (+ float64 for blob input)
        torch = _torch()
        from posecnn_amd import ops
        dv = _dev()
        w1, b1, ut2, b2 = (d[k].to(dv) for k in ("w1", "b1", "ut2", "b2"))
        if raw:
            d16 = torch.from_numpy(d["d16"]).to(dv) if d["d16"] is not None else None
            v = ops.conv3x3_c3_winograd43_raw(d["im8"].to(dv), d16, w1, b1, True)
        else:
            v = ops.conv3x3_c3_winograd43(d["x"].to(dv), w1, b1, True, groups=groups)
        want = ops.winograd43_conv(v, ut2, b2, B, H, W, True, 1, groups).cpu().numpy()
        same(o["y"], want, "fused conv1_1 -> conv1_2 -> pool1")
        same(o["y_frag"], want, "fragment-major filter bank")
    covers = ("pcnn_conv1_1_conv1_2_fused_raw_fwd",) if raw else ("pcnn_conv1_1_conv1_2_fused_fwd",)
    add(name, covers, make, run, check)


_conv12("conv12_fused_1x16x16", 1, 16, 16, 1, False)
_conv12("conv12_fused_4x48x32_g2", 4, 48, 32, 2, False)
_conv12("conv12_fused_raw_rgbd_2x32x48", 2, 32, 48, 2, True)
_conv12("conv12_fused_raw_colour_3x32x32", 3, 32, 32, 1, True)


def _wino2(name, shape):
    B, H, W, C = shape

    def make():
        rng = np.random.default_rng(61)
        return dict(x=rng.standard_normal(shape).astype(F), m=rng.standard_normal((16, B * (H // 2) * (W // 2), C)).astype(F),
                    b=rng.standard_normal(C).astype(F))

    def run(c):
        from posecnn_amd import ops
        m, b = c.e("m"), c.e("b")
        return dict(v=ops.winograd_input(c.e("x")), y_relu=ops.winograd_output(m, b, B, H, W, True, pool=False),
                    y=ops.winograd_output(m, b, B, H, W, False, pool=False), y_pool=ops.winograd_output(m, b, B, H, W, True, pool=True))

    def check(d, o):
        same(o["v"], np_wino_input(d["x"]), "input transform")
        want = np_wino_output(d["m"], d["b"], B, H, W, True)
        same(o["y_relu"], want, "output relu")
        same(o["y"], np_wino_output(d["m"], d["b"], B, H, W, False), "output")
        same(o["y_pool"], want.reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4)), "output pool")
    add(name, ("pcnn_winograd_input_fwd", "pcnn_winograd_output_fwd"), make, run, check)


_wino2("wino2_1x2x2x4", (1, 2, 2, 4))
_wino2("wino2_3x6x4x260", (3, 6, 4, 260))


def _wino4(name, shape):
    B, H, W, C = shape
    Tn = B * ((H + 3) // 4) * ((W + 3) // 4)
    even = H % 2 == 0 and W % 2 == 0

    def make():
        rng = np.random.default_rng(63)
        return dict(x=rng.standard_normal(shape).astype(F), m=rng.standard_normal((36, Tn, C)).astype(F), b=rng.standard_normal(C).astype(F))

    def run(c):
        from posecnn_amd import ops
        m, b = c.e("m"), c.e("b")
        out = dict(v=ops.winograd_input(c.e("x"), tile=4), y_relu=ops.winograd_output(m, b, B, H, W, True, pool=False, tile=4),
                   y=ops.winograd_output(m, b, B, H, W, False, pool=False, tile=4))
        if even:
            out["y_pool"] = ops.winograd_output(m, b, B, H, W, True, pool=True, tile=4)
            out["both_y"], out["both_pool"] = ops.winograd43_output_both(m, b, B, H, W, True)
        return out

    def check(d, o):
        same(o["v"], np_wino43_input(d["x"]), "input transform")
        want = np_wino43_output(d["m"], d["b"], B, H, W, True)
        same(o["y_relu"], want, "output relu")
        same(o["y"], np_wino43_output(d["m"], d["b"], B, H, W, False), "output")
        if even:
            pooled = want.reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))
            same(o["y_pool"], pooled, "output pool"); same(o["both_y"], want, "both: y"); same(o["both_pool"], pooled, "both: pool")
    covers = ("pcnn_winograd43_input_fwd", "pcnn_winograd43_output_fwd") + (("pcnn_winograd43_output_both_fwd",) if even else ())
    add(name, covers, make, run, check)


_wino4("wino4_1x1x1x8", (1, 1, 1, 8))
_wino4("wino4_2x5x7x36", (2, 5, 7, 36))
_wino4("wino4_1x17x9x128", (1, 17, 9, 128))
_wino4("wino4_2x22x38x64", (2, 22, 38, 64))


def _wino43_conv(name, shape, cout, pool, groups):
    B, H, W, C = shape

    def make():
        torch = _torch()
        from posecnn_amd import ops
        rng = np.random.default_rng(81)
        x = np.maximum(rng.standard_normal(shape), 0).astype(F)
        w = (rng.standard_normal((groups, cout, C, 3, 3)) * np.sqrt(2.0 / (9 * C))).astype(F)
        b = rng.standard_normal((groups, cout)).astype(F)
        xt, wt = torch.from_numpy(x).to(_dev()), torch.from_numpy(w).to(_dev())
        v = ops.winograd_input(xt, 4)
        ut = torch.stack([ops.winograd_filter(wt[g], 4).transpose(1, 2) for g in range(groups)]).contiguous()
        return dict(x=x, w=w, b=b, v=v, ut=ut)

    def run(c):
        from posecnn_amd import ops
        out = ops.winograd43_conv(c.e("v"), c.e("ut"), c.e("b"), B, H, W, True, pool, groups)
        if pool == 2:
            return dict(y=out[0], y_pool=out[1])
        return dict(y_pool=out) if pool == 1 else dict(y=out)

    def check(d, o):   # tests/test_gpu_ops.py::test_winograd43_mfma_conv_kernel
        torch = _torch()
        from posecnn_amd import ops
        torch.backends.cuda.matmul.allow_tf32 = False
        xt, wt, bt = (torch.from_numpy(d[k]).to(_dev()) for k in ("x", "w", "b"))
        Bg = B // groups
        for g in range(groups):
            sl = slice(g * Bg, (g + 1) * Bg)
            ref = torch.nn.functional.conv2d(xt[sl].double().permute(0, 3, 1, 2), wt[g].double(), bt[g].double(), padding=1).permute(0, 2, 3, 1)
            ref = np.maximum(ref.cpu().numpy(), 0)
            scale = np.abs(ref).max()
            if "y" in o:
                vg = ops.winograd_input(xt[sl].contiguous(), 4)
                want = ops.winograd_output(torch.bmm(vg, ops.winograd_filter(wt[g], 4)), bt[g], Bg, H, W, True, False, 4).cpu().numpy()
                assert o["y"].shape == (B, H, W, cout)
                assert np.abs(o["y"][sl] - ref).max() <= 5e-5 * scale
                assert np.abs(o["y"][sl] - want).max() <= 3e-5 * scale
                assert (np.abs(o["y"][sl] - want) > 1e-3 * scale).sum() == 0
            if "y_pool" in o:
                refp = ref.reshape(Bg, H // 2, 2, W // 2, 2, cout).max(axis=(2, 4))
                assert np.abs(o["y_pool"][sl] - refp).max() <= 5e-5 * scale
        if pool == 2:
            same(o["y_pool"], o["y"].reshape(B, H // 2, 2, W // 2, 2, cout).max(axis=(2, 4)), "pool of own output")
    add(name, ("pcnn_winograd43_conv_fwd",), make, run, check)


_wino43_conv("wino43_conv_1x6x6x128_split", (1, 6, 6, 128), 64, 0, 1)
_wino43_conv("wino43_conv_1x14x18x512_split_pool", (1, 14, 18, 512), 512, 1, 1)
_wino43_conv("wino43_conv_2x30x38x256_split_both_g2", (2, 30, 38, 256), 256, 2, 2)
_wino43_conv("wino43_conv_2x10x14x512_split_g2", (2, 10, 14, 512), 128, 0, 2)
_wino43_conv("wino43_conv_3x5x7x64_ragged", (3, 5, 7, 64), 64, 0, 1)
_wino43_conv("wino43_conv_2x478x638x64_g2_big", (2, 478, 638, 64), 128, 0, 2)


# =====================================================================================================================
# Fully connected layers (tests/test_gpu_round2.py, round3, round5, round6: float64 within the existing tolerances)
_FC_CACHE = {}


def _fc_base(M, K, N, seed):
    key = (M, K, N, seed)
    if key not in _FC_CACHE:
        torch = _torch()
        g = torch.Generator(device=_dev()).manual_seed(seed)
        x = torch.randn((M, K), generator=g, device=_dev())
        wt = torch.randn((N, K), generator=g, device=_dev()) / K ** 0.5
        b = torch.randn((N,), generator=g, device=_dev())
        _FC_CACHE.clear()
        _FC_CACHE[key] = (x, wt, b)
    return _FC_CACHE[key]


def _fc_rows(name, M, K, N, count, relu=True, addend=False):
    n = M if count is None else count

    def make():
        x, wt, b = _fc_base(M, K, N, 7)
        x = x.clone()
        if n < M:
            x[n:] = float("nan")          # dead rows must never reach the result
        d = dict(x=x, wt=wt, b=b, count=None if count is None else np.array([count], np.int32))
        if addend:
            d["add"] = _torch().randn((M, N), generator=G(9)).to(_dev())
        return d

    def run(c):
        from posecnn_amd import ops
        return dict(y=ops.fc_rows(c.e("x"), c.e("wt"), c.e("b"), relu, num_rows=c.e("count"), addend=c.e("add") if addend else None))

    def check(d, o):
        torch = _torch()
        torch.backends.cuda.matmul.allow_tf32 = False
        x, wt, b = d["x"][:n], d["wt"], d["b"]
        ref = x.double() @ wt.double().t() + b.double()
        if addend:
            ref = ref + d["add"][:n].double()
        if relu:
            ref = torch.relu(ref)
        if not n:
            return
        y = torch.from_numpy(o["y"][:n]).to(_dev()).double()
        scale = float(ref.abs().max())
        err = float((y - ref).abs().max())
        if addend:   # tests/test_gpu_round2.py::test_fc_rows_addend_is_a_conv_over_a_concatenation
            assert err <= 4e-6 * scale + 1e-6, (err, scale)
            return
        lib = torch.addmm(b, x, wt.t())
        if relu:
            lib = torch.relu(lib)
        err_lib = float((lib.double() - ref).abs().max())
        assert err <= max(3.0 * err_lib, 4e-6 * scale), (err, err_lib, scale)
    add(name, ("pcnn_fc_rows_fwd",), make, run, check, zero={"y": np.s_[n:]})


for _n in (0, 1, 64, 65, 512, 513, 684, 1500, 3024):       # every side of every fc_split branch at capacity 3024 (S <= 2)
    _fc_rows("fc_rows_cap3024_k8192_n%d" % _n, 3024, 8192, 4096, _n)
_fc_rows("fc_rows_cap3024_k25088_n684", 3024, 25088, 4096, 684)
for _n in (1, 64, 65, 200):                                 # a small capacity: grid.y up to 8 splits
    _fc_rows("fc_rows_cap200_k25088_n%d" % _n, 200, 25088, 256, _n)
_fc_rows("fc_rows_cap64_all", 64, 128, 64, None, relu=False)
_fc_rows("fc_rows_addend_77_of_100", 100, 2048, 128, 77, addend=True)


def _fc_split_make():
    x, wt, b = _fc_base(130, 512, 192, 3)
    x = x.clone(); x[70:] = float("nan")
    return dict(x=x, wt=wt, b=b, count=np.array([70], np.int32))


def _fc_split_run(c):
    from posecnn_amd import ops
    ya, yb = ops.fc_rows_split(c.e("x"), c.e("wt"), c.e("b"), 128, relu_a=True, relu_b=False, num_rows=c.e("count"))
    return dict(y_a=ya, y_b=yb)


def _fc_split_check(d, o):   # the header: bit-identical to two pcnn_fc_rows_fwd calls
    torch = _torch()
    from posecnn_amd import ops
    cnt = torch.tensor([70], dtype=torch.int32, device=_dev())
    ya = ops.fc_rows(d["x"], d["wt"][:128].contiguous(), d["b"][:128].contiguous(), True, num_rows=cnt)
    yb = ops.fc_rows(d["x"], d["wt"][128:].contiguous(), d["b"][128:].contiguous(), False, num_rows=cnt)
    same(o["y_a"], ya.cpu().numpy(), "y_a"); same(o["y_b"], yb.cpu().numpy(), "y_b")


add("fc_rows_split_70_of_130", ("pcnn_fc_rows_split_fwd",), _fc_split_make, _fc_split_run, _fc_split_check,
    zero={"y_a": np.s_[70:], "y_b": np.s_[70:]})


def _fc_cols(name, M, K, N, cnt):
    npad = (N + 63) // 64 * 64

    def make():
        torch = _torch()
        g = G(5 + M)
        x = torch.randn((M, K), generator=g)
        x[cnt:] = float("nan")
        w = torch.randn((N, K), generator=g) / K ** 0.5
        b = torch.randn((N,), generator=g)
        wp = torch.zeros((npad, K)); wp[:N] = w
        bp = torch.zeros((npad,)); bp[:N] = b
        return dict(x=x, wp=wp, bp=bp, w=w, b=b, count=np.array([cnt], np.int32))

    def run(c):
        from posecnn_amd import ops
        x, wp, bp, cn = c.e("x"), c.e("wp"), c.e("bp"), c.e("count")
        y, t = ops.fc_rows_cols(x, wp, bp, N, "tanh", num_rows=cn)
        return dict(y=y, y_tanh=t, y_relu=ops.fc_rows_cols(x, wp, bp, N, "relu", num_rows=cn))

    def check(d, o):   # tests/test_gpu_round5.py::test_fc_rows_cols_is_fc8_and_tanh_in_one_launch
        torch = _torch()
        ref = d["x"][:cnt].double() @ d["w"].double().t() + d["b"].double()
        y, t, yr = (torch.from_numpy(o[k][:cnt]).double() for k in ("y", "y_tanh", "y_relu"))
        scale = max(1.0, float(ref.abs().max())) if cnt else 1.0
        if cnt:
            assert float((y - ref).abs().max()) < 2e-5 * scale
            assert float((t - torch.tanh(y)).abs().max()) < 1e-6
            assert float((yr - torch.relu(ref)).abs().max()) < 2e-5 * scale
    add(name, ("pcnn_fc_rows_cols_fwd",), make, run, check,
        zero={"y": np.s_[cnt:], "y_tanh": np.s_[cnt:], "y_relu": np.s_[cnt:]})


_fc_cols("fc_rows_cols_88_of_128", 300, 4096, 88, 131)
_fc_cols("fc_rows_cols_56_of_64", 64, 256, 56, 64)
_fc_cols("fc_rows_cols_4_count1", 130, 128, 4, 1)
_fc_cols("fc_rows_cols_count0", 70, 512, 128, 0)

SKINNY_SHAPES = {"fc6": (25088, 4096, "relu"), "fc7": (4096, 4096, "relu"), "fc8": (4096, 88, "tanh")}


def _fc_skinny(name, M, K, N, count, act):
    n = M if count is None else count

    def make():
        torch = _torch()
        g = G(M * 7 + N)
        x = torch.randn((M, K), generator=g)
        if n < M:
            x[n:] = float("nan")
        w = torch.randn((K, N), generator=g) / K ** 0.5
        return dict(x=x, wt=w.t().contiguous(), b=torch.randn((N,), generator=g), count=None if count is None else np.array([count], np.int32))

    def run(c):
        from posecnn_amd import ops
        out = ops.fc_skinny(c.e("x"), c.e("wt"), c.e("b"), act, num_rows=c.e("count"))
        return dict(y=out[0], y_act=out[1]) if act == "tanh" else dict(y=out)

    def check(d, o):   # tests/test_gpu_round3.py::test_fc_skinny_matches_float64_and_is_deterministic
        torch = _torch()
        ref = d["x"][:n].double().to(_dev()) @ d["wt"].double().t().to(_dev()) + d["b"].double().to(_dev())
        if act == "relu":
            ref = torch.relu(ref)
        y = torch.from_numpy(o["y"][:n]).to(_dev()).double()
        if n:
            scale = max(1.0, float(ref.abs().max()))
            assert float((y - ref).abs().max()) < 2e-5 * scale
            if act == "tanh":
                assert float((torch.from_numpy(o["y_act"][:n]).double() - torch.tanh(y.cpu())).abs().max()) < 3e-7
    zero = {"y": np.s_[n:]}
    if act == "tanh":
        zero["y_act"] = np.s_[n:]
    add(name, ("pcnn_fc_skinny_fwd",), make, run, check, zero=zero)


_fc_skinny("fc_skinny_m1_none", 1, 256, 40, None, "none")
_fc_skinny("fc_skinny_m1_count0", 1, 4096, 88, 0, "tanh")
_fc_skinny("fc_skinny_m16_count0_relu", 16, 1024, 130, 0, "relu")
_fc_skinny("fc_skinny_m16_fc7_count16", 16, 4096, 4096, 16, "relu")
_fc_skinny("fc_skinny_m17_fc8_count1", 17, 4096, 88, 1, "tanh")
_fc_skinny("fc_skinny_m17_fc7_count17", 17, 4096, 4096, 17, "relu")
_fc_skinny("fc_skinny_m32_fc6_count16", 32, 25088, 4096, 16, "relu")
_fc_skinny("fc_skinny_m32_fc8_count17", 32, 4096, 88, 17, "tanh")
_fc_skinny("fc_skinny_m32_none_count32", 32, 2064, 200, 32, "none")


# =====================================================================================================================
# Small heads and the detection rows (tests/test_gpu_round3.py, round5)
def _head(name, B, h, w, U, Cout, plant, mfma, direct_too):
    def make():
        rng = np.random.default_rng(21)
        return dict(a=rng.standard_normal((B, h, w, U)).astype(F), b5=rng.standard_normal((B, h // 2, w // 2, U)).astype(F),
                    pl=rng.standard_normal((B, h, w, U)).astype(F) if plant else None,
                    wt=(rng.standard_normal((U, Cout)) / U ** 0.5).astype(F))

    def run(c):
        from posecnn_amd import ops
        a, b5, pl = c.e("a"), c.e("b5"), c.e("pl")
        out = {}
        if mfma:
            out["add_mfma"], out["z_mfma"] = ops.head_lowres_mfma(a, b5, ops.head_lowres_mfma_filter(c.e("wt")), Cout, planted=pl)
        if direct_too:
            out["add"], out["z"] = ops.head_lowres(a, b5, c.e("wt"), planted=pl)
        return out

    def check(d, o):
        torch = _torch()
        from posecnn_amd import ops
        t = lambda v: torch.from_numpy(v).to(_dev())
        want = t(d["a"]) + ops.deconv_bilinear(t(d["b5"]), 4, 2)
        if plant:
            want = want + t(d["pl"])
        zr = want.double().reshape(-1, U) @ t(d["wt"]).double()
        for sfx in (("_mfma",) if mfma else ()) + (("",) if direct_too else ()):
            same(o["add" + sfx], want.cpu().numpy(), "add_score" + sfx)
            z = torch.from_numpy(o["z" + sfx]).to(_dev()).double().reshape(-1, Cout)
            assert float((z - zr).abs().max()) < 1e-5 * max(1.0, float(zr.abs().max()))
    covers = (("pcnn_head_lowres_mfma_fwd",) if mfma else ()) + (("pcnn_head_lowres_fwd",) if direct_too else ())
    add(name, covers, make, run, check)


_head("head_22_planted", 2, 12, 16, 64, 22, True, True, True)
_head("head_66", 1, 12, 16, 128, 66, False, True, True)
_head("head_93_mfma_only", 1, 12, 16, 128, 93, True, True, False)
_head("head_5_ragged", 3, 6, 10, 64, 5, True, True, True)
_head("head_3_tiny", 1, 2, 2, 16, 3, False, True, True)


def _pose_l2(name, R, C, cnt):
    def make():
        rng = np.random.default_rng(8)
        x = np.tanh(rng.standard_normal((R, 4 * C))).astype(F)
        w = np.zeros((R, 4 * C), F)
        for r in range(R):
            if r % 3:
                c = int(rng.integers(1, C)); w[r, 4 * c:4 * c + 4] = 1
        return dict(x=x, w=w, count=np.array([cnt], np.int32))

    def run(c):
        from posecnn_amd import ops
        return dict(out=ops.pose_l2_normalize(c.e("x"), c.e("w"), num_rows=c.e("count")))

    def check(d, o):
        mul = d["x"].astype(np.float64) * d["w"]
        want = mul / np.sqrt(np.maximum((mul * mul).sum(1, keepdims=True), 1e-12))
        if cnt:
            assert np.abs(o["out"][:cnt] - want[:cnt]).max() < 3e-7
    add(name, ("pcnn_pose_l2_normalize_fwd",), make, run, check, zero={"out": np.s_[cnt:]})


_pose_l2("pose_l2_30_of_45", 45, 22, 30)
_pose_l2("pose_l2_full", 9, 14, 9)
_pose_l2("pose_l2_count0", 200, 64, 0)


def _det(name, n, stride, R=27, C=22):
    n_out = (R + stride - 1) // stride

    def make():
        rng = np.random.default_rng(3)
        rois = rng.standard_normal((R, 7)).astype(F)
        rois[:, 0] = rng.integers(0, 16, R)
        rois[:, 1] = rng.integers(0, C, R)
        rois[5, 1] = -1
        return dict(rois=rois, pt=rng.standard_normal((R, 4 * C)).astype(F), tp=rng.standard_normal((R, 7)).astype(F),
                    count=np.array([n], np.int32))

    def run(c):
        from posecnn_amd import ops
        rois, pt, tp, cnt = c.e("rois"), c.e("pt"), c.e("tp"), c.e("count")
        rows, count = ops.det_assemble(rois, pt, tp, cnt, row_stride=stride)
        _, count_p, block = ops.det_assemble(rois, pt, tp, cnt, row_stride=stride, frame_offset=48)
        return dict(rows=rows, count=count, block=block, count_packed=count_p)

    def check(d, o):
        want = np.zeros((n_out, 14), F)
        for i in range(n_out):
            ri = i * stride
            if ri < n:
                c = max(int(d["rois"][ri, 1]), 0)
                want[i] = np.concatenate([d["rois"][ri], d["pt"][ri, 4 * c:4 * c + 4], d["tp"][ri, 4:]])
        same(o["rows"], want, "rows")
        assert int(o["count"][0]) == int(o["count_packed"][0]) == n // stride
        block = np.zeros((n_out + 1, 14), F)
        block[:n_out] = want
        written = np.arange(n_out) * stride < n        # the header: every written row is shifted, counted or not
        block[:n_out, 0] += written * F(48)
        block[n_out, 0] = n // stride
        same(o["block"], block, "packed block")
    add(name, ("pcnn_det_assemble_fwd", "pcnn_det_assemble_packed_fwd"), make, run, check, zero={"rows": np.s_[-(-n // stride):]})


for _n in (0, 1, 27):
    for _s in (1, 9):
        _det("det_assemble_n%d_s%d" % (_n, _s), _n, _s)


# =====================================================================================================================
# Pose refinement at (100, 131), and at (120, 160) for the workspace-reuse pairs (tests/test_gpu_icp.py,
# test_gpu_icp_render.py: oracle bit-exact)
def _scaled_K(W):
    K = config.DEMO_INTRINSICS.copy()
    K[:2] *= W / 640.0
    return K


def _icp_make(H, W):
    K = _scaled_K(W)
    rng = np.random.default_rng(H)
    d = dict(K=K, depths=[], labels=[], pv=[], pn=[])
    for k in range(2):
        T_true = S.pose(S.rot([0.3 + k, 1, 0.2], 0.7 + 0.3 * k), [-0.05 + 0.1 * k, 0.02, 0.7 + 0.1 * k])
        T_init = S.pose(S.rot([1, -1, 0.5], np.radians(2.5)) @ T_true[:, :3], T_true[:, 3] + np.array([0.004, -0.005, 0.006]))
        depth, label, pv, pn = S.scene(T_true, T_init, (0.09, 0.07, 0.05), K, H, W, noise=0.0005, rng=rng)
        d["depths"].append(depth.astype(np.uint16)); d["labels"].append(label.astype(np.int32)); d["pv"].append(pv); d["pn"].append(pn)
    d["pv"], d["pn"] = np.stack(d["pv"]).astype(F), np.stack(d["pn"]).astype(F)
    return d


def _icp_run(c):
    torch = _torch()
    from posecnn_amd import icp
    K = c.d["K"]
    lives = [icp.backproject(c.e(dp), c.e(lb), 3, K, 10000.0) for dp, lb in zip(c.d["depths"], c.d["labels"])]
    unmasked = icp.backproject(c.e(c.d["depths"][0]), None, 0, K, 10000.0)
    live = c.e(torch.stack([t.clone() for t in lives]))
    upd, stats = icp.icp(live, c.e("pv"), c.e("pn"), K, iterations=5, want_stats=True)
    return dict(live0=lives[0], live1=lives[1], unmasked=unmasked, update=upd, stats=stats)


def _icp_check(d, o):
    K = d["K"]
    for k in range(2):
        same(o["live%d" % k], oracle.icp_backproject(d["depths"][k], d["labels"][k], 3, K, 10000.0), "live %d" % k)
    same(o["unmasked"], oracle.icp_backproject(d["depths"][0], None, 0, K, 10000.0), "unmasked")
    want_u, want_s = oracle.icp_refine(np.stack([o["live0"], o["live1"]]), d["pv"], d["pn"], K, iterations=5)
    assert np.array_equal(o["update"].view(np.uint64), want_u.view(np.uint64))
    same(o["stats"], want_s, "stats")


for _H, _W in ((100, 131), (120, 160)):
    add("icp_backproject_refine_%dx%d" % (_H, _W), ("pcnn_icp_backproject_fwd", "pcnn_icp_refine_fwd"),
        lambda H=_H, W=_W: _icp_make(H, W), _icp_run, _icp_check)


def _render_scene_make(H, W):
    from test_gpu_icp_render import make_case
    obj = 5
    K, (v, n, f), T_true, T_est, depth, label = make_case(H, W, 0.004, obj)
    label = label.astype(np.int32)
    label[: H // 4] = np.where(label[: H // 4] > 0, 9, 0)
    holes = (np.arange(H * W).reshape(H, W) % 11 == 0) & (label > 0)
    depth = np.where(holes, 0, depth).astype(np.uint16)
    maps = oracle.render_mesh(v, n, f, T_est[None], K, H, W, model_index=obj - 1)
    live = oracle.icp_backproject(depth, label, obj, K, 10000.0)
    hyps = np.repeat(T_est[None], 6, 0)
    hyps[:, 2, 3] += np.array([-0.004, 0.0, -0.02, 0.012, 0.05, 1.0])
    poses = np.stack([T_est, S.pose(S.rot([0, 1, 0], 0.3), T_true[:, 3])]).astype(F)
    T_pol = S.pose(S.rot([0, 1, 0], 0.05) @ T_true[:, :3], T_true[:, 3] + np.array([0.004, -0.003, 0.02]))
    pv_pol = oracle.render_mesh(v, n, f, T_pol[None], K, H, W, want=("vertices",))["vertices"][0][..., :3].copy()
    live_pol = oracle.icp_backproject(depth, label, obj, K, 10000.0)
    return dict(K=K, v=np.asarray(v, F), n=np.asarray(n, F), f=np.asarray(f, np.int32), obj=obj, H=H, W=W, label=label, live=live,
                can=maps["canonical"][0], pv=maps["vertices"][0], pn=maps["normals"][0], hyps=hyps.astype(F), poses=poses,
                pv_pol=pv_pol, live_pol=live_pol)


def _render_scene_run(c):
    from posecnn_amd import icp
    d = c.d
    mesh = icp.Mesh(d["v"], d["f"], d["n"], device="cpu")
    mesh.vertices, mesh.normals, mesh.faces = c.e(mesh.vertices_np), c.e(mesh.normals_np), c.e(mesh.faces_np)
    maps = icp.render(mesh, d["poses"], d["K"], d["H"], d["W"], model_index=d["obj"] - 1, want=("vertices", "normals", "canonical"))
    lab, live, can = c.e("label"), c.e("live"), c.e("can")
    sums, mask = icp.center(lab, live, can, c.e("pv"), c.e("pn"), d["obj"], 0.0035)
    hits = icp.score(live, can, mask, d["hyps"], d["K"], 0.01)
    x, info = icp.polish_async(lab, c.e("live_pol"), c.e("pv_pol"), d["obj"], max_evaluations=20)
    return dict(vertices=maps["vertices"], normals=maps["normals"], canonical=maps["canonical"], sums=sums, mask=mask, hits=hits,
                polish_x=x, polish_info=info)


def _render_scene_check(d, o):
    want = oracle.render_mesh(d["v"], d["n"], d["f"], d["poses"], d["K"], d["H"], d["W"], (0.25, 6.0), d["obj"] - 1)
    for key in ("vertices", "normals", "canonical"):
        same(o[key], want[key], key)
    want_s, want_m = oracle.icp_center(d["label"], d["live"], d["can"], d["pv"], d["pn"], d["obj"], 0.0035)
    assert np.array_equal(o["sums"].view(np.uint64), want_s.view(np.uint64)), (o["sums"], want_s)
    same(o["mask"], want_m, "mask")
    same(o["hits"], oracle.icp_score(d["live"], d["can"], want_m, d["hyps"], 0.01), "hits")
    wx, we, wn = oracle.icp_polish(d["label"], d["live_pol"], d["pv_pol"], d["obj"], maxeval=20)
    assert np.array_equal(o["polish_x"].view(np.uint64), np.asarray(wx, np.float64).view(np.uint64)), (o["polish_x"], wx)
    assert o["polish_info"][0] == we and o["polish_info"][1] == wn


for _H, _W in ((100, 131), (120, 160)):
    add("icp_render_center_score_polish_%dx%d" % (_H, _W),
        ("pcnn_render_mesh_fwd", "pcnn_icp_center_fwd", "pcnn_icp_score_fwd", "pcnn_icp_polish_fwd"),
        lambda H=_H, W=_W: _render_scene_make(H, W), _render_scene_run, _render_scene_check)


# =====================================================================================================================
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_memory_contract(gpu, case):
    execute(case)


def _by_name(name):
    return next(c for c in CASES if c.name == name)


# Workspace reuse: the first case of each pair (larger) leaves its workspace behind, the second must not see it. Every
# entry that takes a workspace is the second case of some pair.
WORKSPACE_PAIRS = [
    ("hough_b16_cap8", "hough_17x19"),
    ("hough_lowres_k4s2", "hough_lowres_k16s8"),
    ("adl_7_of_16", "adl_count_cap"),
    ("backproject_big_k2", "backproject_ws_k3"),
    ("wino43_conv_1x14x18x512_split_pool", "wino43_conv_1x6x6x128_split"),
    ("fc_rows_cap3024_k8192_n684", "fc_rows_cap200_k25088_n65"),      # 684 live rows: the balance split (S = 2)
    ("fc_rows_cap200_k25088_n200", "fc_rows_cap200_k25088_n1"),
    ("fc_skinny_m32_fc6_count16", "fc_skinny_m17_fc8_count1"),
    ("smooth_l1_n300001", "smooth_l1_n1"),
    ("icp_backproject_refine_120x160", "icp_backproject_refine_100x131"),
    ("icp_render_center_score_polish_120x160", "icp_render_center_score_polish_100x131"),
]


@pytest.mark.parametrize("big,small", WORKSPACE_PAIRS, ids=["%s->%s" % p for p in WORKSPACE_PAIRS])
def test_workspace_reuse_after_a_larger_call(gpu, big, small):
    """The second call finds the first call's workspaces (same buffers, large enough, holding what the first call wrote
    rather than the poison) and must give the bits of its fresh run."""
    from posecnn_amd import ops
    big, small = _by_name(big), _by_name(small)
    d_small = small.make()
    with guarded("P1") as (g, rec):
        fresh = small.run(Ctx(g, rec, d_small))
        _finish(g)
        fresh = _numpy(fresh)
        need = {k: ws._buf.numel() for k, ws in ops._default_ws.items()}   # fresh caches: exactly what the small case asks
    assert need, "%s takes no workspace" % small.name
    d_big = big.make()
    with guarded("P1") as (g, rec):
        big.run(Ctx(g, rec, d_big))
        _finish(g)
        left = {k: ws._buf for k, ws in ops._default_ws.items()}
        for k, n in need.items():
            assert k in left and left[k].numel() >= n, "%s leaves no workspace %s of %d bytes behind" % (big.name, k[1], n)
            assert bool((left[k][:n] != 0xFF).any()), "%s never wrote the part of workspace %s that %s uses" % (big.name, k[1], small.name)
        stale = small.run(Ctx(g, rec, small.make()))
        _finish(g)
        stale = _numpy(stale)
        for k in need:
            assert ops._default_ws[k]._buf is left[k], "%s reallocated workspace %s" % (small.name, k[1])
    assert sorted(fresh) == sorted(stale)
    for k in fresh:
        a, b = np.ascontiguousarray(stale[k]), np.ascontiguousarray(fresh[k])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s after %s: %s differs" % (small.name, big.name, k)


def test_fc_skinny_exchange_on_a_poisoned_workspace(gpu):
    """The last workgroup of a column group reads the other workgroups' partial sums: with the workspace refilled with NaN
    bytes on the stream before every launch, a partial read before it lands shows as NaN (or a neighbour's value)."""
    torch = _torch()
    from posecnn_amd import ops
    dev = _dev()
    M, n = 21, 17
    sets = {}
    for s in range(2):
        g = torch.Generator(device=dev).manual_seed(40 + s)
        for name, (K, N, act) in SKINNY_SHAPES.items():
            x = torch.randn((M, K), generator=g, device=dev)
            x[n:] = float("nan")
            wt = torch.randn((N, K), generator=g, device=dev) / K ** 0.5
            sets[(name, s)] = (x, wt, torch.randn((N,), generator=g, device=dev), act)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    need = 0
    for (x, wt, b, act) in sets.values():
        nb, nc = ops.ctypes.c_size_t(), ops.ctypes.c_int()
        ops._lib.check("ws", ops.lib().pcnn_fc_skinny_workspace_bytes(M, x.shape[1], wt.shape[0], ops.ctypes.byref(nb), ops.ctypes.byref(nc)))
        need = max(need, nb.value)
    with guarded("P1") as (g, rec):
        ws = ops._ws(dev, "fc_skinny").get(need, dev)
        names = list(SKINNY_SHAPES)
        order = [(names[i % 3], (i // 3) % 2) for i in range(16)]
        outs = []
        for key in order:
            x, wt, b, act = sets[key]
            ws.view(torch.uint8).fill_(0xFF)                   # NaN bytes, on the stream, no host sync
            y = ops.fc_skinny(x, wt, b, act, num_rows=cnt)
            outs.append((key, y[0] if act == "tanh" else y))
        _finish(g)
        assert ops._default_ws[(dev.index, "fc_skinny", torch.cuda.current_stream(dev).cuda_stream)]._buf is ws
    first = {}
    for key, y in outs:
        y = y.cpu().numpy()
        if key in first:
            same(y, first[key], "%s set %d: repeat differs from its first run" % key)
        else:
            first[key] = y
    assert len(first) == 6
    for key, y in first.items():
        x, wt, b, act = sets[key]
        ref = x[:n].double() @ wt.double().t() + b.double()
        if act == "relu":
            ref = torch.relu(ref)
        assert float((torch.from_numpy(y[:n]).to(dev).double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())), key
        assert not y[n:].view(np.uint32).any()


def test_graph_replay_with_new_inputs_on_guarded_buffers(gpu):
    """One Hough forward and one fc_skinny call captured in one single-stream graph on guarded buffers, replayed twice with
    new input contents copied in: guards intact, outputs equal to eager calls on those inputs."""
    torch = _torch()
    from posecnn_amd import ops
    dev = _dev()
    B, H, W = 1, 120, 160
    inputs = []
    for k in range(3):
        label, vertex, meta, _ = frames(300 + k, B, H=H, W=W, C=22, n_obj=3)
        g = torch.Generator(device="cpu").manual_seed(k)
        inputs.append(dict(label=label, vertex=vertex, meta=meta, x=torch.randn((16, 4096), generator=g)))
    ext = np.ascontiguousarray(config.LOV_EXTENTS)
    g0 = torch.Generator(device="cpu").manual_seed(99)
    wt = torch.randn((88, 4096), generator=g0) / 64.0
    bias = torch.randn((88,), generator=g0)

    def eager(inp):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if isinstance(a, np.ndarray) else a.to(dev)
        h = ops.hough_voting_gpu_padded(t(inp["label"]), t(inp["vertex"]), t(ext), t(inp["meta"]), None, 0, -1.0, 0.02, 10, label_threshold=60)
        y = ops.fc_skinny(t(inp["x"]), t(wt), t(bias), "tanh")
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in h] + [y[0].cpu().numpy(), y[1].cpu().numpy()]

    wants = [eager(inp) for inp in inputs[1:]]
    with guarded("P2") as (g, rec):
        c = Ctx(g, rec, inputs[0])
        lab, ver, ex, me = c.e("label"), c.e("vertex"), c.e(ext), c.e("meta")
        xx, w_, b_ = c.e("x"), c.e(wt), c.e(bias)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            hout = ops.hough_voting_gpu_padded(lab, ver, ex, me, None, 0, -1.0, 0.02, 10, label_threshold=60)
            ops.fc_skinny(xx, w_, b_, "tanh")                       # warm: workspace and tickets of stream s
            s.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                ops.hough_voting_gpu_padded(lab, ver, ex, me, None, 0, -1.0, 0.02, 10, label_threshold=60, out=hout)
                yo = ops.fc_skinny(xx, w_, b_, "tanh")
        torch.cuda.synchronize()
        for inp, want in zip(inputs[1:], wants):
            g.refresh(lab, inp["label"]); g.refresh(ver, inp["vertex"]); g.refresh(me, inp["meta"]); g.refresh(xx, inp["x"])
            graph.replay()
            _finish(g)
            got = [o.cpu().numpy() for o in hout] + [yo[0].cpu().numpy(), yo[1].cpu().numpy()]
            for k, (a, b) in enumerate(zip(got, want)):
                same(a, b, "replay output %d" % k)
        del graph
