"""An independent numpy restatement of posecnn_amd/csrc/synth_scene.hip (TEST INFRASTRUCTURE): a per-triangle rasteriser,
the depth test with its (slot, face) tie rule, attribute interpolation, the lighting of canonicalVertsAndColor.frag /
canonicalVertsAndTexture.frag, the bilinear texture fetch, quantisation, background compositing, pixel counts and the
`valid` flag — every operation an IEEE float32 numpy operation with one rounding, in the kernel's documented order, so the
device's bytes must equal these.

A scene description here is plain data:
  meshes     list of dicts: vertices f32 [n,3], normals f32 [n,3], faces int32 [m,3], optional colors f32 [n,3],
             uvs f32 [n,2], texture uint8 [h,w,3]
  scenes     list (one per scene) of lists of instances (mesh index, class id, pose 3x4, shininess)
  lights     f32 [S,4]"""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SMALL_BOX = 64


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def transform(T, p):
    """rd_transform: T f32 [12], p f32 [...,3] -> camera frame"""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([((T[0] * x + T[1] * y) + T[2] * z) + T[3],
                     ((T[4] * x + T[5] * y) + T[6] * z) + T[7],
                     ((T[8] * x + T[9] * y) + T[10] * z) + T[11]], axis=-1)


def setup(T, vertices, faces, K4, H, W, z_near):
    """rd_setup for every face: dict of per-face arrays (cam [m,3,3], u, v, z [m,3], flip [m,3], box, ok)"""
    fx, fy, px, py = (F(k) for k in K4)
    cam = transform(T, vertices)[faces]                       # [m,3(vertex),3(xyz)]
    z = cam[..., 2]
    with np.errstate(all="ignore"):
        u = cam[..., 0] / z * fx + px
        v = cam[..., 1] / z * fy + py
        ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
        ok &= ((z >= F(z_near)) & (np.abs(u) < F(1e7)) & (np.abs(v) < F(1e7))).all(axis=1)
    flip = np.stack([faces[:, 1] > faces[:, 2], faces[:, 2] > faces[:, 0], faces[:, 0] > faces[:, 1]], axis=1)
    us, vs = np.where(ok[:, None], u, F(0)), np.where(ok[:, None], v, F(0))
    x0 = np.maximum(0, np.ceil(us.min(1)).astype(np.int64))
    x1 = np.minimum(W - 1, np.floor(us.max(1)).astype(np.int64))
    y0 = np.maximum(0, np.ceil(vs.min(1)).astype(np.int64))
    y1 = np.minimum(H - 1, np.floor(vs.max(1)).astype(np.int64))
    ok &= (x0 <= x1) & (y0 <= y1)
    return dict(cam=cam, u=u, v=v, z=z, flip=flip, x0=x0, x1=x1, y0=y0, y1=y1, ok=ok)


def _edge(au, av, bu, bv, x, y):
    return (bu - au) * (y - av) - (bv - av) * (x - au)


def weights(u, v, z, flip, x, y):
    """rd_weights; u, v, z, flip: [...,3] broadcastable against x, y [...]. Returns (inside, w [3, ...], s)."""
    def e(a, b, fl):
        fwd = _edge(u[..., a], v[..., a], u[..., b], v[..., b], x, y)
        rev = -_edge(u[..., b], v[..., b], u[..., a], v[..., a], x, y)
        return np.where(fl, rev, fwd)
    e0, e1, e2 = e(1, 2, flip[..., 0]), e(2, 0, flip[..., 1]), e(0, 1, flip[..., 2])
    pos = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
    neg = (e0 <= 0) & (e1 <= 0) & (e2 <= 0)
    area = (e0 + e1) + e2
    with np.errstate(all="ignore"):
        w = [e0 / area / z[..., 0], e1 / area / z[..., 1], e2 / area / z[..., 2]]
        s = (w[0] + w[1]) + w[2]
        inside = (pos | neg) & (area != 0) & (s > 0)
    return inside, w, s


def interp(w, s, a0, a1, a2):
    with np.errstate(all="ignore"):
        return ((w[0] * a0 + w[1] * a1) + w[2] * a2) / s


def rasterise(zkey, tri, slot, z_near, z_far, stats=None):
    """One instance into the scene's key buffer (uint64 [H,W]), triangle by triangle."""
    for f in np.nonzero(tri["ok"])[0]:
        x0, x1, y0, y1 = int(tri["x0"][f]), int(tri["x1"][f]), int(tri["y0"][f]), int(tri["y1"][f])
        if stats is not None:
            stats.setdefault("boxes", []).append((x1 - x0 + 1) * (y1 - y0 + 1))
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        u, v, z, fl = tri["u"][f], tri["v"][f], tri["z"][f], tri["flip"][f]
        inside, w, s = weights(u, v, z, fl, xs.astype(F), ys.astype(F))
        with np.errstate(all="ignore"):
            zz = ((w[0] * z[0] + w[1] * z[1]) + w[2] * z[2]) / s
            inside &= (zz >= F(z_near)) & (zz <= F(z_far))
        key = (zz.astype(F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64((slot << 27) | int(f))
        key = np.where(inside, key, EMPTY)
        zkey[y0:y1 + 1, x0:x1 + 1] = np.minimum(zkey[y0:y1 + 1, x0:x1 + 1], key)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(a):
    ln = np.sqrt(_dot(a, a))
    with np.errstate(all="ignore"):
        return np.where((ln > 0)[..., None], a / ln[..., None], a)


def powi(x, n):
    """x^n, n >= 1, by left-to-right binary powering in float32"""
    n = int(n)
    assert n >= 1
    r = x
    for bit in range(n.bit_length() - 2, -1, -1):
        r = r * r
        if (n >> bit) & 1:
            r = r * x
    return r


def texture_sample(tex, uv):
    """bilinear, texel centres at +0.5, clamp to edge, v flipped; tex uint8 [h,w,3], uv f32 [n,2] -> f32 [n,3]"""
    th, tw = tex.shape[:2]
    fu = np.fmin(np.fmax(uv[:, 0] * F(tw) - F(0.5), F(-1)), F(tw))
    fv = np.fmin(np.fmax((F(1) - uv[:, 1]) * F(th) - F(0.5), F(-1)), F(th))
    xf, yf = np.floor(fu), np.floor(fv)
    ax, ay = (fu - xf)[:, None], (fv - yf)[:, None]
    x0, x1 = np.clip(xf.astype(np.int64), 0, tw - 1), np.clip(xf.astype(np.int64) + 1, 0, tw - 1)
    y0, y1 = np.clip(yf.astype(np.int64), 0, th - 1), np.clip(yf.astype(np.int64) + 1, 0, th - 1)
    t = lambda y, x: tex[y, x].astype(F) / F(255)
    bx, by = F(1) - ax, F(1) - ay
    return (t(y0, x0) * bx + t(y0, x1) * ax) * by + (t(y1, x0) * bx + t(y1, x1) * ax) * ay


def shade(pos, n, col, light, shininess):
    """ApplyLight for one point light: pos, n (unit), col f32 [m,3]; light f32 [4]; shininess int [m] -> linear RGB f32 [m,3]"""
    li = F(light[3])
    L = _f(light[:3])[None] - pos
    dist = np.sqrt(_dot(L, L))
    with np.errstate(all="ignore"):
        L = np.where((dist > 0)[:, None], L / dist[:, None], L)
    att = F(1) / (F(1) + F(0.01) * (dist * dist))
    V = _normalize(-pos)
    diff = np.fmax(F(0), _dot(n, L))
    I = -L
    two = F(2) * _dot(n, I)
    r = I - two[:, None] * n
    sd = np.fmax(F(0), _dot(V, r))
    spec = np.zeros_like(diff)
    for sh in np.unique(shininess):
        m = shininess == sh
        spec[m] = powi(sd[m], sh)
    spec = np.where(diff > 0, spec, F(0))
    sp = (spec * li)[:, None]
    return (F(0.5) * col) * li + att[:, None] * ((diff[:, None] * col) * li + sp)


def to_byte(lin):
    return np.fmin(np.fmax(F(255) * lin, F(0)), F(255)).astype(np.int32).astype(np.uint8)


def render_scenes(meshes, scenes, lights, K4, H, W, z_near=0.25, z_far=6.0, factor_depth=1000.0, min_pixels=800,
                  background=None, stats=None):
    """-> dict(color uint8 [S,H,W,4], depth uint16 [S,H,W], label int32 [S,H,W], vertmap f32 [S,H,W,3],
    pixel_counts int32 [N], valid int32 [S]) and, for the tests of the geometry, camz f32 [S,H,W]: the winning camera depth"""
    S = len(scenes)
    lights = _f(lights).reshape(S, 4)
    color = np.zeros((S, H, W, 4), np.uint8)
    depth = np.zeros((S, H, W), np.uint16)
    label = np.zeros((S, H, W), np.int32)
    vertmap = np.zeros((S, H, W, 3), F)
    camz = np.zeros((S, H, W), F)
    counts, valid = [], np.ones((S,), np.int32)
    for sc, instances in enumerate(scenes):
        if background is not None:
            color[sc, :, :, :3] = background[sc]
        zkey = np.full((H, W), EMPTY, np.uint64)
        tris = []
        for slot, (mi, cls, pose, shin) in enumerate(instances):
            m = meshes[mi]
            T = _f(pose).reshape(12)
            faces = np.asarray(m["faces"], np.int32).reshape(-1, 3)
            good = ((faces >= 0) & (faces < len(m["vertices"]))).all(axis=1)
            tri = setup(T, _f(m["vertices"]), np.where(good[:, None], faces, 0), K4, H, W, z_near)
            tri["ok"] &= good
            rasterise(zkey, tri, slot, z_near, z_far, stats)
            tris.append((tri, T))
        hit = zkey != EMPTY
        low = (zkey & np.uint64(0xFFFFFFFF)).astype(np.int64)
        pslot, pface = low >> 27, low & ((1 << 27) - 1)
        zwin = (zkey >> np.uint64(32)).astype(np.uint32).view(F)
        for slot, (mi, cls, pose, shin) in enumerate(instances):
            sel = hit & (pslot == slot)
            counts.append(int(sel.sum()))
            if counts[-1] < min_pixels:
                valid[sc] = 0
            if not sel.any():
                continue
            m = meshes[mi]
            tri, T = tris[slot]
            ys, xs = np.nonzero(sel)
            f = pface[ys, xs]
            inside, w, s = weights(tri["u"][f], tri["v"][f], tri["z"][f], tri["flip"][f], xs.astype(F), ys.astype(F))
            assert inside.all()
            fi = np.asarray(m["faces"], np.int32).reshape(-1, 3)[f]
            vtx = _f(m["vertices"])
            cam = tri["cam"][f]
            pos = np.stack([interp(w, s, cam[:, 0, k], cam[:, 1, k], cam[:, 2, k]) for k in range(3)], axis=1)
            obj = np.stack([interp(w, s, vtx[fi[:, 0], k], vtx[fi[:, 1], k], vtx[fi[:, 2], k]) for k in range(3)], axis=1)
            nr = _f(m["normals"])
            R = T.reshape(3, 4)
            rot = np.stack([(R[r, 0] * nr[:, 0] + R[r, 1] * nr[:, 1]) + R[r, 2] * nr[:, 2] for r in range(3)], axis=1)
            rot = _normalize(rot)
            n = np.stack([interp(w, s, rot[fi[:, 0], k], rot[fi[:, 1], k], rot[fi[:, 2], k]) for k in range(3)], axis=1)
            n = _normalize(n)
            tex = m.get("texture")
            if tex is not None and tex.shape[1] > 0:
                uvs = _f(m["uvs"])
                uv = np.stack([interp(w, s, uvs[fi[:, 0], k], uvs[fi[:, 1], k], uvs[fi[:, 2], k]) for k in range(2)], axis=1)
                col = texture_sample(np.asarray(tex, np.uint8), uv)
            elif m.get("colors") is not None:
                c = _f(m["colors"])
                col = np.stack([interp(w, s, c[fi[:, 0], k], c[fi[:, 1], k], c[fi[:, 2], k]) for k in range(3)], axis=1)
            else:
                col = np.ones_like(pos)
            lin = shade(pos, n, col, lights[sc], np.full(len(f), int(shin)))
            color[sc, ys, xs, :3] = to_byte(lin)[:, ::-1]
            color[sc, ys, xs, 3] = 255
            depth[sc, ys, xs] = np.fmin(F(65535), F(factor_depth) * zwin[ys, xs]).astype(np.int32).astype(np.uint16)
            label[sc, ys, xs] = cls
            camz[sc, ys, xs] = zwin[ys, xs]
            vertmap[sc, ys, xs] = obj
    return dict(color=color, depth=depth, label=label, vertmap=vertmap, pixel_counts=np.asarray(counts, np.int32), valid=valid,
                camz=camz)
