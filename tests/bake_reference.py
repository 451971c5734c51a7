"""Texture baking restated in numpy: every rule of include/recmv_hip.h's section on csrc/texture_bake.hip, in float64 / float32
exactly as stated there (numpy's element-wise operations round once each and never fuse), and the coverage rule once more in
exact arithmetic (fractions.Fraction on the same float64 inputs) to show where the float64 formula and the geometry part."""
import math
from fractions import Fraction

import numpy as np

NO_OWNER = np.int32(2 ** 31 - 1)
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))      # (dx, dy): W, E, N, S, NW, NE, SW, SE


# ------------------------------------------------------------------------------------------------------------- fit_uv
def fit_uv(uv, size, margin):
    """uv [V,2] float64 scaled uniformly in texels and shifted so that the chart keeps `margin` texels from every side of the
    H x W image and is centred in what remains; unit coordinates (texel / W, texel / H)."""
    H, W = size
    uv = np.asarray(uv, np.float64)
    lo = uv.min(0)
    ext = uv.max(0) - lo
    avail = np.array([W - 2. * margin, H - 2. * margin])
    if not (np.isfinite(uv).all() and avail.min() > 0 and ext.max() > 0):
        raise ValueError("fit_uv: the chart must be finite and not a point, the margins must leave room")
    s = min(avail[k] / ext[k] for k in range(2) if ext[k] > 0)
    off = margin + (avail - ext * s) / 2.
    return ((uv - lo) * s + off) / np.array([float(W), float(H)])


# ------------------------------------------------------------------------------------------------------------- coverage
def edge(uv, a, b, px, py):
    lo, hi = min(a, b), max(a, b)
    ul, vl = uv[lo, 0], uv[lo, 1]
    e = (uv[hi, 0] - ul) * (py - vl) - (uv[hi, 1] - vl) * (px - ul)
    return -e if a > b else e


def area(uv, row):
    """A of a face row, or None when the face covers nothing."""
    V = uv.shape[0]
    i0, i1, i2 = (int(x) for x in row)
    if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= V or len({i0, i1, i2}) < 3:
        return None
    with np.errstate(all="ignore"):
        A = edge(uv, i0, i1, uv[i2, 0], uv[i2, 1])
    return float(A) if np.isfinite(A) and A != 0. else None


def box(uv, row, H, W):
    u, v = uv[list(row), 0], uv[list(row), 1]
    w, h = float(W), float(H)
    x0, x1 = max(0., math.floor(u.min() * w - 0.5)), min(w - 1., math.ceil(u.max() * w - 0.5))
    y0, y1 = max(0., math.floor(h - 0.5 - v.max() * h)), min(h - 1., math.ceil(h - 0.5 - v.min() * h))
    return (int(x0), int(x1), int(y0), int(y1)) if x0 <= x1 and y0 <= y1 else None


def centres(x0, x1, y0, y1, H, W):
    x, y = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1))
    return x, y, (x.astype(np.float64) + 0.5) / float(W), ((H - y).astype(np.float64) - 0.5) / float(H)


def cover(uv, row, A, px, py):
    i0, i1, i2 = (int(x) for x in row)
    e = [edge(uv, i1, i2, px, py), edge(uv, i2, i0, px, py), edge(uv, i0, i1, px, py)]
    if A < 0:
        e = [-x for x in e]
    return e, (e[0] >= 0.) & (e[1] >= 0.) & (e[2] >= 0.)


def rasterize(uv, faces, size):
    """(face [H,W] int32, bary [H,W,3] float32, count [H,W] int32)."""
    H, W = size
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    owner = np.full((H, W), NO_OWNER, np.int32)
    count = np.zeros((H, W), np.int32)
    bary = np.zeros((H, W, 3), np.float32)
    boxes = {}
    for t, row in enumerate(np.asarray(faces).reshape(-1, 3)):
        A = area(uv, row)
        b = box(uv, row, H, W) if A is not None and H > 0 and W > 0 else None
        if b is None:
            continue
        x, y, px, py = centres(*b, H, W)
        _, inside = cover(uv, row, A, px, py)
        owner[y[inside], x[inside]] = np.minimum(owner[y[inside], x[inside]], t)
        count[y[inside], x[inside]] += 1
        boxes[t] = (row, A, b)
    for t, (row, A, b) in boxes.items():
        x, y, px, py = centres(*b, H, W)
        mine = owner[y, x] == t
        if not mine.any():
            continue
        with np.errstate(all="ignore"):
            e, _ = cover(uv, row, A, px[mine], py[mine])
            S = e[0] + e[1] + e[2]
            bary[y[mine], x[mine]] = np.stack([(e[k] / S).astype(np.float32) for k in range(3)], -1)
    face = np.where(owner == NO_OWNER, np.int32(-1), owner).astype(np.int32)
    return face, bary, count


def rasterize_exact(uv, faces, size):
    """(owner, count) by the same rule in exact arithmetic on the same float64 inputs, the coordinates and the texel centres:
    what the three edge functions are when nothing is rounded on the way."""
    H, W = size
    uv = np.asarray(uv, np.float64)
    q = [[Fraction(float(x)) for x in r] for r in uv]
    cx = [Fraction((x + 0.5) / float(W)) for x in range(W)]
    cy = [Fraction((float(H - y) - 0.5) / float(H)) for y in range(H)]
    owner = np.full((H, W), -1, np.int32)
    count = np.zeros((H, W), np.int32)

    def ex(a, b, px, py):
        lo, hi = min(a, b), max(a, b)
        e = (q[hi][0] - q[lo][0]) * (py - q[lo][1]) - (q[hi][1] - q[lo][1]) * (px - q[lo][0])
        return -e if a > b else e
    for t, row in enumerate(np.asarray(faces).reshape(-1, 3)):
        i0, i1, i2 = (int(x) for x in row)
        A = ex(i0, i1, q[i2][0], q[i2][1])
        if A == 0:
            continue
        sign = -1 if A < 0 else 1
        us, vs = [q[i][0] for i in (i0, i1, i2)], [q[i][1] for i in (i0, i1, i2)]
        xs = [x for x in range(W) if min(us) <= cx[x] <= max(us)]
        ys = [y for y in range(H) if min(vs) <= cy[y] <= max(vs)]
        for y in ys:
            for x in xs:
                px, py = cx[x], cy[y]
                if sign * ex(i1, i2, px, py) >= 0 and sign * ex(i2, i0, px, py) >= 0 and sign * ex(i0, i1, px, py) >= 0:
                    count[y, x] += 1
                    if owner[y, x] < 0:
                        owner[y, x] = t
    return owner, count


# --------------------------------------------------------------------------------------------------------------- gutter
def gutter(face, passes):
    face = np.asarray(face)
    H, W = face.shape
    src = np.where(face >= 0, np.arange(H * W, dtype=np.int32).reshape(H, W), np.int32(-1)).astype(np.int32)
    for _ in range(passes):
        p = np.full((H + 2, W + 2), -1, np.int32)
        p[1:-1, 1:-1] = src
        nxt = src.copy()
        for dx, dy in NEIGHBOURS:
            c = p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            take = (nxt < 0) & (c >= 0)
            nxt[take] = c[take]
        src = nxt
    return src


def pad(image, src):
    flat = image.reshape(src.size, -1)
    s = src.reshape(-1)
    out = np.where((s >= 0)[:, None], flat[np.clip(s, 0, None)], np.float32(0))
    return out.reshape(image.shape).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- attributes
def mix(rows, b, attr, normalise):
    """(b0 a0 + b1 a1) + b2 a2 in float32 for corner rows [T,3], bary [T,3] float32, attr [V,C] float32."""
    attr = np.asarray(attr, np.float32)
    b = np.asarray(b, np.float32)
    with np.errstate(all="ignore"):
        v = b[:, 0:1] * attr[rows[:, 0]] + b[:, 1:2] * attr[rows[:, 1]] + b[:, 2:3] * attr[rows[:, 2]]
        if normalise:
            x, y, z = (v[:, k].astype(np.float64) for k in range(3))
            n = np.sqrt(x * x + y * y + z * z)
            ok = np.isfinite(n) & (n > 0)
            for k, c in enumerate((x, y, z)):
                v[ok, k] = (c[ok] / n[ok]).astype(np.float32)
    return v.astype(np.float32)


def valid_faces(idx, faces, V):
    faces = np.asarray(faces).reshape(-1, 3)
    idx = np.asarray(idx).astype(np.int64)
    ok = (idx >= 0) & (idx < faces.shape[0])
    rows = faces[np.where(ok, idx, 0)] if faces.shape[0] else np.zeros((idx.shape[0], 3), np.int64)
    ok &= ((rows >= 0) & (rows < V)).all(1) & (rows[:, 0] != rows[:, 1]) & (rows[:, 0] != rows[:, 2]) & (rows[:, 1] != rows[:, 2])
    return ok, rows


def interpolate(face, bary, faces, attr, normalise=False):
    attr = np.asarray(attr, np.float32)
    shape = face.shape
    ok, rows = valid_faces(face.reshape(-1), faces, attr.shape[0])
    out = np.zeros((ok.shape[0], attr.shape[1]), np.float32)
    out[ok] = mix(rows[ok], bary.reshape(-1, 3)[ok], attr, normalise)
    return out.reshape(shape + (attr.shape[1],))


def dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def cross3(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def transfer(src_face, src_point, src_verts, src_faces, src_attr, normalise=False):
    """(bary [T,3] float32, out [T,C] float32) of the hits on the source mesh."""
    src_attr = np.asarray(src_attr, np.float32)
    ok, rows = valid_faces(src_face, src_faces, src_verts.shape[0])
    T = ok.shape[0]
    bary, out = np.zeros((T, 3), np.float32), np.zeros((T, src_attr.shape[1]), np.float32)
    p = np.asarray(src_verts, np.float32).astype(np.float64)
    p0, p1, p2 = p[rows[ok, 0]], p[rows[ok, 1]], p[rows[ok, 2]]
    e1, e2, d = p1 - p0, p2 - p0, np.asarray(src_point, np.float32).astype(np.float64)[ok] - p0
    with np.errstate(all="ignore"):
        d11, d12, d22, r1, r2 = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2), dot3(d, e1), dot3(d, e2)
        det = d11 * d22 - d12 * d12
        good = np.isfinite(det) & (det > 0)
        b1 = np.where(good, (d22 * r1 - d12 * r2) / det, 0.)
        b2 = np.where(good, (d11 * r2 - d12 * r1) / det, 0.)
    b = np.stack([1. - b1 - b2, b1, b2], -1).astype(np.float32)
    bary[ok] = b
    out[ok] = mix(rows[ok], b, src_attr, normalise)
    return bary, out


def adjacency(faces, V):
    """Per vertex the faces in the order of recmv.shading.vertex_face_adjacency: corner 1, corner 2, corner 0, each over the
    faces in order, sorted stably by vertex."""
    fans = [[] for _ in range(V)]
    for c in (1, 2, 0):
        for t, row in enumerate(faces):
            fans[int(row[c])].append(t)
    return fans


def vertex_tangents(verts, faces, uv, normals):
    """[V,4] float32: the tangent and its handedness."""
    verts = np.asarray(verts, np.float32).astype(np.float64)
    uv = np.asarray(uv, np.float64)
    faces = np.asarray(faces).reshape(-1, 3)
    V = verts.shape[0]
    out = np.zeros((V, 4), np.float32)
    out[:, 3] = 1
    contrib = {}
    with np.errstate(all="ignore"):
        for t, row in enumerate(faces):
            A = area(uv, row)
            if A is None:
                continue
            p0, p1, p2 = verts[row[0]], verts[row[1]], verts[row[2]]
            e1, e2 = p1 - p0, p2 - p0
            n = cross3(e1, e2)
            a3 = 0.5 * np.sqrt(dot3(n, n))
            if not (np.isfinite(a3) and a3 > 0):
                continue
            du1, dv1 = uv[row[1]] - uv[row[0]]
            du2, dv2 = uv[row[2]] - uv[row[0]]
            w = a3 / A
            contrib[t] = (w * (e1 * dv2 - e2 * dv1), w * (e2 * du1 - e1 * du2))
        nrm = np.asarray(normals, np.float32).astype(np.float64)
        for i, fan in enumerate(adjacency(faces, V)):
            T, B = np.zeros(3), np.zeros(3)
            for t in fan:
                if t in contrib:
                    T = T + contrib[t][0]
                    B = B + contrib[t][1]
            n = nrm[i]
            t = T - n * dot3(n, T)
            length = np.sqrt(dot3(t, t))
            if np.isfinite(length) and length > 0:
                t = t / length
                out[i, :3] = t.astype(np.float32)
                out[i, 3] = -1. if dot3(cross3(n, t), B) < 0 else 1.
    return out


def encode_normal(face, normal, frame_n, frame_t):
    """[..., 3] float32: 0.5 + 0.5 (N.t', w N.(n x t'), N.n), t' = t made orthogonal to n; zeros where face < 0."""
    N, n = np.asarray(normal, np.float32).astype(np.float64), np.asarray(frame_n, np.float32).astype(np.float64)
    ft = np.asarray(frame_t, np.float32)
    t, w = ft[..., :3].astype(np.float64), np.where(ft[..., 3] < 0, -1., 1.)
    with np.errstate(all="ignore"):
        o = t - n * dot3(n, t)[..., None]
        length = np.sqrt(dot3(o, o))
        ok = np.isfinite(length) & (length > 0)
        t = np.where(ok[..., None], o / np.where(ok, length, 1.)[..., None], t)
        c = np.stack([0.5 + 0.5 * dot3(N, t), 0.5 + 0.5 * (w * dot3(N, cross3(n, t))), 0.5 + 0.5 * dot3(N, n)], -1)
    return np.where((np.asarray(face) >= 0)[..., None], c, 0.).astype(np.float32)


def quantise(x):
    """round(255 clamp(x)) as uint8, the PNGs' values (NaN -> 0)."""
    x = np.nan_to_num(np.asarray(x, np.float32), nan=0.)
    return np.rint(255. * np.clip(x, 0., 1.).astype(np.float64)).astype(np.uint8)


def project_how(hit_f, t_f, hit_b, t_b):
    """The codes of recmv.bake.HOW per point for projection 'normal': 1 the forward hit (also on a tie), 2 the backward hit, 3 the
    closest-point fallback where neither segment hits."""
    how = []
    for hf, tf, hb, tb in zip(hit_f, t_f, hit_b, t_b):
        if hf and hb:
            how.append(1 if tf <= tb else 2)
        else:
            how.append(1 if hf else (2 if hb else 3))
    return np.array(how, np.uint8)
