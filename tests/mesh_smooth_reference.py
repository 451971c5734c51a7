"""numpy float64 restatement of csrc/mesh_smooth.hip's four kernels and of recmv.smooth.smooth, the reference of
tests/test_mesh_smooth_cpu.py and tests/test_gpu_mesh_smooth.py.  Plain loops in table order.  Beside every result come the
ingredients of its error bound: the number of terms of each output's sum and the sum of the terms' magnitudes (every term as
the magnitude its rounding scales with), so that a test can state |got - ref| <= 1/2 ulp_f32(ref) + gamma_n * sum |terms|."""
import math

import numpy as np

U = 2.0 ** -53
PASS_BAND = 0.1
STEP_OPS = 8            # beside the row's terms: the product with the weight, the division, the difference, lambda, the sum
COT_OPS = 24            # one half-cotangent: 6 differences, 9 products and 5 sums of dot and cross, the squares, root, division
FILTER_OPS = 40         # one weight: 6 differences, two squared lengths, two scalings, two exp (a few ulps each), two products
UPDATE_OPS = 16         # one face: the centroid (3 sums, a division), the difference, the dot product, the product, the division


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1. - n * U)


def ulp32(x):
    """The spacing of float32 at |x| (of the binade that holds x; the smallest normal spacing below it)."""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (e - 23)


def valid_index_faces(f, V):
    f = np.asarray(f, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


class Tables:
    """The tables of the faces with valid indices (the others take no part; `f` keeps every row so that slots and face ids
    are those of the input): nbr[i] ascending neighbours, slots[i] ascending corner slots, ff[k] ascending edge-adjacent faces,
    bnbr [V,2], boundary [V] bool, and the flat CSR forms the kernels read."""

    def __init__(self, f, V):
        f = np.asarray(f, np.int64).reshape(-1, 3)
        self.f, self.V, self.F = f, V, len(f)
        ok = valid_index_faces(f, V)
        edge_faces = {}
        self.slots = [[] for _ in range(V)]
        for k in np.nonzero(ok)[0]:
            for c in range(3):
                self.slots[f[k, c]].append(3 * k + c)
                a, b = int(f[k, (c + 1) % 3]), int(f[k, (c + 2) % 3])
                edge_faces.setdefault((min(a, b), max(a, b)), []).append(int(k))
        self.edge_faces = edge_faces
        nbr = [set() for _ in range(V)]
        bn = [[] for _ in range(V)]
        ff = [set() for _ in range(self.F)]
        for (a, b), faces in edge_faces.items():
            nbr[a].add(b)
            nbr[b].add(a)
            if len(faces) == 1:
                bn[a].append(b)
                bn[b].append(a)
            for x in faces:
                ff[x].update(y for y in faces if y != x)
        self.nbr = [sorted(s) for s in nbr]
        self.ff = [sorted(s) for s in ff]
        self.boundary = np.array([len(b) > 0 for b in bn], bool)
        self.bnbr = np.full((V, 2), -1, np.int64)
        for i, b in enumerate(bn):
            b = sorted(b)
            if len(b) == 2:
                self.bnbr[i] = b
            elif b:
                self.bnbr[i, 0] = b[0]

    @staticmethod
    def csr(rows, dtype):
        off = np.cumsum([0] + [len(r) for r in rows]).astype(dtype)
        return off, np.array([x for r in rows for x in r], dtype)


def _cross(u, w):
    return np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])


def _dot(u, w):
    return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]


def face_geometry(v, f):
    """(unit normals [F,3], areas [F], centroids [F,3], good [F]) float64 as recmv.smooth.face_geometry; rows with invalid indices
    are not good."""
    v = np.asarray(v, np.float32).astype(np.float64)
    F = len(f)
    unit, area, cen, good = np.zeros((F, 3)), np.zeros(F), np.zeros((F, 3)), np.zeros(F, bool)
    ok = valid_index_faces(f, len(v))
    with np.errstate(all="ignore"):
        for k in range(F):
            if not ok[k]:
                continue
            a, b, c = v[f[k, 0]], v[f[k, 1]], v[f[k, 2]]
            n = _cross(b - a, c - a)
            length = math.sqrt(_dot(n, n)) if _dot(n, n) >= 0 else float("nan")
            cen[k] = (a + b + c) / 3.
            if np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all() and 0 < length < math.inf:
                unit[k], area[k], good[k] = n / length, 0.5 * length, True
    return unit, area, cen, good


def _half_cot(p, c):
    """(1/2 max(0, cot) at corner c of the corners p [3,3], the magnitude its rounding error scales with)."""
    e1, e2 = p[(c + 1) % 3] - p[c], p[(c + 2) % 3] - p[c]
    n = _cross(e1, e2)
    length = math.sqrt(_dot(n, n))
    if not 0 < length < math.inf:
        return 0., 0.
    cot = _dot(e1, e2) / length
    a_dot = abs(e1[0] * e2[0]) + abs(e1[1] * e2[1]) + abs(e1[2] * e2[2])
    prods = np.array([abs(e1[1] * e2[2]) + abs(e1[2] * e2[1]), abs(e1[2] * e2[0]) + abs(e1[0] * e2[2]),
                      abs(e1[0] * e2[1]) + abs(e1[1] * e2[0])])
    spread = float((np.abs(n) * prods).sum()) / (length * length)                 # >= 1: how much the cross product cancels
    mag = 0.5 * (a_dot / length + abs(cot) * spread)
    return (0.5 * cot if cot > 0 else 0.), mag


def cotan_weights(v, f, t=None):
    """(w: one row per vertex in t.nbr's order, invalid faces, terms: the faces that added to each entry, mags: the sum of
    the terms' magnitudes) — rows as lists of arrays."""
    v64 = np.asarray(v, np.float32).astype(np.float64)
    V = len(v64)
    t = Tables(f, V) if t is None else t
    good = face_geometry(v, t.f)[3]
    w = [np.zeros(len(r)) for r in t.nbr]
    terms = [np.zeros(len(r), np.int64) for r in t.nbr]
    mags = [np.zeros(len(r)) for r in t.nbr]
    with np.errstate(all="ignore"):
        for i in range(V):
            where = {j: k for k, j in enumerate(t.nbr[i])}
            for slot in t.slots[i]:
                k, c = divmod(slot, 3)
                if not good[k]:
                    continue
                p = v64[t.f[k]]
                for other, corner in (((c + 1) % 3, (c + 2) % 3), ((c + 2) % 3, (c + 1) % 3)):
                    val, mag = _half_cot(p, corner)
                    at = where[int(t.f[k, other])]
                    w[i][at] += val
                    terms[i][at] += 1
                    mags[i][at] += mag
    return w, int((~good).sum()), terms, mags


def laplacian_step(x, t, lam, w=None, fixed=None, bnbr=None):
    """(out float32, the unrounded float64 result, terms [V], mags [V,3]) of one step on x [V,3] float32; w: rows as
    cotan_weights gives them, or None."""
    xf = np.asarray(x, np.float32)
    x = xf.astype(np.float64)
    V = len(x)
    ref, terms, mags = x.copy(), np.zeros(V, np.int64), np.abs(x)
    moved = np.zeros(V, bool)
    for i in range(V):
        if fixed is not None and fixed[i]:
            continue
        p = x[i]
        if bnbr is not None and (bnbr[i, 0] >= 0 or bnbr[i, 1] >= 0):
            if not (0 <= bnbr[i, 0] < V and 0 <= bnbr[i, 1] < V):
                continue
            a, b = x[bnbr[i, 0]], x[bnbr[i, 1]]
            m, mm, cnt = 0.5 * (a + b), 0.5 * (np.abs(a) + np.abs(b)), 2
        else:
            s, sm, total, cnt = np.zeros(3), np.zeros(3), 0., 0
            for k, j in enumerate(t.nbr[i]):
                wk = 1. if w is None else w[i][k]
                if not 0 < wk < math.inf:
                    continue
                s = s + (wk * x[j] if w is not None else x[j])
                sm = sm + wk * np.abs(x[j])
                total += wk
                cnt += 1
            if cnt == 0 or not 0 < total < math.inf:
                continue
            m, mm = s / total, sm / total
        ref[i] = p + lam * (m - p)
        terms[i] = cnt
        mags[i] = np.abs(p) + abs(lam) * (mm + np.abs(p))
        moved[i] = True
    out = xf.copy()
    out[moved] = ref[moved].astype(np.float32)
    return out, ref, terms, mags


def normal_filter(n, area, cen, t, sigma_c, sigma_s):
    """(out float32, the unrounded float64 unit normals, terms [F], rel [F]: sum |w_j| |n_j| over the length of the sum, gain [F]:
    how much a change of the input normals (2-norm) can grow in this face's output) of one filter iteration."""
    nf = np.asarray(n, np.float32)
    n = nf.astype(np.float64)
    F = len(n)
    inv2c, inv2s = 1. / (2. * sigma_c * sigma_c), 1. / (2. * sigma_s * sigma_s)
    ref, terms, rel, gain = n.copy(), np.ones(F, np.int64), np.zeros(F), np.zeros(F)
    moved = np.zeros(F, bool)
    with np.errstate(all="ignore"):
        for i in range(F):
            s = area[i] * n[i]
            tot = abs(area[i]) * np.linalg.norm(n[i])
            sens = abs(area[i])
            for j in t.ff[i]:
                dc, dn = cen[i] - cen[j], n[i] - n[j]
                wj = area[j] * math.exp(-(_dot(dc, dc) * inv2c)) * math.exp(-(_dot(dn, dn) * inv2s))
                s = s + wj * n[j]
                tot += abs(wj) * np.linalg.norm(n[j])
                sens += abs(wj) * (1. + 2. * np.linalg.norm(dn) * 2. * inv2s * np.linalg.norm(n[j]))
                terms[i] += 1
            length = math.sqrt(_dot(s, s))
            if 0 < length < math.inf:
                ref[i], moved[i] = s / length, True
                rel[i], gain[i] = tot / length, 2. * sens / length
            else:
                gain[i] = 1.
    out = nf.copy()
    out[moved] = ref[moved].astype(np.float32)
    return out, ref, terms, rel, gain


def vertex_update(x, f, n, t, fixed=None):
    """(out float32, the unrounded float64 result, terms [V], mags [V,3], reach [V]: the largest |c_f - x_i| of a vertex's faces) of
    one vertex update."""
    xf = np.asarray(x, np.float32)
    x = xf.astype(np.float64)
    n = np.asarray(n, np.float32).astype(np.float64)
    V = len(x)
    ref, terms, mags, reach = x.copy(), np.zeros(V, np.int64), np.abs(x), np.zeros(V)
    moved = np.zeros(V, bool)
    with np.errstate(all="ignore"):
        for i in range(V):
            if fixed is not None and fixed[i]:
                continue
            s, sm, cnt = np.zeros(3), np.zeros(3), 0
            for slot in t.slots[i]:
                k = slot // 3
                q = x[f[k]]
                d = (q[0] + q[1] + q[2]) / 3. - x[i]
                h = _dot(n[k], d)
                if not (np.isfinite(h) and 0 < _dot(n[k], n[k]) < math.inf):
                    continue
                s = s + n[k] * h
                sm = sm + np.abs(n[k]) * float((np.abs(n[k]) * (np.abs(q).sum(0) / 3. + np.abs(x[i]))).sum())
                reach[i] = max(reach[i], float(np.linalg.norm(d)))
                cnt += 1
            if cnt == 0:
                continue
            ref[i] = x[i] + s / cnt
            terms[i], mags[i], moved[i] = cnt, np.abs(x[i]) + sm / cnt, True
    out = xf.copy()
    out[moved] = ref[moved].astype(np.float32)
    return out, ref, terms, mags, reach


def step_bound(ref, terms, mags, ops):
    """1/2 ulp_f32(ref) + gamma_(terms + ops) * mags, per output."""
    return 0.5 * ulp32(ref) + gamma(terms + ops)[:, None] * mags


def default_mu(lam):
    return 1. / (PASS_BAND - 1. / lam)


def mean_centroid_distance(cen, t):
    d = [np.linalg.norm(cen[i] - cen[j]) for i in range(len(cen)) for j in t.ff[i]]
    return float(np.mean(d)) if d else 1.


def smooth(v, f, method="taubin", iterations=10, lam=0.5, mu=None, weights="uniform", reweight=False, boundary="fixed",
           fixed=None, normal_iterations=5, vertex_iterations=10, sigma_s=0.35, sigma_c=None):
    """The driver, rounding to float32 after every step as the kernels do: (verts' float32, bound: how far a path that meets every
    one-step bound can be from this result, one number for the whole mesh, infinity-norm).

    The bound is propagated step by step: a difference D of the two paths' states before a step becomes at most gain * D + b
    after it, b the largest one-step bound of that step plus one float32 spacing where the two float64 results, however
    close, may round to different neighbours.  lam step: gain |1 - lam| + |lam| = 1 on (0, 1]; mu step: 1 + 2 |mu|;
    cotangent weights add the weights' own relative error times the reach of a row.  The normal filter's gain is taken from
    its own sums (normal_filter); a vertex update's is 2 in the 2-norm (I - mean n n^T and mean n n^T are both
    non-expansive) plus twice the reach times the difference of the normals."""
    v = np.asarray(v, np.float32)
    V = len(v)
    t = Tables(f, V)
    pinned = np.zeros(V, bool)
    if boundary == "fixed":
        pinned |= t.boundary
    if fixed is not None:
        pinned |= np.asarray(fixed, bool)
    bnbr = t.bnbr if boundary == "curve" else None
    x, D = v.copy(), 0.
    if method == "bilateral":
        unit, area, cen, _ = face_geometry(v, t.f)
        sigma_c = mean_centroid_distance(cen, t) if sigma_c is None else sigma_c
        n, Dn = unit.astype(np.float32), 0.
        for _ in range(normal_iterations):
            n, ref, terms, rel, gain = normal_filter(n, area, cen, t, sigma_c, sigma_s)
            b = float((ulp32(ref).max(1) * math.sqrt(3) + 2. * gamma(terms + FILTER_OPS) * rel).max()) if len(ref) else 0.
            Dn = float(gain.max()) * Dn + b if len(ref) else 0.
        for _ in range(vertex_iterations):
            x, ref, terms, mags, reach = vertex_update(x, t.f, n, t, pinned)
            b = float((step_bound(ref, terms, mags, UPDATE_OPS) + 0.5 * ulp32(ref)).max()) * math.sqrt(3)
            D = 2. * D + b + 2. * float(reach.max()) * Dn + 2. * D * Dn
        return x, D, {"sigma_c": sigma_c, "normal_bound": Dn}
    mu = default_mu(lam) if mu is None else mu
    w = rho = None
    for it in range(iterations):
        if weights == "cotangent" and (w is None or reweight):
            w, _, wt, wm = cotan_weights(x, t.f, t)
            rho = max([float((gamma(a + COT_OPS) * m).sum() / max(r.sum(), 1e-300)) for a, m, r in zip(wt, wm, w) if len(r)] + [0.])
        for step in ((lam, mu) if method == "taubin" else (lam,)):
            spread = float(np.abs(x).max()) if V else 0.
            x, ref, terms, mags = laplacian_step(x, t, step, w, pinned, bnbr)
            b = float((step_bound(ref, terms, mags, STEP_OPS) + 0.5 * ulp32(ref)).max()) if V else 0.
            if rho is not None:
                b += 4. * abs(step) * rho * spread
            D = (abs(1. - step) + abs(step)) * D + b
    return x, D, {"mu": mu}


# ---- what the quality tests measure ---------------------------------------------------------------------------------------------------
def roughness(v, f):
    """The mean dihedral angle over the edges with two faces, weighted by the two faces' areas."""
    t = Tables(f, len(v))
    unit, area, _, _ = face_geometry(v, t.f)
    num = den = 0.
    for faces in t.edge_faces.values():
        if len(faces) == 2:
            a, b = faces
            c = _cross(unit[a], unit[b])
            num += (area[a] + area[b]) * math.atan2(math.sqrt(_dot(c, c)), _dot(unit[a], unit[b]))
            den += area[a] + area[b]
    return num / den if den > 0 else 0.


def volume(v, f):
    v = np.asarray(v, np.float64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum()) / 6.


def area(v, f):
    return float(face_geometry(v, f)[1].sum())
