"""A numpy float64 restatement of csrc/mesh_param.hip (include/recmv_hip.h has the definitions): the system that
tests/cg_reference.py's conjugate gradients solve in the canonical summation order, the flat frames and corner weights, the ARAP
local step with the right-hand side and the energy, the distortion, the cotangent weights, and a dense solve of the same system
as the independent answer.  numpy neither fuses nor reorders these operations, so the GPU's bits are expected."""
import numpy as np

from cg_reference import canon_partials, canon_sum, cg, padded, rowsum


# ---------------------------------------------------------------------------------------------------------- tables
def neighbours_csr(faces, V):
    """recmv.connectivity.neighbours_csr: (offsets int32 [V+1], neighbours int32, ascending per row)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]], 0)
    e = np.unique(np.sort(e, 1), axis=0) if e.size else e.reshape(0, 2)
    rows, cols = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    order = np.lexsort((cols, rows))
    off = np.zeros(V + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(rows, minlength=V))
    return off.astype(np.int32), cols[order].astype(np.int32)


def slots_csr(faces, V):
    """recmv.connectivity.vertex_slots_csr: (offsets int64 [V+1], corner slots int64 ascending per row)."""
    fv = np.asarray(faces, np.int64).reshape(-1)
    order = np.argsort(fv, kind="stable")
    off = np.zeros(V + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(fv, minlength=V))
    return off, order.astype(np.int64)


# ---------------------------------------------------------------------------------------------------------- faces
def _corners(verts, faces):
    """(p [F,3,3] float64 with unusable faces zeroed, usable [F]): distinct indices in [0, V), finite corners, |e1 x e2| finite > 0."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = v.shape[0]
    ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])
    p = v[np.where(ok[:, None], f, 0)] if V else np.zeros((f.shape[0], 3, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= np.isfinite(p).all((1, 2))
        p = np.where(ok[:, None, None], p, 0.)
        n = _cross3(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        length = np.sqrt(_dot3(n, n))
    ok &= np.isfinite(length) & (length > 0)
    return np.where(ok[:, None, None], p, 0.), ok


def _cross3(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                     u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def _dot3(u, w):
    return u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1] + u[:, 2] * w[:, 2]


def _half_cot(p, c):
    a, b = (c + 1) % 3, (c + 2) % 3
    e1, e2 = p[:, a] - p[:, c], p[:, b] - p[:, c]
    n = _cross3(e1, e2)
    length = np.sqrt(_dot3(n, n))
    good = np.isfinite(length) & (length > 0)
    cot = _dot3(e1, e2) / np.where(good, length, 1.)
    return np.where(good & (cot > 0), 0.5 * cot, 0.)


def face_frames(verts, faces):
    """(frames [F,4] = (x1, x2, y2, area), cots [F,3]); zeros for unusable faces."""
    p, ok = _corners(verts, faces)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = _cross3(e1, e2)
    length, x1 = np.sqrt(_dot3(n, n)), np.sqrt(_dot3(e1, e1))
    ok = ok & np.isfinite(x1) & (x1 > 0)
    sx = np.where(ok, x1, 1.)
    frames = np.stack([x1, _dot3(e1, e2) / sx, length / sx, 0.5 * length], 1)
    cots = np.stack([_half_cot(p, c) for c in range(3)], 1)
    return np.where(ok[:, None], frames, 0.), np.where(ok[:, None], cots, 0.)


def cotan_weights(verts, faces, off, nbr):
    """recmv_cotan_weights on valid faces: per neighbour entry, the sum over the edge's faces, ascending, of the half cotangent
    opposite the edge."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    _, cots = face_frames(verts, faces)
    w = np.zeros(nbr.shape[0])
    off = off.astype(np.int64)
    for t in range(f.shape[0]):
        for c in range(3):
            if cots[t].any():
                a, b = int(f[t, (c + 1) % 3]), int(f[t, (c + 2) % 3])
                for i, j in ((a, b), (b, a)):
                    k = off[i] + np.searchsorted(nbr[off[i]:off[i + 1]], j)
                    w[k] += cots[t, c]
    return w


def _flat(frames):
    X = np.zeros((frames.shape[0], 3, 2))
    X[:, 1, 0] = frames[:, 0]
    X[:, 2, 0] = frames[:, 1]
    X[:, 2, 1] = frames[:, 2]
    return X


def _usable(faces, V, frames):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2]) & (frames[:, 3] > 0)


# ---------------------------------------------------------------------------------------------------------- the solve
class System:
    """The counted entries of the neighbour CSR as a padded table, d, the active vertices."""

    def __init__(self, off, nbr, w, fixed):
        V = off.shape[0] - 1
        self.V = V
        pos, valid = padded(off, nbr.shape[0])
        self.j = nbr.astype(np.int64)[pos] if nbr.size else np.zeros(pos.shape, np.int64)
        wk = np.asarray(w, np.float64)[pos] if nbr.size else np.zeros(pos.shape)
        i = np.arange(V)[:, None]
        with np.errstate(invalid="ignore"):
            self.counted = valid & (self.j >= 0) & (self.j < V) & (self.j != i) & np.isfinite(wk) & (wk > 0)
        self.j = np.where(self.counted, self.j, 0)
        self.w = np.where(self.counted, wk, 0.)
        self.fixed = np.asarray(fixed).astype(bool)
        self.d = rowsum(self.w)
        self.active = ~self.fixed & (self.d > 0)
        self.zero_rows = int((~self.fixed & ~(self.d > 0)).sum())
        self.dinv = np.where(self.active, 1. / np.where(self.active, self.d, 1.), 0.)

    def apply(self, x):
        """sum_k w_k (x_i - x_j) for the active vertices, 0 elsewhere; x [V,2]"""
        t = np.where(self.counted[:, :, None], self.w[:, :, None] * (x[:, None, :] - x[self.j]), 0.)
        return np.where(self.active[:, None], rowsum(t), 0.)

    def fixed_sum(self, u):
        t = np.where((self.counted & self.fixed[self.j])[:, :, None], self.w[:, :, None] * u[self.j], 0.)
        return rowsum(t)

    def dense(self, rhs, u):
        """The same system by numpy.linalg.solve: (u with the active rows solved, cond(A))."""
        idx = np.flatnonzero(self.active)
        where = -np.ones(self.V, np.int64)
        where[idx] = np.arange(idx.shape[0])
        A = np.zeros((idx.shape[0], idx.shape[0]))
        b = rhs[idx].astype(np.float64).copy()
        for r, i in enumerate(idx):
            for k in np.flatnonzero(self.counted[i]):
                j, wk = self.j[i, k], self.w[i, k]
                A[r, r] += wk
                if self.active[j]:
                    A[r, where[j]] -= wk
                else:
                    b[r] += wk * u[j]
        out = u.copy()
        if idx.size:
            out[idx] = np.linalg.solve(A, b)
        return out, (np.linalg.cond(A) if idx.size else 1.)


def solve(off, nbr, w, fixed, rhs, u, tol=1e-12, max_iter=None):
    """(u [V,2], iterations, residuals [2], zero_rows): the recurrence of include/recmv_hip.h."""
    S = System(off, nbr, w, fixed)
    V = S.V
    u = np.array(u, np.float64)
    rhs = np.asarray(rhs, np.float64)
    max_iter = 10 * V + 100 if max_iter is None else max_iter
    if V == 0:
        return u, 0, [0., 0.], 0
    act = S.active[:, None]
    r = np.where(act, rhs - S.apply(u), 0.)
    b = np.where(act, rhs + S.fixed_sum(u), 0.)
    u, iters, res, _ = cg(S.apply, S.dinv, r, b, u, S.active, tol, max_iter)
    return u, iters, res, S.zero_rows


# ---------------------------------------------------------------------------------------------------------- ARAP
def arap_faces(faces, V, frames, cots, uv):
    """(rot [F,2], per-face energy [F]) of the local step."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = _usable(f, V, frames)
    fs = np.where(ok[:, None], f, 0)
    X = _flat(frames)
    S = np.zeros((f.shape[0], 4))
    du, dx = [], []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        du.append(uv[fs[:, a]] - uv[fs[:, b]])
        dx.append(X[:, a] - X[:, b])
        ck = cots[:, k]
        S[:, 0] = S[:, 0] + ck * (du[k][:, 0] * dx[k][:, 0])
        S[:, 1] = S[:, 1] + ck * (du[k][:, 0] * dx[k][:, 1])
        S[:, 2] = S[:, 2] + ck * (du[k][:, 1] * dx[k][:, 0])
        S[:, 3] = S[:, 3] + ck * (du[k][:, 1] * dx[k][:, 1])
    ca, cb = S[:, 0] + S[:, 3], S[:, 2] - S[:, 1]
    with np.errstate(all="ignore"):
        length = np.sqrt(ca * ca + cb * cb)
        good = ok & np.isfinite(length) & (length > 0)
        ra = np.where(good, ca / np.where(good, length, 1.), 1.)
        rb = np.where(good, cb / np.where(good, length, 1.), 0.)
    e = np.zeros(f.shape[0])
    for k in range(3):
        d0 = du[k][:, 0] - (ra * dx[k][:, 0] - rb * dx[k][:, 1])
        d1 = du[k][:, 1] - (rb * dx[k][:, 0] + ra * dx[k][:, 1])
        e = e + cots[:, k] * (d0 * d0 + d1 * d1)
    return np.stack([ra, rb], 1), np.where(ok, e, 0.)


def arap_rhs(faces, V, frames, cots, uv):
    """(rot [F,2], rhs [V,2], energy partials, energy)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = f.shape[0]
    rot, e = arap_faces(f, V, frames, cots, uv)
    ok = _usable(f, V, frames)
    X = _flat(frames)
    inside = np.where((f >= 0) & (f < V), f, V)
    soff, slots = slots_csr(inside, V + 1)
    pos, valid = padded(soff[:V + 1], slots.shape[0])
    rhs = np.zeros((V, 2))
    for col in range(pos.shape[1]):
        slot = slots[pos[:, col]] if slots.size else np.zeros(V, np.int64)
        t, k = slot // 3, slot % 3
        use = valid[:, col] & ok[t] if F else np.zeros(V, bool)
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        ra, rb = rot[t, 0], rot[t, 1]
        c1, c2 = cots[t, k2], cots[t, k1]
        a = X[t, k] - X[t, k1]
        b = X[t, k] - X[t, k2]
        add = lambda s, x: np.where(use, s + x, s)  # noqa: E731
        rhs[:, 0] = add(rhs[:, 0], c1 * (ra * a[:, 0] - rb * a[:, 1]))
        rhs[:, 1] = add(rhs[:, 1], c1 * (rb * a[:, 0] + ra * a[:, 1]))
        rhs[:, 0] = add(rhs[:, 0], c2 * (ra * b[:, 0] - rb * b[:, 1]))
        rhs[:, 1] = add(rhs[:, 1], c2 * (rb * b[:, 0] + ra * b[:, 1]))
    return rot, rhs, canon_partials(e), canon_sum(e)


def distortion(faces, V, frames, uv):
    """[F,3] = (s1, s2, det); NaN, NaN, 0 for unusable faces."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = _usable(f, V, frames)
    fs = np.where(ok[:, None], f, 0)
    a, b = uv[fs[:, 1]] - uv[fs[:, 0]], uv[fs[:, 2]] - uv[fs[:, 0]]
    x1, x2, y2 = (np.where(ok, frames[:, k], 1.) for k in range(3))
    J00, J10 = a[:, 0] / x1, a[:, 1] / x1
    J01, J11 = (b[:, 0] - J00 * x2) / y2, (b[:, 1] - J10 * x2) / y2
    E, Fh, G, H = (J00 + J11) * 0.5, (J00 - J11) * 0.5, (J10 + J01) * 0.5, (J10 - J01) * 0.5
    Q, R = np.sqrt(E * E + H * H), np.sqrt(Fh * Fh + G * G)
    out = np.stack([Q + R, np.where(Q > R, Q - R, R - Q), J00 * J11 - J01 * J10], 1)
    return np.where(ok[:, None], out, np.array([np.nan, np.nan, 0.])[None, :])


# ---------------------------------------------------------------------------------------------------------- the maps
def boundary_loop(faces):
    """The one boundary loop of a disk, by recmv.connectivity.boundary_loops' rule (lowest start, lowest unwalked neighbour)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]], 0), 1)
    u, cnt = np.unique(e, axis=0, return_counts=True)
    nbrs = {}
    for a, b in u[cnt == 1].tolist():
        nbrs.setdefault(a, []).append(b)
        nbrs.setdefault(b, []).append(a)
    start = min(nbrs)
    loop, used, cur = [start], set(), start
    while True:
        nxt = [n for n in sorted(nbrs[cur]) if (min(cur, n), max(cur, n)) not in used]
        if not nxt:
            break
        used.add((min(cur, nxt[0]), max(cur, nxt[0])))
        if nxt[0] == start:
            break
        loop.append(nxt[0])
        cur = nxt[0]
    ahead = set(map(tuple, np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0).tolist()))
    return loop if (loop[0], loop[1]) in ahead else [loop[0]] + loop[:0:-1]      # along the faces' own half-edges


def circle_boundary(verts, loop):
    """The loop's vertices on the unit circle, angles proportional to cumulative edge length: [len(loop), 2] float64."""
    p = np.asarray(verts, np.float32).astype(np.float64)[loop]
    d = np.roll(p, -1, 0) - p
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    cum = np.concatenate([[0.], np.cumsum(length)[:-1]])
    ang = 2. * np.pi * (cum / length.sum())
    return np.stack([np.cos(ang), np.sin(ang)], 1)


def harmonic_system(verts, faces, weights="cotangent"):
    """(off, nbr, w, fixed, rhs, u0) of the harmonic map of a disk."""
    V = verts.shape[0]
    off, nbr = neighbours_csr(faces, V)
    w = cotan_weights(verts, faces, off, nbr) if weights == "cotangent" else np.ones(nbr.shape[0])
    loop = boundary_loop(faces)
    fixed = np.zeros(V, np.uint8)
    fixed[loop] = 1
    u0 = np.zeros((V, 2))
    u0[loop] = circle_boundary(verts, loop)
    return off, nbr, w, fixed, np.zeros((V, 2)), u0


def arap_iteration(verts, faces, uv, tol=1e-12, max_iter=None, tables=None):
    """One local/global iteration from uv: (uv', rot, rhs, energy before, CG iterations)."""
    V = verts.shape[0]
    frames, cots = face_frames(verts, faces)
    off, nbr = neighbours_csr(faces, V)
    w = cotan_weights(verts, faces, off, nbr) if tables is None else tables
    rot, rhs, _, energy = arap_rhs(faces, V, frames, cots, uv)
    fixed = np.zeros(V, np.uint8)
    fixed[0] = 1
    out, iters, _, _ = solve(off, nbr, w, fixed, rhs, uv, tol, max_iter)
    return out, rot, rhs, energy, iters
