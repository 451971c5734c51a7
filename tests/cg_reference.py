"""A numpy float64 restatement of what csrc/mesh_cg.h and csrc/mesh_device.h give the two mesh solvers: the canonical summation
order (the xor butterfly as array operations, then the waves, then the slots) and the Jacobi-preconditioned conjugate-gradient
recurrence over C columns with its per-column freezes; and, from csrc/lap_align.hip's header comment, the system of
recmv_lap_align_solve.  tests/param_reference.py has the parameterisation's system.  numpy neither fuses nor reorders these
operations, so the GPU's bits are expected."""
import numpy as np

BLOCK, WAVE = 256, 64


# ---------------------------------------------------------------------------------------------------------- the sums
def canon_sum(terms):
    """One dot product's terms [n] (term i of vertex or face i) in the canonical order."""
    n = terms.shape[0]
    nslots = max((n + BLOCK - 1) // BLOCK, 1)
    x = np.zeros(nslots * BLOCK)
    x[:n] = terms
    slots = _block(x.reshape(nslots, BLOCK))
    acc = np.zeros(BLOCK)
    for s0 in range(0, nslots, BLOCK):                      # accumulator t adds the slots t, t + 256, ...
        part = slots[s0:s0 + BLOCK]
        acc[:part.shape[0]] = acc[:part.shape[0]] + part
    return float(_block(acc[None, :])[0])


def canon_partials(terms):
    n = terms.shape[0]
    nslots = (n + BLOCK - 1) // BLOCK
    x = np.zeros(nslots * BLOCK)
    x[:n] = terms
    return _block(x.reshape(nslots, BLOCK))


def _block(x):
    """[m, 256] -> [m]: the xor butterfly over each wave's 64 lanes, then the four waves from 0."""
    x = x.reshape(x.shape[0], BLOCK // WAVE, WAVE)
    lane = np.arange(WAVE)
    off = WAVE // 2
    while off:
        x = x + x[:, :, lane ^ off]
        off //= 2
    t = np.zeros(x.shape[0])
    for w in range(BLOCK // WAVE):
        t = t + x[:, w, 0]
    return t


# ---------------------------------------------------------------------------------------------------------- tables
def padded(off, n):
    """A CSR's rows as a table: (position [R, D], valid [R, D])."""
    off = np.asarray(off, np.int64)
    cnt = off[1:] - off[:-1]
    D = int(cnt.max()) if cnt.size else 0
    col = np.arange(D)
    return np.minimum(off[:-1, None] + col[None, :], max(n - 1, 0)), col[None, :] < cnt[:, None]


def rowsum(terms):
    """sum over a row's entries, in row order, from 0 (terms of entries that do not count are +0)"""
    s = np.zeros(terms.shape[:1] + terms.shape[2:])
    for k in range(terms.shape[1]):
        s = s + terms[:, k]
    return s


# ---------------------------------------------------------------------------------------------------------- the recurrence
def cg(apply, dinv, r, b, u, live, tol, max_iter):
    """csrc/mesh_cg.h's recurrence over the C columns of r, b, u [V, C] from the first residual r and the right-hand side b:
    (u, iterations, residuals [C], the iteration count at which each column froze).  `apply` is q = A p, dinv [V] the inverse
    diagonal, live [V] the vertices that take part (the others keep u, with r = p = 0)."""
    C = r.shape[1]
    act = live[:, None]
    z = r * dinv[:, None]
    bb = [canon_sum(b[:, c] * b[:, c]) for c in range(C)]
    rz = [canon_sum(r[:, c] * z[:, c]) for c in range(C)]
    rr = [canon_sum(r[:, c] * r[:, c]) for c in range(C)]
    active = [rr[c] > tol * tol * bb[c] for c in range(C)]
    alpha, beta = [0.] * C, [0.] * C
    p = np.zeros(r.shape)                                   # (lap_align.hip begins with p = z: z + 0 * z, the same value)
    iters = 0
    frozen_at = [None if a else 0 for a in active]
    done = not any(active) or max_iter <= 0
    with np.errstate(all="ignore"):
        while not done:
            p = np.where(act, z + np.array(beta)[None, :] * p, 0.)
            q = apply(p)
            for c in range(C):
                pq = canon_sum(p[:, c] * q[:, c])
                al = np.float64(rz[c]) / np.float64(pq)
                ok = active[c] and pq > 0 and np.isfinite(al)
                alpha[c] = float(al) if ok else 0.
                active[c] = bool(ok)
            iters += 1
            u = np.where(act, u + np.array(alpha)[None, :] * p, u)
            r = np.where(act, r - np.array(alpha)[None, :] * q, 0.)
            z = r * dinv[:, None]
            for c in range(C):
                if active[c]:
                    nrz, nrr = canon_sum(r[:, c] * z[:, c]), canon_sum(r[:, c] * r[:, c])
                    be = np.float64(nrz) / np.float64(rz[c]) if rz[c] != 0. else np.float64(0.)
                    beta[c], rz[c], rr[c] = float(be), nrz, nrr
                    if not (nrr > tol * tol * bb[c]) or not np.isfinite(be):
                        active[c] = False
                if not active[c]:
                    beta[c] = 0.
                    frozen_at[c] = iters if frozen_at[c] is None else frozen_at[c]
            done = not any(active) or iters >= max_iter
    frozen_at = [iters if k is None else k for k in frozen_at]
    res = [float(np.sqrt(rr[c] / bb[c])) if bb[c] > 0 else (float(np.sqrt(rr[c])) if rr[c] > 0 else 0.) for c in range(C)]
    return u, iters, res, frozen_at


# ---------------------------------------------------------------------------------------------------------- lap_align
class LapSystem:
    """recmv_lap_align_solve's operator over the symmetric neighbour CSR, as gathers in row order: t = L p with
    (L x)_i = (1 / deg_i) sum_j x_j - x_i, q = L^T t + cw p with (L^T y)_j = sum_i y_i / deg_i - y_j, and the diagonal
    1 + sum_i 1 / deg_i^2 + cw_j."""

    def __init__(self, off, nbr, cw):
        V = off.shape[0] - 1
        assert V <= 2048 * BLOCK, "beyond stream_grid's cap a thread holds several vertices: another summation order"
        pos, self.valid = padded(off, nbr.shape[0])
        self.j = np.where(self.valid, np.asarray(nbr, np.int64)[pos], 0) if nbr.size else np.zeros(pos.shape, np.int64)
        deg = np.diff(np.asarray(off, np.int64))
        self.invdeg = np.where(deg > 0, 1. / np.maximum(deg, 1), 0.)
        self.w = np.where(self.valid, self.invdeg[self.j], 0.)
        self.cw = np.asarray(cw, np.float64)
        d = np.ones(V)
        for k in range(self.w.shape[1]):
            d = d + self.w[:, k] * self.w[:, k]
        self.dinv = 1. / (d + self.cw)

    def L(self, x):
        return rowsum(np.where(self.valid[:, :, None], x[self.j], 0.)) * self.invdeg[:, None] - x

    def Lt(self, y):
        return rowsum(np.where(self.valid[:, :, None], y[self.j] * self.w[:, :, None], 0.)) - y

    def apply(self, p):
        return self.Lt(self.L(p)) + self.cw[:, None] * p


def lap_solve(off, nbr, v, cw, cwt, tol, max_iter):
    """(u [V,3] float32, iterations, residuals [3], the iteration at which each column froze) of recmv_lap_align_solve: from
    u = v widened, first residual cwt - cw v, |rhs|^2 from L^T (L v) + cwt; u rounded to float32 once."""
    v32 = np.asarray(v, np.float32)
    u = v32.astype(np.float64)
    cwt = np.asarray(cwt, np.float64)
    if u.shape[0] == 0:
        return v32.copy(), 0, [0., 0., 0.], [0, 0, 0]
    S = LapSystem(off, nbr, cw)
    b = S.Lt(S.L(u)) + cwt
    r = cwt - S.cw[:, None] * u
    u, iters, res, frozen_at = cg(S.apply, S.dinv, r, b, u, np.ones(u.shape[0], bool), tol, max_iter)
    return u.astype(np.float32), iters, res, frozen_at
