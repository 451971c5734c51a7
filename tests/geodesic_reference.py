"""The numpy restatement of the geodesic distance field of include/recmv_hip.h (csrc/geodesic.hip): Jacobi sweeps of the
first-order Hopf-Lax update, float64 on float32 coordinates, in the header's order of operations.  Every sweep recomputes every
candidate of every usable corner slot (no "changed" bookkeeping), vectorised over the slots.  Also an edge-graph Dijkstra, the
upper bound of the tests, and the helpers' restatements.
"""
import heapq

import numpy as np

INF = np.inf


def usable_faces(verts, faces):
    """Bool [F]: three distinct indices in [0, V) and nine finite coordinates."""
    V = verts.shape[0]
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])
    fin = np.isfinite(np.asarray(verts, np.float32)).all(1)
    ok[ok] &= fin[f[ok]].all(1)
    return ok


def _length3(x):
    return np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])


def _dot3(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


class Slots:
    """The corner slots (v, a, b) of the usable faces — a the next corner of the face, b the one after — and what U needs of
    their geometry, each a fixed function of the coordinates in the header's order."""

    def __init__(self, verts, faces):
        verts = np.asarray(verts, np.float32)
        f = np.asarray(faces, np.int64).reshape(-1, 3)[usable_faces(verts, faces)]
        self.V = verts.shape[0]
        self.v = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
        self.a = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
        self.b = np.concatenate([f[:, 2], f[:, 0], f[:, 1]])
        p = verts.astype(np.float64)
        pv, pa, pb = p[self.v], p[self.a], p[self.b]
        with np.errstate(all="ignore"):
            w, u, e = pv - pa, pv - pb, pb - pa
            self.la, self.lb = _length3(w), _length3(u)
            self.L2 = _dot3(e, e)
            self.L = np.sqrt(self.L2)
            n = np.stack([w[:, 1] * e[:, 2] - w[:, 2] * e[:, 1], w[:, 2] * e[:, 0] - w[:, 0] * e[:, 2],
                          w[:, 0] * e[:, 1] - w[:, 1] * e[:, 0]], 1)
            self.h = _length3(n) / self.L
            self.t0 = _dot3(w, e) / self.L2

    def candidates(self, D):
        """U of every slot from the field D [V]."""
        Da, Db = D[self.a], D[self.b]
        with np.errstate(all="ignore"):
            ca, cb = Da + self.la, Db + self.lb
            U = np.where(cb < ca, cb, ca)
            delta = Db - Da
            ok = (Da < INF) & (Db < INF) & (self.L > 0.) & (np.abs(delta) < self.L) & (self.h > 0.)
            ts = self.t0 - (delta * self.h) / (self.L * np.sqrt(self.L2 - delta * delta))
            ok &= (ts > 0.) & (ts < 1.)
            r = ts - self.t0
            ci = (Da + ts * delta) + np.sqrt(self.h * self.h + self.L2 * (r * r))
            take = ok & (ci < U)
        return np.where(take, ci, U)

    def sweep(self, D):
        out = D.copy()
        np.minimum.at(out, self.v, self.candidates(D))
        return out


def initial(V, sources, values=None):
    D = np.full(V, INF)
    src = np.asarray(sources, np.int64).reshape(-1)
    val = np.zeros(src.shape[0]) if values is None else np.asarray(values, np.float64).reshape(-1)
    np.minimum.at(D, src, val)
    return D


def distance(verts, faces, sources, values=None, max_sweeps=None, slots=None):
    """(D [V] float64, K): D^K for the least K with D^{K+1} = D^K.  ValueError when K would pass max_sweeps (V + 1)."""
    slots = slots or Slots(verts, faces)
    V = slots.V
    D = initial(V, sources, values)
    cap = V + 1 if max_sweeps is None else max_sweeps
    K = 0
    while True:
        nxt = slots.sweep(D)
        if np.array_equal(nxt, D):
            return D, K
        if K + 1 > cap:
            raise ValueError("not converged within %d sweeps" % cap)
        D, K = nxt, K + 1


def dijkstra(verts, faces, sources, values=None):
    """Shortest paths over the edges of the usable faces, float64."""
    verts = np.asarray(verts, np.float32).astype(np.float64)
    V = verts.shape[0]
    f = np.asarray(faces, np.int64).reshape(-1, 3)[usable_faces(verts, faces)]
    nbr = [set() for _ in range(V)]
    for a, b, c in f.tolist():
        nbr[a] |= {b, c}
        nbr[b] |= {a, c}
        nbr[c] |= {a, b}
    D = initial(V, sources, values)
    heap = [(d, i) for i, d in enumerate(D.tolist()) if d < INF]
    heapq.heapify(heap)
    while heap:
        d, i = heapq.heappop(heap)
        if d > D[i]:
            continue
        for j in nbr[i]:
            c = d + float(np.sqrt(((verts[i] - verts[j]) ** 2).sum()))
            if c < D[j]:
                D[j] = c
                heapq.heappush(heap, (c, j))
    return D


def nearest_source(fields):
    """(min over the fields [V], label [V]): the lowest field index among equal values, -1 where every field is inf."""
    fields = np.asarray(fields, np.float64)
    best = np.full(fields.shape[1], INF)
    label = np.full(fields.shape[1], -1, np.int64)
    for b in range(fields.shape[0]):
        take = fields[b] < best
        best[take] = fields[b][take]
        label[take] = b
    return best, label


def farthest_points(verts, faces, k, first=0):
    """(ids, running minimum): each new point the argmax of the running minimum over its finite entries, lowest id on ties."""
    slots = Slots(verts, faces)
    ids, run = [], np.full(slots.V, INF)
    nxt = int(first)
    while len(ids) < k:
        ids.append(nxt)
        run = np.minimum(run, distance(verts, faces, [nxt], slots=slots)[0])
        fin = np.where(np.isfinite(run), run, -INF)
        if not (fin.max() > 0.):
            break
        nxt = int(np.argmax(fin))                          # numpy's argmax returns the first of equal maxima
    return ids, run
