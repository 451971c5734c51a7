"""Float64 numpy restatement of csrc/tri_tri.h and csrc/mesh_intersect.hip: which faces of two meshes cross.

Definition.  orient(a, b, c, d) = det[b - a; c - a; d - a], and exactly 0 when two of the four points are
the same position.  Edge pq pierces triangle abc iff orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs and
orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) strictly the same sign.  Two triangles cross iff one of the six
edge-against-triangle tests holds, none of the determinants is NaN, and neither triangle has all three corners of the other
exactly in its plane (coplanar, or a plane of a triangle with a repeated corner).  Pairs are taken over the faces whose closed
axis-aligned boxes meet; a face with an index outside its mesh crosses nothing.

Besides the crossing pairs, every tested pair gets its MARGIN: the smallest |det| / L^3 among the determinants that decided
it — the six plane sides, and the three determinants of condition (2) of every edge that passed condition (1) — L the largest
coordinate difference among the six points.  Determinants that are 0 because two positions coincide are left out: they are
0 in every arithmetic.  A float32 evaluation whose determinants err by less than the margin takes every decision alike.
"""
import numpy as np


def _same(a, b):
    return (a == b).all(-1)


def orient(a, b, c, d):
    """(det [N], structural [N] bool) for points [N,3] float64."""
    det = np.einsum('ij,ij->i', b - a, np.cross(c - a, d - a))
    structural = _same(a, b) | _same(a, c) | _same(a, d) | _same(b, c) | _same(b, d) | _same(c, d)
    return np.where(structural, 0., det), structural


def _fold(margin, det, structural, active):
    """margin <- min(margin, |det|) where the determinant counts."""
    return np.where(active & ~structural, np.minimum(margin, np.abs(det)), margin)


def _half(T, E, margin):
    """The three edges of E [N,3,3] against the triangles T: (hit, margin, plane sides [3][N])."""
    n = T.shape[0]
    yes = np.ones(n, bool)
    side = []
    for k in range(3):
        d, st = orient(T[:, 0], T[:, 1], T[:, 2], E[:, k])
        margin = _fold(margin, d, st, yes)
        side.append(d)
    hit = np.zeros(n, bool)
    for p, q in ((0, 1), (1, 2), (2, 0)):
        c1 = ((side[p] > 0) & (side[q] < 0)) | ((side[p] < 0) & (side[q] > 0))
        pos, neg = c1.copy(), c1.copy()
        for x, y in ((0, 1), (1, 2), (2, 0)):
            d, st = orient(E[:, p], E[:, q], T[:, x], T[:, y])
            margin = _fold(margin, d, st, c1)
            pos &= d > 0
            neg &= d < 0
        hit |= pos | neg
    return hit, margin, side


def tri_tri(A, B):
    """A, B [N,3,3] float64 (N pairs of triangles): (cross [N] bool, margin [N] = smallest deciding |det| / L^3; inf for a
    pair with a non-finite coordinate, which is no crossing in any arithmetic)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    pts = np.concatenate([A, B], 1)
    finite = np.isfinite(pts).all((1, 2))
    A, B = np.where(finite[:, None, None], A, 0.), np.where(finite[:, None, None], B, 0.)
    pts = np.concatenate([A, B], 1)
    L = (pts.max(1) - pts.min(1)).max(1)
    margin = np.full(A.shape[0], np.inf)
    hit_a, margin, side_a = _half(B, A, margin)                      # A's edges through B
    hit_b, margin, side_b = _half(A, B, margin)
    flat = np.all([s == 0 for s in side_a], 0) | np.all([s == 0 for s in side_b], 0)
    cross = (hit_a | hit_b) & ~flat & finite
    with np.errstate(divide='ignore', invalid='ignore'):
        margin = np.where(finite & (L > 0), margin / L ** 3, np.where(finite, 0., np.inf))
    return cross, margin


def _valid(f, V):
    return ((f >= 0) & (f < V)).all(1)


def candidates(av, af, bv, bf, self_mode=False):
    """The pairs (i, j) [N,2] whose closed boxes meet, of faces with valid indices; self_mode: i < j and no shared index."""
    av, bv = np.asarray(av, np.float64), np.asarray(bv, np.float64)
    af, bf = np.asarray(af), np.asarray(bf)
    ia, ib = np.nonzero(_valid(af, av.shape[0]))[0], np.nonzero(_valid(bf, bv.shape[0]))[0]
    ta, tb = av[af[ia]], bv[bf[ib]]
    with np.errstate(invalid='ignore'):
        alo, ahi, blo, bhi = np.nanmin(ta, 1), np.nanmax(ta, 1), np.nanmin(tb, 1), np.nanmax(tb, 1)
        meet = ((alo[:, None] <= bhi[None]) & (blo[None] <= ahi[:, None])).all(-1)
    i, j = np.nonzero(meet)
    i, j = ia[i], ib[j]
    if self_mode:
        keep = i < j
        shared = (af[i][:, :, None] == bf[j][:, None, :]).any((1, 2))
        keep &= ~shared
        i, j = i[keep], j[keep]
    return np.stack([i, j], 1)


def intersections(av, af, bv, bf, self_mode=False):
    """(crossing pairs [K,2] sorted by (i, j), tested pairs [N,2], cross [N] bool, margin [N])."""
    cand = candidates(av, af, bv, bf, self_mode)
    av, bv = np.asarray(av, np.float64), np.asarray(bv, np.float64)
    cross, margin = tri_tri(av[np.asarray(af)[cand[:, 0]]], bv[np.asarray(bf)[cand[:, 1]]])
    pairs = cand[cross]
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))], cand, cross, margin
