"""Float64 numpy restatement of csrc/seg_tri.h and csrc/segment_mesh.hip: which faces a segment hits, and where.

Definition.  orient(a, b, c, d) = det[b - a; c - a; d - a], exactly 0 when two of the four points are the
same position (mesh_intersect_reference.orient).  The segment pq hits the triangle abc iff
  (1) sp = orient(a,b,c,p) and sq = orient(a,b,c,q) have strictly opposite signs, and
  (2) e0 = orient(p,q,a,b), e1 = orient(p,q,b,c), e2 = orient(p,q,c,a) have strictly the same sign,
and nothing is NaN or infinite; t = sp / (sp - sq).  Pairs are taken over the faces with valid indices whose closed box meets
the closed box of the segment's endpoints (a hit point lies in both, so no other pair hits in exact arithmetic, and the f32
kernels refuse the others by the same exact comparisons).

MARGIN of a pair: the smallest |det| / L^3 among the determinants that decide it, L the largest coordinate difference among
the five points.  A float32 evaluation whose determinants err by less than the margin decides alike:
  * sp and sq of strictly equal sign: no hit whatever (2) says — unless two of e0..e2 have opposite signs, which decides it
    as well: the margin is the larger of min(|sp|, |sq|) and the best such pair's min(|ei|, |ej|);
  * otherwise, two of e0..e2 of opposite signs: no hit whatever (1) says; the margin is the best such pair's min(|ei|, |ej|);
  * otherwise (1) and (2) decide together: min(|sp|, |sq|, |e0|, |e1|, |e2|).
Determinants that are 0 because two positions coincide count as 0 (they are 0 in every arithmetic, and decide "no hit"
firmly: such a pair gets margin inf).

T_TOL of a pair: with |error of sp|, |error of sq| <= B = 20 eps32 L^3 (csrc/tri_tri.h) and D = sp - sq, to first order
t' - t = (e_p (1 - t) + e_q t) / D, at most B / |D|, plus the roundings of the difference and the quotient, t eps32 together.
The tolerance is twice that: 2 B / |D| + 2 eps32.
"""
import numpy as np

from mesh_intersect_reference import orient

EPS32 = 2.0 ** -23
BOUND_C = 20.0


def _mixed(e):
    """Best pair of opposite signs among e [3][N]: max over pairs of min(|ei|, |ej|), 0 where no pair is opposite."""
    best = np.zeros_like(e[0])
    for i, j in ((0, 1), (1, 2), (2, 0)):
        opp = ((e[i] > 0) & (e[j] < 0)) | ((e[i] < 0) & (e[j] > 0))
        best = np.where(opp, np.maximum(best, np.minimum(np.abs(e[i]), np.abs(e[j]))), best)
    return best


def seg_tri(P, Q, T):
    """P, Q [N,3], T [N,3,3] float64: (hit [N] bool, t [N] (NaN: no hit), margin [N] in units of L^3, t_tol [N], t_low [N]).
    t_low: the smallest parameter an f32 evaluation could report for the pair if it called it a hit — the plane crossing
    sp / (sp - sq) less its tolerance where condition (1) holds firmly (both |sp|, |sq| above the bound), else 0."""
    P, Q, T = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(T, np.float64)
    pts = np.concatenate([P[:, None], Q[:, None], T], 1)
    finite = np.isfinite(pts).all((1, 2))
    pts = np.where(finite[:, None, None], pts, 0.)
    P, Q, T = pts[:, 0], pts[:, 1], pts[:, 2:]
    L = (pts.max(1) - pts.min(1)).max(1)
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    sp, st_p = orient(a, b, c, P)
    sq, st_q = orient(a, b, c, Q)
    e, st_e = zip(*(orient(P, Q, x, y) for x, y in ((a, b), (b, c), (c, a))))
    opposite = ((sp > 0) & (sq < 0)) | ((sp < 0) & (sq > 0))
    same_pq = ((sp > 0) & (sq > 0)) | ((sp < 0) & (sq < 0))
    all_same = ((e[0] > 0) & (e[1] > 0) & (e[2] > 0)) | ((e[0] < 0) & (e[1] < 0) & (e[2] < 0))
    hit = opposite & all_same & finite
    mixed = _mixed(e)
    m_pq = np.minimum(np.abs(sp), np.abs(sq))
    m_all = np.minimum(m_pq, np.minimum(np.abs(e[0]), np.minimum(np.abs(e[1]), np.abs(e[2]))))
    margin = np.where(same_pq, np.maximum(m_pq, mixed), np.where(mixed > 0, mixed, m_all))
    structural = (st_p | st_q | st_e[0] | st_e[1] | st_e[2]) & ~hit                # an exact 0 by coincidence: firmly no hit
    with np.errstate(divide='ignore', invalid='ignore'):
        margin = np.where(L > 0, margin / L ** 3, 0.)
        margin = np.where(structural | ~finite, np.inf, margin)
        D = sp - sq
        t = np.where(hit, sp / D, np.nan)
        tol = 2. * BOUND_C * EPS32 * L ** 3 / np.abs(D) + 2. * EPS32
        t_tol = np.where(hit, tol, np.nan)
        firm = opposite & (m_pq > BOUND_C * EPS32 * L ** 3)
        t_low = np.where(firm, sp / D - tol, 0.)
    return hit, t, margin, t_tol, t_low


def candidates(p, q, v, f, chunk=256):
    """(segment, face) [N,2] of the faces with valid indices whose closed box meets the segment's."""
    p, q, v, f = np.asarray(p, np.float64), np.asarray(q, np.float64), np.asarray(v, np.float64), np.asarray(f)
    ok = np.nonzero(((f >= 0) & (f < v.shape[0])).all(1))[0]
    tri = v[f[ok]]
    with np.errstate(invalid='ignore'):
        flo, fhi = np.nanmin(tri, 1), np.nanmax(tri, 1)
        slo, shi = np.fmin(p, q), np.fmax(p, q)
    out = []
    for s0 in range(0, p.shape[0], chunk):
        with np.errstate(invalid='ignore'):
            meet = ((slo[s0:s0 + chunk, None] <= fhi[None]) & (flo[None] <= shi[s0:s0 + chunk, None])).all(-1)
        i, j = np.nonzero(meet)
        out.append(np.stack([i + s0, ok[j]], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def segment_hits(p, q, v, f):
    """The reference's answer for segments p, q [S,3] against the mesh v, f.  A dict:
    cand [N,2] the tested pairs, hit / t / margin / t_tol [N] per pair; per segment count [S], face [S] (-1: none), t [S],
    t_tol [S] (of the first hit), pairs_decided [S] (every tested pair of the segment has margin > 20 eps32: its hit set and
    count are decided) and first_decided [S]: the first hit's own pair is decided, no other hit's t lies within the sum of the
    two tolerances of the first hit's t, and no undecided pair of the segment could be reported in front of it (its t_low
    lies beyond the first hit's t plus tolerance) — the first face is what any evaluation within the bound finds.  A segment
    that hits nothing has first_decided = pairs_decided."""
    p, q, v, f = np.asarray(p, np.float64), np.asarray(q, np.float64), np.asarray(v, np.float64), np.asarray(f)
    S = p.shape[0]
    cand = candidates(p, q, v, f)
    hit, t, margin, t_tol, t_low = seg_tri(p[cand[:, 0]], q[cand[:, 0]], v[f[cand[:, 1]]])
    decided = margin > BOUND_C * EPS32
    count = np.bincount(cand[hit, 0], minlength=S)
    pairs_decided = np.ones(S, bool)
    np.logical_and.at(pairs_decided, cand[:, 0], decided)
    face = np.full(S, -1, np.int64)
    tf = np.full(S, np.nan)
    tol = np.full(S, np.nan)
    first_decided = pairs_decided.copy()
    und_low = np.full(S, np.inf)                                                   # the earliest an undecided pair could show up
    np.minimum.at(und_low, cand[~decided, 0], t_low[~decided])
    hs, hf, ht, htol, hdec = cand[hit, 0], cand[hit, 1], t[hit], t_tol[hit], decided[hit]
    order = np.lexsort((hf, ht, hs))                                               # by segment, then t, then face id
    hs, hf, ht, htol, hdec = hs[order], hf[order], ht[order], htol[order], hdec[order]
    start = np.nonzero(np.r_[True, hs[1:] != hs[:-1]])[0] if len(hs) else np.zeros(0, np.int64)
    face[hs[start]], tf[hs[start]], tol[hs[start]] = hf[start], ht[start], htol[start]
    second = start + 1                                                             # the runner-up of the same segment
    has = (second < len(hs)) & (hs[np.minimum(second, len(hs) - 1)] == hs[start]) if len(hs) else np.zeros(0, bool)
    close = np.zeros(len(start), bool)
    close[has] = ht[second[has]] - ht[start[has]] <= htol[second[has]] + htol[start[has]]
    first_decided[hs[start]] = hdec[start] & ~close & (und_low[hs[start]] > ht[start] + htol[start])
    return {'cand': cand, 'hit': hit, 't_pair': t, 'margin': margin, 't_tol_pair': t_tol, 'count': count, 'face': face, 't': tf,
            't_tol': tol, 'pairs_decided': pairs_decided, 'first_decided': first_decided}


def points_inside(points, v, f, directions, reach):
    """Majority of the three crossing parities, float64: (inside [P] bool, decided [P] bool).  A ray is decided when every
    tested pair of it is; a point when two decided rays give the same parity — the majority then stands whatever the third
    ray is counted as."""
    points = np.asarray(points, np.float64)
    P = points.shape[0]
    par = np.zeros((3, P), np.int64)
    dec = np.zeros((3, P), bool)
    for k, d in enumerate(directions):
        r = segment_hits(points, points + np.asarray(reach, np.float64).reshape(-1, 1) * np.asarray(d, np.float64)[None], v, f)
        par[k] = r['count'] & 1
        dec[k] = r['pairs_decided']
    decided = ((dec & (par == 1)).sum(0) >= 2) | ((dec & (par == 0)).sum(0) >= 2)
    return par.sum(0) >= 2, decided
