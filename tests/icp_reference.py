"""Numpy restatement of recmv.align in float64 / np.longdouble, and the fixtures its tests share.

  potato, open_copy, applied, transform_points, maxres   the shapes and the motion of the tests
  border_flags        recmv.align.border_flags from a dictionary of edges
  sums                recmv_icp_accumulate's 56 sums over the pairs a mask accepts, in longdouble, and per entry the same sum
                      with every factor replaced by its magnitude (every difference u - w by |u| + |w|): the M of the bound
  solve_point, solve_plane   the two solvers, written from the definitions (Umeyama 1991; Gauss-Newton on the plane distance)
  icp                 the iteration on mesh_metrics_reference.nearest (float64 throughout)

Used by tests/test_icp_cpu.py (pinned there on hand cases) and as the judge of tests/test_gpu_icp.py.
"""
import math

import numpy as np

import collide_reference as CR
import mesh_metrics_reference as MR

LD = np.longdouble
N_SUMS = 56
AXIS = np.array([1., 2., 3.]) / math.sqrt(14.)
ANGLE = math.radians(12.)
SHIFT = np.array([0.04, -0.03, 0.02])
SCALE = 1.08


def potato(level):
    """test_gpu_animation._irregular_body(level) with the axes scaled by (1.0, 0.7, 0.45) and 0.25 y^2 / 0.35 added to x,
    rounded to float32: no symmetry, box diagonal about 1.27.  (verts float32 [V,3], faces int64 [F,3]) as numpy arrays."""
    from test_gpu_animation import _irregular_body
    v, f = _irregular_body(level)
    v = v.double().numpy() * np.array([1.0, 0.7, 0.45])
    v[:, 0] += 0.25 * v[:, 1] ** 2 / 0.35
    return v.astype(np.float32), f.numpy().astype(np.int64)


def open_copy(verts, faces, cut=0.2):
    """The mesh without the faces whose centroid has x >= cut (same vertices): an open surface with a border."""
    cen = np.asarray(verts, np.float64)[faces].mean(1)
    return faces[cen[:, 0] < cut]


def diagonal(verts):
    v = np.asarray(verts, np.float64)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0., -a[2], a[1]], [a[2], 0., -a[0]], [-a[1], a[0], 0.]])
    return np.eye(3) + math.sin(angle) * K + (1. - math.cos(angle)) * (K @ K)


def applied(similarity):
    """(s, R, t) of the tests' motion: 12 degrees about (1, 2, 3) / sqrt 14, t = (0.04, -0.03, 0.02), s = 1.08 or 1."""
    return (SCALE if similarity else 1.), rotation(AXIS, ANGLE), SHIFT.copy()


def transform_points(T, x):
    s, R, t = T
    return s * (np.asarray(x, np.float64) @ np.asarray(R, np.float64).T) + np.asarray(t, np.float64)


def maxres(T_est, T_applied, verts):
    """max over the vertices |T_est(T_applied(v)) - v|."""
    v = np.asarray(verts, np.float64)
    return float(np.linalg.norm(transform_points(T_est, transform_points(T_applied, v)) - v, axis=1).max())


def border_flags(faces, n_verts):
    """uint8 [F]: bit 0 / 1 / 2 edge ab / ac / bc used by one face only; bit 3 / 4 / 5 vertex a / b / c an end of such an edge."""
    use = {}
    for f in faces:
        for i, j in ((0, 1), (0, 2), (1, 2)):
            e = (min(f[i], f[j]), max(f[i], f[j]))
            use[e] = use.get(e, 0) + 1
    on = set()
    for (i, j), n in use.items():
        if n == 1:
            on.update((i, j))
    out = np.zeros(len(faces), np.uint8)
    for k, f in enumerate(faces):
        for bit, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
            if use[(min(f[i], f[j]), max(f[i], f[j]))] == 1:
                out[k] |= 1 << bit
        for bit in range(3):
            if f[bit] in on:
                out[k] |= 8 << bit
    return out


def sums(x, q, face, accept, verts, faces, centre, plane):
    """(S [56], M [56]) in longdouble over the pairs with accept[i]: the table of include/recmv_hip.h, and the magnitudes."""
    acc = np.asarray(accept, bool)
    c = np.asarray(centre, np.float64).astype(LD)
    u = np.asarray(x)[acc].astype(LD) - c
    w = np.asarray(q)[acc].astype(LD) - c
    au, aw = np.abs(u), np.abs(w)
    e, ae = u - w, au + aw
    n = int(acc.sum())
    S, M = np.zeros(N_SUMS, LD), np.zeros(N_SUMS, LD)
    S[0] = M[0] = n
    S[1:4], M[1:4] = u.sum(0), au.sum(0)
    S[4:7], M[4:7] = w.sum(0), aw.sum(0)
    S[7:16], M[7:16] = (u.T @ w).reshape(-1), (au.T @ aw).reshape(-1)
    S[16], S[17], S[18] = (u * u).sum(), (w * w).sum(), (e * e).sum()
    M[16], M[17], M[18] = S[16], S[17], (ae * ae).sum()
    if plane and n:
        v = np.asarray(verts).astype(LD)
        f = np.asarray(faces)[np.asarray(face)[acc]]
        m = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        m = m / np.sqrt((m * m).sum(1, keepdims=True))
        am = np.abs(m)
        J = np.concatenate([np.cross(u, m), m, (u * m).sum(1, keepdims=True)], 1)
        # |u x m| and |u . m| term by term: every product of magnitudes
        aJ = np.concatenate([np.stack([au[:, 1] * am[:, 2] + au[:, 2] * am[:, 1], au[:, 2] * am[:, 0] + au[:, 0] * am[:, 2],
                                       au[:, 0] * am[:, 1] + au[:, 1] * am[:, 0]], 1), am, (au * am).sum(1, keepdims=True)], 1)
        r, ar = (e * m).sum(1), (ae * am).sum(1)
        iu = np.triu_indices(7)
        S[19:47], M[19:47] = (J.T @ J)[iu], (aJ.T @ aJ)[iu]
        S[47:54], M[47:54] = J.T @ r, aJ.T @ ar
        S[54], M[54] = (r * r).sum(), (ar * ar).sum()
    return S, M


def pair_sums(u, w, normals=None):
    """The sums about the origin of given pairs (u_i, w_i) with given unit normals, all accepted, as float64."""
    u, w = np.asarray(u).astype(LD), np.asarray(w).astype(LD)
    S = np.zeros(N_SUMS, LD)
    e = u - w
    S[0] = len(u)
    S[1:4], S[4:7], S[7:16] = u.sum(0), w.sum(0), (u.T @ w).reshape(-1)
    S[16], S[17], S[18] = (u * u).sum(), (w * w).sum(), (e * e).sum()
    if normals is not None:
        m = np.asarray(normals).astype(LD)
        J = np.concatenate([np.cross(u, m), m, (u * m).sum(1, keepdims=True)], 1)
        r = (e * m).sum(1)
        S[19:47], S[47:54], S[54] = (J.T @ J)[np.triu_indices(7)], J.T @ r, (r * r).sum()
    return S.astype(np.float64)


def solve_point(S, scale):
    """Umeyama (1991), eq. 40-42, for u -> w: covariance Sigma = mean (w - mw)(u - mu)^T = U D V^T, R = U diag(1, 1,
    det U det V) V^T, c = tr(D diag) / var u, t = mw - c R mu."""
    S = np.asarray(S, np.float64)
    n = S[0]
    if n < 3:
        raise ValueError("fewer than 3 pairs")
    mu, mw = S[1:4] / n, S[4:7] / n
    Sigma = (S[7:16].reshape(3, 3) / n - np.outer(mu, mw)).T                       # [w, u]
    U, D, Vt = np.linalg.svd(Sigma)
    if D[1] <= 1e-10 * D[0]:
        raise ValueError("rank < 2")
    sgn = np.array([1., 1., np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ np.diag(sgn) @ Vt
    c = float((D * sgn).sum() / (S[16] / n - mu @ mu)) if scale else 1.
    return c, R, mw - c * (R @ mu)


def solve_plane(S, scale):
    """delta = -A^-1 b of the 6 or 7 unknowns (omega, tau[, sigma]); (1 + sigma, exp([omega]x), tau)."""
    S = np.asarray(S, np.float64)
    k = 7 if scale else 6
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = S[19:47]
    A = (A + A.T - np.diag(np.diag(A)))[:k, :k]
    d = np.sqrt(np.diag(A))
    if not np.all(d > 0) or np.linalg.eigvalsh(A / np.outer(d, d)).min() <= 1e-10:
        raise ValueError("not positive definite")
    delta = -np.linalg.solve(A, S[47:47 + k])
    th = np.linalg.norm(delta[:3])
    R = rotation(delta[:3], th) if th > 0 else np.eye(3)
    return (1. + delta[6] if scale else 1.), R, delta[3:6]


def icp(points, dst_v, dst_f, mode='rigid', metric='plane', iters=10, reject_border=True):
    """recmv.align.icp in float64 (no trimming, no tolerance: `iters` steps and a last search): a dict with `T` = (s, R, t),
    `rms` (one per search) and `pairs` (accepted in the last search)."""
    p = np.asarray(points, np.float64)
    v, f = np.asarray(dst_v, np.float64), np.asarray(dst_f, np.int64)
    centre = 0.5 * (v.min(0) + v.max(0))
    flags = border_flags(f, len(v)) if reject_border else None
    s, R, t = 1., np.eye(3), np.zeros(3)
    history, pairs = [], 0
    for it in range(iters + 1):
        x = transform_points((s, R, t), p)
        face, _ = MR.nearest(x, v, f)
        tri = v[f[face]]
        _, w = CR.closest_on_triangle(x, tri[:, 0], tri[:, 1], tri[:, 2])
        q = (w[:, :, None] * tri).sum(1)
        accept = np.ones(len(p), bool)
        if flags is not None:
            zero = w == 0.
            # one weight zero: the edge opposite that corner (c: ab, b: ac, a: bc); two: the corner that is left
            for corner, bit in ((2, 0), (1, 1), (0, 2)):
                accept &= ~((zero.sum(1) == 1) & zero[:, corner] & ((flags[face] >> bit) & 1).astype(bool))
            for corner in range(3):
                accept &= ~((zero.sum(1) == 2) & ~zero[:, corner] & ((flags[face] >> (3 + corner)) & 1).astype(bool))
        S, _ = sums(x, q, face, accept, v, f, centre, metric == 'plane')
        S = S.astype(np.float64)
        pairs = int(S[0])
        history.append(math.sqrt(S[54 if metric == 'plane' else 18] / pairs))
        if it == iters:
            break
        ds, dR, dt = (solve_plane if metric == 'plane' else solve_point)(S, mode == 'similarity')
        s, R, t = ds * s, dR @ R, centre + ds * (dR @ (t - centre)) + dt
    return {'T': (s, R, t), 'rms': history, 'pairs': pairs}
