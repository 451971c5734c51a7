"""Rigid and similarity alignment of a mesh to a mesh by ICP (csrc/icp.hip) — what eval_fl.py --align runs before the metrics.
The reference has the closed-form rigid fit on nearest neighbours (engineer/optimizer/icp_optimzier.py, `ICP_Optimizer`; its
port on this module's solver is recmv/engineer/optimizer/icp_optimzier.py); the iteration on the exact closest point of the
target SURFACE, the point-to-plane step, the similarity and the rejection rules are additions.

  border_flags   per face of an open mesh, which of its edges and vertices lie on the border
  icp_sums       recmv_icp_accumulate: the 56 float64 sums of one iteration from given correspondences
  solve_point    Umeyama's closed form from the sums (point-to-point)
  solve_plane    one Gauss-Newton step from the sums (point-to-plane)
  icp            the iteration: source mesh -> target mesh, 'rigid' or 'similarity'
  apply          the resulting transform on vertices

The transform is x' = s R x + t, kept in float64 on the host.  One iteration: x = s p R^T + t in float32 from the ORIGINAL
points p (rounding does not accumulate), the exact closest point q of every x on the target (metrics._nearest: the kernels of
the metrics, the same bits through the grid and by the brute force), the sums about the centre c of the target's box, one
read-back of 56 doubles, and a step x' = c + ds dR (x - c) + dt from one of the solvers.

A pair (x, q) takes part iff the closest point was found on a valid face, everything is finite, its squared distance is at
most the threshold (the `trim` quantile of the finite squared distances and / or max_dist^2), with `reject_border` the closest
point does not lie on a border edge or border vertex of the target (a sample beyond the border of an open garment surface has
its closest point ON the border and would pull the source across it), and for the plane metric the face has an area.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import metrics
from .connectivity import EdgeTable
from .mesh_args import check_mesh, check_points

N_SUMS = 56                     # RECMV_ICP_SUMS of include/recmv_hip.h
MODES = ('rigid', 'similarity')
METRICS = ('plane', 'point')
# A covariance's second singular value, or a pivot of the plane system scaled to a unit diagonal, at or below this share
# counts as zero: the pairs do not determine the motion (points on a line; one plane).  Exactly dependent data leave about
# 1e-16 there, data that determine the motion something of order 1e-3 .. 1.
RANK_TOL = 1e-10


def border_flags(faces, n_verts):
    """uint8 [F] for faces [F,3] int64 (CPU or CUDA): bit 0 / 1 / 2 — the edge ab / ac / bc is used by exactly one face (a
    border edge); bit 3 / 4 / 5 — the vertex a / b / c is an end of some border edge (a border vertex, in every face that
    contains it).  A closed mesh gives zeros."""
    table = EdgeTable(faces, n_verts)
    edge = table.boundary_edge[table.face_to_edge[:, [2, 1, 0]]]                   # ab, ac, bc
    bits = torch.cat([edge, table.boundary_vertex[faces]], 1).to(torch.uint8)      # [F,6]
    weight = torch.tensor([1, 2, 4, 8, 16, 32], dtype=torch.uint8, device=faces.device)
    return (bits * weight).sum(1, dtype=torch.int32).to(torch.uint8)


def icp_sums(x, q, face, dist2, verts, faces, border=None, max_dist2=None, centre=(0., 0., 0.), plane=True):
    """recmv_icp_accumulate (include/recmv_hip.h has the acceptance rules and the layout): float64 [56] on the device from
    x [P,3] f32 and its closest points q [P,3] f32 / face [P] int64 / dist2 [P] f32 on the mesh verts [V,3] f32 / faces
    [F,3] int64 (CUDA tensors on one device).  `border`: border_flags of the mesh, uint8 [F] on the device; `max_dist2`: a
    number, or a float32 tensor of one element on the device (no read-back); `centre`: three host numbers."""
    verts, faces = check_mesh(verts, faces, allow_empty=False)
    dev = verts.device
    for t, name, dtype, shape in ((x, "x", torch.float32, (-1, 3)), (q, "q", torch.float32, (-1, 3)),
                                  (face, "face", torch.int64, (-1,)), (dist2, "dist2", torch.float32, (-1,))):
        L.require_cuda(t, name)
        if t.dtype != dtype or t.dim() != len(shape) or (len(shape) == 2 and t.shape[1] != 3):
            raise ValueError("%s must be %s of shape %s" % (name, dtype, "[P,3]" if len(shape) == 2 else "[P]"))
        if t.device != dev:
            raise ValueError("the pairs and the mesh must be on one device")
    P = x.shape[0]
    if q.shape[0] != P or face.shape[0] != P or dist2.shape[0] != P:
        raise ValueError("x, q, face and dist2 must have one length")
    if border is not None:
        L.require_cuda(border, "border")
        if border.dtype != torch.uint8 or border.shape != (faces.shape[0],) or border.device != dev:
            raise ValueError("border must be uint8 of shape [F] on the mesh's device")
        border = border.contiguous()
    if max_dist2 is not None:
        if isinstance(max_dist2, torch.Tensor):
            L.require_cuda(max_dist2, "max_dist2")
            if max_dist2.dtype != torch.float32 or max_dist2.numel() != 1 or max_dist2.device != dev:
                raise ValueError("max_dist2 must be a number or a float32 tensor of one element on the mesh's device")
            max_dist2 = max_dist2.reshape(1).contiguous()
        else:
            max_dist2 = torch.tensor([float(max_dist2)], dtype=torch.float32, device=dev)
    c = (C.c_double * 3)(*(float(v) for v in centre))
    x, q, face, dist2 = (t.contiguous() for t in (x, q, face, dist2))
    sums = L.scratch((N_SUMS,), torch.float64, dev)
    ws = L.workspace(nbytes := int(L.lib().recmv_icp_accumulate_workspace_bytes(P)), dev, "icp_accumulate_workspace_bytes")
    L.launch("icp_accumulate", dev, L.ptr(x), L.ptr(q), L.ptr(face), L.ptr(dist2), P, L.ptr(verts), verts.shape[0], L.ptr(faces),
             faces.shape[0], L.ptr(border), L.ptr(max_dist2), c, int(bool(plane)), L.ptr(sums), L.ptr(ws), nbytes)
    return sums


def _host(sums):
    s = np.asarray(sums.detach().cpu() if isinstance(sums, torch.Tensor) else sums, dtype=np.float64).reshape(-1)
    if s.shape[0] != N_SUMS:
        raise ValueError("sums must hold %d numbers (got %d)" % (N_SUMS, s.shape[0]))
    if not np.all(np.isfinite(s)):
        raise ValueError("the sums are not finite")
    return s


def solve_point(sums, scale):
    """(ds, dR, dt) in float64 on the host — the similarity (ds = 1 unless `scale`) u -> ds dR u + dt that minimises
    sum |ds dR u + dt - w|^2 over the accepted pairs, from entries 0 .. 17 of the sums: Umeyama's closed form, with the
    reference's reflection guard R = V diag(1, 1, det(V U^T)) U^T on the SVD U S V^T of the covariance sum (u - mean u)
    (w - mean w)^T.  u and w are relative to the centre the sums were formed about, and so is the step:
    x' = c + ds dR (x - c) + dt.  ValueError with fewer than 3 pairs or a covariance of rank < 2."""
    s = _host(sums)
    n = s[0]
    if n < 3:
        raise ValueError("solve_point: %d pairs, at least 3 needed" % int(n))
    mu, mw = s[1:4] / n, s[4:7] / n
    H = s[7:16].reshape(3, 3) / n - np.outer(mu, mw)                               # [a, b]: u_a w_b
    var_u = s[16] / n - mu @ mu
    U, S, Vt = np.linalg.svd(H)
    if not (S[0] > 0. and S[1] > RANK_TOL * S[0]) or not var_u > 0.:
        raise ValueError("solve_point: the pairs do not determine a rotation (covariance of rank < 2)")
    V = Vt.T
    d = np.linalg.det(V @ U.T)
    D = np.diag([1., 1., d])
    R = V @ D @ U.T
    ds = float((S * np.diag(D)).sum() / var_u) if scale else 1.
    return ds, R, mw - ds * (R @ mu)


def _rodrigues(w):
    """exp([w]x) for a rotation vector w [3]: orthonormal to rounding at every angle."""
    th = float(np.linalg.norm(w))
    K = np.array([[0., -w[2], w[1]], [w[2], 0., -w[0]], [-w[1], w[0], 0.]])
    if th < 1e-8:
        a, b = 1. - th * th / 6., 0.5 - th * th / 24.
    else:
        a, b = math.sin(th) / th, 2. * math.sin(0.5 * th) ** 2 / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def solve_plane(sums, scale):
    """(ds, dR, dt) in float64 on the host — one Gauss-Newton step of sum ((x' - q) . m)^2 over the accepted pairs with
    x' = c + (1 + sigma) exp([omega]x) (x - c) + tau linearised at the identity: the residual becomes r + J . delta with
    delta = (omega, tau, sigma) and the J, r of the sums, so A delta = -b with A = sum J J^T (entries 19 .. 46) and b =
    sum J r (47 .. 53); the 6x6 system without sigma unless `scale`.  Solved by Cholesky on the system scaled to a unit
    diagonal; dR = exp([omega]x) by Rodrigues' formula, ds = 1 + sigma, dt = tau.  ValueError when A is not positive
    definite (points on one plane, too few pairs)."""
    s = _host(sums)
    k = 7 if scale else 6
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = s[19:47]
    A = (A + np.triu(A, 1).T)[:k, :k]
    b = s[47:47 + k]
    diag = np.diag(A)
    if s[0] < 3 or not np.all(diag > 0.):
        raise ValueError("solve_plane: the normal matrix is not positive definite (%d pairs)" % int(s[0]))
    scl = 1. / np.sqrt(diag)
    try:
        Lc = np.linalg.cholesky(A * scl[:, None] * scl[None, :])
    except np.linalg.LinAlgError:
        raise ValueError("solve_plane: the normal matrix is not positive definite") from None
    if float(np.diag(Lc).min()) ** 2 <= RANK_TOL:
        raise ValueError("solve_plane: the pairs do not determine the motion (the normal matrix is singular to rounding)")
    y = np.linalg.solve(Lc, -b * scl)
    delta = np.linalg.solve(Lc.T, y) * scl
    return (1. + float(delta[6]) if scale else 1.), _rodrigues(delta[0:3]), delta[3:6].copy()


def _matrix(s, R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    return M


def _initial(init):
    """(s, R, t) float64 of `init`: None, a result of icp (or any dict with 'scale', 'R', 't'), or a 4x4 similarity matrix."""
    if init is None:
        return 1., np.eye(3), np.zeros(3)
    if isinstance(init, dict):
        s, R, t = float(init['scale']), np.array(init['R'], np.float64).reshape(3, 3), np.array(init['t'], np.float64).reshape(3)
    else:
        M = np.array(init, np.float64).reshape(4, 4)
        s = float(np.cbrt(np.linalg.det(M[:3, :3])))
        if not s > 0.:
            raise ValueError("icp: init is not a similarity (determinant %g)" % np.linalg.det(M[:3, :3]))
        R, t = M[:3, :3] / s, M[:3, 3].copy()
    if not (np.isfinite(s) and s > 0. and np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        raise ValueError("icp: init is not finite")
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0.:
        raise ValueError("icp: the rotation of init is not a rotation")
    return s, R, t


def _result(s, R, t, **more):
    out = {'scale': float(s), 'R': [[float(v) for v in row] for row in R], 't': [float(v) for v in t],
           'matrix': [[float(v) for v in row] for row in _matrix(s, R, t)]}
    out.update(more)
    return out


@torch.no_grad()
def icp(src_v, src_f, dst_v, dst_f, mode='rigid', metric='plane', samples=20000, points=None, seed=0, iters=50, tol=1e-6,
        trim=1.0, max_dist=None, reject_border=True, init=None, method='auto'):
    """Align the source mesh (src_v [V,3] f32, src_f [F,3] int64) to the target mesh (CUDA tensors on one device): the
    transform x' = s R x + t ('rigid': s stays at its initial value) that brings the source's points onto the target's
    surface, by the iteration of the module docstring.

    The source points are `points` [P,3] f32 when given, else the source's vertices when `samples` = 0, else `samples`
    area-weighted surface samples (metrics.sample_surface, a generator seeded with `seed`).  `metric`: 'plane' (Gauss-Newton
    on the distance to the closest point's face plane: quadratic convergence near the solution) or 'point' (the closed form
    on the closest points themselves: linear convergence).  `trim` in (0, 1]: the share of the pairs with the smallest
    distances that takes part; `max_dist`: the largest distance of a pair; `reject_border`: drop the pairs whose closest
    point lies on the target's border.  `init`: None, an earlier result, or a 4x4 similarity matrix.  `method`: the search,
    as everywhere in recmv.metrics; a grid is built once.

    The iteration stops when the rms (of the distances for 'point', of the plane distances for 'plane', over the accepted
    pairs) changes by less than `tol` of itself between two searches, or after `iters` steps.  Returns a dict of python
    numbers: `scale`, `R` [3][3], `t` [3], `matrix` [4][4], `iterations` (steps taken), `converged`, `rms_before`,
    `rms_after`, `rms` (one per search), `pairs` (accepted in the last search), `points` (P), and `reason` when the iteration
    had to stop (fewer than 3 pairs accepted, or a solver refused): the transform is then the last good one."""
    if mode not in MODES:
        raise ValueError("mode must be 'rigid' or 'similarity' (got %r)" % (mode,))
    if metric not in METRICS:
        raise ValueError("metric must be 'plane' or 'point' (got %r)" % (metric,))
    if not (0. < float(trim) <= 1.):
        raise ValueError("trim must be in (0, 1] (got %r)" % (trim,))
    if max_dist is not None and not float(max_dist) > 0.:
        raise ValueError("max_dist must be positive (got %r)" % (max_dist,))
    if int(iters) < 0 or int(samples) < 0:
        raise ValueError("iters and samples must not be negative")
    metrics.use_grid(method, 0, 0)
    dst_v, dst_f = check_mesh(dst_v, dst_f, allow_empty=False)
    dev = dst_v.device
    if points is not None:
        p = check_points(points, "points", shape="[P,3]")
    else:
        check_mesh(src_v, src_f, allow_empty=False)
        p = src_v if int(samples) == 0 else metrics.sample_surface(
            src_v, src_f, int(samples), torch.Generator(device=src_v.device).manual_seed(int(seed)))[0]
    if p.device != dev:
        raise ValueError("the source and the target must be on one device")
    p = p.contiguous()
    P = p.shape[0]
    if P < 3:
        raise ValueError("icp: %d source points, at least 3 needed" % P)
    s, R, t = _initial(init)
    box = torch.stack([dst_v.amin(0), dst_v.amax(0)]).double().cpu().numpy()
    if not np.all(np.isfinite(box)):
        raise ValueError("icp: the target's vertices are not finite")
    centre = 0.5 * (box[0] + box[1])
    grid = metrics.MeshGrid(dst_v, dst_f) if metrics.use_grid(method, P, dst_f.shape[0]) else None
    border = border_flags(dst_f, dst_v.shape[0]) if reject_border else None
    plane, with_scale = metric == 'plane', mode == 'similarity'
    keep = int(math.ceil(float(trim) * P))
    limit2 = None if max_dist is None else float(max_dist) ** 2

    def search():
        """The sums of the current transform, on the host: the one read-back of an iteration."""
        M = torch.tensor(s * R, dtype=torch.float32, device=dev)
        x = p @ M.T + torch.tensor(t, dtype=torch.float32, device=dev)
        face, q, d2 = metrics._nearest(x, dst_v, dst_f, method, grid=grid)
        thr = None
        if keep < P:
            thr = torch.kthvalue(torch.where(torch.isfinite(d2), d2, torch.full_like(d2, float("inf"))), keep).values.reshape(1)
            if limit2 is not None:
                thr = thr.clamp(max=limit2)
        elif limit2 is not None:
            thr = limit2
        return icp_sums(x, q, face, d2, dst_v, dst_f, border=border, max_dist2=thr, centre=centre, plane=plane).cpu().numpy()

    history, reason, converged, steps, pairs = [], None, False, 0, 0
    while True:
        sums = search()
        pairs = int(sums[0])
        if pairs < 3 or not np.all(np.isfinite(sums)):
            reason = ("%d pairs accepted, at least 3 needed" % pairs) if pairs < 3 else "the sums are not finite"
            history.append(float("nan") if pairs < 1 else math.sqrt(max(sums[54 if plane else 18], 0.) / pairs))
            break
        rms = math.sqrt(max(sums[54 if plane else 18], 0.) / pairs)
        if history and abs(history[-1] - rms) <= float(tol) * history[-1]:
            converged = True
        history.append(rms)
        if converged or steps >= int(iters):
            break
        try:
            ds, dR, dt = solve_plane(sums, with_scale) if plane else solve_point(sums, with_scale)
        except ValueError as e:
            reason = str(e)
            break
        # x' = c + ds dR (x - c) + dt behind x = s R p + t
        s, R, t = ds * s, dR @ R, centre + ds * (dR @ (t - centre)) + dt
        steps += 1
    out = _result(s, R, t, iterations=steps, converged=converged, rms_before=history[0], rms_after=history[-1],
                  rms=history, pairs=pairs, points=P)
    if reason is not None:
        out['reason'] = reason
    return out


def apply(result, verts):
    """The transform of an icp result on verts [..,3]: float32, computed in float64 on the tensor's device."""
    M = torch.tensor(result['matrix'], dtype=torch.float64, device=verts.device)
    return (verts.double() @ M[:3, :3].T + M[:3, 3]).float()
