"""Laplacian alignment of a garment template to the feature curves: the building blocks of `Laplacian_Optimizer`
(engineer/optimizer/lap_deform_optimizer.py:25-190, with `Garment_Mesh.best_match`, engineer/utils/garment_structure.py:647-724).

Matching (plain numpy / torch, once per epoch, on the CPU):
  boundary_loops          closed walks over the edges that only one face uses (recmv.connectivity)
  assign_loops            which loop stands for which feature line: the templates here are plain meshes without the SMPL
                          colour labels the reference cuts its fields by, so every field of GARMENT_FL_MATCH[garment] gets a
                          distinct loop by a linear assignment on the squared distance between loop and curve centroids
  best_match              the reference's match of a field: curve resampling, linear assignment on squared distances,
                          centred-direction filter (cos > 0.5)
  constraint_weights      cw [V] = w * (pairs on the vertex), cwt [V,3] = w * (sum of their targets), in f64, by a stable sort
                          and a segment sum in a fixed order
Solve (argmin_u |L u - L v|^2 + w |C u - t|^2) and smoothing (u <- D^-1 A u):
  solve / smooth          the HIP kernels of csrc/lap_align.hip (matrix-free Jacobi-CG in f64, one gather pass)
  solve_torch / smooth_torch  the same minimiser by a dense f64 solve of the normal equations (parity oracle and the
                          --torch-path fallback; more accurate than the reference's f32 inverse), and the same pass in torch
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import nricp
from .connectivity import boundary_loops  # noqa: F401  (the walk; callers say lap_align.boundary_loops)

TOL = 1e-10                  # CG stops when |r| <= TOL |rhs| in every column
MAX_ITER = 50000             # ... or after this many iterations
DENSE_MAX_V = 12000          # solve_torch refuses larger templates: its V x V f64 matrices would take gigabytes
COS_MIN = 0.5                # best_match's centred-direction filter (garment_structure.py:705)


# ------------------------------------------------------------------------------------------------- matching
def assign_loops(loops, verts, curves, fields, log=print, garment=''):
    """{field: loop index}: every field of `fields` that has a curve in `curves` ({name: [S,3]}) gets a distinct loop by
    linear_sum_assignment on the squared distance between the loop's and the curve's centroids.  A field without a curve,
    or left over when there are fewer loops than fields, is logged and skipped; loops without a field stay free."""
    from scipy.optimize import linear_sum_assignment
    tag = ('%s: ' % garment) if garment else ''
    present = []
    for f in fields:
        if f in curves and curves[f] is not None:
            present.append(f)
        else:
            log('%sLaplacian align: no curve for %s in this run, skipped' % (tag, f))
    if not present or not loops:
        for f in present:
            log('%sLaplacian align: the template has no boundary loop for %s, skipped' % (tag, f))
        return {}
    v = np.asarray(verts.detach().cpu().double().numpy())
    lc = np.stack([v[sorted(set(l))].mean(0) for l in loops])
    cc = np.stack([np.asarray(torch.as_tensor(curves[f]).detach().cpu().double().numpy()).reshape(-1, 3).mean(0)
                   for f in present])
    cost = ((cc[:, None, :] - lc[None, :, :]) ** 2).sum(-1)
    rows, cols = linear_sum_assignment(cost)
    out = {present[r]: int(c) for r, c in zip(rows, cols)}
    for f in present:
        if f not in out:
            log('%sLaplacian align: %d boundary loop(s) for %d fields, no loop left for %s, skipped'
                % (tag, len(loops), len(present), f))
    return {f: out[f] for f in present if f in out}


def resample_curve(curve, n):
    """The reference's resampling of a curve [T,3] for n boundary vertices: `idx = arange(0, T, (T-1)/n).long()`."""
    T = curve.shape[0]
    if T < 2 or n < 1:
        raise ValueError("best_match: a curve needs at least 2 samples and a field at least one vertex (T=%d, n=%d)" % (T, n))
    idx = torch.arange(0, T, (T - 1) / n).long()
    return curve[idx]


def best_match(verts, source_ids, curve):
    """One field of Garment_Mesh.best_match: (vertex indices [k] int64, targets [k,3] f32).  `source_ids` are the field's
    boundary vertices (ascending), `curve` [T,3] its feature curve."""
    from scipy.optimize import linear_sum_assignment
    source_ids = torch.as_tensor(source_ids, dtype=torch.int64).cpu()
    source_bo = verts.detach().cpu().float()[source_ids].numpy()
    target_bo = resample_curve(torch.as_tensor(curve).detach().cpu().float(), source_ids.shape[0]).numpy()
    s64, t64 = source_bo.astype(np.float64), target_bo.astype(np.float64)
    distance = ((s64[:, None, :] - t64[None, :, :]) ** 2).sum(-1)              # ot.dist (sqeuclidean)
    rows, cols = linear_sum_assignment(distance)
    source_n = (source_bo - source_bo.mean(axis=0))[rows]
    target_n = (target_bo - target_bo.mean(axis=0))[cols]
    with np.errstate(invalid='ignore', divide='ignore'):
        sim = ((source_n * target_n) / (np.linalg.norm(source_n, axis=1, keepdims=True)
                                        * np.linalg.norm(target_n, axis=1, keepdims=True))).sum(axis=-1)
    keep = sim > COS_MIN
    return source_ids[torch.from_numpy(rows[keep])], torch.from_numpy(target_bo[cols[keep]]).float()


def match(verts, loops, field_loops, curves):
    """All fields of `field_loops` ({field: loop index}): (vertex indices [m], targets [m,3] f32, {field: pairs})."""
    ids, tgts, counts = [], [], {}
    for f, li in field_loops.items():
        src = sorted(set(loops[li]))
        i, t = best_match(verts, src, curves[f])
        ids.append(i)
        tgts.append(t)
        counts[f] = int(i.shape[0])
    if not ids:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, 3), counts
    return torch.cat(ids), torch.cat(tgts), counts


def constraint_weights(idx, targets, V, weight):
    """cw [V] f64 = weight x (pairs on the vertex), cwt [V,3] f64 = weight x (sum of their targets): a stable sort by vertex
    and a segment sum in that order, so a vertex matched twice counts twice, as in the dense reference."""
    idx = np.asarray(torch.as_tensor(idx).cpu().numpy(), dtype=np.int64)
    t = np.asarray(torch.as_tensor(targets).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3)
    cw = np.zeros(V, dtype=np.float64)
    cwt = np.zeros((V, 3), dtype=np.float64)
    if idx.size:
        if idx.min() < 0 or idx.max() >= V:
            raise ValueError("constraint_weights: vertex index out of range [0, %d)" % V)
        order = np.argsort(idx, kind='stable')
        si, st = idx[order], t[order]
        starts = np.flatnonzero(np.r_[True, si[1:] != si[:-1]])
        verts = si[starts]
        cw[verts] = weight * np.diff(np.r_[starts, si.size]).astype(np.float64)
        cwt[verts] = weight * np.add.reduceat(st, starts, axis=0)
    return torch.from_numpy(cw), torch.from_numpy(cwt)


def boundary_distance(verts, loops, field_loops, curves):
    """Mean over the assigned loops' vertices of the distance to the nearest sample of their field's curve."""
    d = []
    v = verts.detach().cpu().double()
    for f, li in field_loops.items():
        p = v[sorted(set(loops[li]))]
        c = torch.as_tensor(curves[f]).detach().cpu().double().reshape(-1, 3)
        d.append(torch.cdist(p, c).min(1).values)
    return float(torch.cat(d).mean()) if d else float('nan')


# ------------------------------------------------------------------------------------------------- kernels
class Topology:
    """The neighbour CSR of a template (nricp.neighbours_csr) and its unique edges, on one device."""

    def __init__(self, faces, V, device):
        faces = torch.as_tensor(faces).to(device=device, dtype=torch.int64)
        self.V = V
        self.edges, _ = nricp.edges_packed(faces, V) if faces.numel() else (torch.zeros(0, 2, dtype=torch.int64,
                                                                                          device=device), None)
        self.nbr = nricp.neighbours_csr(self.edges, V)


def solve(topo, v, cw, cwt, tol=TOL, max_iter=MAX_ITER):
    """recmv_lap_align_solve: (u [V,3] f32, CG iterations, [3] final relative residuals).  v [V,3] f32, cw [V], cwt [V,3]
    on the device of v (cast to f64 here)."""
    L.require_cuda(v, "v")
    V = topo.V
    if v.dtype != torch.float32 or v.shape != (V, 3):
        raise ValueError("lap_align_solve: v must be float32 [%d,3]" % V)
    v = v.contiguous()
    cw = torch.as_tensor(cw).to(device=v.device, dtype=torch.float64).contiguous()
    cwt = torch.as_tensor(cwt).to(device=v.device, dtype=torch.float64).contiguous()
    if cw.shape != (V,) or cwt.shape != (V, 3):
        raise ValueError("lap_align_solve: cw must be [%d] and cwt [%d,3]" % (V, V))
    u = L.scratch_like(v)
    iters = C.c_int32(0)
    res = (C.c_double * 3)()
    ws = L.workspace(nbytes := int(L.lib().recmv_lap_align_workspace_bytes(V)), v.device, "lap_align_workspace_bytes", floor=256)
    off, nbr = topo.nbr
    L.launch("lap_align_solve", v.device, L.ptr(off), L.ptr(nbr), V, nbr.shape[0], L.ptr(v), L.ptr(cw), L.ptr(cwt), float(tol),
             int(max_iter), L.ptr(u), C.byref(iters), res, L.ptr(ws), nbytes)
    return u, int(iters.value), [float(r) for r in res]


def smooth(topo, u):
    """recmv_lap_smooth: every vertex becomes the mean of its neighbours (an isolated vertex the origin)."""
    L.require_cuda(u, "u")
    V = topo.V
    if u.dtype != torch.float32 or u.shape != (V, 3):
        raise ValueError("lap_smooth: u must be float32 [%d,3]" % V)
    u = u.contiguous()
    out = L.scratch_like(u)
    off, nbr = topo.nbr
    L.launch("lap_smooth", u.device, L.ptr(off), L.ptr(nbr), V, nbr.shape[0], L.ptr(u), L.ptr(out))
    return out


# ------------------------------------------------------------------------------------------------- torch path
def laplacian_dense(edges, V, dtype=torch.float64, device='cpu'):
    """pytorch3d 0.4.0 `laplacian_packed` of one mesh as a dense [V,V] matrix: 1/deg_i on each edge (i,j), -1 on the
    diagonal (an isolated vertex: a zero row with -1 on the diagonal)."""
    edges = edges.to(device)
    deg = torch.zeros(V, dtype=dtype, device=device)
    ones = torch.ones(edges.shape[0], dtype=dtype, device=device)
    deg.index_add_(0, edges[:, 0], ones).index_add_(0, edges[:, 1], ones)
    inv = torch.where(deg > 0, 1. / deg.clamp(min=1.), deg)
    Lm = torch.zeros(V, V, dtype=dtype, device=device)
    Lm[edges[:, 0], edges[:, 1]] = inv[edges[:, 0]]
    Lm[edges[:, 1], edges[:, 0]] = inv[edges[:, 1]]
    Lm.diagonal().fill_(-1.)
    return Lm


def solve_torch(topo, v, cw, cwt):
    """The minimiser of `solve` by torch.linalg.solve of the dense f64 normal equations (L^T L + diag(cw)) u = L^T L v + cwt:
    u [V,3] f32 on v's device.  Refuses templates of more than DENSE_MAX_V vertices."""
    V = topo.V
    if V > DENSE_MAX_V:
        raise ValueError("solve_torch: %d vertices; the dense solve is limited to %d (its V x V float64 matrices would take "
                         "%.1f GB): use the kernel path" % (V, DENSE_MAX_V, 3 * V * V * 8 / 1e9))
    dev = v.device
    Lm = laplacian_dense(topo.edges, V, device=dev)
    A = Lm.t() @ Lm
    A.diagonal().add_(torch.as_tensor(cw).to(device=dev, dtype=torch.float64))
    v64 = v.detach().double()
    b = Lm.t() @ (Lm @ v64) + torch.as_tensor(cwt).to(device=dev, dtype=torch.float64)
    return torch.linalg.solve(A, b).float()


def smooth_torch(topo, u):
    """`smooth` in torch: (1/deg_i) sum_{j in N(i)} u_j in f64, rounded once; an isolated vertex -> 0."""
    off, nbr = topo.nbr
    V = topo.V
    deg = (off[1:] - off[:-1]).to(torch.float64)
    rows = torch.repeat_interleave(torch.arange(V, device=u.device), (off[1:] - off[:-1]).long())
    s = torch.zeros(V, 3, dtype=torch.float64, device=u.device).index_add_(0, rows, u.double()[nbr.long()])
    inv = torch.where(deg > 0, 1. / deg.clamp(min=1.), deg)
    return (s * inv[:, None]).float()
