"""Mesh smoothing (csrc/mesh_smooth.hip) — an ADDITION to the reference, whose marching-cubes exports were smoothed by hand in
MeshLab: take the grid-aligned staircase noise off an extracted surface without moving its open boundaries.

  cotangent_weights     one float64 weight per neighbour entry (recmv_cotan_weights)
  laplacian_step        x + lambda (weighted mean of the neighbours - x) (recmv_laplacian_step)
  filter_face_normals   one iteration of bilateral normal filtering (recmv_face_normal_filter)
  update_vertices       one iteration of the vertex update toward the filtered normals (recmv_vertex_from_normals)
  smooth                the driver: (verts', info)
Each kernel has a plain-torch restatement in float64 (`*_torch`); `use_kernels=False` takes them and runs on CPU tensors too.

Definitions (include/recmv_hip.h and DESIGN.md repeat them; tests/mesh_smooth_reference.py restates them in numpy):
  weights      'uniform': every neighbour counts 1.  'cotangent': w_ij = the sum over the faces of edge (i, j), ascending, of
               1/2 max(0, cot) of the angle opposite the edge.  The clamp at 0 keeps every step a convex combination; there is no
               upper clamp because the step divides by the row's sum.  w_ij == w_ji bit for bit.
  lambda step  x + lambda (sum_j w_ij x_j / sum_j w_ij - x); a vertex that is fixed, has no valid neighbour or a weight sum that is
               not > 0 is copied bit for bit.  'laplacian' is this step alone (it shrinks); 'taubin' (Taubin 1995) follows every
               lambda step with a mu step, mu < -lambda < 0, which gives most of the lost volume back; mu = None means
               1 / (k_PB - 1 / lambda) with the pass-band k_PB = 0.1.
  bilateral    Zheng, Fu, Au, Tai 2011: `normal_iterations` of n'_i = normalize(sum_{j in N(i) + i} A_j exp(-|c_i - c_j|^2 / 2
               sigma_c^2) exp(-|n_i - n_j|^2 / 2 sigma_s^2) n_j) over the faces that share an edge with i (areas A and centroids c
               of the input), then `vertex_iterations` of x'_i = x_i + 1/|F_i| sum_f n_f (n_f . (c_f - x_i)).  It keeps creases
               that the lambda step rounds off.
  boundary     'fixed' pins every boundary vertex; 'curve' moves a boundary vertex with two boundary neighbours toward their
               midpoint (along its own curve, never inward) and leaves the others; 'free' treats the boundary like the interior
               (it shrinks open boundaries: there to show why it is not the default).
Same input, same output bits on the kernel path: every float64 sum has one order and nothing is summed with atomics.
"""
import math

import torch

from . import _lib as L
from .connectivity import EdgeTable, boundary_neighbours, face_neighbours_csr, neighbours_csr, vertex_slots_csr
from .mesh_args import check_csr, check_mesh, check_points
from .topology import valid_faces

PASS_BAND = 0.1             # Taubin's k_PB
METHODS = ('taubin', 'laplacian', 'bilateral')
WEIGHTS = ('uniform', 'cotangent')
BOUNDARIES = ('fixed', 'curve', 'free')


def _mask(fixed, V, dev):
    if fixed is None:
        return None
    if fixed.dim() != 1 or fixed.shape[0] != V:
        raise ValueError("the fixed mask must have %d entries" % V)
    return fixed.to(device=dev, dtype=torch.uint8).contiguous()


def _out(out, like):
    if out is None:
        return L.scratch_like(like)
    if out.shape != like.shape or out.dtype != like.dtype or out.device != like.device or not out.is_contiguous():
        raise ValueError("out must be contiguous and of the input's shape, dtype and device")
    return out


def _tables(faces, V):
    table = EdgeTable(faces, V)
    return table, neighbours_csr(table.edges, V), vertex_slots_csr(faces, V)


def _rows(off, n):
    """A CSR's rows as a padded table: (position [R, D] into the entries, valid [R, D])."""
    off = off.to(torch.int64)
    cnt = off[1:] - off[:-1]
    D = int(cnt.max()) if cnt.numel() else 0
    col = torch.arange(D, device=off.device)
    valid = col[None, :] < cnt[:, None]
    return (off[:-1, None] + col[None, :]).clamp(max=max(n - 1, 0)), valid


def _cross(u, w):
    """u x w with the kernels' products and differences (no fused multiply-add)."""
    return torch.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                        u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def _dot(u, w):
    return u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1] + u[:, 2] * w[:, 2]


def face_geometry(verts, faces):
    """(unit normals [F,3], areas [F], centroids [F,3], good [F]) in float64 of valid faces: the cross product at the first corner,
    half its length, (a + b + c) / 3.  good: every corner finite and the length finite and > 0; the other faces get the normal
    0 and the area 0, so they add nothing to any sum."""
    x = verts.double()
    a, b, c = x[faces[:, 0]], x[faces[:, 1]], x[faces[:, 2]]
    n = _cross(b - a, c - a)
    length = _dot(n, n).sqrt()
    good = torch.isfinite(a).all(1) & torch.isfinite(b).all(1) & torch.isfinite(c).all(1) & (length > 0) & torch.isfinite(length)
    unit = torch.where(good[:, None], n / torch.where(good, length, torch.ones_like(length))[:, None], torch.zeros_like(n))
    return unit, torch.where(good, 0.5 * length, torch.zeros_like(length)), (a + b + c) / 3., good


# ------------------------------------------------------------------------------------------------- kernels and restatements
def cotangent_weights(verts, faces, nbr_csr=None, slots_csr=None, return_counts=False):
    """recmv_cotan_weights: w [nnz] float64, one weight per entry of nbr_csr = connectivity.neighbours_csr, of verts [V,3] f32 /
    faces [F,3] int64 (CUDA); slots_csr = connectivity.vertex_slots_csr.  Tables that are absent are built (the faces must then
    be valid).  `return_counts`: also the number of faces that added nothing."""
    verts, faces = check_mesh(verts, faces)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    if nbr_csr is None or slots_csr is None:
        _, nbr, slots = _tables(faces, V)
        nbr_csr = nbr if nbr_csr is None else nbr_csr
        slots_csr = slots if slots_csr is None else slots_csr
    off, idx = check_csr(nbr_csr, V, torch.int32, "nbr_csr")
    soff, sidx = check_csr(slots_csr, V, torch.int64, "slots_csr")
    w = L.scratch((idx.numel(),), torch.float64, dev)
    counts = torch.zeros(1, dtype=torch.int32, device=dev)
    if V:
        L.launch("cotan_weights", dev, L.ptr(verts), V, L.ptr(faces), F, L.ptr(soff), L.ptr(sidx), sidx.numel(), L.ptr(off),
                 L.ptr(idx), idx.numel(), L.ptr(w), L.ptr(counts))
    return (w, int(counts.item())) if return_counts else w


def cotangent_weights_torch(verts, faces, nbr_csr=None, slots_csr=None, return_counts=False):
    """cotangent_weights in plain torch (float64, the same sums in the same order; valid faces)."""
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    if nbr_csr is None:
        nbr_csr = _tables(faces, V)[1]
    off, idx = nbr_csr[0].to(torch.int64), nbr_csr[1].to(torch.int64)
    w = torch.zeros(idx.numel(), dtype=torch.float64, device=dev)
    if F == 0 or idx.numel() == 0:
        return (w, 0) if return_counts else w
    x = verts.double()
    p = [x[faces[:, 0]], x[faces[:, 1]], x[faces[:, 2]]]
    good = face_geometry(verts, faces)[3]
    half = []
    for c in range(3):                                                             # 1/2 max(0, cot) at corner c
        e1, e2 = p[(c + 1) % 3] - p[c], p[(c + 2) % 3] - p[c]
        n = _cross(e1, e2)
        length = _dot(n, n).sqrt()
        ok = good & (length > 0) & torch.isfinite(length)
        cot = _dot(e1, e2) / torch.where(ok, length, torch.ones_like(length))
        half.append(torch.where(ok & (cot > 0), 0.5 * cot, torch.zeros_like(cot)))
    # every corner c of every face adds cot(corner c + 2) to (i -> next) and cot(corner c + 1) to (i -> previous)
    rows = torch.cat([faces[:, c] for c in range(3)] * 2)
    cols = torch.cat([faces[:, (c + 1) % 3] for c in range(3)] + [faces[:, (c + 2) % 3] for c in range(3)])
    vals = torch.cat([half[(c + 2) % 3] for c in range(3)] + [half[(c + 1) % 3] for c in range(3)])
    face = torch.arange(F, device=dev).repeat(6)
    keys = torch.repeat_interleave(torch.arange(V, device=dev), off[1:] - off[:-1]) * V + idx   # ascending: the CSR's order
    want = rows * V + cols
    at = torch.searchsorted(keys, want).clamp(max=keys.numel() - 1)
    have = keys[at] == want
    at, vals, face = at[have], vals[have], face[have]
    o = torch.argsort(at * F + face)                                               # by (entry, face): faces ascending
    at, vals = at[o], vals[o]
    first = torch.ones_like(at, dtype=torch.bool)
    first[1:] = at[1:] != at[:-1]
    start = torch.cummax(torch.where(first, torch.arange(at.numel(), device=dev), torch.zeros_like(at)), 0)[0]
    rank = torch.arange(at.numel(), device=dev) - start
    for k in range(int(rank.max()) + 1 if rank.numel() else 0):                    # a fixed summation order
        m = rank == k
        w[at[m]] = w[at[m]] + vals[m]
    return (w, int((~good).sum())) if return_counts else w


def laplacian_step(verts, nbr_csr, lam, weights=None, fixed=None, bnbr=None, out=None):
    """recmv_laplacian_step: x + lam (weighted mean of the neighbours - x) of verts [V,3] f32 (CUDA) over nbr_csr; weights [nnz]
    float64 or None (uniform); fixed [V] bool or None; bnbr [V,2] int64 = connectivity.boundary_neighbours or None."""
    verts = check_points(verts, "verts", shape="[V,3]")
    if not math.isfinite(float(lam)):
        raise ValueError("laplacian_step: lam must be finite")
    V, dev = verts.shape[0], verts.device
    off, idx = check_csr(nbr_csr, V, torch.int32, "nbr_csr")
    L.require_cuda(off, "nbr_csr")
    if weights is not None:
        L.require_cuda(weights, "weights")
        if weights.dtype != torch.float64 or weights.shape != idx.shape:
            raise ValueError("weights must be float64, one per neighbour entry")
        weights = weights.contiguous()
    if bnbr is not None:
        L.require_cuda(bnbr, "bnbr")
        if bnbr.dtype != torch.int64 or bnbr.shape != (V, 2):
            raise ValueError("bnbr must be int64 of shape [V,2]")
        bnbr = bnbr.contiguous()
    fx = _mask(fixed, V, dev)
    out = _out(out, verts)
    if V:
        L.launch("laplacian_step", dev, L.ptr(off), L.ptr(idx), V, idx.numel(), L.ptr(verts), L.ptr(weights), L.ptr(fx),
                 L.ptr(bnbr), float(lam), L.ptr(out))
    return out


def laplacian_step_torch(verts, nbr_csr, lam, weights=None, fixed=None, bnbr=None):
    """laplacian_step in plain torch (float64 sums in row order, one rounding to float32)."""
    V, dev = verts.shape[0], verts.device
    xf = verts.float()
    if V == 0:
        return xf.clone()
    x = xf.double()
    idx = nbr_csr[1].to(torch.int64)
    pos, valid = _rows(nbr_csr[0], idx.numel())
    s, total = torch.zeros_like(x), torch.zeros(V, dtype=torch.float64, device=dev)
    cnt = torch.zeros(V, dtype=torch.int64, device=dev)
    for k in range(pos.shape[1]):                                                  # a fixed summation order
        j = idx[pos[:, k]] if idx.numel() else pos[:, k]
        ok = valid[:, k] & (j >= 0) & (j < V)
        j = j.clamp(0, V - 1)
        if weights is not None:
            wk = weights[pos[:, k]]
            ok &= (wk > 0) & torch.isfinite(wk)
            s = s + torch.where(ok[:, None], wk[:, None] * x[j], torch.zeros_like(x))
            total = total + torch.where(ok, wk, torch.zeros_like(wk))
        else:
            s = s + torch.where(ok[:, None], x[j], torch.zeros_like(x))
        cnt += ok.long()
    if weights is None:
        total = cnt.double()
    move = (cnt > 0) & (total > 0) & torch.isfinite(total)
    m = s / torch.where(move, total, torch.ones_like(total))[:, None]
    if bnbr is not None:
        b0, b1 = bnbr[:, 0], bnbr[:, 1]
        on = (b0 >= 0) | (b1 >= 0)
        both = (b0 >= 0) & (b0 < V) & (b1 >= 0) & (b1 < V)
        m = torch.where(on[:, None], 0.5 * (x[b0.clamp(0, V - 1)] + x[b1.clamp(0, V - 1)]), m)
        move = torch.where(on, both, move)
    if fixed is not None:
        move &= ~fixed.to(device=dev, dtype=torch.bool)
    return torch.where(move[:, None], (x + float(lam) * (m - x)).float(), xf)


def filter_face_normals(normals, areas, centroids, ff_csr, sigma_c, sigma_s, out=None):
    """recmv_face_normal_filter: one bilateral iteration on normals [F,3] f32 with areas [F] / centroids [F,3] float64 (CUDA)
    over ff_csr = connectivity.face_neighbours_csr."""
    L.require_cuda(normals, "normals")
    L.require_cuda(areas, "areas")
    L.require_cuda(centroids, "centroids")
    F, dev = normals.shape[0], normals.device
    if normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[1] != 3:
        raise ValueError("normals must be float32 of shape [F,3]")
    if areas.dtype != torch.float64 or areas.shape != (F,) or centroids.dtype != torch.float64 or centroids.shape != (F, 3):
        raise ValueError("areas [F] and centroids [F,3] must be float64")
    for name, s in (("sigma_c", sigma_c), ("sigma_s", sigma_s)):
        if not (float(s) > 0. and math.isfinite(float(s))):
            raise ValueError("filter_face_normals: %s must be finite and > 0" % name)
    off, idx = check_csr(ff_csr, F, torch.int32, "ff_csr")
    L.require_cuda(off, "ff_csr")
    normals, areas, centroids = normals.contiguous(), areas.contiguous(), centroids.contiguous()
    out = _out(out, normals)
    if F:
        L.launch("face_normal_filter", dev, L.ptr(off), L.ptr(idx), F, idx.numel(), L.ptr(normals), L.ptr(areas), L.ptr(centroids),
                 float(sigma_c), float(sigma_s), L.ptr(out))
    return out


def filter_face_normals_torch(normals, areas, centroids, ff_csr, sigma_c, sigma_s):
    """filter_face_normals in plain torch (float64 sums in row order, one rounding to float32)."""
    F = normals.shape[0]
    nf = normals.float()
    if F == 0:
        return nf.clone()
    n = nf.double()
    inv2c, inv2s = 1. / (2. * float(sigma_c) * float(sigma_c)), 1. / (2. * float(sigma_s) * float(sigma_s))
    idx = ff_csr[1].to(torch.int64)
    pos, valid = _rows(ff_csr[0], idx.numel())
    s = areas[:, None] * n
    me = torch.arange(F, device=n.device)
    for k in range(pos.shape[1]):
        j = idx[pos[:, k]] if idx.numel() else pos[:, k]
        ok = valid[:, k] & (j >= 0) & (j < F) & (j != me)
        j = j.clamp(0, F - 1)
        dc, dn = centroids - centroids[j], n - n[j]
        wj = areas[j] * torch.exp(-(_dot(dc, dc) * inv2c)) * torch.exp(-(_dot(dn, dn) * inv2s))
        s = s + torch.where(ok[:, None], wj[:, None] * n[j], torch.zeros_like(s))
    length = _dot(s, s).sqrt()
    ok = (length > 0) & torch.isfinite(length)
    return torch.where(ok[:, None], (s / torch.where(ok, length, torch.ones_like(length))[:, None]).float(), nf)


def update_vertices(verts, faces, normals, slots_csr=None, fixed=None, out=None):
    """recmv_vertex_from_normals: one iteration of x_i + 1/|F_i| sum_f n_f (n_f . (c_f - x_i)) on verts [V,3] f32 / faces [F,3]
    int64 with normals [F,3] f32 (CUDA); slots_csr = connectivity.vertex_slots_csr, built when absent (valid faces then)."""
    verts, faces = check_mesh(verts, faces)
    L.require_cuda(normals, "normals")
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    if normals.dtype != torch.float32 or normals.shape != (F, 3):
        raise ValueError("normals must be float32 of shape [F,3]")
    normals = normals.contiguous()
    soff, sidx = check_csr(vertex_slots_csr(faces, V) if slots_csr is None else slots_csr, V, torch.int64, "slots_csr")
    fx = _mask(fixed, V, dev)
    out = _out(out, verts)
    if V:
        L.launch("vertex_from_normals", dev, L.ptr(verts), V, L.ptr(faces), F, L.ptr(soff), L.ptr(sidx), sidx.numel(),
                 L.ptr(normals), L.ptr(fx), L.ptr(out))
    return out


def update_vertices_torch(verts, faces, normals, slots_csr=None, fixed=None):
    """update_vertices in plain torch (float64 sums in row order, one rounding to float32; valid faces)."""
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    xf = verts.float()
    if V == 0 or F == 0:
        return xf.clone()
    x, n = xf.double(), normals.float().double()
    cen = (x[faces[:, 0]] + x[faces[:, 1]] + x[faces[:, 2]]) / 3.
    soff, sidx = vertex_slots_csr(faces, V) if slots_csr is None else slots_csr
    pos, valid = _rows(soff, sidx.numel())
    s = torch.zeros_like(x)
    cnt = torch.zeros(V, dtype=torch.int64, device=dev)
    for k in range(pos.shape[1]):
        face = sidx[pos[:, k]] // 3
        nf = n[face]
        h = _dot(nf, cen[face] - x)
        ok = valid[:, k] & torch.isfinite(h) & (_dot(nf, nf) > 0) & torch.isfinite(_dot(nf, nf))
        s = s + torch.where(ok[:, None], nf * h[:, None], torch.zeros_like(s))
        cnt += ok.long()
    move = cnt > 0
    if fixed is not None:
        move &= ~fixed.to(device=dev, dtype=torch.bool)
    return torch.where(move[:, None], (x + s / cnt.clamp(min=1).double()[:, None]).float(), xf)


# ------------------------------------------------------------------------------------------------- the driver
def _measure(verts, faces, table, whole=True):
    """(area, signed volume or None, roughness) of valid faces, float64: the volume only of a watertight mesh (topology.report's
    rule: no boundary, non-manifold or inconsistently oriented edge, no face without area); roughness = the mean dihedral
    angle over the edges with two faces, weighted by the two faces' areas."""
    F = faces.shape[0]
    if F == 0:
        return 0., None, 0.
    unit, area, _, good = face_geometry(verts, faces)
    x = verts.double()
    two = table.count == 2
    o = torch.argsort(table.face_to_edge.reshape(-1), stable=True)                 # slots by edge, faces ascending
    start = torch.cumsum(table.count, 0) - table.count
    f0, f1 = o[start[two]] // 3, o[(start[two] + 1).clamp(max=3 * F - 1)] // 3
    rough = 0.
    if f0.numel():
        c = _cross(unit[f0], unit[f1])
        angle = torch.atan2(_dot(c, c).sqrt(), _dot(unit[f0], unit[f1]))
        wgt = area[f0] + area[f1]
        total = float(wgt.sum())
        rough = float((wgt * angle).sum()) / total if total > 0 else 0.
    ahead = torch.zeros(table.E, dtype=torch.int64, device=faces.device).index_add_(0, table.face_to_edge.reshape(-1),
                                                                                    table.forward.reshape(-1).long())
    watertight = whole and bool(good.all()) and bool((two & (ahead == 1)).all())   # whole: no face was left out as invalid
    volume = None
    if watertight:
        a, b, c = x[faces[:, 0]], x[faces[:, 1]], x[faces[:, 2]]
        volume = float(_dot(a, _cross(b, c)).sum()) / 6.
    return float(area.sum()), volume, rough


@torch.no_grad()
def smooth(verts, faces, method='taubin', iterations=10, lam=0.5, mu=None, weights='uniform', reweight=False, boundary='fixed',
           fixed=None, normal_iterations=5, vertex_iterations=10, sigma_s=0.35, sigma_c=None, use_kernels=True, log=None):
    """Smooth one triangle mesh (verts [V,3], faces [F,3] int64, one device): (verts' f32, info); the faces do not change.
    method 'taubin': `iterations` of a lam step and a mu step; 'laplacian': of the lam step alone; 'bilateral':
    `normal_iterations` of the normal filter, then `vertex_iterations` of the vertex update (sigma_c = None: the mean distance
    between the centroids of edge-adjacent faces of the input).  weights 'cotangent' are taken from the input once, with
    `reweight` before every iteration.  boundary 'fixed' | 'curve' | 'free' and a mask `fixed` [V] bool of further vertices that
    stay.  Faces with an index outside [0, V) or a repeated one take no part; non-manifold edges are fine.  info: method and
    the parameters as used, invalid_faces, moved (vertices whose bits changed), displacement_mean / _max, area_before /
    _after, volume_before / _after (None unless watertight), roughness_before / _after.  `use_kernels=False`: the same driver on
    the float64 restatements (CPU tensors too).  The module docstring has the definitions."""
    if method not in METHODS:
        raise ValueError("smooth: method must be one of %s" % (METHODS,))
    if weights not in WEIGHTS:
        raise ValueError("smooth: weights must be one of %s" % (WEIGHTS,))
    if boundary not in BOUNDARIES:
        raise ValueError("smooth: boundary must be one of %s" % (BOUNDARIES,))
    if int(iterations) < 0 or int(normal_iterations) < 0 or int(vertex_iterations) < 0:
        raise ValueError("smooth: iteration counts must not be negative")
    lam = float(lam)
    if not math.isfinite(lam) or not (0. < lam <= 1.):
        raise ValueError("smooth: lam must be in (0, 1]")
    if mu is None:
        mu = 1. / (PASS_BAND - 1. / lam)
    mu = float(mu)
    if not math.isfinite(mu):
        raise ValueError("smooth: mu must be finite")
    if method == 'taubin' and not mu < 0.:
        raise ValueError("smooth: taubin needs mu < 0")
    if not (float(sigma_s) > 0. and math.isfinite(float(sigma_s))):
        raise ValueError("smooth: sigma_s must be finite and > 0")
    if sigma_c is not None and not (float(sigma_c) > 0. and math.isfinite(float(sigma_c))):
        raise ValueError("smooth: sigma_c must be finite and > 0")
    check_mesh(verts, faces, cuda=use_kernels, float_verts=True)
    V, dev = verts.shape[0], verts.device
    if fixed is not None and (not isinstance(fixed, torch.Tensor) or fixed.dim() != 1 or fixed.shape[0] != V):
        raise ValueError("smooth: the fixed mask must have %d entries" % V)
    x0 = verts.float().contiguous()
    keep = valid_faces(faces, V)
    fv = faces[keep].contiguous()                                                  # the faces that take part
    table, nbr, slots = _tables(fv, V)
    unit, area, cen, good = face_geometry(x0, fv)
    pinned = torch.zeros(V, dtype=torch.bool, device=dev)
    bnbr = None
    if boundary == 'fixed':
        pinned |= table.boundary_vertex
    elif boundary == 'curve':
        bnbr = boundary_neighbours(table)
    if fixed is not None:
        pinned |= fixed.to(device=dev, dtype=torch.bool)
    fx = pinned.to(torch.uint8)
    info = {'method': method, 'boundary': boundary, 'invalid_faces': int(faces.shape[0] - fv.shape[0]) + int((~good).sum())}
    whole = fv.shape[0] == faces.shape[0]
    before = _measure(x0, fv, table, whole)
    x = x0
    if method == 'bilateral':
        ff = face_neighbours_csr(table)
        if sigma_c is None:
            rows = torch.repeat_interleave(torch.arange(fv.shape[0], device=dev), (ff[0][1:] - ff[0][:-1]).long())
            d = cen[rows] - cen[ff[1].long()]
            sigma_c = float(_dot(d, d).sqrt().mean()) if rows.numel() else 1.
            if not sigma_c > 0.:
                sigma_c = 1.
        info.update({'normal_iterations': int(normal_iterations), 'vertex_iterations': int(vertex_iterations),
                     'sigma_s': float(sigma_s), 'sigma_c': float(sigma_c)})
        n = unit.float().contiguous()
        for _ in range(int(normal_iterations)):
            n = (filter_face_normals(n, area, cen, ff, sigma_c, sigma_s) if use_kernels
                 else filter_face_normals_torch(n, area, cen, ff, sigma_c, sigma_s))
        for _ in range(int(vertex_iterations)):
            x = update_vertices(x, fv, n, slots, fx) if use_kernels else update_vertices_torch(x, fv, n, slots, pinned)
    else:
        info.update({'iterations': int(iterations), 'lam': lam, 'mu': mu if method == 'taubin' else None, 'weights': weights,
                     'reweight': bool(reweight)})
        cot = cotangent_weights if use_kernels else cotangent_weights_torch
        w = cot(x, fv, nbr, slots) if weights == 'cotangent' else None
        for it in range(int(iterations)):
            if w is not None and reweight and it:
                w = cot(x, fv, nbr, slots)
            for step in ((lam, mu) if method == 'taubin' else (lam,)):
                x = (laplacian_step(x, nbr, step, w, fx, bnbr) if use_kernels
                     else laplacian_step_torch(x, nbr, step, w, pinned, bnbr))
    after = _measure(x, fv, table, whole)                                            # the first read-back: the loop above only enqueues
    d = (x.double() - x0.double())
    dist = _dot(d, d).sqrt()
    info.update({'moved': int((x.view(torch.int32) != x0.view(torch.int32)).any(1).sum()) if V else 0,
                 'displacement_mean': float(dist.mean()) if V else 0., 'displacement_max': float(dist.max()) if V else 0.,
                 'area_before': before[0], 'area_after': after[0], 'volume_before': before[1], 'volume_after': after[1],
                 'roughness_before': before[2], 'roughness_after': after[2]})
    if log is not None:
        log("smooth %s: %d of %d vertices moved, largest displacement %.3g, roughness %.4f -> %.4f"
            % (method, info['moved'], V, info['displacement_max'], before[2], after[2]))
    return (x0.clone() if x is x0 else x).contiguous(), info
