"""Generalized winding numbers (csrc/winding.hip) — an ADDITION to the reference: an inside test that survives holes,
overlapping pieces and inward orientation.

  winding_number    w(q) of points about a mesh, [P] float64: the sum of the faces' signed solid angles over 4 pi.  An integer
                    for a closed mesh (0 outside, +-1 inside, +-2 inside two overlapping pieces), smooth for an open one.
                    method='exact' (the default): every face for every point.  method='tree': a pyramid of cells whose far
                    nodes contribute their first-order (dipole) term — APPROXIMATE, so it is never chosen silently
  WindingTree       the pyramid of a mesh, reusable across calls; .query(points, beta)
  points_inside     |w| > threshold, bool [P]; two-sided, so a mesh that is consistently oriented inward works; NaN is outside

The definitions (the formula, f32 terms and f64 sums, skipped and degenerate faces, queries that are not finite or lie on a
face) are those of include/recmv_hip.h and INTEGRATION.md §5.  The result of a query does not depend on the other queries of
the call: large query sets are answered in slices so that the workspace stays bounded, with the same bits.

DEFAULT_BETA = 3: a node is taken as one dipole when the query is more than 3 node radii from its centre.  Against exact
float64 on the meshes and lattices of the tests the pyramid rule then errs by at most 0.0105 (0.0264 at beta = 2), and by 0.016
on a lattice of 257^3 nodes around a mesh of 158 700 faces: inside the 0.05 that keeps the share of undecided
nodes below the project's cap.
"""
import ctypes as C
import math

import torch

from . import _lib as L
from .mesh_args import check_mesh, check_points

DEFAULT_BETA = 3.
MAX_LEVELS = 7
FACES_PER_CELL = 8               # the finest level is the first whose occupied cells hold at most this many faces on average
WORKSPACE_BYTES = 256 << 20      # the partials of one slice of queries on the exact route
TREE_SLICE = 1 << 22             # queries per call on the tree route (bounds the sort's temporaries)
METHODS = ('exact', 'tree')


def _check(points, verts, faces):
    points, (verts, faces) = check_points(points, "points", shape="[P,3]"), check_mesh(verts, faces)
    if points.device != verts.device:
        raise ValueError("the points and the mesh must be on one device")
    return points, verts, faces


def chunk_faces():
    """recmv_winding_chunk_faces(): the fixed number of faces per partial sum of the exact route."""
    return int(L.lib().recmv_winding_chunk_faces())


def exact_partials(points, verts, faces):
    """One call of recmv_winding_exact on all the points: (w [P] f64, partials [chunks, P] f64) — the workspace the header
    defines, for tests and tools.  winding_number slices large query sets; this does not."""
    points, verts, faces = _check(points, verts, faces)
    P, F, dev = points.shape[0], faces.shape[0], points.device
    ws = L.workspace(nbytes := int(L.lib().recmv_winding_exact_workspace_bytes(P, F)), dev, "winding_exact_workspace_bytes",
                     dtype=torch.float64)
    w = L.scratch((P,), torch.float64, dev)
    L.launch("winding_exact", dev, L.ptr(points), P, L.ptr(verts), verts.shape[0], L.ptr(faces), F, L.ptr(w), L.ptr(ws), nbytes)
    chunks = -(-F // chunk_faces())
    return w, ws[:chunks * P].view(chunks, P)


def _exact(points, verts, faces):
    P, F = points.shape[0], faces.shape[0]
    chunks = max(-(-F // chunk_faces()), 1)
    step = max(WORKSPACE_BYTES // (8 * chunks), 1024)
    if P <= step:
        return exact_partials(points, verts, faces)[0]
    return torch.cat([exact_partials(points[a:a + step], verts, faces)[0] for a in range(0, P, step)])


def choose_levels(cells, max_levels=MAX_LEVELS, faces_per_cell=FACES_PER_CELL):
    """The number of levels for faces whose cells at level `max_levels` are `cells` [n] int64 ((i * n + j) * n + k): the first
    level at which the occupied cells hold at most `faces_per_cell` faces on average, `max_levels` when none does.  One
    read-back."""
    n = int(cells.shape[0])
    if n == 0:
        return 1
    m = 1 << max_levels
    i, j, k = cells // (m * m), (cells // m) % m, cells % m
    occupied = []
    for l in range(1, max_levels + 1):
        s = max_levels - l
        occupied.append(torch.unique((((i >> s) << l) + (j >> s) << l) + (k >> s)).shape[0])
    for l, occ in zip(range(1, max_levels + 1), occupied):
        if n <= faces_per_cell * occ:
            return l
    return max_levels


class WindingTree:
    """The dense pyramid of the mesh verts [V,3] f32 / faces [F,3] int64 (CUDA) for the far-field route: a cube around the
    mesh's bounding box, `levels` levels (1 .. 7; by default the first whose occupied finest cells hold about 8 faces), the
    faces sorted by finest cell (a stable torch sort: ascending face id within a cell), the node table and the sorted corner
    table.  Read-backs at build time: the box, the level choice and the number of usable faces.  A face with an index outside
    [0, V) is left out; a face with a corner that is not finite makes every answer NaN."""

    def __init__(self, verts, faces, levels=None):
        self.verts, self.faces = check_mesh(verts, faces)
        if levels is not None and not (1 <= int(levels) <= MAX_LEVELS):
            raise ValueError("levels must be 1 .. %d (got %r)" % (MAX_LEVELS, levels))
        dev = self.device = verts.device
        V, F = verts.shape[0], faces.shape[0]
        lib = L.lib()
        self.poisoned = False
        origin, side = (0., 0., 0.), 1.
        if V and F:
            used = self.verts[self.faces.clamp(0, V - 1).reshape(-1)]
            box = torch.stack([used.amin(0), used.amax(0)]).cpu()
            if bool(torch.isfinite(box).all()):
                lo, hi = box[0].double(), box[1].double()
                ext = float((hi - lo).max())
                side = ext * (1. + 1e-3) if ext > 0. else max(float(box.abs().max()), 1.) * 1e-3
                origin = tuple((0.5 * (lo + hi) - 0.5 * side).tolist())
            else:
                self.poisoned = True
        d = self.desc = L.WindingTreeDesc()
        d.origin[:] = origin
        d.side = side
        self.origin, self.side = tuple(d.origin), float(d.side)

        def cells_at(lv):
            d.levels = lv
            cells = L.scratch((F,), torch.int64, dev)
            if F:
                L.launch("winding_tree_cells", dev, L.ptr(self.verts), V, L.ptr(self.faces), F, C.byref(d), L.ptr(cells))
            return cells
        if levels is None:
            cells = cells_at(MAX_LEVELS)
            levels = choose_levels(cells[cells >= 0])
            if levels != MAX_LEVELS:
                cells = cells_at(levels)
        else:
            levels = int(levels)
            cells = cells_at(levels)
        self.levels = d.levels = levels
        n_cells = 8 ** levels
        sorted_cells, order = torch.sort(cells, stable=True)                        # the skipped faces (-1, -2) come first
        counts = torch.stack([(cells < 0).sum(), (cells == -2).sum()]).cpu().tolist() if F else [0, 0]
        self.poisoned = self.poisoned or counts[1] > 0
        self.order = order[counts[0]:].contiguous()
        self.n_faces = d.n_faces = F - counts[0]
        self.cell_start = torch.zeros(n_cells + 1, dtype=torch.int64, device=dev)
        if self.n_faces:
            self.cell_start[1:] = torch.bincount(sorted_cells[counts[0]:], minlength=n_cells).cumsum(0)
        self.nodes = L.scratch((int(lib.recmv_winding_tree_nodes(levels)), 16), torch.float32, dev)
        self.tris = L.scratch((max(self.n_faces, 1), 9), torch.float32, dev)
        d.nodes, d.cell_start, d.tris = self.nodes.data_ptr(), self.cell_start.data_ptr(), self.tris.data_ptr()
        L.launch("winding_tree_build", dev, L.ptr(self.verts), V, L.ptr(self.faces), F, L.ptr(self.order), C.byref(d))
        self._token = L.publish(dev)

    def query_order(self, points):
        """A permutation [P] int64 that sorts the points by the finest cell they fall into (clamped to the cube), so that
        neighbouring lanes walk the same nodes.  It changes no result."""
        n = 1 << self.levels
        o = torch.tensor(self.origin, dtype=torch.float32, device=points.device)
        ijk = ((points - o) * (n / self.side)).nan_to_num(0., 0., 0.).floor().clamp_(0, n - 1).long()
        return torch.argsort((ijk[:, 0] * n + ijk[:, 1]) * n + ijk[:, 2])

    @torch.no_grad()
    def query(self, points, beta=None, sort=True):
        """w of the points [P,3] f32 (CUDA, the tree's device), [P] float64.  `beta` (DEFAULT_BETA): finite, at least 1."""
        beta = DEFAULT_BETA if beta is None else float(beta)
        if not (math.isfinite(beta) and beta >= 1.):
            raise ValueError("beta must be finite and at least 1 (got %r)" % (beta,))
        points = check_points(points, "points", shape="[P,3]")
        if points.device != self.device:
            raise ValueError("the points and the tree must be on one device")
        P = points.shape[0]
        if self.poisoned:
            return torch.full((P,), float("nan"), dtype=torch.float64, device=self.device)
        if P > TREE_SLICE:
            return torch.cat([self.query(points[a:a + TREE_SLICE], beta, sort) for a in range(0, P, TREE_SLICE)])
        w = L.scratch((P,), torch.float64, self.device)
        if P:
            L.acquire(self._token)
            order = self.query_order(points) if sort else None
            L.launch("winding_tree_query", self.device, L.ptr(points), P, L.ptr(order), C.byref(self.desc), beta, L.ptr(w))
        return w


@torch.no_grad()
def winding_number(points, verts, faces, method='exact', beta=None, levels=None):
    """w of the points [P,3] f32 about the mesh verts [V,3] f32 / faces [F,3] int64 (CUDA tensors on one device): [P] float64.
    method='exact' evaluates every face; method='tree' builds a WindingTree (`levels`) and queries it with `beta`."""
    if method not in METHODS:
        raise ValueError("method must be 'exact' or 'tree' (got %r)" % (method,))
    points, verts, faces = _check(points, verts, faces)
    if method == 'tree':
        return WindingTree(verts, faces, levels=levels).query(points, beta)
    if beta is not None or levels is not None:
        raise ValueError("beta and levels belong to method='tree'")
    return _exact(points, verts, faces)


def inside_from_winding(w, threshold=0.5):
    """|w| > threshold; NaN is outside."""
    return w.abs() > threshold


@torch.no_grad()
def points_inside(points, verts, faces, threshold=0.5, method='exact', beta=None, levels=None):
    """Which of the points lie inside the mesh: |winding_number| > threshold, bool [P].  Two-sided: a closed mesh that is
    oriented inward has w = -1 inside.  A point that is not finite is outside."""
    threshold = float(threshold)
    if not (0. < threshold < 1.):
        raise ValueError("threshold must be in (0, 1) (got %r)" % (threshold,))
    return inside_from_winding(winding_number(points, verts, faces, method=method, beta=beta, levels=levels), threshold)
