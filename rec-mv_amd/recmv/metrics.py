"""Surface metrics between a reconstructed and a ground-truth mesh (csrc/mesh_grid.hip) — an ADDITION to the reference,
whose tools/comparison_results.py stops after loading a mesh.

  MeshGrid          a uniform grid over a triangle mesh (recmv_mesh_grid_count / recmv_mesh_grid_fill); `.closest_point(p)`
                    is iso_remesh.closest_point's exact search through it (recmv_closest_point_grid): the same bits
                    `.intersections(verts, faces)` / `.self_intersections()` the faces of another mesh / of its own that
                    cross its faces (recmv_mesh_intersect_grid_count / _fill, csrc/mesh_intersect.hip)
                    `.segment_hits(p, q)` the first face every segment p -> q hits and the number of faces it hits
                    (recmv_segment_mesh_grid, csrc/segment_mesh.hip)
  segment_hits      the same through the grid or by the brute force (recmv_segment_mesh_brute)
  points_inside     which points lie inside a closed mesh: the majority of three crossing parities
  penetration       inside test plus the closest-point distance of the points inside: how deep a garment sinks into a body
  mesh_intersections, self_intersections   the crossing face pairs of two meshes / of one mesh, the faces involved and their
                    share of the mesh — through the grid or by the brute force (recmv_mesh_intersect_brute)
  sample_surface    loop.sample_fan_mesh's area-weighted surface samples, with the picked faces
  surface_distance  accuracy / completeness / Chamfer / normal consistency / precision, recall and F-score at thresholds
                    between two meshes taken to be in one frame (recmv.align.icp brings them into one; eval_fl.py --align),
                    from surface samples in both directions

Definitions (d the unsquared distance sqrt(dist2) of a sample to the other SURFACE, in the meshes' length unit; every
reduction in float64 on the device, one read-back):
  accuracy            mean d over the samples of the prediction (accuracy_rms, accuracy_max: its rms and maximum)
  completeness        the same over the samples of the ground truth (completeness_rms, completeness_max)
  chamfer_l1          (accuracy + completeness) / 2
  chamfer_l2          mean d^2 over the prediction's samples + mean d^2 over the ground truth's
  normal_consistency  per direction (…_pred_to_gt, …_gt_to_pred) the mean of |n_source_face . n_nearest_face| with unit face
                      normals; `normal_consistency` is the average of the two
  precision_<t>       the share of the prediction's samples with d <= t; recall_<t> the same for the ground truth's;
                      fscore_<t> their harmonic mean (0 when both are 0)
Crossing (csrc/tri_tri.h): two faces cross when an edge of one properly pierces the other — every
inequality strict, so touching, coplanar overlap, faces without area and NaN are no crossing.  Exact integers: the grid and
the brute force give the same pairs.
Segment hit (csrc/seg_tri.h): the segment pq hits a face when its endpoints lie strictly on opposite sides
of the face's plane and the segment passes strictly inside the three edges — touching, a segment in the face's plane, a face
without area, a segment without length and anything not finite are no hit; t = sp / (sp - sq) from the two plane
determinants.  The grid and the brute force give the same bits.
"""
import ctypes as C
import math

import torch

from . import _lib as L
from .mesh_args import check_mesh, check_points

FACES_PER_CELL = 3.0           # the cell size aims at this many faces per occupied cell (h about 1.5 mean edges on a closed surface)
MAX_CELLS = 1 << 22            # offsets table of 16 MiB
MAX_ENTRIES = 1 << 28          # (cell, face) entries of 1 GiB: beyond that the grid is coarsened
QUERY_LANES = 1                # lanes of a wave per query and whether the queries are sorted by cell: to be settled by
QUERY_SORTED = True            # tools/mesh_distance_timing.py (profiles/mesh_distance_timing.json); not measured yet, a guess
# method='auto': the grid (build + query) from this many point-triangle tests P * F on, brute force below.  The crossover
# comes from profiles/mesh_distance_timing.json (tools/mesh_distance_timing.py; DESIGN.md §8 "Evaluation"); that file has not
# been recorded yet, so the value is unreachable and 'auto' chooses the brute force at every size.
AUTO_GRID_MIN_TESTS = 1 << 62
DEFAULT_THRESHOLDS = (0.005, 0.01, 0.02)
# The crossing query.  Both constants are to be read off profiles/mesh_intersect_timing.json (tools/mesh_intersect_timing.py;
# DESIGN.md §8 "Crossing faces"): the lanes per face of A with the lowest summed query time, and the number of face pairs
# FA * FB from which the grid (build + count + fill) is faster than the brute force (count + fill).  That file has not been
# recorded on an MI355X yet: the lanes are a guess, and the crossover is unreachable, so 'auto' chooses the brute force at
# every size until it exists (method='grid' is there for large meshes).
INTERSECT_LANES = 8
AUTO_GRID_MIN_PAIRS = 1 << 62
# The segment query.  Both constants are to be read off profiles/segment_mesh_timing.json (tools/segment_mesh_timing.py;
# DESIGN.md §8 "Segment queries"): the lanes per segment with the lowest summed time, and the smallest number of
# segment-face tests S * F from which the grid (build + query) was faster than the brute force in every repeat.  NOT MEASURED:
# that file has not been recorded on an MI355X yet, so the lanes are a guess (a segment's slab holds a handful of cells: one
# lane has them all to itself, 64 would mostly idle) and the crossover is unreachable: 'auto' chooses the brute force at every
# size until the file exists (method='grid' is there for large inputs).
SEGMENT_LANES = 8
AUTO_GRID_MIN_SEGMENT_TESTS = 1 << 62
# points_inside: three fixed unit directions, mutually non-parallel, none along an axis or a diagonal of the axes (a ray along
# a coordinate axis runs in the planes, edges and vertices of every axis-aligned mesh and would touch instead of cross)
INSIDE_DIRECTIONS = ((0.5310514366481575, 0.6638142958101968, 0.5266260080094228),
                     (-0.7072061522754515, 0.32773186373169966, 0.6264593232434947),
                     (0.3090895268685805, -0.8275622816158767, 0.46861960525236396))


def choose_grid(lo, hi, n_faces, faces_per_cell=FACES_PER_CELL, max_cells=MAX_CELLS):
    """Grid over the box lo .. hi (three floats each) for a mesh of `n_faces`: (cell size, (nx, ny, nz)).  Cubic cells; the
    size aims at `faces_per_cell` faces per cell a surface of the box's area passes through, h^2 = area * faces_per_cell /
    n_faces; a zero-extent axis gets one cell; the cells are enlarged until there are at most `max_cells`."""
    ext = [max(float(b) - float(a), 0.) for a, b in zip(lo, hi)]
    if not all(math.isfinite(e) for e in ext):
        raise ValueError("choose_grid: the bounding box is not finite")
    area = 2. * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0])
    n = max(int(n_faces), 1)
    if area > 0:
        h = math.sqrt(area * faces_per_cell / n)
    elif max(ext) > 0:
        h = max(ext) * faces_per_cell / n
    else:
        h = 1.
    h = max(h, max(ext) * 2. ** -20, 1e-30)
    while True:
        h = float(torch.tensor(h, dtype=torch.float32))                     # the kernels get a float32
        dims = tuple(int(e / h) + 1 if e > 0 else 1 for e in ext)
        cells = dims[0] * dims[1] * dims[2]
        if cells <= max_cells:
            return h, dims
        h *= 1.02 * (cells / max_cells) ** (1. / max(sum(d > 1 for d in dims), 1))


class MeshGrid:
    """A uniform grid over the mesh verts [V,3] f32 / faces [F,3] int64 (CUDA).  The bounding box and the number of
    (cell, face) entries are read back: two host synchronisations per build.  `dims` (and optionally `cell_size`) force a
    grid instead of choose_grid's (tests, tools)."""

    def __init__(self, verts, faces, dims=None, cell_size=None, faces_per_cell=FACES_PER_CELL):
        self.verts, self.faces = check_mesh(verts, faces, allow_empty=False)
        dev = verts.device
        box = torch.stack([self.verts.amin(0), self.verts.amax(0)]).cpu()
        if not bool(torch.isfinite(box).all()):
            raise ValueError("MeshGrid: the vertices are not finite")
        lo, hi = box[0].tolist(), box[1].tolist()
        forced = dims is not None
        if forced:
            dims = tuple(int(d) for d in dims)
            if cell_size is None:
                cell_size = max(max((b - a) / d for a, b, d in zip(lo, hi, dims)) * (1 + 1e-6), 1e-30)
            h = float(torch.tensor(float(cell_size), dtype=torch.float32))
        else:
            h, dims = choose_grid(lo, hi, faces.shape[0], faces_per_cell)
        self._mesh = mesh = (L.ptr(self.verts), self.verts.shape[0], L.ptr(self.faces), self.faces.shape[0])
        self.desc = desc = L.MeshGridDesc()                 # recmv_mesh_grid: points into offsets, entries and tris below
        self.origin = desc.origin
        desc.origin[:] = lo
        while True:
            desc.cell_size, (desc.nx, desc.ny, desc.nz) = h, dims
            cells = dims[0] * dims[1] * dims[2]
            counts = L.scratch((cells,), torch.int32, dev)
            total = L.scratch((1,), torch.int64, dev)
            L.launch("mesh_grid_count", dev, *mesh, C.byref(desc), L.ptr(counts), L.ptr(total))
            n = int(total.item())
            if n <= MAX_ENTRIES:
                break
            if forced:
                raise ValueError("MeshGrid: %d (cell, face) entries in the forced grid, at most %d" % (n, MAX_ENTRIES))
            h, dims = float(torch.tensor(2 * h, dtype=torch.float32)), tuple((d + 1) // 2 for d in dims)
        self.cell_size, self.dims, self.n_entries = h, dims, n
        self.offsets = L.scratch((cells + 1,), torch.int32, dev)
        self.entries = L.scratch((max(n, 1),), torch.int32, dev)
        self.tris = L.scratch((self.faces.shape[0], 12), torch.float32, dev)
        desc.offsets, desc.entries, desc.tris = self.offsets.data_ptr(), self.entries.data_ptr(), self.tris.data_ptr()
        desc.n_entries = n
        ws = L.workspace(nbytes := int(L.lib().recmv_mesh_grid_workspace_bytes(cells)), dev, "mesh_grid_workspace_bytes")
        L.launch("mesh_grid_fill", dev, *mesh, C.byref(desc), L.ptr(counts), L.ptr(ws), nbytes)
        self.counts = counts

    def cell_of(self, p):
        """Linear cell index [P] int64 of the points p (clamped into the grid), for sorting the queries."""
        o = torch.tensor(list(self.origin), dtype=torch.float32, device=p.device)
        n = torch.tensor(self.dims, dtype=torch.float32, device=p.device)
        c = torch.minimum(((p - o) / self.cell_size).floor().nan_to_num(0.).clamp_(min=0.), n - 1).long()
        return (c[:, 2] * self.dims[1] + c[:, 1]) * self.dims[0] + c[:, 0]

    def closest_point(self, p, lanes=None, sort=None):
        """iso_remesh.closest_point(p, verts, faces) through the grid: (face [P] int64, point [P,3] f32, squared distance
        [P] f32), ties to the lowest face id, the same bits.  `lanes` (1, 8 or 64 lanes per query) and `sort` (queries
        ordered by cell) choose the launch shape; they do not change the result."""
        p = check_points(p, "p", shape="[P,3]")
        if p.device != self.verts.device:
            raise ValueError("p and the mesh must be on one device")
        P, dev = p.shape[0], p.device
        face = L.scratch((P,), torch.int64, dev)
        point = L.scratch((P, 3), torch.float32, dev)
        dist2 = L.scratch((P,), torch.float32, dev)
        if P == 0:
            return face, point, dist2
        lanes = QUERY_LANES if lanes is None else int(lanes)
        order = torch.sort(self.cell_of(p))[1].contiguous() if (QUERY_SORTED if sort is None else sort) else None
        L.launch("closest_point_grid", dev, L.ptr(p), P, L.ptr(order), self.faces.shape[0], C.byref(self.desc), lanes,
                 L.ptr(face), L.ptr(point), L.ptr(dist2))
        return face, point, dist2

    def segment_hits(self, p, q, count=False, lanes=None):
        """The faces of the grid's mesh the segments p [S,3] -> q [S,3] (f32, CUDA) hit: a dict with `face` [S] int64 (the hit
        with the smallest t, ties to the lowest face id; -1: none), `t` [S] f32 (NaN: none), `point` [S,3] = p + t (q - p)
        (NaN: none) and `count` [S] int32, the number of faces hit (None unless `count`; without it the walk may stop behind
        the first hit).  `lanes` (1, 8 or 64 lanes per segment) chooses the launch shape; it does not change the result."""
        p, q = _check_segments(p, q, self.verts.device)
        S, dev = p.shape[0], p.device
        face = L.scratch((S,), torch.int64, dev)
        t = L.scratch((S,), torch.float32, dev)
        cnt = L.scratch((S,), torch.int32, dev) if count else None
        lanes = SEGMENT_LANES if lanes is None else int(lanes)
        if lanes not in (1, 8, 64):
            raise ValueError("lanes must be 1, 8 or 64 (got %r)" % (lanes,))
        if S:
            L.launch("segment_mesh_grid", dev, L.ptr(p), L.ptr(q), S, *self._mesh, C.byref(self.desc), lanes, int(bool(count)),
                     L.ptr(face), L.ptr(t), L.ptr(cnt))
        return _segment_result(p, q, face, t, cnt)

    def _crossings(self, verts, faces, self_mode, lanes):
        lanes = INTERSECT_LANES if lanes is None else int(lanes)
        dev = self.verts.device
        FA = faces.shape[0]
        grid = (C.byref(self.desc), lanes, int(self_mode), int(self_mode))
        mesh = (L.ptr(verts), verts.shape[0], L.ptr(faces), FA, *self._mesh)
        lib = L.lib()

        def count(counts, total):
            L.check(lib.recmv_mesh_intersect_grid_count(*mesh, *grid, L.ptr(counts), L.ptr(total), L.stream_ptr(dev)),
                    "mesh_intersect_grid_count")

        def fill(offsets, pairs, capacity, cursor, dropped):
            L.check(lib.recmv_mesh_intersect_grid_fill(*mesh, *grid, L.ptr(offsets), L.ptr(pairs), capacity, L.ptr(cursor),
                                                       L.ptr(dropped), L.stream_ptr(dev)), "mesh_intersect_grid_fill")
        return _two_passes(count, fill, FA, dev)

    def intersections(self, verts, faces, lanes=None):
        """The faces of the mesh verts [V,3] f32 / faces [F,3] int64 (mesh A) that cross faces of the grid's mesh (B): (pairs
        [K,2] int64 of (face of A, face of B) sorted by (i, j), counts [F] int32 of pairs per face of A).  One read-back, for
        K.  `lanes` (1, 8 or 64 lanes per face of A) chooses the launch shape; it does not change the result."""
        verts, faces = check_mesh(verts, faces)
        if verts.device != self.verts.device:
            raise ValueError("the two meshes must be on one device")
        return self._crossings(verts, faces, False, lanes)

    def self_intersections(self, lanes=None):
        """The pairs i < j of the grid's own faces that cross and share no vertex index: (pairs [K,2] int64 sorted, counts
        [F] int32 per lower face)."""
        return self._crossings(self.verts, self.faces, True, lanes)


def _two_passes(count, fill, FA, dev):
    """count(counts, total), the scan, fill(offsets, pairs, capacity, cursor, dropped); the pairs sorted by (i, j)."""
    counts = L.scratch((FA,), torch.int32, dev)
    total = L.scratch((1,), torch.int64, dev)
    with L.device_guard(dev):
        count(counts, total)
    K = int(total.item())                                                         # the one read-back
    if K >= 1 << 30:
        raise ValueError("%d crossing pairs: at most 2^30 - 1" % K)
    if K == 0:
        return torch.zeros((0, 2), dtype=torch.int64, device=dev), counts
    offsets = torch.zeros(FA + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)
    pairs = L.scratch((K, 2), torch.int32, dev)
    cursor = L.scratch((FA,), torch.int32, dev)
    dropped = L.scratch((1,), torch.int64, dev)
    with L.device_guard(dev):
        fill(offsets, pairs, K, cursor, dropped)
    pairs = pairs.long()
    order = torch.sort(pairs[:, 0] * (1 << 31) + pairs[:, 1])[1]                   # face ids are below 2^31
    return pairs[order].contiguous(), counts


def _brute_crossings(a_v, a_f, b_v, b_f, self_mode):
    dev = a_v.device
    FA = a_f.shape[0]
    mesh = (L.ptr(a_v), a_v.shape[0], L.ptr(a_f), FA, L.ptr(b_v), b_v.shape[0], L.ptr(b_f), b_f.shape[0], int(self_mode),
            int(self_mode))
    lib = L.lib()

    def count(counts, total):
        L.check(lib.recmv_mesh_intersect_brute(*mesh, L.ptr(counts), L.ptr(total), None, None, 0, None, None,
                                               L.stream_ptr(dev)), "mesh_intersect_brute")

    def fill(offsets, pairs, capacity, cursor, dropped):
        L.check(lib.recmv_mesh_intersect_brute(*mesh, None, None, L.ptr(offsets), L.ptr(pairs), capacity, L.ptr(cursor),
                                               L.ptr(dropped), L.stream_ptr(dev)), "mesh_intersect_brute")
    return _two_passes(count, fill, FA, dev)


def use_grid_for_pairs(method, n_faces_a, n_faces_b):
    if method not in ('auto', 'grid', 'brute'):
        raise ValueError("method must be 'auto', 'grid' or 'brute' (got %r)" % (method,))
    return method == 'grid' or (method == 'auto' and n_faces_a * n_faces_b >= AUTO_GRID_MIN_PAIRS)


def _involved(faces_col, n_faces):
    f = torch.unique(faces_col)
    return f, float(f.shape[0]) / max(int(n_faces), 1)


@torch.no_grad()
def mesh_intersections(a_v, a_f, b_v, b_f, method='auto', lanes=None):
    """The crossings of mesh A (a_v [V,3] f32, a_f [F,3] int64) and mesh B (CUDA tensors on one device): a dict with `pairs`
    [K,2] int64 (face of A, face of B) sorted by (i, j), `n_pairs`, `faces_a` / `faces_b` (the distinct faces involved,
    sorted) and `ratio_a` / `ratio_b` (their number over the mesh's face count).  'grid': a MeshGrid over B; 'brute': every
    pair of faces; 'auto': by the number of face pairs.  The same integers either way."""
    a_v, a_f = check_mesh(a_v, a_f, allow_empty=False)
    b_v, b_f = check_mesh(b_v, b_f, allow_empty=False)
    if a_v.device != b_v.device:
        raise ValueError("the two meshes must be on one device")
    if use_grid_for_pairs(method, a_f.shape[0], b_f.shape[0]):
        pairs, _ = MeshGrid(b_v, b_f).intersections(a_v, a_f, lanes=lanes)
    else:
        pairs, _ = _brute_crossings(a_v, a_f, b_v, b_f, False)
    fa, ra = _involved(pairs[:, 0], a_f.shape[0])
    fb, rb = _involved(pairs[:, 1], b_f.shape[0])
    return {'pairs': pairs, 'n_pairs': int(pairs.shape[0]), 'faces_a': fa, 'faces_b': fb, 'ratio_a': ra, 'ratio_b': rb}


@torch.no_grad()
def self_intersections(v, f, method='auto', lanes=None):
    """The crossings of a mesh with itself: pairs i < j of faces that cross and share no vertex index.  A dict with `pairs`
    [K,2] int64 sorted, `n_pairs`, `faces` (the distinct faces involved) and `ratio` (their number over the face count)."""
    v, f = check_mesh(v, f, allow_empty=False)
    if use_grid_for_pairs(method, f.shape[0], f.shape[0]):
        pairs, _ = MeshGrid(v, f).self_intersections(lanes=lanes)
    else:
        pairs, _ = _brute_crossings(v, f, v, f, True)
    faces, ratio = _involved(pairs.reshape(-1), f.shape[0])
    return {'pairs': pairs, 'n_pairs': int(pairs.shape[0]), 'faces': faces, 'ratio': ratio}


def _check_segments(p, q, device=None):
    p, q = check_points(p, "p", shape="[S,3]"), check_points(q, "q", shape="[S,3]")
    if p.shape != q.shape:
        raise ValueError("p and q must have the same shape (got %s and %s)" % (tuple(p.shape), tuple(q.shape)))
    if p.device != q.device or (device is not None and p.device != device):
        raise ValueError("the segments and the mesh must be on one device")
    return p, q


def _segment_result(p, q, face, t, count):
    return {'face': face, 't': t, 'point': p + t[:, None] * (q - p), 'count': count}


def use_grid_for_segments(method, n_segments, n_faces):
    if method not in ('auto', 'grid', 'brute'):
        raise ValueError("method must be 'auto', 'grid' or 'brute' (got %r)" % (method,))
    return method == 'grid' or (method == 'auto' and n_segments * n_faces >= AUTO_GRID_MIN_SEGMENT_TESTS)


@torch.no_grad()
def segment_hits(p, q, verts, faces, count=False, method='auto', lanes=None):
    """MeshGrid.segment_hits for the mesh verts [V,3] f32 / faces [F,3] int64 (CUDA tensors on one device).  'grid': through a
    MeshGrid; 'brute': every face (it always counts; `count` only decides whether the counts are returned); 'auto': by the
    number of segment-face tests.  The same bits either way."""
    verts, faces = check_mesh(verts, faces, allow_empty=False)
    p, q = _check_segments(p, q, verts.device)
    if use_grid_for_segments(method, p.shape[0], faces.shape[0]):
        return MeshGrid(verts, faces).segment_hits(p, q, count=count, lanes=lanes)
    S, dev = p.shape[0], p.device
    face = L.scratch((S,), torch.int64, dev)
    t = L.scratch((S,), torch.float32, dev)
    cnt = L.scratch((S,), torch.int32, dev)
    if S:
        L.launch("segment_mesh_brute", dev, L.ptr(p), L.ptr(q), S, L.ptr(verts), verts.shape[0], L.ptr(faces), faces.shape[0],
                 L.ptr(face), L.ptr(t), L.ptr(cnt))
    return _segment_result(p, q, face, t, cnt if count else None)


def _check_rule(rule):
    if rule not in ('parity', 'winding'):
        raise ValueError("rule must be 'parity' or 'winding' (got %r)" % (rule,))


@torch.no_grad()
def points_inside(points, verts, faces, method='auto', rule='parity'):
    """Which of the points [P,3] f32 lie inside the mesh verts / faces (CUDA): bool [P].  Every point casts three segments
    along INSIDE_DIRECTIONS, each ending beyond the mesh's bounding box (1.5 box diagonals plus the point's distance to the
    box's centre away), and the result is the majority of the three parities of the number of faces crossed: a ray that
    grazes an edge or a vertex (touching is no hit, so it may count one face too few or too many) is outvoted.  The mesh
    is taken to be closed and free of self-intersections; a mesh that is not closed gives whatever the parities give.  A point
    that is not finite is outside.
    rule='winding' takes recmv.winding.points_inside instead (the exact generalized winding number, |w| > 1/2): sound for a mesh
    with holes, for overlapping closed pieces (their union) and for either orientation; `method` then only is checked."""
    _check_rule(rule)
    check_mesh(verts, faces, allow_empty=False)
    points = check_points(points, "points", shape="[P,3]")
    if points.device != verts.device:
        raise ValueError("the points and the mesh must be on one device")
    use_grid_for_segments(method, 0, 0)
    P = points.shape[0]
    if P == 0:
        return torch.zeros(0, dtype=torch.bool, device=points.device)
    if rule == 'winding':
        from . import winding
        return winding.points_inside(points, verts, faces)
    lo, hi = verts.amin(0), verts.amax(0)
    reach = 1.5 * (hi - lo).norm() + (points - 0.5 * (lo + hi)).norm(dim=1, keepdim=True)                    # [P,1]
    dirs = torch.tensor(INSIDE_DIRECTIONS, dtype=torch.float32, device=points.device)                        # [3,3]
    p = points[None].expand(3, P, 3).reshape(-1, 3)
    q = (points[None] + reach[None] * dirs[:, None, :]).reshape(-1, 3)
    grid = use_grid_for_segments(method, 3 * P, faces.shape[0])
    cnt = segment_hits(p, q, verts, faces, count=True, method='grid' if grid else 'brute')['count'].reshape(3, P)
    return (cnt & 1).sum(0) >= 2


@torch.no_grad()
def penetration(points, body_v, body_f, method='auto', rule='parity'):
    """How deep the points [P,3] f32 (a garment's vertices) lie inside the closed mesh body_v / body_f: a dict with `inside`
    [P] bool (points_inside), `depth` [P] f32 = the distance to the nearest point of the surface for the points inside and 0
    for the others (the closest-point query of this module, unchanged), `count` (points inside), `max_depth` and `mean_depth`
    (over the points inside; 0 when there are none) — python numbers, one read-back.  `rule`: points_inside's ('winding' takes a
    body with holes or of several overlapping pieces)."""
    inside = points_inside(points, body_v, body_f, method=method, rule=rule)
    if points.shape[0] == 0:
        return {'inside': inside, 'depth': points.new_zeros(0), 'count': 0, 'max_depth': 0., 'mean_depth': 0.}
    _, _, dist2 = _nearest(points.contiguous(), body_v.contiguous(), body_f.contiguous(), method)
    depth = torch.where(inside, dist2.sqrt(), torch.zeros_like(dist2))
    n = inside.sum()
    stats = torch.stack([n.double(), depth.max().double(), depth.double().sum() / n.clamp(min=1).double()]).cpu().tolist()
    return {'inside': inside, 'depth': depth, 'count': int(stats[0]), 'max_depth': stats[1], 'mean_depth': stats[2]}


def sample_surface(verts, faces, count, generator=None):
    """loop.sample_fan_mesh's samples (faces picked in proportion to their area by the inverse CDF, a uniform point of each
    from two uniforms reflected into the lower-left half of the unit square) with the picked faces: (points [count,3],
    face [count] int64)."""
    tri = verts[faces]                                                                     # [F,3,3]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area = 0.5 * torch.linalg.cross(e1, e2, dim=-1).norm(dim=-1)
    cum = torch.cumsum(area, 0)
    u = torch.rand(count, device=verts.device, generator=generator) * cum[-1]
    f = torch.searchsorted(cum, u).clamp_(max=faces.shape[0] - 1)
    r = torch.rand(count, 2, device=verts.device, generator=generator)
    r = torch.where((r.sum(1, keepdim=True) > 1.0), r - 1.0, r).abs()
    return tri[f, 0] + e1[f] * r[:, 0:1] + e2[f] * r[:, 1:2], f


def face_normals(verts, faces):
    """Unit face normals [F,3] f32 (zero for a face without area)."""
    tri = verts[faces]
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1)
    return torch.nan_to_num(n / n.norm(dim=-1, keepdim=True), nan=0., posinf=0., neginf=0.)


def use_grid(method, n_points, n_faces):
    if method not in ('auto', 'grid', 'brute'):
        raise ValueError("method must be 'auto', 'grid' or 'brute' (got %r)" % (method,))
    return method == 'grid' or (method == 'auto' and n_points * n_faces >= AUTO_GRID_MIN_TESTS)


def _nearest(p, verts, faces, method, grid=None):
    """(face, point, squared distance) of p on the mesh; `grid`: a MeshGrid of the mesh built before (recmv.align iterates)."""
    if use_grid(method, p.shape[0], faces.shape[0]):
        return (grid if grid is not None else MeshGrid(verts, faces)).closest_point(p)
    from .iso_remesh import closest_point
    return closest_point(p, verts, faces)


def _direction(p, src_face, src_v, src_f, dst_v, dst_f, thresholds, method):
    """Device scalars (float64) of one direction: mean d, mean d^2, max d, normal consistency, share of d <= t per t."""
    face, _, dist2 = _nearest(p, dst_v, dst_f, method)
    d2 = dist2.double()
    d = d2.sqrt()
    dots = (face_normals(src_v, src_f)[src_face] * face_normals(dst_v, dst_f)[face.clamp(min=0)]).double().sum(-1).abs()
    vals = [d.mean(), d2.mean(), d.max(), dots.mean()] + [(d <= float(t)).double().mean() for t in thresholds]
    return torch.stack(vals), face


@torch.no_grad()
def surface_distance(pred_v, pred_f, gt_v, gt_f, samples=100000, seed=0, thresholds=DEFAULT_THRESHOLDS, method='auto',
                     return_samples=False):
    """The metrics of the module docstring between the prediction (pred_v [V,3] f32, pred_f [F,3] int64) and the ground truth
    (CUDA tensors on one device): a dict of python floats.  `samples` surface samples per direction from a generator seeded
    with `seed` (the prediction's first).  `return_samples`: also {'pred': (points, source face, nearest face of the ground
    truth), 'gt': (…)}."""
    pred_v, pred_f = check_mesh(pred_v, pred_f, allow_empty=False)
    gt_v, gt_f = check_mesh(gt_v, gt_f, allow_empty=False)
    use_grid(method, 0, 0)
    if samples < 1:
        raise ValueError("surface_distance: at least one sample")
    gen = torch.Generator(device=pred_v.device).manual_seed(int(seed))
    thresholds = tuple(float(t) for t in thresholds)
    pp, pf = sample_surface(pred_v, pred_f, samples, gen)
    gp, gf = sample_surface(gt_v, gt_f, samples, gen)
    a, a_near = _direction(pp, pf, pred_v, pred_f, gt_v, gt_f, thresholds, method)
    c, c_near = _direction(gp, gf, gt_v, gt_f, pred_v, pred_f, thresholds, method)
    a, c = torch.stack([a, c]).cpu().tolist()                                     # the one read-back
    out = {'accuracy': a[0], 'accuracy_rms': math.sqrt(a[1]), 'accuracy_max': a[2],
           'completeness': c[0], 'completeness_rms': math.sqrt(c[1]), 'completeness_max': c[2],
           'chamfer_l1': 0.5 * (a[0] + c[0]), 'chamfer_l2': a[1] + c[1],
           'normal_consistency_pred_to_gt': a[3], 'normal_consistency_gt_to_pred': c[3],
           'normal_consistency': 0.5 * (a[3] + c[3])}
    for k, t in enumerate(thresholds):
        pr, rc = a[4 + k], c[4 + k]
        out['precision_%g' % t], out['recall_%g' % t] = pr, rc
        out['fscore_%g' % t] = 2. * pr * rc / (pr + rc) if pr + rc > 0 else 0.
    if return_samples:
        return out, {'pred': (pp, pf, a_near), 'gt': (gp, gf, c_near)}
    return out
