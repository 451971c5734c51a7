"""A host restatement of the generalized winding number (csrc/winding.hip, csrc/solid_angle.h, recmv/winding.py) for the tests:
the exact sum in float64, the same sum with float32 terms (the kernels' arithmetic), and the pyramid — its binning, its node
sums, its accept rule and its traversal — in float64.  numpy throughout, except the all-pairs terms, which are element-wise
operations on CPU tensors so that they spread over the cores.  Nothing here reads the code under test.

Measured with this file alone (tests/test_winding_cpu.py re-measures and pins the figures), on the five meshes and lattices of
CASES and on the queries that lie at least 1e-3 box diagonals from the surface:

    mesh        nodes   far enough   max |w32 - w64|   pyramid beta=2   pyramid beta=3   levels   within 0.05 of |w| = 1/2
    body        15525     15479        1.5e-07          0.0159           0.0077          3        0.00 %
    cap_z       15525     15486        1.5e-07          0.0150           0.0061          3        0.80 %
    cap_x       15525     15488        1.6e-07          0.0144           0.0063          3        0.84 %
    torus       18375     18230        3.3e-06          0.0154           0.0077          3        0.00 %
    two_bodies  18900     18796        1.9e-07          0.02643          0.01047         4        0.00 %

(cap_z, cap_x: the body without the faces whose centroid has z >= 0.3, x >= 0.3; two_bodies: two bodies 0.3 apart along x.)  On
the closed meshes w64 is an integer to 3e-15.  At beta = 3 the pyramid rule spends 83 .. 268 dipoles and 57 .. 204 exact faces
per query on these meshes of 768 .. 2560 faces; at beta = 2, 49 .. 126 and 17 .. 86.

TOL_EXACT = 8 x the largest |w32 - w64| (the margin covers a device atan2f that is not numpy's and the contraction of
multiply-adds that the kernels forbid but a compiler's library may not).  TOL_TREE[beta] = 2 x the largest error of the
pyramid rule in float64 against the exact float64 + TOL_EXACT (the factor 2 covers accept decisions that tip the other way in
f32 at a tie).  Flags are compared where ||w64| - 1/2| exceeds the tolerance of the route; the nodes left out stay below UNDECIDED_CAP = 3 %
(at most 0.9 % at TOL_TREE[2]).  TOL_TREE[3] is below 0.05, so DEFAULT_BETA stays 3.
"""
import functools
import math

import numpy as np

MEASURED_F32 = 3.3e-6            # the largest |w32 - w64| above (the torus, whose lattice has nodes 1.1e-3 diagonals from the surface)
MEASURED_TREE = {2.: 0.02643, 3.: 0.01047}                     # the largest pyramid errors above (two_bodies)
TOL_EXACT = 8 * MEASURED_F32
TOL_TREE = {beta: 2 * e + TOL_EXACT for beta, e in MEASURED_TREE.items()}       # 0.0529, 0.0210
DEFAULT_BETA = 3.
SURFACE_MARGIN = 1e-3            # in box diagonals
DECISION_MARGIN = 0.05           # a flag is compared only where ||w64| - 1/2| > this
UNDECIDED_CAP = 0.03
MAX_LEVELS = 7
FACES_PER_CELL = 8
FOUR_PI = 4. * math.pi


# ------------------------------------------------------------------------------------------------------------ the sums
def _terms(q, tri, dtype):
    """Omega [Q, F] of the faces tri [F, 3, 3] seen from q [Q, 3], every operation rounded to `dtype`, in the kernels' order
    (CPU tensors: element-wise operations, each rounded once, spread over the cores)."""
    import torch
    dt = torch.float32 if dtype == np.float32 else torch.float64
    q, tri = torch.from_numpy(np.array(q)).to(dt), torch.from_numpy(np.array(tri)).to(dt)
    a, b, c = ([tri[None, :, i, k] - q[:, None, k] for k in range(3)] for i in range(3))
    la, lb, lc = (torch.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) for x in (a, b, c))
    det = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]))
    dot = lambda x, y: x[0] * y[0] + x[1] * y[1] + x[2] * y[2]  # noqa: E731
    den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
    out = 2 * torch.atan2(det, den)
    assert out.dtype == dt
    return out.numpy()


def corners(verts, faces):
    """[F', 3, 3] float32 corners of the faces with every index inside [0, V): the others contribute 0."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int64)
    ok = ((faces >= 0) & (faces < len(verts))).all(1)
    return verts[faces[ok]]


def winding(points, verts, faces, terms=np.float64, block=512):
    """w [P] float64: the terms in `terms` (np.float64: the judge; np.float32: the kernels' arithmetic), the sum in float64."""
    tri, points = corners(verts, faces), np.asarray(points, np.float32)
    out = np.zeros(len(points))
    if len(tri):
        for s in range(0, len(points), block):
            out[s:s + block] = _terms(points[s:s + block], tri, terms).astype(np.float64).sum(1)
    out[~np.isfinite(points).all(1)] = np.nan
    return out / FOUR_PI


def inside(w, threshold=0.5):
    return np.abs(w) > threshold


def decided(w64, margin=DECISION_MARGIN):
    return np.abs(np.abs(w64) - 0.5) > margin


# ---------------------------------------------------------------------------------------------------------- the pyramid
def cube(verts, faces):
    """(origin [3] f32, side f32): recmv.winding.WindingTree's cube — centred on the box of the vertices the faces use, 1.001
    times its longest extent."""
    verts = np.asarray(verts, np.float32)
    used = verts[np.clip(np.asarray(faces, np.int64), 0, len(verts) - 1).reshape(-1)]
    lo, hi = used.min(0).astype(np.float64), used.max(0).astype(np.float64)
    ext = float((hi - lo).max())
    side = ext * (1. + 1e-3) if ext > 0. else max(float(np.abs(used).max()), 1.) * 1e-3
    return (0.5 * (lo + hi) - 0.5 * side).astype(np.float32), np.float32(side)


def cells(tri, origin, side, levels):
    """The finest cell (i, j, k) [F, 3] of each face's centroid, in the kernels' f32 arithmetic."""
    n = 1 << levels
    tri = tri.astype(np.float32)
    cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / np.float32(3)
    t = np.floor((cen - np.asarray(origin, np.float32)) / (np.float32(side) / np.float32(n)))
    return np.clip(t, 0, n - 1).astype(np.int64)


def choose_levels(tri, origin, side):
    if len(tri) == 0:
        return 1
    ijk = cells(tri, origin, side, MAX_LEVELS)
    for l in range(1, MAX_LEVELS + 1):
        c = ijk >> (MAX_LEVELS - l)
        if len(tri) <= FACES_PER_CELL * len(np.unique((c[:, 0] << (2 * l)) + (c[:, 1] << l) + c[:, 2])):
            return l
    return MAX_LEVELS


class Pyramid:
    """The dense pyramid in float64: level l is a dict of arrays of shape [2^l, 2^l, 2^l(, 3)]."""

    def __init__(self, verts, faces, levels=None, origin=None, side=None):
        self.tri = corners(verts, faces)
        if origin is None:
            origin, side = cube(verts, faces)
        self.origin, self.side = np.asarray(origin, np.float32), np.float32(side)
        self.levels = L = choose_levels(self.tri, self.origin, self.side) if levels is None else int(levels)
        tri = self.tri.astype(np.float64)
        n = 1 << L
        ijk = cells(self.tri, self.origin, self.side, L)
        flat = (ijk[:, 0] * n + ijk[:, 1]) * n + ijk[:, 2]
        self.order = np.argsort(flat, kind='stable')
        self.start = np.searchsorted(flat[self.order], np.arange(n ** 3 + 1))
        nvec = 0.5 * np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        area = np.linalg.norm(nvec, axis=1)
        cen = tri.sum(1) / 3.
        lv = {'count': np.zeros(n ** 3, np.int64), 'area': np.zeros(n ** 3), 'csum': np.zeros((n ** 3, 3)), 'N': np.zeros((n ** 3, 3)),
              'lo': np.full((n ** 3, 3), np.inf), 'hi': np.full((n ** 3, 3), -np.inf)}
        np.add.at(lv['count'], flat, 1)
        np.add.at(lv['area'], flat, area)
        np.add.at(lv['csum'], flat, area[:, None] * cen)
        np.add.at(lv['N'], flat, nvec)
        np.minimum.at(lv['lo'], flat, tri.min(1))
        np.maximum.at(lv['hi'], flat, tri.max(1))
        self.level = [None] * (L + 1)
        self.level[L] = {k: x.reshape((n, n, n) + x.shape[1:]) for k, x in lv.items()}
        for l in range(L - 1, -1, -1):
            c, m = self.level[l + 1], 1 << l
            kids = lambda x: x.reshape((m, 2, m, 2, m, 2) + x.shape[3:])  # noqa: E731
            self.level[l] = {'count': kids(c['count']).sum((1, 3, 5)), 'area': kids(c['area']).sum((1, 3, 5)),
                             'csum': kids(c['csum']).sum((1, 3, 5)), 'N': kids(c['N']).sum((1, 3, 5)),
                             'lo': kids(c['lo']).min((1, 3, 5)), 'hi': kids(c['hi']).max((1, 3, 5))}

    def centre_radius(self, l, cell):
        """(centre [K, 3], r [K]) of the nodes cell [K, 3] of level l (which hold faces)."""
        lv, idx = self.level[l], (cell[:, 0], cell[:, 1], cell[:, 2])
        area, lo, hi = lv['area'][idx], lv['lo'][idx], lv['hi'][idx]
        centre = np.where((area > 0)[:, None], lv['csum'][idx] / np.where(area > 0, area, 1.)[:, None], 0.5 * (lo + hi))
        r = np.linalg.norm(np.maximum(centre - lo, hi - centre), axis=1)
        return centre, r

    def query(self, points, beta=DEFAULT_BETA, stats=None):
        """w [P] float64 by the pyramid rule: a node with |q - centre| > beta r contributes N . (centre - q) / |centre - q|^3, any
        other is descended into, the faces of a finest cell are summed exactly.  Level by level instead of depth-first: the
        same set of terms.  `stats` (a dict) receives the numbers of dipoles and of exact faces."""
        points = np.asarray(points, np.float32)
        q = points.astype(np.float64)
        P, tri = len(q), self.tri.astype(np.float64)
        total = np.zeros(P)
        dipoles = faces = 0
        live = np.isfinite(q).all(1)
        qi, cell = np.nonzero(live)[0], np.zeros((int(live.sum()), 3), np.int64)
        offsets = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
        for l in range(self.levels + 1):
            keep = self.level[l]['count'][cell[:, 0], cell[:, 1], cell[:, 2]] > 0
            qi, cell = qi[keep], cell[keep]
            centre, r = self.centre_radius(l, cell)
            d = centre - q[qi]
            dist = np.linalg.norm(d, axis=1)
            far = dist > beta * r
            N = self.level[l]['N'][cell[far, 0], cell[far, 1], cell[far, 2]]
            np.add.at(total, qi[far], (N * d[far]).sum(1) / dist[far] ** 3)
            dipoles += int(far.sum())
            qi, cell = qi[~far], cell[~far]
            if l < self.levels:
                qi = np.repeat(qi, 8)
                cell = (2 * cell[:, None, :] + offsets[None]).reshape(-1, 3)
        n = 1 << self.levels
        flat = (cell[:, 0] * n + cell[:, 1]) * n + cell[:, 2]
        cnt = self.start[flat + 1] - self.start[flat]
        faces += int(cnt.sum())
        for s in range(0, len(qi), 4096):                    # the near finest cells, exactly
            c, f0, k = cnt[s:s + 4096], self.start[flat[s:s + 4096]], qi[s:s + 4096]
            pair_q = np.repeat(k, c)
            pair_f = self.order[np.repeat(f0, c) + (np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c))]
            np.add.at(total, pair_q, _pair_terms(q[pair_q], tri[pair_f]))
        if stats is not None:
            stats.update({'dipoles': dipoles / max(P, 1), 'faces': faces / max(P, 1)})
        total[~live] = np.nan
        return total / FOUR_PI


def _pair_terms(q, tri):
    """Omega [K] of face tri[k] seen from q[k], float64."""
    a, b, c = (tri[:, i] - q for i in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=1) for x in (a, b, c))
    det = (a * np.cross(b, c)).sum(1)
    den = la * lb * lc + (a * b).sum(1) * lc + (b * c).sum(1) * la + (c * a).sum(1) * lb
    return 2. * np.arctan2(det, den)


# ------------------------------------------------------------------------------------------------------------ the cases
CAP = 0.3
TWO_BODIES_OFFSET = 0.3
TWO_BODIES_DIMS = (28, 25, 27)
NAMES = ('body', 'cap_z', 'cap_x', 'torus', 'two_bodies')
CLOSED = ('body', 'torus', 'two_bodies')


def drop_cap(v, f, axis):
    """The faces whose centroid's coordinate `axis` is below CAP."""
    cen = v[f].mean(1)
    return f[cen[:, axis] < CAP]


@functools.lru_cache(maxsize=None)
def case(name):
    """(verts f32 [V,3], faces int64 [F,3], lattice) as numpy arrays and a recmv.voxelize.Lattice (plain python: no GPU)."""
    import torch
    import test_voxelize_cpu as TV
    if name == 'torus':
        v, f = TV.torus()
        return v.numpy(), f.numpy(), TV.torus_lattice(v)
    v, f = TV.body()
    lat = TV.body_lattice(v)
    v, f = v.numpy(), f.numpy()
    if name == 'cap_z':
        f = drop_cap(v, f, 2)
    elif name == 'cap_x':
        f = drop_cap(v, f, 0)
    elif name == 'two_bodies':
        lat = TV.body_lattice(torch.from_numpy(v), TWO_BODIES_DIMS)
        v2 = v.copy()
        v2[:, 0] += np.float32(TWO_BODIES_OFFSET)
        v, f = np.concatenate([v, v2]), np.concatenate([f, f + len(v)])
    else:
        assert name == 'body', name
    return v, f, lat


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """The queries (every node of the case's lattice, [N,3] f32), w64 [N], and the mask of the nodes at least SURFACE_MARGIN
    box diagonals from the surface — computed once per process and shared."""
    import voxelize_reference as VR
    v, f, lat = case(name)
    pts = VR.nodes(lat.origin, lat.step, lat.dims)
    w64 = winding(pts, v, f, np.float64)
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
    # a point of a face lies within the longest edge of one of its corners: only the nodes nearer than that (and the margin) to
    # a vertex can be near the surface, and only they get the exact distance
    v64 = v.astype(np.float64)
    edge = max(float(np.linalg.norm(v64[f[:, i]] - v64[f[:, (i + 1) % 3]], axis=1).max()) for i in range(3))
    used = v64[np.unique(f)]
    near = np.zeros(len(pts), bool)
    for s in range(0, len(pts), 2048):
        d = np.linalg.norm(pts[s:s + 2048, None, :].astype(np.float64) - used[None], axis=2).min(1)
        near[s:s + 2048] = d < edge + SURFACE_MARGIN * diag
    far = np.ones(len(pts), bool)
    d2, _, _ = VR.band_distance(pts[near], v64, f, 1.)
    far[near] = d2 >= (SURFACE_MARGIN * diag) ** 2
    for x in (pts, w64, far):
        x.setflags(write=False)
    return pts, w64, far
