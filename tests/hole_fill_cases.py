"""The loops and meshes of the hole-filling tests, built in code with fixed seeds (numpy on the host)."""
import math
from functools import lru_cache

import numpy as np

LDS_MAX = 85                                               # recmv.holes.LDS_MAX_EDGES (test_hole_fill_cpu.py checks it)
AUTO_MAX = 64                                              # recmv.holes.AUTO_MAX_EDGES: n64 / n65 below sit on either side


def circle(n, noise=0., seed=0, radius=1.):
    t = 2. * math.pi * np.arange(n) / n
    p = np.stack([radius * np.cos(t), radius * np.sin(t), np.zeros(n)], 1)
    if noise:
        p = p + noise * np.random.default_rng(seed).standard_normal((n, 3))
    return p.astype(np.float32)


def loop_cases():
    """name -> points [n,3] f32, in a fixed order."""
    c = {}
    c['n3'] = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    c['n4_square'] = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)              # both diagonals tie
    c['n4_saddle'] = np.array([[0, 0, 0], [1, 0, 1], [1, 1, 0], [0, 1, 1]], np.float32)
    c['n4_saddle_long'] = np.array([[0, 0, 0], [1, 0, .25], [3, 3, 0], [0, 1, .25]], np.float32)
    c['n5'] = circle(5, .2, 5)
    c['n6_hexagon'] = circle(6)
    c['n7'] = circle(7, .2, 7)
    c['n8'] = circle(8, .3, 8)
    c['n16_convex'] = circle(16)                                                                     # near-ties everywhere
    c['n33'] = circle(33, .05, 33)
    c['n64'] = circle(64, .03, 64)
    c['n65'] = circle(65, .03, 65)
    c['n_lds'] = circle(LDS_MAX, .02, 85)
    c['n_lds_plus_1'] = circle(LDS_MAX + 1, .02, 86)
    c['n300'] = circle(300, .005, 300)
    rep = circle(9, .2, 9)
    rep[4] = rep[3]                                                                                  # zero-area triangles
    c['n9_repeated_point'] = rep
    nan = circle(10, .2, 10)
    nan[6, 1] = np.nan
    c['n10_nan'] = nan
    return c


def pack(point_sets):
    """(verts [sum n, 3] f32, loop_verts, loop_offsets) with the loops' vertices shuffled into one table by a fixed seed."""
    total = sum(len(p) for p in point_sets)
    perm = np.random.default_rng(1234).permutation(total)
    verts = np.zeros((total, 3), np.float32)
    lv, lo, at = [], [0], 0
    for p in point_sets:
        ids = perm[at:at + len(p)]
        verts[ids] = p
        lv.append(ids)
        at += len(p)
        lo.append(at)
    return verts, np.concatenate(lv).astype(np.int64), np.array(lo, np.int64)


def many_small_loops(count=200, seed=77):
    rng = np.random.default_rng(seed)
    return [circle(int(n), .25, int(s)) + rng.standard_normal(3).astype(np.float32)
            for n, s in zip(rng.integers(3, 13, count), rng.integers(0, 1 << 30, count))]


# ------------------------------------------------------------------------------------------------- meshes
@lru_cache(maxsize=None)
def icosphere(level):
    t = (1. + math.sqrt(5.)) / 2.
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / math.sqrt(1. + t * t) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int64)


def without_vertices(faces, ids):
    """The faces that touch none of the vertices ids."""
    return faces[~np.isin(faces, list(ids)).any(1)]


def ring(faces, vid):
    return sorted(set(faces[(faces == vid).any(1)].reshape(-1).tolist()) - {vid})


def holed_icosphere(level=1, vids=(0,)):
    """An icosphere without the fans of the vertices vids: one hole of 5 or 6 edges each (the vertices stay, unreferenced)."""
    v, f = icosphere(level)
    return v, without_vertices(f, vids)


def icosphere_hole12():
    """Level 2 without a valence-6 vertex and its ring: one hole of 12 edges."""
    v, f = icosphere(2)
    vid = next(i for i in range(12, v.shape[0]) if len(ring(f, i)) == 6 and all(len(ring(f, j)) == 6 for j in ring(f, i)))
    return v, without_vertices(f, [vid] + ring(f, vid))


def cylinder(segments=16, rows=3, radius=1., height=2.):
    """An open cylinder, outward oriented: two boundary loops of `segments` edges."""
    v, f = [], []
    for r in range(rows):
        for s in range(segments):
            t = 2. * math.pi * s / segments
            v.append((radius * math.cos(t), radius * math.sin(t), height * r / (rows - 1)))
    for r in range(rows - 1):
        for s in range(segments):
            a, b = r * segments + s, r * segments + (s + 1) % segments
            c, d = a + segments, b + segments
            f += [(a, b, d), (a, d, c)]
    return np.array(v, np.float32), np.array(f, np.int64)


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)
    return v, f


def mesh_cases():
    """name -> (verts, faces, fill keyword arguments)."""
    c = {}
    c['icosphere_one_hole'] = holed_icosphere(1, (0,)) + ({},)
    v, f = icosphere(1)
    far = 12 + int(np.argmin(v[12:] @ v[0]))                                 # a valence-6 vertex on the other side
    c['icosphere_two_holes'] = (v, without_vertices(f, (0, far)), {})
    c['icosphere_two_holes_max_edges_5'] = (v, without_vertices(f, (0, far)), {'max_edges': 5})
    for k in (0, 1, 2):
        c['cylinder_keep_%d' % k] = cylinder() + ({'keep_largest': k},)
    v, f = tetrahedron()
    c['tetrahedron_minus_one'] = (v, f[:3], {})
    c['lone_triangle'] = (v, f[:1], {})
    c['tetrahedron_minus_two'] = (v, f[:2], {})
    c['bowtie'] = (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [-1, 0, 0], [-1, -1, 0]], np.float32),
                   np.array([[0, 1, 2], [0, 3, 4]], np.int64), {})
    c['closed'] = icosphere(1) + ({},)
    c['hole12_max_perimeter'] = icosphere_hole12() + ({'max_perimeter': 0.5},)
    return c
