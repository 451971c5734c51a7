"""The meshes and point clouds of the repair tests (numpy; float32 vertices [V,3], int64 faces [F,3]).  All of them are tiny."""
import numpy as np

import mesh_topology_cases as TC

WELD_EPS = 1e-3                                            # far below the icosphere's edge length (about 0.27)


def _by_first_use(v, f):
    """The mesh with its vertices numbered in the order the face table first uses them (what welding a soup and dropping the
    unused vertices gives)."""
    order = []
    seen = set()
    for i in f.reshape(-1).tolist():
        if i not in seen:
            seen.add(i)
            order.append(i)
    new = np.full(len(v), -1, np.int64)
    new[order] = np.arange(len(order))
    return v[order].astype(np.float32), new[f].astype(np.int64)


def icosphere(levels=2):
    """A unit icosphere, 20 * 4^levels faces (320), closed and consistently oriented, numbered by first use."""
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return _by_first_use(np.array(v, np.float32), np.array(f, np.int64))


def soup(mesh):
    """Every face given its own three vertices."""
    v, f = mesh
    return v[f.reshape(-1)].astype(np.float32), np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)


def jittered(mesh, eps=WELD_EPS, seed=3):
    """Every vertex moved by less than eps / 4 (at most eps / 8 along every axis, so by at most 0.217 eps)."""
    v, f = mesh
    g = np.random.default_rng(seed)
    return (v.astype(np.float64) + g.uniform(-eps / 8, eps / 8, v.shape)).astype(np.float32), f.copy()


def book():
    """Three free triangles on the edge (0, 1)."""
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, -1, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int64)


def every_third_flipped(mesh):
    v, f = mesh
    f = f.copy()
    f[::3] = f[::3][:, [0, 2, 1]]
    return v, f


def moebius(n=8):
    """A Moebius strip of 2 n faces: not orientable, one boundary loop."""
    v = []
    for i in range(n):
        a = 2 * np.pi * i / n
        for s in (-0.3, 0.3):
            r = 1 + s * np.cos(a / 2)
            v.append([r * np.cos(a), r * np.sin(a), s * np.sin(a / 2)])
    f = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        c, d = (2 * i + 2, 2 * i + 3) if i + 1 < n else (1, 0)       # the last quad joins the first with the sides swapped
        f += [[a, b, d], [a, d, c]]
    return np.array(v, np.float32), np.array(f, np.int64)


def tied_strip(n=6):
    """A closed strip (an open cylinder of 2 n faces) with every second face flipped: the two sides tie."""
    v, f = TC.tube(n=n, m=2)
    f = f.copy()
    f[1::2] = f[1::2][:, [0, 2, 1]]
    return v, f


def defects():
    """A tetrahedron and, behind it: an index of -1, an index of V, a repeated index, a face with a NaN corner, a zero-area face
    (three collinear integer points), and three faces on one vertex set, one of them reversed."""
    v = np.concatenate([TC.TETRA_V, np.array([[2, 0, 0], [4, 0, 0], [6, 0, 0], [np.nan, 1, 1], [2, 2, 0], [3, 2, 0], [2, 3, 1]],
                                              np.float32)]).astype(np.float32)
    V = len(v)
    extra = np.array([[0, 1, -1], [0, V, 2], [3, 3, 1], [0, 1, 7], [4, 5, 6], [8, 9, 10], [10, 9, 8], [9, 10, 8]], np.int64)
    return v, np.concatenate([TC.TETRA_F[:2], extra[:4], TC.TETRA_F[2:], extra[4:]])


def with_isolated_vertex():
    v, f = TC.tetrahedron()
    return np.concatenate([v[:2], np.array([[9, 9, 9]], np.float32), v[2:]]).astype(np.float32), np.where(f >= 2, f + 1, f)


def empty(V=0):
    return np.zeros((V, 3), np.float32), np.zeros((0, 3), np.int64)


def meshes():
    """name -> (verts, faces, weld eps or None, orientable)."""
    ico = icosphere()
    return {
        'icosphere': (*ico, None, True),
        'soup': (*soup(ico), 0., True),
        'jittered_soup': (*jittered(soup(ico)), WELD_EPS, True),
        'hinged_tetrahedra': (*TC.hinged_tetrahedra(), None, True),
        'pinched_tetrahedra': (*TC.pinched_tetrahedra(), None, True),
        'book': (*book(), None, True),
        'every_third_flipped': (*every_third_flipped(ico), None, True),
        'moebius': (*moebius(), None, False),
        'tied_strip': (*tied_strip(), None, True),
        'defects': (*defects(), None, True),
        'isolated_vertex': (*with_isolated_vertex(), 0., True),
        'empty': (*empty(0), 0., True),
        'no_faces': (*empty(3), 0., True),
    }


# ---- point clouds of the pair search ----------------------------------------------------------------------------------------------
def lattice(n=6, shift=0.):
    a = np.arange(n, dtype=np.float32) + np.float32(shift)
    return np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)


def clouds():
    """name -> (verts, eps, max_pairs or None)."""
    g = np.random.default_rng(17)
    out = {}
    out['V=0'] = (np.zeros((0, 3), np.float32), 0.5, None)
    out['V=1'] = (np.ones((1, 3), np.float32), 0.5, None)
    out['V=2'] = (np.array([[0, 0, 0], [0.25, 0, 0]], np.float32), 0.5, None)
    for V in (255, 256, 257):
        out['random V=%d' % V] = (g.random((V, 3)).astype(np.float32), 0.12, None)
    out['300 coincident'] = (np.tile(np.array([[0.5, -2., 3.]], np.float32), (300, 1)), 0., 44850)
    out['lattice'] = (lattice(), 1., None)
    out['lattice negative'] = (lattice(shift=-40.), 1., None)
    out['lattice straddling 0'] = (lattice(shift=-3.), 1., None)
    z = np.array([[0., 0., 0.], [-0., 0., -0.], [0., -0., 0.], [1., 0., 0.], [1., -0., 0.], [1., 0., 1e-30]], np.float32)
    out['signed zeros'] = (z, 0., None)
    bad = g.random((40, 3)).astype(np.float32)
    bad[3, 0], bad[9, 2], bad[17, 1], bad[30] = np.nan, np.inf, -np.inf, np.nan
    bad[4], bad[10], bad[31] = bad[5], bad[11], bad[32]                            # pairs next to the bad rows
    out['nan and inf'] = (bad, 0.2, None)
    far = np.concatenate([g.random((30, 3)) * 2e-6, g.random((30, 3)) * 2e-6 + 1e6]).astype(np.float32)
    out['two clusters 1e6 apart'] = (far, 1e-6, None)
    out['eps beyond the box'] = (g.random((64, 3)).astype(np.float32), 10., None)
    return out
