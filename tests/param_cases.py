"""The meshes of the parameterisation tests: (verts [V,3] float32, faces [F,3] int64) as numpy arrays, each with its reason."""
import numpy as np


def grid(n, m=None):
    """An n x m grid of unit squares in the plane z = 0, the diagonals alternating; vertex i * m + j at (i, j)."""
    m = n if m is None else m
    ii, jj = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    v = np.stack([ii, jj, np.zeros_like(ii)], -1).reshape(-1, 3).astype(np.float32)
    f = []
    for i in range(n - 1):
        for j in range(m - 1):
            a, b, c, d = i * m + j, (i + 1) * m + j, (i + 1) * m + j + 1, i * m + j + 1
            f += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return v, np.array(f, np.int64).reshape(-1, 3)


def planar_irregular(n=17, seed=5):
    """grid(n) with a jittered interior, rotated rigidly out of the plane: (verts, faces, the planar coordinates [V,2] float64).
    Every planar coordinate is a multiple of 25/64 and both rotations are 3-4-5, so the float32 vertices are the rotated
    points exactly: the mesh is planar to the last bit and the planar coordinates are an isometric uv."""
    _, f = grid(n)
    rng = np.random.RandomState(seed)
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    inner = (ii > 0) & (jj > 0) & (ii < n - 1) & (jj < n - 1)
    a = 16 * ii + np.where(inner, rng.randint(-5, 6, ii.shape), 0)
    b = 16 * jj + np.where(inner, rng.randint(-5, 6, ii.shape), 0)
    a, b = a.reshape(-1), b.reshape(-1)
    # (x, y) = 25 (a, b) / 64; about the x axis: (y, z) = (0.6 y, 0.8 y); then about the z axis: (x, y) = (0.6 x - 0.8 y, 0.8 x + 0.6 y)
    v = np.stack([15 * a - 12 * b, 20 * a + 9 * b, 20 * b], 1) / 64.           # integers below 2^24 over 64: exact in float32
    return v.astype(np.float32), f, np.stack([25 * a, 25 * b], 1) / 64.


def cap(n=17):
    """A spherical cap: grid(n) over [-0.7, 0.7]^2 lifted to the unit sphere; 289 vertices, curved, a disk."""
    v, f = grid(n)
    xy = (v[:, :2].astype(np.float64) / (n - 1) - 0.5) * 1.4
    z = np.sqrt(1. - (xy * xy).sum(1))
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32), f


def cylinder(k=16, rings=9, step=0.25):
    """An open cylinder of radius 1: `rings` rings of k vertices, vertex r * k + j; 2 loops, height (rings - 1) * step."""
    ang = 2. * np.pi * np.arange(k) / k
    v = np.array([[np.cos(a), np.sin(a), r * step] for r in range(rings) for a in ang], np.float32)
    f = []
    for r in range(rings - 1):
        for j in range(k):
            a, b = r * k + j, r * k + (j + 1) % k
            f += [[a, b, b + k], [a, b + k, a + k]]
    return v, np.array(f, np.int64)


def shirt(k=24, rings=15):
    """A sphere without its poles (neck, waist) and without the faces of two vertices on opposite sides (the arm holes):
    genus 0, 4 loops, 358 vertices."""
    v, f = [], []
    for r in range(rings):
        th = np.pi * (r + 1) / (rings + 1)
        for j in range(k):
            ph = 2. * np.pi * j / k
            v.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), 1.3 * np.cos(th)])
    for r in range(rings - 1):
        for j in range(k):
            a, b = r * k + j, r * k + (j + 1) % k
            f += [[a, a + k, b + k], [a, b + k, b]]
    v, f = np.array(v, np.float32), np.array(f, np.int64)
    drop = [4 * k, 4 * k + k // 2]
    f = f[~np.isin(f, drop).any(1)]
    keep = np.ones(v.shape[0], bool)
    keep[drop] = False
    new = np.cumsum(keep) - 1
    return v[keep], new[f]


def flawed():
    """grid(5) with an isolated vertex (25) and a face without area (0, 5, 10: three vertices of one grid line): a zero-weight
    row and an unusable face."""
    v, f = grid(5)
    v = np.concatenate([v, np.array([[9., 9., 9.]], np.float32)], 0)
    return v, np.concatenate([f, np.array([[0, 5, 10]], np.int64)], 0)


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)


def torus_strip(k=8, m=6):
    """A torus with the two faces of one square removed: genus 1, one loop."""
    v, f = [], []
    for i in range(k):
        for j in range(m):
            a, b = 2. * np.pi * i / k, 2. * np.pi * j / m
            v.append([(2. + np.cos(b)) * np.cos(a), (2. + np.cos(b)) * np.sin(a), np.sin(b)])
            p, q, r, s = i * m + j, ((i + 1) % k) * m + j, ((i + 1) % k) * m + (j + 1) % m, i * m + (j + 1) % m
            f += [[p, q, r], [p, r, s]]
    return np.array(v, np.float32), np.array(f[2:], np.int64)


def two_grids():
    v, f = grid(4)
    w = v.copy()
    w[:, 0] += 10.
    return np.concatenate([v, w], 0), np.concatenate([f, f + v.shape[0]], 0)


def fin():
    """Three faces on one edge: not edge-manifold."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)


# name -> (builder, reason); the disks are the cases of the solver and of the maps
DISKS = {
    "grid5": (lambda: grid(5), "25 vertices, 9 free: one partial slot"),
    "grid17": (lambda: grid(17), "289 vertices: two slots, the second partial"),
    "grid33": (lambda: grid(33), "1089 vertices: more than one pass of a 1024-thread workgroup"),
    "planar": (lambda: planar_irregular()[:2], "planar, irregular"),
    "cap": (lambda: cap(), "a curved disk"),
}
