"""The seeded meshes shared by tests/test_geodesic_cpu.py and tests/test_gpu_geodesic.py: (verts float32 [V,3], faces int64 [F,3])
as numpy arrays."""
import numpy as np


def triangle():
    return np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32), np.array([[0, 1, 2]], np.int64)


def square(through_source):
    """The unit square 0 (0,0), 1 (1,0), 2 (1,1), 3 (0,1), cut by the diagonal through vertex 0 or by the other one."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    f = [[0, 1, 2], [0, 2, 3]] if through_source else [[0, 1, 3], [1, 2, 3]]
    return v, np.array(f, np.int64)


def cylinder(n_around=24, n_rings=9, dz=0.25, radius=1.):
    """An open cylinder: ring r holds the vertices r * n_around .. and lies at height r * dz."""
    ang = 2. * np.pi * np.arange(n_around) / n_around
    v = np.array([[radius * np.cos(a), radius * np.sin(a), r * dz] for r in range(n_rings) for a in ang], np.float32)
    f = []
    for r in range(n_rings - 1):
        for i in range(n_around):
            a, b = r * n_around + i, r * n_around + (i + 1) % n_around
            f += [[a, b, a + n_around], [b, b + n_around, a + n_around]]
    return v, np.array(f, np.int64)


def grid(n, jitter=0., noise=0., seed=0, step=None):
    """n x n vertices on the unit square (or `step` apart) with alternating diagonals; vertex (i, j) is i * n + j.  `jitter`
    (in cells) moves the inner vertices in the plane and `noise` (absolute) lifts every vertex, both seeded."""
    step = 1. / (n - 1) if step is None else step
    rng = np.random.default_rng(seed)
    v = np.zeros((n, n, 3))
    v[..., 0], v[..., 1] = np.meshgrid(np.arange(n) * step, np.arange(n) * step, indexing="ij")
    if jitter:
        v[1:-1, 1:-1, :2] += rng.uniform(-jitter, jitter, (n - 2, n - 2, 2)) * step
    if noise:
        v[..., 2] = rng.uniform(-noise, noise, (n, n))
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
            f += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return v.reshape(-1, 3).astype(np.float32), np.array(f, np.int64)


def icosphere(level):
    """10 * 4^level + 2 vertices on the unit sphere: 42, 162, 642 for level 1, 2, 3."""
    t = (1. + 5. ** 0.5) / 2.
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    v = [list(np.array(p, np.float64) / np.linalg.norm(p)) for p in v]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = (np.array(v[a]) + np.array(v[b])) / 2.
                v.append(list(p / np.linalg.norm(p)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int64)


def fan(n=70):
    """n triangles around vertex 0 (valence n, more than a wave), the rim wavy in height."""
    ang = 2. * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(5 * ang)], 1)
    v = np.concatenate([np.zeros((1, 3)), rim]).astype(np.float32)
    f = [[0, 1 + i, 1 + (i + 1) % n] for i in range(n)]
    return v, np.array(f, np.int64)


def two_pieces():
    """A 6 x 6 grid and, apart from it, a 4 x 4 grid (vertices 36 ..)."""
    v0, f0 = grid(6)
    v1, f1 = grid(4)
    return np.concatenate([v0, v1 + np.float32([3, 0, 0])]), np.concatenate([f0, f1 + 36])


def broken():
    """A jittered 7 x 7 grid with a NaN vertex (24, the centre) and, appended, faces with an index out of range, a repeated
    corner, and without area (three collinear grid vertices; twice the same point through two vertex ids)."""
    v, f = grid(7, jitter=0.3, noise=0.02, seed=5)
    v = np.concatenate([v, v[10:11]])                      # vertex 49: a copy of vertex 10's point
    v[24, 1] = np.nan
    extra = [[0, 1, 49 + 1], [-1, 2, 3], [5, 5, 6], [8, 9, 8], [0, 7, 14], [10, 49, 11], [3, 4, 1 << 40]]
    return v, np.concatenate([f, np.array(extra, np.int64)])


def with_count(V):
    """A mesh of exactly V vertices: the largest square grid that fits, 0.01 apart, and a strip of triangles along its last
    row's far side for the rest."""
    n = int(np.floor(np.sqrt(V)))
    v, f = grid(n, step=0.01)
    extra = V - n * n
    ev, ef, prev = [], [], (n * n - 2, n * n - 1)          # the strip grows from the grid's last edge
    for i in range(extra):
        ev.append([0.01 * (n - 1) + 0.008 * (1 + i // 2), 0.01 * (n - 1) - 0.01 * (i % 2) + 0.002 * i / max(extra, 1), 0.])
        new = n * n + i
        ef.append([prev[0], prev[1], new])
        prev = (prev[1], new)
    if extra:
        v = np.concatenate([v, np.array(ev, np.float32)])
        f = np.concatenate([f, np.array(ef, np.int64)])
    assert v.shape[0] == V
    return v, f
