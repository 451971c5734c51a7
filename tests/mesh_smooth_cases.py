"""The meshes of the smoothing tests (tests/test_mesh_smooth_cpu.py runs the float64 torch path on CPU tensors,
tests/test_gpu_mesh_smooth.py the kernel path) and what the quality tests measure on them.  numpy; float32 vertices, int64
faces.  tube, flat_grid and fan are mesh_simplify_cases', the two tetrahedron pairs mesh_topology_cases'."""
import numpy as np

import mesh_simplify_cases as SC
import mesh_topology_cases as TC

tube, flat_grid, fan = SC.tube, SC.flat_grid, SC.fan
hinged_tetrahedra, pinched_tetrahedra = TC.hinged_tetrahedra, TC.pinched_tetrahedra


def icosphere(level=3):
    """The unit icosphere: 10 * 4^level + 2 vertices, 20 * 4^level faces, outward."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [tuple(np.array(p, np.float64) / np.linalg.norm(p)) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = np.array(v[a]) + np.array(v[b])
                v.append(tuple(p / np.linalg.norm(p)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int64)


def mean_edge_length(v, f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return float(np.linalg.norm(v[e[:, 0]].astype(np.float64) - v[e[:, 1]], axis=1).mean())


def noisy_sphere(seed=7):
    """(noisy vertices, faces, clean vertices): the level-3 icosphere (642 vertices, 1 280 faces) with Gaussian noise of 0.2 x the
    mean edge length on every vertex."""
    v, f = icosphere(3)
    noise = np.random.default_rng(seed).standard_normal(v.shape) * (0.2 * mean_edge_length(v, f))
    return (v + noise).astype(np.float32), f, v


def cube(n=8):
    """The welded surface of the unit cube [0, 1]^3, n x n quads per side (n = 8: 386 vertices, 768 faces), outward."""
    ids, v, f = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(v)
            v.append(p)
        return ids[p]
    for axis in range(3):
        for side in (0, 1):
            for i in range(n):
                for j in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side * n, i + di, j + dj
                        q.append(vid(tuple(p)))
                    if not side:
                        q = q[::-1]
                    f += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return (np.array(v, np.float64) / n).astype(np.float32), np.array(f, np.int64)


def noisy_cube(seed=11, n=8):
    """(noisy vertices, faces, clean vertices): Gaussian noise of 0.1 x the cell size."""
    v, f = cube(n)
    noise = np.random.default_rng(seed).standard_normal(v.shape) * (0.1 / n)
    return (v + noise).astype(np.float32), f, v


def rms_radial_error(v):
    return float(np.sqrt(((np.linalg.norm(v.astype(np.float64), axis=1) - 1.) ** 2).mean()))


def rms_distance_to_unit_cube(v):
    """The root mean square distance of the points to the surface of [0, 1]^3."""
    p = v.astype(np.float64)
    outside = np.linalg.norm(p - np.clip(p, 0., 1.), axis=1)
    inside = np.minimum(p, 1. - p).min(1)                  # > 0 only inside
    return float(np.sqrt((np.where(outside > 0, outside, inside) ** 2).mean()))


def with_isolated_vertex(mesh):
    v, f = mesh
    return np.concatenate([v, [[5., 5., 5.]]]).astype(np.float32), f


def with_invalid_faces(mesh):
    """Three invalid faces (-1, V, a repeated corner), a corner that is not a number, and a last vertex whose only faces are
    invalid: (v, f, the vertex with the NaN, the vertex with invalid faces only)."""
    v, f = mesh
    v, f = v.copy(), f.copy()
    V = len(v)
    lonely = V
    v = np.concatenate([v, [[2., 2., 2.]]]).astype(np.float32)
    f[5, 0], f[17, 2] = -1, V + 1
    f = np.concatenate([f, [[lonely, lonely, 3]]]).astype(np.int64)
    nan_at = int(f[40, 1])
    v[nan_at, 1] = np.nan
    return v, f, nan_at, lonely
