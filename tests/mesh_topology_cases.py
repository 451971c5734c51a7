"""The meshes and link sets of the topology tests (numpy; float32 vertices [V,3], int64 faces [F,3])."""
import numpy as np

TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)        # closed, consistently oriented (outward)


def tetrahedron(scale=1., shift=(0., 0., 0.)):
    return (TETRA_V * np.float32(scale) + np.asarray(shift, np.float32)).astype(np.float32), TETRA_F.copy()


def merge(*meshes):
    """The meshes side by side: vertices and faces appended in order."""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32))
        fs.append(np.asarray(f, np.int64) + base)
        base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int64)


def _grid_faces(n, m, wrap_m):
    """Two triangles per quad of an n (around, wrapped) x m grid of vertices j * n + i; the last row joins the first if wrap_m."""
    f = []
    for j in range(m if wrap_m else m - 1):
        for i in range(n):
            a, b = j * n + i, j * n + (i + 1) % n
            c, d = ((j + 1) % m) * n + i, ((j + 1) % m) * n + (i + 1) % n
            f += [[a, b, d], [a, d, c]]
    return np.array(f, np.int64)


def tube(n=12, m=5, radius=0.3, length=1.):
    """An open cylinder: two boundary loops, Euler characteristic 0, genus 0."""
    t = 2 * np.pi * np.arange(n) / n
    v = np.array([[radius * np.cos(a), radius * np.sin(a), length * j / (m - 1)] for j in range(m) for a in t], np.float32)
    return v, _grid_faces(n, m, False)


def torus(n=12, m=9, R=1., r=0.3):
    """Closed, genus 1."""
    v = np.array([[(R + r * np.cos(2 * np.pi * i / n)) * np.cos(2 * np.pi * j / m), (R + r * np.cos(2 * np.pi * i / n)) * np.sin(2 * np.pi * j / m),
                   r * np.sin(2 * np.pi * i / n)] for j in range(m) for i in range(n)], np.float32)
    return v, _grid_faces(n, m, True)


def pinched_tetrahedra():
    """Two tetrahedra that share one vertex: one piece by vertices, two by edges."""
    v = np.concatenate([TETRA_V, TETRA_V[1:] + np.float32(1.)]).astype(np.float32)
    second = np.array([3, 4, 5, 6])[TETRA_F]
    return v, np.concatenate([TETRA_F, second])


def hinged_tetrahedra():
    """Two tetrahedra that share the edge (2, 3): it has four faces."""
    v = np.concatenate([TETRA_V, np.array([[-1, 1, 1], [0, 2, 2]], np.float32)]).astype(np.float32)
    second = np.array([2, 3, 4, 5])[TETRA_F]
    return v, np.concatenate([TETRA_F, second])


def flipped(mesh, face=0):
    v, f = mesh
    f = f.copy()
    f[face] = f[face][::-1]
    return v, f


def floaters(count, seed=11, distance=3., size=0.01):
    """`count` small tetrahedra far from the origin, every one 7 % larger than the one before (no two areas tie)."""
    g = np.random.default_rng(seed)
    d = g.normal(size=(count, 3))
    d = distance * (1 + g.random((count, 1))) * d / np.linalg.norm(d, axis=1, keepdims=True)
    return merge(*[tetrahedron(size * 1.07 ** i, d[i]) for i in range(count)])


def strip_faces(n_faces, numbering, seed=5):
    """A triangle strip (i, i + 1, i + 2) over n_faces + 2 vertices numbered 'ascending', 'descending' or by a fixed random
    permutation: (faces [F,3], vertices)."""
    n = n_faces + 2
    p = np.arange(n)
    if numbering == 'descending':
        p = p[::-1].copy()
    elif numbering == 'random':
        p = np.random.default_rng(seed).permutation(n)
    i = np.arange(n_faces)
    return np.stack([p[i], p[i + 1], p[i + 2]], 1).astype(np.int64), n


def face_edges(f):
    """The rows (a, b), (b, c), (c, a) of faces as links [3 F, 2], face by face."""
    f = np.asarray(f, np.int64)
    return np.stack([f, np.roll(f, -1, 1)], 2).reshape(-1, 2)


def hub_faces(count=5000, hub=None):
    """`count` triangles that share one vertex and nothing else: (faces, vertices).  hub: its id (default: the last)."""
    n = 2 * count + 1
    hub = n - 1 if hub is None else hub
    other = np.array([x for x in range(n) if x != hub], np.int64).reshape(count, 2)
    return np.concatenate([np.full((count, 1), hub, np.int64), other], 1), n


def with_invalid_rows(links, n, every=7):
    """Every `every`-th row spoilt in turn by -1, by n, by a repeated neighbour, by a repeat of its first id."""
    l = np.array(links, np.int64)
    K = l.shape[1]
    for k, i in enumerate(range(0, len(l), every)):
        if k % 4 == 0:
            l[i, 0] = -1
        elif k % 4 == 1:
            l[i, K - 1] = n
        elif k % 4 == 2:
            l[i, 1] = l[i, 0]
        else:
            l[i, K - 1] = l[i, 0]
    return l
