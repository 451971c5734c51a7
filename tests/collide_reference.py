"""Float64 numpy restatement of recmv.collide (csrc/mesh_collide.hip), written independently of the kernel's formulation: the
closest point of a triangle is the foot of the perpendicular when that lies inside the triangle, else the nearest of the
closest points of its three edges (clamped projections) — no Voronoi-region case analysis.  Pinned on hand-computed cases by
tests/test_animation_cpu.py and used as the judge of the GPU tests."""
import numpy as np


def _dot(a, b):
    return (a * b).sum(-1)


def _segment(p, a, b):
    """Closest point of segment ab to p (broadcast): (squared distance, parameter u in [0, 1])."""
    ab = b - a
    den = _dot(ab, ab)
    u = np.clip(_dot(p - a, ab) / np.where(den > 0, den, 1.), 0., 1.)
    d = p - (a + u[..., None] * ab)
    return _dot(d, d), u


def closest_on_triangle(p, a, b, c):
    """Broadcast over p / a / b / c [...,3] (float64): (squared distance, barycentric weights [...,3] of the closest point)."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    ab, ac, ap = b - a, c - a, p - a
    n = np.cross(ab, ac)
    nn = _dot(n, n)
    safe = np.where(nn > 0, nn, 1.)
    # barycentric coordinates of the foot of the perpendicular
    w1 = _dot(np.cross(ap, ac), n) / safe
    w2 = _dot(np.cross(ab, ap), n) / safe
    w0 = 1. - w1 - w2
    inside = (nn > 0) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
    d_in = _dot(ap, n) ** 2 / safe
    best_d = np.where(inside, d_in, np.inf)
    shape = best_d.shape
    best_w = np.stack([np.broadcast_to(w0, shape), np.broadcast_to(w1, shape), np.broadcast_to(w2, shape)], -1).copy()
    for (i, j), (x, y) in (((0, 1), (a, b)), ((0, 2), (a, c)), ((1, 2), (b, c))):       # edges ab, ac, bc in this order
        d, u = _segment(p, x, y)
        take = d < best_d
        w = np.zeros(shape + (3,))
        w[..., i], w[..., j] = 1. - u, u
        best_w = np.where(take[..., None], w, best_w)
        best_d = np.where(take, d, best_d)
    return best_d, best_w


def nearest(p, verts, faces, rows=256):
    """Brute force over the faces for every point of p [N,3]: (face [N] — the lowest index among equal minima —, squared
    distance [N], second-smallest squared distance over the faces [N] (inf for a single face), barycentric weights [N,3])."""
    p, verts = np.asarray(p, np.float64), np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    N = p.shape[0]
    face = np.zeros(N, np.int64)
    d1, d2, w = np.zeros(N), np.full(N, np.inf), np.zeros((N, 3))
    for s in range(0, N, rows):
        d, bw = closest_on_triangle(p[s:s + rows, None, :], a[None], b[None], c[None])
        i = d.argmin(1)
        r = np.arange(i.shape[0])
        face[s:s + rows], d1[s:s + rows], w[s:s + rows] = i, d[r, i], bw[r, i]
        if faces.shape[0] > 1:
            d[r, i] = np.inf
            d2[s:s + rows] = d.min(1)
    return face, d1, d2, w


def vertex_normals(verts, faces):
    """Unit vertex normals: the sum of the cross products of the incident faces (area weighted, pytorch3d's), float64."""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    fn = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    n = np.zeros_like(verts)
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)


def signed_distance(p, verts, faces, vnormals=None):
    """(s [N] = (p - q) . n with q the closest point and n the interpolated unit normal there, n [N,3], face [N])."""
    p, verts = np.asarray(p, np.float64), np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    vn = vertex_normals(verts, faces) if vnormals is None else np.asarray(vnormals, np.float64)
    face, _, _, w = nearest(p, verts, faces)
    tri = faces[face]
    q = (w[..., None] * verts[tri]).sum(1)
    n = (w[..., None] * vn[tri]).sum(1)
    n = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    return _dot(p - q, n), n, face


def push(p, verts, faces, eps, max_depth, vnormals=None):
    """One pass: (p_out [N,3], moved [N] bool, unresolved [N] bool, s [N])."""
    p = np.asarray(p, np.float64)
    s, n, _ = signed_distance(p, verts, faces, vnormals)
    unresolved = s < -max_depth
    moved = (s < eps) & ~unresolved
    out = np.where(moved[:, None], p + (eps - s)[:, None] * n, p)
    return out, moved, unresolved, s


def resolve(p, verts, faces, eps=2e-3, max_depth=3e-2, iters=3):
    """`iters` passes, stopping after one that moves nothing: (p_out, moved-at-least-once [N] bool, unresolved of the last pass
    [N] bool, passes run)."""
    p = np.asarray(p, np.float64)
    vn = vertex_normals(verts, faces)
    ever = np.zeros(p.shape[0], bool)
    passes = 0
    for _ in range(iters):
        p, moved, unresolved, _ = push(p, verts, faces, eps, max_depth, vn)
        ever |= moved
        passes += 1
        if not moved.any():
            break
    return p, ever, unresolved, passes
