"""Numpy restatement of the simplification kernels (csrc/mesh_simplify.hip) and a plain serial greedy quadric-error
simplifier — one heap, one collapse at a time — with the same quadrics, placement and refusals as recmv.simplify: the
independent yardstick of tests/test_mesh_simplify_cpu.py and tests/test_gpu_mesh_simplify.py.  Plain loops, no torch."""
import heapq

import numpy as np

U = 2.0 ** -53
FREE, STAY_A, STAY_B = 0, 1, 2
INVALID_COST = np.finfo(np.float64).max
PLANE_OPS = 24            # rounded operations between the f32 coordinates and one term w * p_i * p_j (normal, length, division,
#                           the plane's offset, the weight, two products) — an upper count


def gamma(n):
    return n * U / (1 - n * U)


def face_valid(row, V):
    a, b, c = (int(x) for x in row)
    return 0 <= a < V and 0 <= b < V and 0 <= c < V and a != b and a != c and b != c


def tables(v, f):
    """(vertex -> faces ascending, border rows (a, b, face) in edge order, vertex -> border rows ascending) of the valid faces."""
    V = len(v)
    vf = [[] for _ in range(V)]
    use = {}
    for k, row in enumerate(f):
        if not face_valid(row, V):
            continue
        for x in row:
            vf[int(x)].append(k)
        for i in range(3):
            a, b = int(row[i]), int(row[(i + 1) % 3])
            use.setdefault((min(a, b), max(a, b)), []).append(k)
    border = [(a, b, ks[0]) for (a, b), ks in sorted(use.items()) if len(ks) == 1]
    vb = [[] for _ in range(V)]
    for r, (a, b, _) in enumerate(border):
        vb[a].append(r)
        vb[b].append(r)
    return vf, border, vb, use


def _normal(v, row, dt):
    """(first corner, (b - a) x (c - a), the same with every product's magnitude: what the cross product's rounding scales with)."""
    a, b, c = (v[int(i)].astype(dt) for i in row)
    u, w = b - a, c - a
    return a, np.cross(u, w), np.abs(u[[1, 2, 0]] * w[[2, 0, 1]]) + np.abs(u[[2, 0, 1]] * w[[1, 2, 0]])


def face_plane(v, row, dt=np.float64):
    """((n, d), area, the plane's entries as magnitudes that bound their rounding: |u_j w_k| + |u_k w_j| for n_i, sum of those
    times |a_i| for d) of a valid face, None when it adds nothing."""
    a, n, nbar = _normal(v, row, dt)
    length = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    if not (length > 0 and np.isfinite(length)):
        return None
    n, nbar = n / length, nbar / length
    return np.array([n[0], n[1], n[2], -(n[0] * a[0] + n[1] * a[1] + n[2] * a[2])], dt), dt(0.5) * length, \
        np.array([nbar[0], nbar[1], nbar[2], (nbar * np.abs(a)).sum()], dt)


def border_plane(v, f, row, dt=np.float64):
    a, b, k = row
    _, n, nbar = _normal(v, f[k], dt)
    pa = v[a].astype(dt)
    e = v[b].astype(dt) - pa
    m = np.cross(n, e)
    mbar = nbar[[1, 2, 0]] * np.abs(e[[2, 0, 1]]) + nbar[[2, 0, 1]] * np.abs(e[[1, 2, 0]])
    length = np.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2])
    if not (length > 0 and np.isfinite(length)):
        return None
    m, mbar = m / length, mbar / length
    return np.array([m[0], m[1], m[2], -(m[0] * pa[0] + m[1] * pa[1] + m[2] * pa[2])], dt), e[0] * e[0] + e[1] * e[1] + e[2] * e[2], \
        np.array([mbar[0], mbar[1], mbar[2], (mbar * np.abs(pa)).sum()], dt)


def _outer(w, p):
    wp = w * p
    return np.array([wp[0] * p[0], wp[0] * p[1], wp[0] * p[2], wp[0] * p[3], wp[1] * p[1], wp[1] * p[2], wp[1] * p[3],
                     wp[2] * p[2], wp[2] * p[3], wp[3] * p[3]], p.dtype)


def vertex_quadrics(v, f, boundary_weight, dt=np.float64):
    """(Q [V,11], A [V,11]: the sums of the terms with every plane entry replaced by the magnitude its rounding scales with, terms [V]: how
    many planes each vertex added, invalid faces): the kernel's sums in the kernel's order, in `dt`."""
    V = len(v)
    vf, border, vb, _ = tables(v, f)
    Q, A, terms = np.zeros((V, 11), dt), np.zeros((V, 11), dt), np.zeros(V, np.int64)
    for i in range(V):
        for k in vf[i]:
            got = face_plane(v, f[k], dt)
            if got is None:
                continue
            p, area, pabs = got
            Q[i, :10] += _outer(area, p)
            Q[i, 10] += area
            A[i, :10] += _outer(area, pabs)
            A[i, 10] += area
            terms[i] += 1
        for r in vb[i]:
            got = border_plane(v, f, border[r], dt)
            if got is None:
                continue
            p, e2, pabs = got
            Q[i, :10] += _outer(dt(boundary_weight) * e2, p)
            A[i, :10] += _outer(dt(boundary_weight) * e2, pabs)
            terms[i] += 1
    return Q, A, terms, sum(0 if face_valid(row, V) else 1 for row in f)


def cost_at(q, p, dt=np.float64):
    """(x^T q x clamped at 0, the sum of its absolute terms) at the point p, the ten terms in the kernel's order, in `dt`."""
    q = q.astype(dt)
    x, y, z = (dt(t) for t in p)
    t = [q[0] * x * x, 2 * q[1] * x * y, 2 * q[2] * x * z, 2 * q[3] * x, q[4] * y * y, 2 * q[5] * y * z, 2 * q[6] * y, q[7] * z * z,
         2 * q[8] * z, q[9]]
    c = t[0]
    for s in t[1:]:
        c = c + s
    return (c if c > 0 else dt(0)), sum(abs(s) for s in t)


def candidates(q, pa, pb, reach):
    """The f32 candidates of a free edge in order: [solved or None, a, b, midpoint] (float64 arithmetic as in the kernel)."""
    q = q.astype(np.float64)
    da, db = pa.astype(np.float64), pb.astype(np.float64)
    mid = 0.5 * (da + db)
    e = db - da
    len2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    c00, c01, c02 = q[4] * q[7] - q[5] * q[5], q[2] * q[5] - q[1] * q[7], q[1] * q[5] - q[2] * q[4]
    c11, c12, c22 = q[0] * q[7] - q[2] * q[2], q[1] * q[2] - q[0] * q[5], q[0] * q[4] - q[1] * q[1]
    det = q[0] * c00 + q[1] * c01 + q[2] * c02
    solved = None
    if det != 0 and np.isfinite(det):
        r0, r1, r2 = -q[3], -q[6], -q[8]
        s = np.array([(c00 * r0 + c01 * r1 + c02 * r2) / det, (c01 * r0 + c11 * r1 + c12 * r2) / det,
                      (c02 * r0 + c12 * r1 + c22 * r2) / det])
        if np.all(np.abs(s) < 3.0e38):
            sf = s.astype(np.float32)
            d = sf.astype(np.float64) - mid
            if d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= (reach * reach) * len2:
                solved = sf
    return [solved, pa.astype(np.float32), pb.astype(np.float32), mid.astype(np.float32)]


def collapse_one(Q, v, a, b, code, reach):
    """(pos f32 [3], cost, weight) of one valid edge."""
    q = Q[a] + Q[b]
    if code == STAY_A:
        cands = [v[a]]
    elif code == STAY_B:
        cands = [v[b]]
    else:
        cands = [c for c in candidates(q, v[a], v[b], reach) if c is not None]
    best, best_cost = None, None
    for c in cands:
        cost = cost_at(q, c)[0]
        if best is None or cost < best_cost:
            best, best_cost = np.asarray(c, np.float32), cost
    return best, float(best_cost), float(q[10])


def edge_collapse_cost(Q, v, edges, code, reach):
    E, V = len(edges), len(v)
    pos, cost, weight, invalid = np.zeros((E, 3), np.float32), np.zeros(E), np.zeros(E), 0
    for i, (a, b) in enumerate(edges):
        a, b = int(a), int(b)
        if not (0 <= a < V and 0 <= b < V and a != b):
            cost[i], invalid = INVALID_COST, invalid + 1
            continue
        pos[i], cost[i], weight[i] = collapse_one(Q, v, a, b, int(code[i]), reach)
    return pos, cost, weight, invalid


def flip_one(v, f, vf, a, b, p, dt=np.float64, dots=None):
    for end in (a, b):
        for k in vf[end]:
            row = [int(x) for x in f[k]]
            if a in row and b in row:
                continue
            c = [v[i].astype(dt) for i in row]
            n_old = np.cross(c[1] - c[0], c[2] - c[0])
            c = [np.asarray(p, np.float32).astype(dt) if i == end else x for i, x in zip(row, c)]
            n_new = np.cross(c[1] - c[0], c[2] - c[0])
            dot = n_old[0] * n_new[0] + n_old[1] * n_new[1] + n_old[2] * n_new[2]
            if dots is not None:
                dots.append(float(dot))
            if not dot > 0:
                return False
    return True


def collapse_flip_check(v, f, edges, pos):
    V = len(v)
    vf = tables(v, f)[0]
    return np.array([0 <= int(a) < V and 0 <= int(b) < V and int(a) != int(b) and flip_one(v, f, vf, int(a), int(b), pos[i])
                     for i, (a, b) in enumerate(edges)], bool)


# ------------------------------------------------------------------------------------------------- serial greedy
class _Mesh:
    def __init__(self, v, f):
        self.v = np.array(v, np.float32)
        self.f = [[int(x) for x in row] for row in f]
        self.alive = [True] * len(self.f)
        self.vf = [set() for _ in range(len(v))]
        for k, row in enumerate(self.f):
            for x in row:
                self.vf[x].add(k)

    def nbrs(self, a):
        return {x for k in self.vf[a] for x in self.f[k]} - {a}

    def edge_faces(self, a, b):
        return self.vf[a] & self.vf[b]

    def on_border(self, a):
        return any(len(self.edge_faces(a, w)) == 1 for w in self.nbrs(a))

    def loop_length(self, a, b):
        """The edges of the boundary loop through the boundary edge (a, b)."""
        prev, cur, n = a, b, 1
        while cur != a and n <= len(self.v):
            nxt = [w for w in sorted(self.nbrs(cur)) if w != prev and len(self.edge_faces(cur, w)) == 1]
            if not nxt:
                return n
            prev, cur, n = cur, nxt[0], n + 1
        return n


def greedy_simplify(v, f, target_faces, boundary_weight, reach, max_error=None):
    """The cheapest valid collapse, one at a time, until the mesh has target_faces faces (or one more, or nothing is left):
    (verts, faces, collapses).  The heap holds (cost, a, b) with the versions of both ends; a collapse re-prices the edges of the
    vertex that stays.  Whether an edge may collapse is asked when it is popped; one that may not waits at its ends and
    returns to the heap when a collapse changes the ring of either."""
    m = _Mesh(v, f)
    Q = vertex_quadrics(m.v, np.asarray(f), boundary_weight)[0]
    version = [0] * len(m.v)
    border = [m.on_border(a) for a in range(len(m.v))]      # a collapse changes it at the vertex that stays only
    waiting = [[] for _ in range(len(m.v))]
    n_faces = len(m.f)
    heap = []

    def price(a, b):
        """(pos, cost, weight) of (a, b), a < b, or None for an interior edge between two boundary vertices."""
        bnd = len(m.edge_faces(a, b)) == 1
        if not bnd and border[a] and border[b]:
            return None
        code = STAY_A if bnd or (border[a] and not border[b]) else (STAY_B if border[b] and not border[a] else FREE)
        return collapse_one(Q, m.v, a, b, code, reach)

    def allowed(a, b, pos):
        shared = m.edge_faces(a, b)
        if len(shared) not in (1, 2) or len(m.nbrs(a) & m.nbrs(b)) != len(shared):      # manifold, link condition
            return False
        if len(shared) == 1 and m.loop_length(a, b) <= 3:
            return False
        if not border[a] and not border[b] and len(m.nbrs(a)) == 3 and len(m.nbrs(b)) == 3:    # an edge of a tetrahedron
            return False
        return flip_one(m.v, m.f, m.vf, a, b, pos)

    def push(a, b):
        a, b = min(a, b), max(a, b)
        got = price(a, b)
        if got is not None and not (max_error is not None and got[1] > max_error * max_error * got[2]):
            heapq.heappush(heap, (got[1], a, b, version[a], version[b]))

    for a in range(len(m.v)):
        for b in m.nbrs(a):
            if a < b:
                push(a, b)
    collapses = 0
    while heap and n_faces > target_faces:
        entry = heapq.heappop(heap)
        cost, a, b, sa, sb = entry
        if version[a] != sa or version[b] != sb:
            continue
        pos = price(a, b)[0]
        takes = len(m.edge_faces(a, b))
        if takes > n_faces - target_faces:
            continue
        if not allowed(a, b, pos):
            waiting[a].append(entry)
            waiting[b].append(entry)
            continue
        for k in list(m.edge_faces(a, b)):
            m.alive[k] = False
            for x in m.f[k]:
                m.vf[x].discard(k)
        for k in list(m.vf[b]):
            m.f[k] = [a if x == b else x for x in m.f[k]]
            m.vf[a].add(k)
        m.vf[b] = set()
        m.v[a] = pos
        Q[a] = Q[a] + Q[b]
        border[a] = border[a] or border[b]
        n_faces -= takes
        collapses += 1
        version[a] += 1
        version[b] += 1
        ring = m.nbrs(a)
        for w in ring:
            push(a, w)
        back = set()
        for x in ring | {a, b}:
            back.update(waiting[x])
            waiting[x] = []
        for e in back:
            if version[e[1]] == e[3] and version[e[2]] == e[4]:
                heapq.heappush(heap, e)
    faces = np.array([row for k, row in enumerate(m.f) if m.alive[k]], np.int64).reshape(-1, 3)
    used = np.zeros(len(m.v), bool)
    used[faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return m.v[used], remap[faces], collapses
