"""recmv.holes restated in numpy float64 and python sets: the loops of a face table, the selection, the minimum-area
interval DP (vectorised over k and over the entries of one diagonal), the pre-order faces, the chord check and the
stitching.  numpy's + - * sqrt on float64 are correctly rounded and never contracted, so the DP's totals and split table
are the kernel's bit for bit."""
import numpy as np

MAX_LOOP_EDGES = 4096
STATUSES = ('filled', 'nonsimple', 'duplicate', 'max_edges', 'max_perimeter', 'keep_largest', 'too_large', 'nonfinite',
            'chord_conflict')


def tri_area(pi, pk, pj):
    """A(i,k,j) of float64 points [..., 3], in the module's operation order."""
    u, v = pk - pi, pj - pi
    cx = u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1]
    cy = u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2]
    cz = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def dp(points):
    """(W [n,n] float64, S [n,n] int) of points [n,3] f32: one diagonal at a time, every entry's candidates as one row."""
    P = np.asarray(points, np.float32).astype(np.float64)
    n = P.shape[0]
    W = np.zeros((n, n))
    S = np.zeros((n, n), np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for d in range(2, n):
            I = np.arange(n - d)[:, None]
            K = I + 1 + np.arange(d - 1)[None]
            J = I + d
            c = (W[I, K] + W[K, J]) + tri_area(P[I], P[K], P[J])
            c = np.where(np.isnan(c), np.inf, c)                   # a NaN never wins
            m = np.argmin(c, 1)                                    # the first minimum: ties to the lowest k
            i = np.arange(n - d)
            W[i, i + d] = c[i, m]
            S[i, i + d] = i + 1 + m                                # (all +inf: m = 0, k = i + 1)
    return W, S


def tree_faces(S, n):
    """Local (j, k, i) triples in pre-order of the split tree, by explicit positions."""
    out = np.zeros((n - 2, 3), np.int64)
    stack = [(0, n - 1, 0)]
    while stack:
        i, j, pos = stack.pop()
        k = int(S[i, j])
        out[pos] = (j, k, i)
        if k - i >= 2:
            stack.append((i, k, pos + 1))
        if j - k >= 2:
            stack.append((k, j, pos + 1 + (k - i - 1)))
    return out


def triangulate(points):
    """(local faces [n-2,3], weight) of one loop's points [n,3] f32."""
    W, S = dp(points)
    n = len(points)
    return tree_faces(S, n), W[0, n - 1]


def triangulate_loops(verts, loop_verts, loop_offsets):
    """(faces [total - 2L, 3] int64, weight [L] float64) — recmv.holes.triangulate_loops."""
    verts = np.asarray(verts, np.float32)
    lv, lo = np.asarray(loop_verts, np.int64), np.asarray(loop_offsets, np.int64)
    faces, weight = [], []
    for l in range(len(lo) - 1):
        ids = lv[lo[l]:lo[l + 1]]
        f, w = triangulate(verts[ids])
        faces.append(ids[f])
        weight.append(w)
    faces = np.concatenate(faces) if faces else np.zeros((0, 3), np.int64)
    return faces.reshape(-1, 3), np.array(weight, np.float64)


def valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1)
    return ok & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def find_loops(verts, faces):
    """(loops: lists of vertex ids, table {'edges', 'perimeter', 'status'}) with status 'open' | 'nonsimple' | 'duplicate'.
    ValueError for a mesh that is not edge-manifold or not consistently oriented."""
    verts = np.asarray(verts, np.float32)
    V = verts.shape[0]
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(f, V)]
    directed, undirected = {}, {}
    for a, b, c in f.tolist():
        for u, w in ((a, b), (b, c), (c, a)):
            directed[(u, w)] = directed.get((u, w), 0) + 1
            key = (min(u, w), max(u, w))
            undirected[key] = undirected.get(key, 0) + 1
    if any(c > 2 for c in undirected.values()):
        raise ValueError("not edge-manifold: repair.repair")
    if any(c > 1 for c in directed.values()):
        raise ValueError("not consistently oriented: repair.repair")
    succ, degree = {}, {}
    for (a, b) in directed:
        if undirected[(min(a, b), max(a, b))] == 1:
            succ.setdefault(a, []).append(b)
            degree[a] = degree.get(a, 0) + 1
            degree[b] = degree.get(b, 0) + 1
    for a in succ:
        succ[a].sort()
    face_sets = {tuple(sorted(t)) for t in f.tolist()}
    loops = []
    for start in sorted(succ):
        while succ[start]:
            loop, cur = [start], start
            while True:
                nxt = succ[cur].pop(0)                                # the lowest unused outgoing edge
                if nxt == start:
                    break
                loop.append(nxt)
                cur = nxt
            loops.append(loop)
    table = {'edges': [], 'perimeter': [], 'status': []}
    P = verts.astype(np.float64)
    for loop in loops:
        per = 0.
        for a, b in zip(loop, loop[1:] + loop[:1]):
            d = P[b] - P[a]
            per = per + float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        status = 'open'
        if any(degree[v] != 2 for v in loop):
            status = 'nonsimple'
        elif len(loop) == 3 and tuple(sorted(loop)) in face_sets:
            status = 'duplicate'
        table['edges'].append(len(loop))
        table['perimeter'].append(per)
        table['status'].append(status)
    return loops, table


def select(table, max_edges=None, max_perimeter=None, keep_largest=0):
    """The status of every loop after the selection: 'candidate' for the loops that go to the triangulation."""
    status = ['candidate' if s == 'open' else s for s in table['status']]
    n, per = table['edges'], table['perimeter']
    L = len(status)
    for l in range(L):
        if status[l] == 'candidate' and max_edges is not None and n[l] > max_edges:
            status[l] = 'max_edges'
    for l in range(L):
        if status[l] == 'candidate' and max_perimeter is not None and per[l] > max_perimeter:
            status[l] = 'max_perimeter'
    cand = sorted((l for l in range(L) if status[l] == 'candidate'), key=lambda l: (-per[l], l))
    for l in cand[:max(int(keep_largest), 0)]:
        status[l] = 'keep_largest'
    for l in range(L):
        if status[l] == 'candidate' and n[l] > MAX_LOOP_EDGES:
            status[l] = 'too_large'
    return status


def fill(verts, faces, max_edges=None, max_perimeter=None, keep_largest=0):
    """(verts, faces', info) — recmv.holes.fill without refine."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = verts.shape[0]
    loops, table = find_loops(verts, faces)
    status = select(table, max_edges, max_perimeter, keep_largest)
    edges = set()
    for t in faces[valid_faces(faces, V)].tolist():
        for u, w in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            edges.add((min(u, w), max(u, w)))
    L = len(loops)
    info = {'loops': L, 'edges': table['edges'], 'perimeter': table['perimeter'], 'status': status, 'patch_area': [None] * L,
            'faces_added': [0] * L, 'verts_added': [0] * L, 'face_start': [-1] * L, 'refine_rounds': 0, 'refine_capped': False}
    out, at = [faces], faces.shape[0]
    for l, loop in enumerate(loops):
        if status[l] != 'candidate':
            continue
        ids = np.array(loop, np.int64)
        local, w = triangulate(verts[ids])
        n = len(loop)
        if not np.isfinite(w):
            status[l] = 'nonfinite'
            continue
        conflict = False
        for j, k, i in local.tolist():
            for a, b in ((i, k), (k, j), (i, j)):
                border = (b - a == 1) or (a == 0 and b == n - 1)
                if not border and (min(loop[a], loop[b]), max(loop[a], loop[b])) in edges:
                    conflict = True
        if conflict:
            status[l] = 'chord_conflict'
            continue
        status[l] = 'filled'
        out.append(ids[local])
        info['patch_area'][l] = float(w)
        info['faces_added'][l] = n - 2
        info['face_start'][l] = at
        at += n - 2
    for s in STATUSES:
        info[s] = sum(1 for x in status if x == s)
    return verts, np.concatenate(out).reshape(-1, 3), info


def all_triangulations(i, j, area):
    """Every triangulation of the polygon i .. j as (list of (i, k, j) triples, total) (Catalan many); area(i, k, j) is a float,
    and a total is summed as the DP sums it: (left + right) + area."""
    if j - i < 2:
        return [([], 0.)]
    out = []
    for k in range(i + 1, j):
        for left, wl in all_triangulations(i, k, area):
            for right, wr in all_triangulations(k, j, area):
                out.append(([(i, k, j)] + left + right, (wl + wr) + area(i, k, j)))
    return out
