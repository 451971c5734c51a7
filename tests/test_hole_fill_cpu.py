"""Hole filling without a GPU: the numpy restatement against brute force and hand cases, the selection and every status, the
host-side loops of recmv.holes against the restatement, the refinement driver, the C ABI's argument checks and the CLI's
parser errors."""
import ctypes as C
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import hole_fill_cases as HC  # noqa: E402
import hole_fill_reference as HR  # noqa: E402
from recmv import holes as H  # noqa: E402
from recmv.connectivity import EdgeTable  # noqa: E402

LOOPS = HC.loop_cases()
MESHES = HC.mesh_cases()


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", [k for k, p in LOOPS.items() if len(p) <= 8 and np.isfinite(p).all()])
def test_dp_is_the_minimum_over_all_triangulations(name):
    pts = LOOPS[name]
    n = len(pts)
    local, weight = HR.triangulate(pts)
    P = pts.astype(np.float64)
    every = HR.all_triangulations(0, n - 1, lambda i, k, j: float(HR.tri_area(P[i], P[k], P[j])))
    assert len(every) == math.comb(2 * (n - 2), n - 2) // (n - 1) <= 132                        # Catalan
    best = min(total for _, total in every)
    assert weight == best                                                                        # the same areas, the same sums
    mine = {tuple(sorted(t)) for t in local.tolist()}
    assert any({tuple(sorted(t)) for t in tri} == mine for tri, total in every if total == best)


def test_hand_cases():
    local, w = HR.triangulate(LOOPS['n3'])
    assert local.tolist() == [[2, 1, 0]] and w == 0.5
    W, S = HR.dp(LOOPS['n4_square'])
    assert S[0, 3] == 1 and W[0, 3] == 1.0                                                       # both diagonals equal: lowest k
    assert HR.triangulate(LOOPS['n4_square'])[0].tolist() == [[3, 1, 0], [3, 2, 1]]              # pre-order
    # the non-planar saddle: folding along the short diagonal (1, 3) costs less area than along the long one (0, 2)
    pts = LOOPS['n4_saddle_long'].astype(np.float64)
    fold02 = HR.tri_area(pts[0], pts[1], pts[2]) + HR.tri_area(pts[0], pts[2], pts[3])
    fold13 = HR.tri_area(pts[0], pts[1], pts[3]) + HR.tri_area(pts[1], pts[2], pts[3])
    assert fold13 < fold02
    W, S = HR.dp(LOOPS['n4_saddle_long'])
    assert S[0, 3] == 1 and W[0, 3] == fold13                                                    # k = 1: the diagonal (1, 3)
    _, w = HR.triangulate(LOOPS['n6_hexagon'])
    assert abs(w - 1.5 * math.sqrt(3.)) < 1e-6                                                   # f32 corners
    _, w = HR.triangulate(LOOPS['n10_nan'])
    assert w == np.inf
    local, w = HR.triangulate(LOOPS['n9_repeated_point'])
    assert np.isfinite(w) and sorted(np.unique(local).tolist()) == list(range(9))


def test_preorder_positions():
    for name in ('n7', 'n16_convex', 'n33'):
        pts = LOOPS[name]
        n = len(pts)
        W, S = HR.dp(pts)
        out = []

        def walk(i, j):
            if j - i < 2:
                return
            k = int(S[i, j])
            out.append([j, k, i])
            walk(i, k)
            walk(k, j)
        walk(0, n - 1)
        assert HR.tree_faces(S, n).tolist() == out and len(out) == n - 2


# ------------------------------------------------------------------------------------------------- selection and statuses
def test_selection_order_and_ties():
    table = {'edges': [4, 10, 6, 6, 5000, 3], 'perimeter': [4., 9., 7., 7., 8., 1.],
             'status': ['open', 'open', 'open', 'open', 'open', 'nonsimple']}
    for select in (HR.select, H.select):
        assert select(table) == ['candidate'] * 4 + ['too_large', 'nonsimple']
        assert select(table, max_edges=6)[:5] == ['candidate', 'max_edges', 'candidate', 'candidate', 'max_edges']
        # max_edges first, then the perimeter, then the largest of what is left: on a tie the lower number stays open
        assert select(table, max_edges=6, max_perimeter=6.5, keep_largest=1) == [
            'keep_largest', 'max_edges', 'max_perimeter', 'max_perimeter', 'max_edges', 'nonsimple']
        assert select(table, keep_largest=3) == ['candidate', 'keep_largest', 'keep_largest', 'candidate', 'keep_largest',
                                                 'nonsimple']
        assert select(table, max_edges=100, keep_largest=2) == ['candidate', 'keep_largest', 'keep_largest', 'candidate',
                                                                'max_edges', 'nonsimple']
    assert H.MAX_LOOP_EDGES == HR.MAX_LOOP_EDGES and H.STATUSES == HR.STATUSES


EXPECTED = {'icosphere_one_hole': ['filled'], 'icosphere_two_holes': ['filled', 'filled'],
            'icosphere_two_holes_max_edges_5': ['max_edges', 'filled'], 'cylinder_keep_0': ['filled', 'filled'],
            'cylinder_keep_1': ['keep_largest', 'filled'], 'cylinder_keep_2': ['keep_largest', 'keep_largest'],
            'tetrahedron_minus_one': ['filled'], 'lone_triangle': ['duplicate'], 'tetrahedron_minus_two': ['chord_conflict'],
            'bowtie': ['nonsimple', 'nonsimple'], 'closed': [], 'hole12_max_perimeter': ['max_perimeter']}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_reference_fill_statuses(name):
    v, f, kw = MESHES[name]
    ov, of, info = HR.fill(v, f, **kw)
    assert info['status'] == EXPECTED[name]
    assert np.array_equal(of[:len(f)], f) and ov is not None
    assert len(of) == len(f) + sum(info['faces_added'])
    if name == 'cylinder_keep_1':                          # equal perimeters or not, the longer (on a tie the lower) stays open
        per = info['perimeter']
        assert per[0] >= per[1]
    if name in ('icosphere_one_hole', 'icosphere_two_holes', 'cylinder_keep_0', 'tetrahedron_minus_one'):
        table = EdgeTable(torch.from_numpy(of), len(v))
        assert int(table.count.min()) == 2 == int(table.count.max())                             # closed and edge-manifold
        assert not HR.find_loops(ov, of)[0]


def test_nonfinite_status_in_the_reference():
    v, f = HC.holed_icosphere(1, (0,))
    v = v.copy()
    v[HC.ring(HC.icosphere(1)[1], 0)[0], 0] = np.nan
    assert HR.fill(v, f)[2]['status'] == ['nonfinite']


@pytest.mark.parametrize("name", sorted(MESHES))
def test_find_loops_matches_the_reference(name):
    v, f, _ = MESHES[name]
    loops, table = HR.find_loops(v, f)
    lv, lo, mine = H.find_loops(torch.from_numpy(v), torch.from_numpy(f))
    assert lv.tolist() == [x for lp in loops for x in lp]
    assert lo.tolist() == np.cumsum([0] + [len(lp) for lp in loops]).tolist()
    assert mine == table                                                                         # perimeters bit for bit


def test_find_loops_ignores_invalid_faces_and_refuses_bad_meshes():
    v, f = HC.holed_icosphere(1, (0,))
    bad = np.concatenate([f, [[0, 0, 1], [1, 2, 99]]])
    a, b = H.find_loops(torch.from_numpy(v), torch.from_numpy(bad)), H.find_loops(torch.from_numpy(v), torch.from_numpy(f))
    assert torch.equal(a[0], b[0]) and a[2] == b[2]
    fan = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int64)                                  # three faces on one edge
    flipped = np.array([[0, 1, 2], [0, 1, 3]], np.int64)                                         # both run 0 -> 1
    for faces in (fan, flipped):
        for find in (lambda x, y: HR.find_loops(x, y), lambda x, y: H.find_loops(torch.from_numpy(x), torch.from_numpy(y))):
            with pytest.raises(ValueError, match="repair.repair"):
                find(np.zeros((5, 3), np.float32), faces)


def test_fill_refuses_cpu_tensors_and_bad_arguments():
    v, f = (torch.from_numpy(x) for x in HC.holed_icosphere(1, (0,)))
    with pytest.raises(RuntimeError):
        H.fill(v, f)
    with pytest.raises(RuntimeError):
        H.triangulate_loops(v, torch.tensor([0, 1, 2]), torch.tensor([0, 3]))
    with pytest.raises(ValueError):
        H.triangulate_loops(v, torch.tensor([0, 1, 2]), torch.tensor([0, 3]), route='fast')


# ------------------------------------------------------------------------------------------------- refinement (plain torch)
def refine_case(v, f):
    """The reference's fill, then recmv.holes._refine on the host."""
    ov, of, info = HR.fill(v, f)
    V, F = len(v), len(f)
    pf = torch.from_numpy(of[F:])
    pl = torch.cat([torch.full((info['faces_added'][l],), l, dtype=torch.int64) for l in range(info['loops'])])
    lbar = torch.tensor([p / n for p, n in zip(info['perimeter'], info['edges'])], dtype=torch.float64)
    table = EdgeTable(torch.from_numpy(f), V)
    keys = table.edges[:, 0] * V + table.edges[:, 1]
    return (torch.from_numpy(v), torch.from_numpy(f), pf, pl, lbar) + H._refine(torch.from_numpy(v), pf, pl, lbar, keys)


@pytest.mark.parametrize("name", ["hole12", "cylinder"])
def test_refine_on_the_host(name):
    v, f = HC.icosphere_hole12() if name == "hole12" else HC.cylinder()
    v0, f0, pf0, pl0, lbar, nv, pf, pl, vloop, rounds, capped = refine_case(v, f)
    assert not capped and 0 < rounds < H.MAX_REFINE_ROUNDS                                       # the cap is not hit here
    assert torch.equal(nv[:len(v)], v0) and nv.shape[0] == len(v) + vloop.shape[0] > len(v)
    whole = torch.cat([f0, pf])
    table = EdgeTable(whole, nv.shape[0])
    assert int(table.count.min()) == 2 == int(table.count.max())                                 # watertight, edge-manifold
    d = torch.cat([whole[:, [0, 1]], whole[:, [1, 2]], whole[:, [2, 0]]])
    assert torch.unique(d[:, 0] * nv.shape[0] + d[:, 1]).numel() == d.shape[0]                  # consistently oriented
    ptab = EdgeTable(pf, nv.shape[0])
    border0 = EdgeTable(pf0, len(v))
    b0 = border0.edges[border0.count == 1]
    b1 = ptab.edges[ptab.count == 1]
    assert torch.equal(b0, b1)                                                                   # every border edge is still one
    inner = ptab.edges[ptab.count == 2]
    length = (nv[inner[:, 0]].double() - nv[inner[:, 1]].double()).norm(dim=1)
    loop_of = torch.zeros(ptab.E, dtype=torch.int64)
    loop_of[ptab.face_to_edge.reshape(-1)] = pl.repeat_interleave(3)
    assert bool((length <= (4. / 3.) * lbar[loop_of[ptab.count == 2]] * (1 + 1e-12)).all())


# ------------------------------------------------------------------------------------------------- the C ABI
def test_abi_symbols_and_argument_errors():
    from recmv import _lib as L
    lib = L.lib()
    assert lib.recmv_abi_version() == L.ABI_VERSION == 11
    assert {"recmv_hole_triangulate", "recmv_hole_triangulate_workspace_bytes", "recmv_hole_fill_lds_max_edges",
            "recmv_hole_fill_auto_max_edges", "recmv_hole_fill_max_edges"} <= set(L.exported_symbols())
    assert lib.recmv_hole_fill_auto_max_edges() == H.AUTO_MAX_EDGES == HC.AUTO_MAX <= H.LDS_MAX_EDGES
    assert lib.recmv_hole_fill_lds_max_edges() == H.LDS_MAX_EDGES == HC.LDS_MAX
    assert lib.recmv_hole_fill_max_edges() == H.MAX_LOOP_EDGES
    n = C.c_void_p(0)
    buf = (C.c_byte * 256)()
    p = C.cast(buf, C.c_void_p)
    q = C.cast(C.byref(buf, 64), C.c_void_p)
    r = C.cast(C.byref(buf, 128), C.c_void_p)

    def offsets(*x):
        a = (C.c_int64 * len(x))(*x)
        return a, C.cast(a, C.c_void_p)
    keep, ok = offsets(0, 3, 8)
    call = lib.recmv_hole_triangulate
    assert call(n, 0, n, n, n, 0, n, n, n, 0, 0, n) == 0                                         # L = 0: a no-op
    assert call(p, 9, p, ok, p, -1, q, r, n, 0, 0, n) == -1 and b"L=-1" in lib.recmv_last_error()
    assert call(p, 9, p, ok, p, 2, q, r, n, 0, 3, n) == -1 and b"route" in lib.recmv_last_error()
    assert call(p, 9, p, n, p, 2, q, r, n, 0, 0, n) == -1 and b"NULL loop_offsets" in lib.recmv_last_error()
    assert call(n, 9, p, ok, p, 2, q, r, n, 0, 0, n) == -1 and b"NULL verts" in lib.recmv_last_error()
    assert call(p, 9, n, ok, p, 2, q, r, n, 0, 0, n) == -1 and b"NULL loop_verts" in lib.recmv_last_error()
    assert call(p, 9, p, ok, n, 2, q, r, n, 0, 0, n) == -1 and b"NULL" in lib.recmv_last_error()
    assert call(p, 9, p, ok, p, 2, n, r, n, 0, 0, n) == -1 and b"NULL output" in lib.recmv_last_error()
    assert call(p, 9, p, ok, p, 2, q, n, n, 0, 0, n) == -1 and b"NULL output" in lib.recmv_last_error()
    assert call(p, -1, p, ok, p, 2, q, r, n, 0, 0, n) == -1 and b"V=-1" in lib.recmv_last_error()
    assert call(p, 9, p, ok, p, 2, p, r, n, 0, 0, n) == -1 and b"alias" in lib.recmv_last_error()
    assert call(p, 9, p, ok, p, 2, q, q, n, 0, 0, n) == -1 and b"alias" in lib.recmv_last_error()
    k2, short = offsets(0, 2, 8)
    assert call(p, 9, p, short, p, 2, q, r, n, 0, 0, n) == -1 and b"at least 3" in lib.recmv_last_error()
    k3, first = offsets(1, 4, 8)
    assert call(p, 9, p, first, p, 2, q, r, n, 0, 0, n) == -1 and b"loop_offsets[0]" in lib.recmv_last_error()
    k4, huge = offsets(0, 3, 3 + H.MAX_LOOP_EDGES + 1)
    assert call(p, 9, p, huge, p, 2, q, r, n, 0, 0, n) == -1 and b"hard cap" in lib.recmv_last_error()
    k5, long_ = offsets(0, 3, 3 + H.LDS_MAX_EDGES + 1)
    assert call(p, 9, p, long_, p, 2, q, r, n, 0, 1, n) == -1 and b"lds route" in lib.recmv_last_error()
    # the global route needs a workspace: NULL, misaligned, short
    assert call(p, 9, p, ok, p, 2, q, r, n, 0, 2, n) == -1 and b"NULL workspace" in lib.recmv_last_error()
    odd = C.cast(C.byref(buf, 193), C.c_void_p)
    assert call(p, 9, p, ok, p, 2, q, r, odd, 1 << 20, 2, n) == -1 and b"aligned" in lib.recmv_last_error()
    w = C.cast(C.byref(buf, 192), C.c_void_p)
    assert call(p, 9, p, ok, p, 2, q, r, w, 8, 2, n) == -4 and b"workspace" in lib.recmv_last_error()


def test_workspace_size():
    from recmv import _lib as L
    lib = L.lib()
    size = lib.recmv_hole_triangulate_workspace_bytes

    def of(sizes, route):
        a = (C.c_int64 * (len(sizes) + 1))(*np.cumsum([0] + list(sizes)).tolist())
        return size(C.cast(a, C.c_void_p), len(sizes), route)

    def segment(n):
        t = n * (n - 1) // 2
        return 24 + 16 * t + (2 * t + 7) // 8 * 8 + (12 * n + 7) // 8 * 8
    assert size(None, 0, 0) == 0
    assert of([3, 50, H.AUTO_MAX_EDGES], 0) == 0 == of([3, 50, H.LDS_MAX_EDGES], 1)              # all in LDS
    assert of([H.AUTO_MAX_EDGES + 1], 0) == segment(H.AUTO_MAX_EDGES + 1)
    assert of([3, 300, 7], 0) == segment(300) and of([3, 300, 7], 2) == segment(3) + segment(300) + segment(7)
    sizes = [of([n], 2) for n in range(3, 200)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))                                          # monotone in n
    assert of([300, 300], 2) == 2 * of([300], 2)
    assert of([2], 0) == -1 and b"at least 3" in lib.recmv_last_error()
    assert of([H.MAX_LOOP_EDGES + 1], 0) == -1
    assert of([H.MAX_LOOP_EDGES], 0) == segment(H.MAX_LOOP_EDGES)
    assert size(None, 2, 0) == -1 and size(None, -1, 0) == -1
    assert of([H.LDS_MAX_EDGES + 1], 1) == -1 and of([5], 7) == -1


def test_lds_threshold_arithmetic():
    def lds_bytes(n):
        return n * (n - 1) // 2 * 18 + 12 * n
    assert lds_bytes(H.LDS_MAX_EDGES) <= 64 * 1024 < lds_bytes(H.LDS_MAX_EDGES + 1)


# ------------------------------------------------------------------------------------------------- the commands
@pytest.mark.parametrize("script,argv,message", [
    ("clean_fl.py", ["--in", "x.obj", "--out", "o", "--fill-max-edges", "8"], "--fill-max-edges needs --fill-holes"),
    ("clean_fl.py", ["--in", "x.obj", "--out", "o", "--fill-max-perimeter", "1.5"], "--fill-max-perimeter needs --fill-holes"),
    ("clean_fl.py", ["--in", "x.obj", "--out", "o", "--fill-keep-largest", "2"], "--fill-keep-largest needs --fill-holes"),
    ("clean_fl.py", ["--in", "x.obj", "--out", "o", "--fill-refine"], "--fill-refine needs --fill-holes"),
    ("clean_fl.py", ["--in", "x.obj", "--out", "o", "--fill-fair-iters", "3"], "--fill-fair-iters needs --fill-holes"),
    ("clean_fl.py", ["--in", "x.obj", "--report-only", "--fill-holes"], "--fill-holes needs --out"),
    ("clean_fl.py", ["--in", "x.obj", "--out", "o", "--fill-holes", "--fill-fair-iters", "3"], "needs --fill-refine"),
    ("clean_fl.py", ["--in", "x.obj", "--out", "o", "--fill-holes", "--fill-keep-largest", "-1"], "must not be negative"),
    ("eval_fl.py", ["--pred", "HERE", "--gt", "HERE", "--fill-max-edges", "8"], "need --fill-holes"),
    ("eval_fl.py", ["--pred", "HERE", "--gt", "HERE", "--fill-keep-largest", "2"], "need --fill-holes"),
])
def test_cli_parser_errors(script, argv, message, tmp_path):
    (tmp_path / "a.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    argv = [str(tmp_path) if a == "HERE" else a for a in argv]
    out = subprocess.run([sys.executable, str(REPO / "rec-mv_amd" / script)] + argv, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and message in out.stderr, out.stderr


def test_cli_help_lists_the_flags():
    out = subprocess.run([sys.executable, str(REPO / "rec-mv_amd" / "clean_fl.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    for flag in ("--fill-holes", "--fill-max-edges", "--fill-max-perimeter", "--fill-keep-largest", "--fill-refine",
                 "--fill-fair-iters"):
        assert flag in out.stdout
