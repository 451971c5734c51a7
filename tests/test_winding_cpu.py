"""Generalized winding numbers without a GPU: the float64 restatement (tests/winding_reference.py) on hand cases, the new C entry
points (declared, exported, argument errors before any HIP call), the refusal of CPU tensors, the commands' new flags, the
tolerances of the GPU test re-measured from the reference alone, the decidability of that test's node sets, and the host build
of the kernels under the sanitizers.
"""
import ctypes as C
import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import host_check  # noqa: E402
import winding_reference as WR  # noqa: E402

TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])            # outward


# ------------------------------------------------------------------------------------------------------ the reference
def test_reference_on_hand_cases():
    inside_pt, outside_pt = TET_V.mean(0, keepdims=True), np.array([[1., 1., 1.]], np.float32)
    for terms, tol in ((np.float64, 1e-15), (np.float32, 1e-6)):
        assert abs(WR.winding(inside_pt, TET_V, TET_F, terms)[0] - 1.) <= tol
        assert abs(WR.winding(inside_pt, TET_V, TET_F[:, ::-1], terms)[0] + 1.) <= tol              # flipped: -1
        assert abs(WR.winding(outside_pt, TET_V, TET_F, terms)[0]) <= tol
    # two nested, overlapping tetrahedra: the second is the first scaled by 2 about the inner point
    c = TET_V.mean(0)
    v2 = np.concatenate([TET_V, c + 2 * (TET_V - c)]).astype(np.float32)
    f2 = np.concatenate([TET_F, TET_F + 4])
    assert abs(WR.winding(inside_pt, v2, f2)[0] - 2.) <= 1e-15
    assert WR.inside(WR.winding(inside_pt, TET_V, TET_F[:, ::-1]))[0] and not WR.inside(np.array([np.nan, 0.4, -0.4])).any()
    # a right triangle with legs L at the origin, seen from height h on the axis through its right-angle corner:
    # Omega = pi / 2 - integral over the quarter turn of h / sqrt(R(t)^2 + h^2), R(t) = L / (cos t + sin t) — an octant as L grows;
    # negative, since the point looks at the face's front
    x, wq = np.polynomial.legendre.leggauss(96)
    t = 0.25 * math.pi * (x + 1.)
    for L_, h in ((1., 0.5), (2., 0.25), (1e4, 1.)):
        R = L_ / (np.cos(t) + np.sin(t))
        omega = 0.5 * math.pi - 0.25 * math.pi * float((wq * h / np.sqrt(R * R + h * h)).sum())
        tri_v = np.array([[0, 0, 0], [L_, 0, 0], [0, L_, 0]], np.float32)
        got = WR.winding(np.array([[0, 0, h]], np.float32), tri_v, np.array([[0, 1, 2]]))[0]
        assert abs(got + omega / (4. * math.pi)) <= 1e-12, (L_, h, got)
    assert abs(got + 0.125) < 1e-4                                                               # the octant
    # skipped and degenerate faces, queries that are not finite
    f3 = np.concatenate([TET_F, [[0, 1, 9], [-1, 2, 3], [2, 2, 2], [0, 1, 1]]])
    assert WR.winding(inside_pt, TET_V, f3)[0] == WR.winding(inside_pt, TET_V, TET_F)[0]
    assert np.isnan(WR.winding(np.array([[np.nan, 0, 0], [np.inf, 0, 0]], np.float32), TET_V, TET_F)).all()
    bad_v = TET_V.copy()
    bad_v[3, 1] = np.inf
    assert np.isnan(WR.winding(inside_pt, bad_v, TET_F)[0])


def test_reference_pyramid_on_hand_cases():
    """The pyramid of the tetrahedron: the root's sums, a beta that accepts nothing gives the exact sum, a far query takes the
    root alone (a closed mesh has N = 0 there)."""
    pyr = WR.Pyramid(TET_V, TET_F, levels=2)
    root = pyr.level[0]
    assert root['count'][0, 0, 0] == 4 and abs(root['area'][0, 0, 0] - (1.5 + math.sqrt(3.) / 2.)) < 1e-12
    assert np.abs(root['N'][0, 0, 0]).max() < 1e-15 and root['lo'][0, 0, 0].tolist() == [0, 0, 0] and root['hi'][0, 0, 0].tolist() == [1, 1, 1]
    assert sum(int(pyr.level[2]['count'].sum()) for _ in (0,)) == 4
    q = np.array([[0.25, 0.25, 0.25], [0.9, 0.9, 0.9], [30., -20., 10.]], np.float32)
    assert np.abs(pyr.query(q, beta=1e30) - WR.winding(q, TET_V, TET_F)).max() < 1e-15
    stats = {}
    assert pyr.query(q[2:], beta=2., stats=stats)[0] == 0. and stats == {'dipoles': 1., 'faces': 0.}
    open_f = TET_F[:3]                                       # without the slanted face: N is its missing area vector
    far = WR.Pyramid(TET_V, open_f, levels=1).query(q[2:], beta=2.)[0]
    assert abs(far - WR.winding(q[2:], TET_V, open_f)[0]) < 1e-5 and far != 0.
    assert WR.choose_levels(WR.corners(TET_V, TET_F), *WR.cube(TET_V, TET_F)) == 1


# ---------------------------------------------------------------------------------------------------------- the C ABI
ONE = C.c_void_p(16)                                       # a non-NULL pointer that is never followed
NAMES = ("recmv_winding_chunk_faces", "recmv_winding_exact_workspace_bytes", "recmv_winding_exact", "recmv_winding_tree_nodes",
         "recmv_winding_tree_cells", "recmv_winding_tree_build", "recmv_winding_tree_query")


def _tree(origin=(0., 0., 0.), side=1., levels=3, n_faces=5, tables=(ONE, ONE, ONE)):
    from recmv import _lib
    d = _lib.WindingTreeDesc()
    d.origin[:] = origin
    d.side, d.levels, d.n_faces = side, levels, n_faces
    d.nodes, d.cell_start, d.tris = (t.value if t is not None else None for t in tables)
    return d


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in NAMES:
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION == 11
    assert C.sizeof(_lib.WindingTreeDesc) == 56
    hdr = (REPO / "include" / "recmv_hip.h").read_text()
    note = hdr[:hdr.index("int recmv_abi_version")]
    assert "recmv_winding_tree_query with the recmv_winding_tree descriptor" in note and "recmv_hole_fill_max_edges (hole filling" in note
    assert lib.recmv_winding_chunk_faces() == 4096
    assert [lib.recmv_winding_tree_nodes(l) for l in (1, 2, 7)] == [9, 73, (8 ** 8 - 1) // 7]


def test_a_library_without_the_symbols_is_rejected():
    from recmv import _lib

    class Partial:
        def __getattr__(self, name):
            if name.startswith("recmv_winding"):
                raise AttributeError(name)
            return getattr(_lib.lib(), name)
    with pytest.raises(AttributeError, match="recmv_winding"):
        _lib._declare(Partial())


def test_argument_errors_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    err = lib.recmv_last_error
    K = lib.recmv_winding_chunk_faces()
    assert lib.recmv_winding_exact_workspace_bytes(10, K) == 80 and lib.recmv_winding_exact_workspace_bytes(10, K + 1) == 160
    assert lib.recmv_winding_exact_workspace_bytes(0, 5) == 0 and lib.recmv_winding_exact_workspace_bytes(7, 0) == 0
    assert lib.recmv_winding_exact_workspace_bytes(-1, 5) == -1 and b"P=-1" in err()
    assert lib.recmv_winding_exact_workspace_bytes(1, -5) == -1 and b"F=-5" in err()
    assert lib.recmv_winding_exact_workspace_bytes(1, K * 65536) == -1 and b"65535 chunks" in err()

    def exact(*, p=(ONE, 10), mesh=(ONE, 3, ONE, 5), w=ONE, ws=(ONE, 80)):
        return lib.recmv_winding_exact(*p, *mesh, w, *ws, None)
    assert exact(p=(ONE, -1)) == -1 and b"P=-1" in err()
    assert exact(mesh=(ONE, -3, ONE, 5)) == -1 and b"V=-3" in err()
    assert exact(mesh=(ONE, 3, ONE, -5)) == -1 and b"F=-5" in err()
    assert exact(p=(None, 10)) == -1 and b"NULL points or output" in err()
    assert exact(w=None) == -1 and b"NULL points or output" in err()
    assert exact(mesh=(None, 3, ONE, 5)) == -1 and b"NULL pointer of the mesh" in err()
    assert exact(mesh=(ONE, 3, None, 5)) == -1 and b"NULL pointer of the mesh" in err()
    assert exact(ws=(None, 80)) == -1 and b"NULL workspace" in err()
    assert exact(ws=(ONE, 79)) == -1 and b"workspace of 79 bytes, 80 needed" in err()
    assert exact(ws=(C.c_void_p(20), 80)) == -1 and b"aligned" in err()
    assert exact(p=(None, 0), w=None, ws=(None, 0)) == 0                             # P = 0: a no-op

    assert lib.recmv_winding_tree_nodes(0) == -1 and b"levels=0" in err()
    assert lib.recmv_winding_tree_nodes(8) == -1 and b"levels=8" in err()

    def bad_trees(call):
        assert call(None) == -1 and b"NULL tree" in err()
        for lv in (0, 8, -1):
            assert call(C.byref(_tree(levels=lv))) == -1 and b"levels=%d" % lv in err()
        for s in (0., -1., float("nan"), float("inf")):
            assert call(C.byref(_tree(side=s))) == -1 and b"side" in err()
        assert call(C.byref(_tree(origin=(0., float("inf"), 0.)))) == -1 and b"origin" in err()
    bad_trees(lambda t: lib.recmv_winding_tree_cells(ONE, 3, ONE, 5, t, ONE, None))
    bad_trees(lambda t: lib.recmv_winding_tree_build(ONE, 3, ONE, 5, ONE, t, None))
    bad_trees(lambda t: lib.recmv_winding_tree_query(ONE, 10, None, t, 3., ONE, None))
    t = C.byref(_tree())
    assert lib.recmv_winding_tree_cells(ONE, -3, ONE, 5, t, ONE, None) == -1 and b"V=-3" in err()
    assert lib.recmv_winding_tree_cells(ONE, 3, ONE, -5, t, ONE, None) == -1 and b"F=-5" in err()
    assert lib.recmv_winding_tree_cells(ONE, 3, None, 5, t, ONE, None) == -1 and b"NULL pointer" in err()
    assert lib.recmv_winding_tree_cells(ONE, 3, ONE, 5, t, None, None) == -1 and b"NULL pointer" in err()
    assert lib.recmv_winding_tree_cells(None, 3, ONE, 5, t, ONE, None) == -1 and b"NULL pointer" in err()
    assert lib.recmv_winding_tree_cells(None, 3, None, 0, t, None, None) == 0       # F = 0: a no-op
    assert lib.recmv_winding_tree_build(ONE, 3, ONE, -5, ONE, t, None) == -1 and b"F=-5" in err()
    assert lib.recmv_winding_tree_build(ONE, 3, ONE, 4, ONE, t, None) == -1 and b"n_faces=5 must be 0 .. F=4" in err()
    assert lib.recmv_winding_tree_build(ONE, 3, ONE, 5, ONE, C.byref(_tree(n_faces=-1)), None) == -1 and b"n_faces=-1" in err()
    assert lib.recmv_winding_tree_build(ONE, 3, ONE, 5, ONE, C.byref(_tree(tables=(None, ONE, ONE))), None) == -1 and b"NULL table" in err()
    assert lib.recmv_winding_tree_build(ONE, 3, ONE, 5, ONE, C.byref(_tree(tables=(ONE, None, ONE))), None) == -1 and b"NULL table" in err()
    assert lib.recmv_winding_tree_build(ONE, 3, ONE, 5, ONE, C.byref(_tree(tables=(ONE, ONE, None))), None) == -1 and b"NULL pointer" in err()
    assert lib.recmv_winding_tree_build(ONE, 3, ONE, 5, None, t, None) == -1 and b"NULL pointer" in err()
    for beta in (0.99, -3., float("nan"), float("inf")):
        assert lib.recmv_winding_tree_query(ONE, 10, None, t, beta, ONE, None) == -1 and b"beta" in err()
    assert lib.recmv_winding_tree_query(ONE, -10, None, t, 3., ONE, None) == -1 and b"P=-10" in err()
    assert lib.recmv_winding_tree_query(None, 10, None, t, 3., ONE, None) == -1 and b"NULL points or output" in err()
    assert lib.recmv_winding_tree_query(ONE, 10, None, t, 3., None, None) == -1 and b"NULL points or output" in err()
    assert lib.recmv_winding_tree_query(ONE, 10, None, C.byref(_tree(tables=(None, ONE, ONE))), 3., ONE, None) == -1 and b"NULL table" in err()
    assert lib.recmv_winding_tree_query(ONE, 10, None, C.byref(_tree(n_faces=-2)), 3., ONE, None) == -1 and b"n_faces=-2" in err()
    assert lib.recmv_winding_tree_query(None, 0, None, t, 3., None, None) == 0      # P = 0: a no-op


# ------------------------------------------------------------------------------------------------------- recmv.winding
def test_cpu_tensors_and_bad_arguments_are_refused():
    from recmv import metrics, voxelize, winding
    v, f = torch.from_numpy(TET_V), torch.from_numpy(TET_F)
    p = torch.zeros(2, 3)
    lat = voxelize.Lattice((0, 0, 0), 0.1, (4, 4, 4))
    for call in (lambda: winding.winding_number(p, v, f), lambda: winding.winding_number(p, v, f, method='tree'),
                 lambda: winding.points_inside(p, v, f), lambda: winding.WindingTree(v, f), lambda: winding.exact_partials(p, v, f),
                 lambda: metrics.points_inside(p, v, f, rule='winding'), lambda: metrics.penetration(p, v, f, rule='winding'),
                 lambda: voxelize.distance_field(v, f, lat, sign='winding'), lambda: voxelize.remesh(v, f, step=0.1, sign='winding'),
                 lambda: voxelize.occupancy(v, f, lat, sign='winding'), lambda: voxelize.volume(v, f, lat, sign='winding'),
                 lambda: voxelize.volume_iou(v, f, v, f, step=0.1, sign='winding')):
        with pytest.raises(RuntimeError):
            call()
    for call in (lambda: winding.winding_number(p, v, f, method='fast'), lambda: winding.points_inside(p, v, f, threshold=0.),
                 lambda: winding.points_inside(p, v, f, threshold=1.), lambda: metrics.points_inside(p, v, f, rule='odd'),
                 lambda: metrics.penetration(p, v, f, rule='odd'), lambda: voxelize.distance_field(v, f, lat, sign='odd'),
                 lambda: voxelize.distance_field(v, f, lat, winding_method='exact'),
                 lambda: voxelize.distance_field(v, f, lat, sign='winding', winding_method='fast'),
                 lambda: voxelize.remesh(v, f, step=0.1, sign='odd'), lambda: voxelize.volume_iou(v, f, v, f, step=0.1, sign='odd')):
        with pytest.raises(ValueError):
            call()
    assert winding.DEFAULT_BETA == WR.DEFAULT_BETA == 3. and WR.TOL_TREE[3.] <= 0.05
    assert winding.MAX_LEVELS == WR.MAX_LEVELS == 7 and winding.FACES_PER_CELL == WR.FACES_PER_CELL
    assert voxelize.DEFAULT_WINDING_METHOD in winding.METHODS
    assert "sign='winding'" in voxelize.__doc__ and "COARSE cap" in voxelize.__doc__


def test_the_commands_carry_the_new_flags_and_they_default_to_parity():
    import clean_fl
    import eval_fl
    me = str(HERE / "winding_reference.py")                # any existing file: the usage errors come before it is read
    assert clean_fl.build_parser().parse_args(["--in", "x"]).voxel_sign == 'parity'
    a = clean_fl.build_parser().parse_args(["--in", "x", "--voxel-remesh", "0.04", "--voxel-sign", "winding"])
    assert a.voxel_sign == 'winding' and a.voxel_force is False
    for bad in (["--voxel-sign", "winding"], ["--voxel-remesh", "0.04", "--voxel-sign", "odd"],
                ["--voxel-remesh", "0.04", "--solidify", "0.2", "--voxel-sign", "winding"]):
        with pytest.raises(SystemExit):                    # before any device work
            clean_fl.main(["--in", me, "--out", "unused"] + bad)
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g"])
    assert a.voxel_sign == 'parity' and a.inside_rule == 'parity'
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g", "--volume", "--voxel-sign", "winding", "--intersections", "--body", "b",
                                           "--penetration", "--inside-rule", "winding"])
    assert a.voxel_sign == 'winding' and a.inside_rule == 'winding'
    for bad in (["--voxel-sign", "winding"], ["--inside-rule", "winding"], ["--volume", "--voxel-sign", "odd"],
                ["--intersections", "--body", me, "--inside-rule", "winding"]):
        with pytest.raises(SystemExit):
            eval_fl.main(["--pred", me, "--gt", me] + bad)


# ------------------------------------------------------------------------------------- the GPU test's tolerances and node sets
@functools.lru_cache(maxsize=None)
def _measured(name):
    """(the f32-term sum's and the pyramid rule's largest error against exact float64 on the far-enough nodes, the levels)."""
    v, f, _ = WR.case(name)
    pts, w64, far = WR.case_reference(name)
    e32 = float(np.abs(WR.winding(pts, v, f, np.float32) - w64)[far].max())
    pyr = WR.Pyramid(v, f)
    return e32, {beta: float(np.abs(pyr.query(pts, beta) - w64)[far].max()) for beta in WR.TOL_TREE}, pyr.levels


@pytest.mark.parametrize("name", WR.NAMES)
def test_tolerances_and_undecided_shares_of_the_gpu_tests_node_sets(name):
    """Re-measured from the reference alone: the f32-term sum and the pyramid rule against exact float64 stay within the figures
    the tolerances are derived from, closed meshes give integers, and at every tolerance the GPU test compares flags with, the
    nodes it leaves out stay below the cap."""
    v, f, lat = WR.case(name)
    pts, w64, far = WR.case_reference(name)
    assert len(pts) == lat.n_nodes and far.mean() > 0.98
    e32, tree, levels = _measured(name)
    shares = {tol: float((~WR.decided(w64, tol)).mean()) for tol in (WR.TOL_EXACT, WR.DECISION_MARGIN, *WR.TOL_TREE.values())}
    print("%s: %d nodes, %d far enough, f32 terms %.3g, pyramid (levels %d) %s, undecided %s" % (
        name, len(pts), far.sum(), e32, levels, {b: round(e, 4) for b, e in tree.items()},
        {t: "%.2f %%" % (100 * s) for t, s in shares.items()}))
    assert e32 <= WR.MEASURED_F32 and all(tree[b] <= WR.MEASURED_TREE[b] for b in tree)
    assert WR.TOL_EXACT == 8 * WR.MEASURED_F32 and all(WR.TOL_TREE[b] == 2 * WR.MEASURED_TREE[b] + WR.TOL_EXACT for b in tree)
    assert max(shares.values()) <= WR.UNDECIDED_CAP
    if name in WR.CLOSED:
        assert np.abs(w64 - np.round(w64))[far].max() < 1e-13 and shares[WR.DECISION_MARGIN] == 0.
        assert WR.inside(w64).sum() >= 2000
        assert (np.round(w64).max() == 2.) == (name == 'two_bodies')
    else:
        assert 0. < shares[WR.DECISION_MARGIN] < 0.01      # the open bodies: under 1 % within 0.05 of 1/2


def test_the_figures_are_the_largest_measured():
    """The two MEASURED constants are not slack: some case reaches 90 % of each."""
    got = [_measured(name) for name in WR.NAMES]
    assert max(g[0] for g in got) >= 0.9 * WR.MEASURED_F32
    assert all(max(g[1][b] for g in got) >= 0.9 * WR.MEASURED_TREE[b] for b in WR.TOL_TREE)


# ------------------------------------------------------------------------------------------------------ the host build
def test_host_build_of_the_kernels_equals_the_brute_loops(tmp_path):
    """tools/winding_host_check: csrc/winding.hip's kernels and csrc/solid_angle.h compiled for the CPU under the address and
    undefined-behaviour sanitizers: the binning, the pyramid's sums, the stack-free traversal (against a recursive walk, bit for
    bit, and against the brute sum) and the chunked exact sum, on seven inputs."""
    r = host_check.run("winding", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count("-> 0 mismatches") == 7, r.stdout + r.stderr
    for name in ("levels 1", "inside one finest cell", "invalid indices and faces without area", "a cube smaller than the mesh",
                 "more than two chunks: 9000 faces (9000 binned), levels 4, 55 queries, 3 chunks"):
        assert name in r.stdout
