"""Mesh simplification without a GPU: the numpy restatement (tests/mesh_simplify_reference.py) on hand cases with known answers,
the host build of the three kernels under the sanitizers (tools/mesh_simplify_host_check), the new C entry points (declared,
exported, argument errors before any HIP call), the driver on its float64 torch path on CPU tensors with the invariants of
tests/mesh_simplify_cases.py, the torch restatements against the numpy one, and clean_fl.py's new flags."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import host_check  # noqa: E402
import mesh_simplify_cases as SC  # noqa: E402
import mesh_simplify_reference as SR  # noqa: E402
import mesh_topology_cases as TC  # noqa: E402
import mesh_topology_reference as TR  # noqa: E402


def run(mesh, **kw):
    from recmv import simplify
    v, f = mesh
    nv, nf, info = simplify.simplify(torch.from_numpy(v), torch.from_numpy(f), use_kernels=False, **kw)
    assert nv.dtype == torch.float32 and nf.dtype == torch.int64
    return nv.numpy(), nf.numpy(), info


# ---- the reference's hand cases ---------------------------------------------------------------------------------------------------
TRIANGLE = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int64))


def test_reference_quadric_of_a_single_triangle():
    Q, A, terms, invalid = SR.vertex_quadrics(*TRIANGLE, boundary_weight=0.)
    want = np.zeros(11)
    want[7], want[10] = 0.5, 0.5                           # area 1/2, the plane z = 0: only zz, and the weight
    assert invalid == 0 and terms.tolist() == [3, 3, 3]       # the face and two boundary edges (of weight 0 here)
    for i in range(3):
        assert np.array_equal(Q[i], want)
    assert SR.cost_at(Q[0], np.array([0.3, -2., 0.], np.float32))[0] == 0
    assert SR.cost_at(Q[0], np.array([0.3, -2., 2.], np.float32))[0] == 0.5 * 4


def test_reference_boundary_edges_add_the_planes_that_stand_on_the_face():
    Q, _, terms, _ = SR.vertex_quadrics(*TRIANGLE, boundary_weight=1.)
    # vertex 0: edge (0, 1) along x gives the plane y = 0 with weight |e|^2 = 1, edge (0, 2) along y the plane x = 0
    want = np.zeros(11)
    want[0], want[4], want[7], want[10] = 1., 1., 0.5, 0.5
    assert np.array_equal(Q[0], want) and terms.tolist() == [3, 3, 3]
    # vertex 1: y = 0 and the plane through the hypotenuse, x + y = 1 with weight 2: m = (1, 1, 0) / sqrt 2, d = -1 / sqrt 2
    w1 = np.array([1., 1., 0., -1., 1. + 1., 0., -1., 0.5, 0., 1., 0.5])
    assert np.abs(Q[1] - w1).max() < 1e-15
    # a point on the hypotenuse's line in the face's plane costs vertex 1 only its distance to y = 0
    assert abs(SR.cost_at(Q[1], np.array([0.25, 0.75, 0.], np.float32))[0] - 0.75 ** 2) < 1e-15


def test_reference_flat_fan_has_rank_one():
    v, f = SC.fan(12)
    v[:, 2] = 0.25                                         # flat, in the plane z = 1/4
    Q, _, _, _ = SR.vertex_quadrics(v, f, boundary_weight=0.)
    g = np.random.default_rng(0)
    for p in g.uniform(-3, 3, (20, 2)):
        assert SR.cost_at(Q[0] + Q[1], np.array([p[0], p[1], 0.25], np.float32))[0] == 0
    assert SR.cost_at(Q[0] + Q[1], np.array([0., 0., 1.25], np.float32))[0] == pytest.approx(Q[0][10] + Q[1][10], rel=1e-14)
    cands = SR.candidates(Q[0] + Q[1], v[0], v[1], 2.)
    pos, cost, weight = SR.collapse_one(Q, v, 0, 1, SR.FREE, 2.)
    assert cost == 0 and np.isfinite(pos).all() and any(c is not None and np.array_equal(pos, c) for c in cands)
    assert np.array_equal(SR.collapse_one(Q, v, 0, 1, SR.STAY_B, 2.)[0], v[1])


def test_reference_greedy_keeps_a_closed_surface_closed():
    v, f = SC.bumpy_sphere()
    gv, gf, n = SR.greedy_simplify(v, f, 640, 10., 2.)
    r = TR.report(gv, gf)
    assert len(gf) == 640 and n == 320 and r['watertight'] and r['euler_characteristic'] == 2 and r['components_vertex'] == 1


# ---- the torch restatements equal the numpy one -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["sphere", "tube", "fan"])
def test_torch_restatements_equal_the_reference(mesh):
    from recmv import connectivity, simplify
    v, f = {"sphere": SC.bumpy_sphere, "tube": SC.tube, "fan": lambda: SC.fan(200)}[mesh]()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    Q, A, terms, _ = SR.vertex_quadrics(v, f, 10.)
    Qt = simplify.vertex_quadrics_torch(tv, tf, None, 10.)
    bound = SR.gamma(terms + SR.PLANE_OPS)[:, None] * A
    assert (np.abs(Qt.numpy() - Q) <= bound).all()
    edges = connectivity.EdgeTable(tf, len(v)).edges
    code = (torch.arange(edges.shape[0]) % 3).to(torch.uint8)
    pos, cost, weight = simplify.edge_collapse_cost_torch(torch.from_numpy(Q), tv, edges, code)
    rpos, rcost, rweight, _ = SR.edge_collapse_cost(Q, v, edges.numpy(), code.numpy(), simplify.REACH)
    assert np.array_equal(pos.numpy(), rpos) and np.array_equal(weight.numpy(), rweight)
    assert np.abs(cost.numpy() - rcost).max() <= 1e-15 * max(np.abs(rcost).max(), 1e-30)
    assert (pos.numpy()[code.numpy() == 1] == v[edges[:, 0].numpy()][code.numpy() == 1]).all()
    from recmv.iso_remesh import _Topo, _flip_ok
    g = torch.Generator().manual_seed(1)
    moved = pos + 0.2 * torch.randn(pos.shape, generator=g) * (torch.arange(pos.shape[0]) % 2)[:, None]
    ok = _flip_ok(tv.double(), tf, _Topo(tf, len(v)), edges[:, 0], edges[:, 1], moved.double())
    want = SR.collapse_flip_check(v, f, edges.numpy(), moved.numpy())
    assert np.array_equal(ok.numpy(), want) and 0 < want.sum() < len(want)


# ---- the driver, float64 torch path on CPU tensors --------------------------------------------------------------------------------
def test_sphere_to_a_quarter_stays_a_closed_sphere():
    SC.check_sphere(*run(SC.bumpy_sphere(), target_faces=320), TR.report)


def test_torus_keeps_its_genus():
    SC.check_torus(*run(SC.torus(), ratio=0.25), TR.report)


def test_tube_keeps_two_loops_on_the_input_border():
    v, f = SC.tube()
    SC.check_tube(*run((v, f), target_faces=64), TR.report, v, f, 64)
    SC.check_tube(*run((v, f), target_faces=99), TR.report, v, f, 99)             # an odd target on an open mesh


def test_flat_grid_stays_flat_and_keeps_its_corners():
    v, f = SC.flat_grid()
    SC.check_flat_grid(*run((v, f), target_faces=16), TR.report, v, f)


def test_max_error_alone_stops_at_the_cap():
    cap = 0.003
    v, f, info = run(SC.bumpy_sphere(), max_error=cap)
    assert info['stopped'] == 'max_error' and 0 < info['max_error'] <= cap and 4 < len(f) < 1280, info
    assert TR.report(v, f)['watertight']
    v2, f2, info2 = run(SC.bumpy_sphere(), target_faces=320, max_error=1e-5)      # the cap stops it before the target
    assert info2['stopped'] == 'max_error' and len(f2) > 320 and info2['max_error'] <= 1e-5


def test_a_target_above_the_face_count_returns_the_compacted_input():
    v, f = SC.torus()
    v2 = np.concatenate([[[9, 9, 9]], v]).astype(np.float32)                       # vertex 0 is used by no face
    nv, nf, info = run((v2, f + 1), target_faces=10 ** 6)
    assert np.array_equal(nv, v) and np.array_equal(nf, f) and info['stopped'] == 'target' and info['collapses'] == 0
    assert info['faces_before'] == info['faces_after'] == len(f) and info['vertices_before'] == len(v) and info['rounds'] == 0


def test_refused_inputs_and_arguments():
    from recmv import simplify
    v, f = (torch.from_numpy(x) for x in TC.hinged_tetrahedra())
    with pytest.raises(ValueError, match="clean_fl.py"):
        simplify.simplify(v, f, target_faces=4, use_kernels=False)                 # an edge with four faces
    tv, tf = (torch.from_numpy(x) for x in TC.tetrahedron())
    bad = tf.clone()
    bad[0, 1] = bad[0, 0]
    with pytest.raises(ValueError, match="topology.report"):
        simplify.simplify(tv, bad, target_faces=2, use_kernels=False)
    bad = tf.clone()
    bad[0, 1] = 4
    with pytest.raises(ValueError, match="clean_fl.py"):
        simplify.simplify(tv, bad, target_faces=2, use_kernels=False)
    for kw in ({}, {'target_faces': 2, 'ratio': 0.5}, {'ratio': 1.5}, {'target_faces': -1}, {'max_error': -1.},
               {'max_error': float('nan')}, {'target_faces': 2, 'boundary_weight': -1.}):
        with pytest.raises(ValueError):
            simplify.simplify(tv, tf, use_kernels=False, **kw)
    with pytest.raises(ValueError):
        simplify.simplify(tv, tf.int(), target_faces=2, use_kernels=False)
    with pytest.raises(RuntimeError):                      # the kernel path refuses host tensors
        simplify.simplify(tv, tf, target_faces=2)
    for call in (lambda: simplify.vertex_quadrics(tv, tf), lambda: simplify.collapse_flip_check(tv, tf, tf[:, :2], tv),
                 lambda: simplify.edge_collapse_cost(torch.zeros(4, 11, dtype=torch.float64), tv, tf[:, :2],
                                                     torch.zeros(4, dtype=torch.uint8))):
        with pytest.raises(RuntimeError):
            call()
    nv, nf, info = simplify.simplify(tv, tf, target_faces=2, use_kernels=False)    # a tetrahedron cannot lose a face
    assert info['stopped'] == 'no_candidates' and nf.shape[0] == 4


def test_the_log_callback_gets_one_line_per_round():
    lines = []
    from recmv import simplify
    v, f = SC.torus()
    _, _, info = simplify.simplify(torch.from_numpy(v), torch.from_numpy(f), ratio=0.5, use_kernels=False, log=lines.append)
    assert len(lines) == info['rounds'] and lines[0].startswith("simplify round 1:")


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("recmv_vertex_quadrics", "recmv_edge_collapse_cost", "recmv_collapse_flip_check")


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION == 11


def test_argument_errors_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    one = C.c_void_p(16)                                   # a non-NULL pointer that is never followed
    err = lib.recmv_last_error

    def quad(V=3, F=1, n_vf=3, B=3, n_vb=6, bw=10., mesh=(one, one), vf=(one, one), vb=(one, one, one), out=(one, one)):
        return lib.recmv_vertex_quadrics(mesh[0], V, mesh[1], F, vf[0], vf[1], n_vf, vb[0], B, vb[1], vb[2], n_vb, bw, *out, None)
    assert quad(V=-1) == -1 and b"V=-1" in err()
    assert quad(F=-2) == -1 and b"F=-2" in err()
    assert quad(B=-3) == -1 and b"B=-3" in err()
    assert quad(n_vf=-1) == -1 and b"n_vf=-1" in err()
    assert quad(V=1 << 31) == -1 and b"2^31" in err()
    assert quad(bw=-1.) == -1 and b"boundary_weight" in err()
    assert quad(bw=float("inf")) == -1 and b"boundary_weight" in err()
    assert quad(bw=float("nan")) == -1 and b"boundary_weight" in err()
    assert quad(mesh=(None, one)) == -1 and b"NULL" in err()
    assert quad(mesh=(one, None)) == -1 and b"NULL faces" in err()
    assert quad(vf=(one, None)) == -1 and b"face table" in err()
    assert quad(vb=(one, None, one)) == -1 and b"boundary-edge table" in err()
    assert quad(out=(one, None)) == -1 and b"NULL" in err()
    assert quad(V=0, F=0, n_vf=0, B=0, n_vb=0, mesh=(None, None), vf=(None, None), vb=(None, None, None), out=(None, None)) == 0

    def cost(V=3, E=2, reach=2., ptrs=(one, one, one, one), out=(one, one, one, one)):
        return lib.recmv_edge_collapse_cost(ptrs[0], ptrs[1], V, ptrs[2], E, ptrs[3], reach, *out, None)
    assert cost(V=-1) == -1 and b"V=-1" in err()
    assert cost(E=-1) == -1 and b"E=-1" in err()
    assert cost(E=1 << 31) == -1 and b"2^31" in err()
    assert cost(reach=-0.5) == -1 and b"reach" in err()
    assert cost(reach=float("nan")) == -1 and b"reach" in err()
    assert cost(ptrs=(one, one, None, one)) == -1 and b"NULL" in err()
    assert cost(ptrs=(None, one, one, one)) == -1 and b"NULL mesh" in err()
    assert cost(out=(one, None, one, one)) == -1 and b"NULL" in err()
    assert cost(E=0, ptrs=(None, None, None, None), out=(None, None, None, None)) == 0

    def flip(V=3, F=1, n_vf=3, E=2, mesh=(one, one), vf=(one, one), ptrs=(one, one, one)):
        return lib.recmv_collapse_flip_check(mesh[0], V, mesh[1], F, vf[0], vf[1], n_vf, ptrs[0], E, ptrs[1], ptrs[2], None)
    assert flip(V=-1) == -1 and b"V=-1" in err()
    assert flip(n_vf=-4) == -1 and b"n_vf=-4" in err()
    assert flip(F=1 << 31) == -1 and b"2^31" in err()
    assert flip(ptrs=(one, one, None)) == -1 and b"NULL" in err()
    assert flip(mesh=(None, one)) == -1 and b"NULL mesh" in err()
    assert flip(vf=(None, one)) == -1 and b"face table" in err()
    assert flip(E=0, mesh=(None, None), vf=(None, None), ptrs=(None, None, None)) == 0


# ---- clean_fl.py ------------------------------------------------------------------------------------------------------------------
def test_clean_fl_carries_the_new_flags_and_they_default_to_off(tmp_path, capsys):
    import clean_fl
    a = clean_fl.build_parser().parse_args(["--in", "x", "--out", "y"])
    assert (a.simplify_faces, a.simplify_ratio, a.simplify_max_error) == (None, None, None)
    a = clean_fl.build_parser().parse_args(["--in", "x", "--out", "y", "--simplify-ratio", "0.25", "--simplify-max-error", "0.01"])
    assert (a.simplify_faces, a.simplify_ratio, a.simplify_max_error) == (None, 0.25, 0.01)
    a = clean_fl.build_parser().parse_args(["--in", "x", "--out", "y", "--simplify-faces", "5000"])
    assert a.simplify_faces == 5000
    me = str(HERE / "mesh_simplify_reference.py")          # any existing file: the usage errors come before it is read
    for bad in (["--simplify-faces", "10", "--simplify-ratio", "0.5"], ["--simplify-ratio", "1.5"], ["--simplify-ratio", "-0.1"],
                ["--simplify-faces", "-1"], ["--simplify-max-error", "-1"]):
        with pytest.raises(SystemExit):
            clean_fl.main(["--in", me, "--out", str(tmp_path)] + bad)
    with pytest.raises(SystemExit):
        clean_fl.main(["--in", me, "--report-only", "--simplify-ratio", "0.5"])    # nothing is written with --report-only
    capsys.readouterr()


# ---- the kernels on the host ------------------------------------------------------------------------------------------------------
def test_host_build_of_the_kernels_under_the_sanitizers(tmp_path):
    """tools/mesh_simplify_host_check: csrc/mesh_simplify.hip's kernels compiled for the CPU under the address and
    undefined-behaviour sanitizers, a stand-alone program: rows of 0, 1, 63, 64, 65 and 257 faces at one vertex, E = 0, 1, 255,
    256, 257, quadrics of rank 0 to 3, invalid faces and edges, a NaN corner, and tables filled with random numbers."""
    r = host_check.run("mesh_simplify", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(" 0 mismatches") == 30
    for name in ("fan of 0", "fan of 1:", "fan of 63", "fan of 64", "fan of 65", "fan of 257", "invalid faces and a NaN corner",
                 "257 edges", "256 edges", "255 edges", "cost rank 0:", "cost rank 1:", "cost rank 2:", "cost rank 3:",
                 "beyond the reach", "with invalid edges", "flip by hand", "random tables"):
        assert name in r.stdout
