"""Mesh repair without a GPU: the numpy restatement (tests/mesh_repair_reference.py) on hand cases whose answers are written
out and against the topology judge on every case, the cell layout, the argument checks of the wrappers and of both parsers, the
new C entry points (declared, exported, argument errors before any HIP call), and the host build of the pair-search kernels
under the sanitizers (tools/mesh_repair_host_check)."""
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
import mesh_repair_cases as RC  # noqa: E402
import mesh_repair_reference as RR  # noqa: E402
import mesh_topology_cases as TC  # noqa: E402
import mesh_topology_reference as TR  # noqa: E402

MESHES = RC.meshes()


# ---- the reference's hand cases ---------------------------------------------------------------------------------------------------
def test_reference_pairs_by_hand():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [np.nan, 0, 0], [-0., 0, 0], [3, 4, 0]], np.float32)
    pairs, nonfinite = RR.points_within(v, 1.)
    assert pairs.tolist() == [[0, 1], [0, 4], [1, 2], [1, 4]] and nonfinite == 1      # (0, 2) lies at sqrt 2
    assert RR.points_within(v, 0.)[0].tolist() == [[0, 4]]                            # +0.0 == -0.0
    assert [0, 5] in RR.points_within(v, 5.)[0].tolist()                              # d2 == eps^2 exactly: included
    assert [0, 5] not in RR.points_within(v, np.nextafter(5., 0.))[0].tolist()


def test_reference_lattice_takes_axis_neighbours_and_no_diagonals():
    pairs, _ = RR.points_within(RC.lattice(), 1.)
    assert len(pairs) == 3 * 6 * 6 * 5
    for shift in (-40., -3.):
        assert np.array_equal(RR.points_within(RC.lattice(shift=shift), 1.)[0], pairs)


def test_reference_book_gives_three_pieces():
    v, f, info = RR.split_nonmanifold(*RC.book())
    assert info == {**info, 'split_vertices': 2, 'added_vertices': 4, 'nonmanifold_edges_before': 1}
    assert f.tolist() == [[0, 1, 2], [5, 7, 3], [6, 8, 4]]  # vertex 0's copies come first (slots 3, 6), then vertex 1's (4, 7)
    assert info['origin'].tolist() == [0, 1, 2, 3, 4, 0, 0, 1, 1]
    assert np.array_equal(v[5:], RC.book()[0][[0, 0, 1, 1]])
    rep = TR.report(v, f)
    assert rep['components_vertex'] == 3 and rep['nonmanifold_edges'] == 0 and rep['boundary_pinch_vertices'] == 0


def test_reference_hinge_gives_two_closed_tetrahedra():
    v, f, info = RR.split_nonmanifold(*TC.hinged_tetrahedra())
    assert (info['split_vertices'], info['added_vertices'], info['nonmanifold_edges_before']) == (2, 2, 1)
    assert f[:4].tolist() == TC.TETRA_F.tolist()           # the first tetrahedron holds the lowest slots of 2 and 3: it keeps them
    assert f[4:].tolist() == np.array([6, 7, 4, 5])[TC.TETRA_F].tolist()
    rep = TR.report(v, f)
    assert rep['components_vertex'] == 2 and rep['watertight'] and rep['euler_characteristic'] == 4


def test_reference_pinch_is_split_and_a_manifold_mesh_is_left_alone():
    v, f, info = RR.split_nonmanifold(*TC.pinched_tetrahedra())
    assert (info['split_vertices'], info['added_vertices'], info['nonmanifold_edges_before']) == (1, 1, 0)
    assert TR.report(v, f)['components_vertex'] == 2
    ico = RC.icosphere()
    v, f, info = RR.split_nonmanifold(*ico)
    assert info['added_vertices'] == 0 and np.array_equal(f, ico[1]) and np.array_equal(v, ico[0])
    with pytest.raises(ValueError):
        RR.split_nonmanifold(*RC.defects())


def test_reference_weld_of_the_soup_is_the_icosphere():
    ico = RC.icosphere()
    assert ico[1].shape == (320, 3) and TR.report(*ico)['watertight']
    for name in ('soup', 'jittered_soup'):
        v, f, eps, _ = MESHES[name]
        assert TR.report(v, f)['components_vertex'] == 320
        wv, wf, info = RR.weld(v, f, eps)
        assert np.array_equal(wv, v) and info['merged_vertices'] == 960 - 162 and info['clusters'] == 162
        assert info['cluster_radius_max'] <= eps and (info['cluster_radius_max'] > 0) == (name == 'jittered_soup')
        cv, cf, _ = RR.compact(wv, wf)
        assert np.array_equal(cf, ico[1])
        if name == 'soup':
            assert np.array_equal(cv, ico[0])


def test_reference_drop_degenerate_counts_every_reason():
    v, f = RC.defects()
    nv, nf, info = RR.drop_degenerate(v, f)
    assert (info['invalid_faces'], info['zero_area_faces'], info['nonfinite_faces'], info['duplicate_faces']) == (3, 1, 1, 2)
    assert info['kept_faces'].tolist() == [0, 1, 6, 7, 9] and np.array_equal(nf, f[[0, 1, 6, 7, 9]])
    assert np.array_equal(nv.view(np.uint32), v.view(np.uint32))


def test_reference_orientation():
    ico = RC.icosphere()
    v, f, info = RR.orient(*RC.every_third_flipped(ico))
    assert np.array_equal(f, ico[1]) and info['flipped_faces'] == 107 and info['non_orientable_pieces'] == 0
    assert info['conflicts_before'] == TR.report(*RC.every_third_flipped(ico))['orientation_conflicts'] > 0
    mv, mf = RC.moebius()
    v, f, info = RR.orient(mv, mf)
    assert np.array_equal(f, mf) and info['non_orientable_pieces'] == 1 and info['flipped_faces'] == 0
    tv, tf = RC.tied_strip()
    v, f, info = RR.orient(tv, tf)
    assert info['flipped_faces'] == 6 and not info['flipped'][0] and info['flipped'][1::2].all()       # the tie spares face 0's side
    assert TR.report(v, f)['orientation_conflicts'] == 0


@pytest.mark.parametrize("name", sorted(MESHES))
def test_reference_repair_leaves_no_defect_and_is_idempotent(name):
    v, f, eps, orientable = MESHES[name]
    rv, rf, info = RR.repair(v, f, weld_eps=eps)
    rep = TR.report(rv, rf)
    for key in ('invalid_faces', 'zero_area_faces', 'duplicate_faces', 'nonmanifold_edges', 'boundary_pinch_vertices',
                'unreferenced_vertices'):
        assert rep[key] == 0, key
    if orientable:
        assert rep['orientation_conflicts'] == 0
    else:
        assert rep['orientation_conflicts'] > 0 and info['orient']['non_orientable_pieces'] == 1
    assert np.array_equal(rv.view(np.uint32), v[info['origin']].view(np.uint32))
    again_v, again_f, again = RR.repair(rv, rf, weld_eps=eps)
    assert np.array_equal(again_v.view(np.uint32), rv.view(np.uint32)) and np.array_equal(again_f, rf)
    if name in ('soup', 'jittered_soup'):
        assert np.array_equal(rf, RC.icosphere()[1]) and rep['watertight']


# ---- the cell layout --------------------------------------------------------------------------------------------------------------
def test_grid_layout_keeps_the_cells_above_eps_and_the_table_small():
    from recmv import repair
    for lo, hi, eps, n in (([0, 0, 0], [1, 1, 1], 0.01, 1000), ([0, 0, 0], [1e6, 1e6, 1e6], 1e-6, 60), ([-5, 0, 2], [-5, 0, 2], 0., 300),
                           ([0, 0, 0], [1, 0, 0], 0., 6), ([0, 0, 0], [3e38, 1, 1], 1e-30, 10), ([0, 0, 0], [1, 1, 1], 1e300, 64),
                           ([-3e38, -3e38, -3e38], [3e38, 3e38, 3e38], 0., 1 << 24)):
        origin, cell, dims = repair.grid_layout(lo, hi, eps, n)
        assert origin == [float(x) for x in lo] and cell > 0 and cell >= eps * (1 + 2. ** -20) and np.isfinite(cell)
        assert all(1 <= d <= 1 << 20 for d in dims)
        assert dims[0] * dims[1] * dims[2] <= min(1 << 24, max(4 * n, 64))
        assert all(int((h - l) / cell) < d for l, h, d in zip(lo, hi, dims))       # the far corner has a cell of its own
    assert repair.grid_layout([0, 0, 0], [1, 1, 1], 0.1, 10 ** 6)[2] == (10, 10, 10)
    assert repair.grid_layout([0, 0, 0], [1e6, 1e6, 1e6], 1e-6, 60)[2] == (4, 4, 4)  # coarser cells, not 10^36 of them


# ---- argument checks --------------------------------------------------------------------------------------------------------------
def test_wrappers_check_their_arguments_before_they_need_a_gpu():
    from recmv import repair
    v, f = (torch.from_numpy(x) for x in TC.tetrahedron())
    for eps in (-1., float('nan'), float('inf')):
        with pytest.raises(ValueError, match="finite and not negative"):
            repair.points_within(v, eps)
        with pytest.raises(ValueError, match="finite and not negative"):
            repair.weld(v, f, eps)
        with pytest.raises(ValueError, match="weld_eps"):
            repair.repair(v, f, weld_eps=eps)
    with pytest.raises(ValueError, match="max_pairs"):
        repair.points_within(v, 0.1, max_pairs=-1)
    for bad in (v.double(), v[:, :2], v.reshape(-1), v.numpy()):
        with pytest.raises(ValueError, match="float32 of shape"):
            repair.points_within(bad, 0.1)
    for fn in (repair.drop_degenerate, repair.split_nonmanifold, repair.orient, repair.repair, repair.weld):
        with pytest.raises(ValueError, match="float32 of shape"):
            fn(v.double(), f)
        with pytest.raises(RuntimeError, match="CUDA"):    # no CPU path: a missing GPU is an error, not a fall-back
            fn(v, f)
    with pytest.raises(RuntimeError, match="CUDA"):
        repair.points_within(v, 0.1)


def test_info_json_keeps_the_numbers_and_drops_the_tensors():
    from recmv import repair
    info = {'weld': {'pairs': 3, 'vertex_map': torch.arange(3), 'cluster_radius_max': 0.5}, 'kept_faces': torch.arange(2), 'dims': (1, 2, 3)}
    assert repair.info_json(info) == {'weld': {'pairs': 3, 'cluster_radius_max': 0.5}, 'dims': [1, 2, 3]}


def test_clean_fl_carries_the_new_flags_and_they_default_to_off(tmp_path, capsys):
    import clean_fl
    a = clean_fl.build_parser().parse_args(["--in", "x", "--out", "y"])
    assert (a.repair, a.weld_eps) == (False, None)
    a = clean_fl.build_parser().parse_args(["--in", "x", "--out", "y", "--repair", "--weld-eps", "1e-4"])
    assert (a.repair, a.weld_eps) == (True, 1e-4)
    me = str(HERE / "mesh_repair_reference.py")            # any existing file: the usage errors come before it is read
    for bad in (["--report-only", "--repair"], ["--report-only", "--weld-eps", "0"], ["--out", str(tmp_path), "--weld-eps", "-1"],
                ["--out", str(tmp_path), "--weld-eps", "nan"], ["--out", str(tmp_path), "--weld-eps", "inf"]):
        with pytest.raises(SystemExit):
            clean_fl.main(["--in", me] + bad)
    assert "clean_fl.py" in clean_fl.__doc__ and "--repair" in clean_fl.__doc__ and "--weld-eps" in clean_fl.__doc__
    capsys.readouterr()


def test_eval_fl_carries_the_new_flags_and_they_default_to_off(capsys):
    import eval_fl
    a = eval_fl.build_parser().parse_args(["--pred", "x", "--gt", "y"])
    assert (a.repair, a.weld_eps) == (False, None)
    a = eval_fl.build_parser().parse_args(["--pred", "x", "--gt", "y", "--weld-eps", "0"])
    assert (a.repair, a.weld_eps) == (False, 0.)
    me = str(HERE / "mesh_repair_reference.py")
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            eval_fl.main(["--pred", me, "--gt", me, "--weld-eps", bad])
    assert "--repair" in eval_fl.__doc__ and "--weld-eps" in eval_fl.__doc__
    capsys.readouterr()


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("recmv_points_within_cells", "recmv_points_within_count", "recmv_points_within_fill", "recmv_points_within_max_cells")


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION == 11
    assert lib.recmv_points_within_max_cells() == 1 << 24
    hdr = (REPO / "include" / "recmv_hip.h").read_text()
    assert "recmv_points_within_cells, recmv_points_within_count, recmv_points_within_fill" in hdr.split("v10:")[0]   # the history note


def test_argument_errors_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    one = C.c_void_p(16)                                   # a non-NULL pointer that is never followed
    err = lib.recmv_last_error

    def cells(V=3, o=(0., 0., 0.), cell=1., dims=(2, 2, 2), ptrs=(one, one)):
        return lib.recmv_points_within_cells(ptrs[0], V, *o, cell, *dims, ptrs[1], None)
    assert cells(V=-1) == -1 and b"V=-1" in err()
    assert cells(V=1 << 31) == -1 and b"2^31" in err()
    assert cells(o=(0., float("nan"), 0.)) == -1 and b"origin" in err()
    assert cells(cell=0.) == -1 and b"cell=0" in err()
    assert cells(cell=float("inf")) == -1 and b"cell=inf" in err()
    assert cells(dims=(0, 1, 1)) == -1 and b"every axis" in err()
    assert cells(dims=((1 << 20) + 1, 1, 1)) == -1 and b"every axis" in err()
    assert cells(dims=(1 << 10, 1 << 10, 1 << 5)) == -1 and b"2^24" in err()
    assert cells(ptrs=(None, one)) == -1 and b"NULL" in err()
    assert cells(ptrs=(one, None)) == -1 and b"NULL" in err()
    assert cells(V=0, ptrs=(None, None)) == 0

    def count(n=3, V=3, eps=0.5, o=(0., 0., 0.), cell=1., dims=(2, 2, 2), ptrs=(one, one, one), out=one):
        return lib.recmv_points_within_count(ptrs[0], ptrs[1], n, V, eps, *o, cell, *dims, ptrs[2], out, None)

    def fill(n=3, V=3, eps=0.5, o=(0., 0., 0.), cell=1., dims=(2, 2, 2), ptrs=(one, one, one), out=(one, one), P=4):
        return lib.recmv_points_within_fill(ptrs[0], ptrs[1], n, V, eps, *o, cell, *dims, ptrs[2], out[0], out[1], P, None)
    for fn, name in ((count, b"points_within_count"), (fill, b"points_within_fill")):
        assert fn(n=-1) == -1 and b"n=-1" in err() and name in err()
        assert fn(V=-2) == -1 and b"V=-2" in err()
        assert fn(n=4) == -1 and b"n=4 sorted vertices of V=3" in err()
        assert fn(V=1 << 31) == -1 and b"2^31" in err()
        assert fn(eps=-0.5) == -1 and b"eps=-0.5" in err()
        assert fn(eps=float("nan")) == -1 and b"eps=nan" in err()
        assert fn(eps=float("inf")) == -1 and b"eps=inf" in err()
        assert fn(eps=2.) == -1 and b"below eps" in err()
        assert fn(cell=-1.) == -1 and b"cell=-1" in err()
        assert fn(dims=(1, 1, -3)) == -1 and b"every axis" in err()
        assert fn(dims=(1 << 20, 1 << 20, 1)) == -1 and b"2^24" in err()
        for k in range(3):
            assert fn(ptrs=tuple(None if i == k else one for i in range(3))) == -1 and b"NULL" in err()
    assert count(out=None) == -1 and b"NULL counts" in err()
    assert count(n=0, V=0, ptrs=(None, None, None), out=None) == 0
    assert fill(P=-1) == -1 and b"P=-1" in err()
    assert fill(out=(None, one)) == -1 and b"NULL" in err()
    assert fill(out=(one, None)) == -1 and b"NULL" in err()
    assert fill(n=0, ptrs=(None, None, None), out=(None, None)) == 0
    assert fill(P=0, out=(None, None)) == 0


# ---- the kernels on the host ------------------------------------------------------------------------------------------------------
def test_host_build_of_the_kernels_under_the_sanitizers(tmp_path):
    """tools/mesh_repair_host_check: csrc/point_grid.hip's kernels compiled for the CPU under the address and
    undefined-behaviour sanitizers, a stand-alone program: the shapes of the GPU test against the O(V^2) loop, a second run, and
    every table filled with random numbers."""
    r = host_check.run("mesh_repair", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(" 0 mismatches") == 15
    for name in ("V=0:", "V=1:", "V=2:", "V=255:", "V=256:", "V=257:", "300 coincident: 300 vertices, 0 not finite, 1 x 1 x 1 cells",
                 "44850 pairs", "lattice:", "lattice negative:", "lattice straddling 0:", "540 pairs", "signed zeros:", "4 pairs",
                 "nan and inf: 40 vertices, 4 not finite", "two clusters 1e6 apart: 60 vertices, 0 not finite, 4 x 4 x 4 cells",
                 "eps beyond the box", "2016 pairs", "random tables"):
        assert name in r.stdout
