"""Mesh evaluation metrics without a GPU: the float64 restatement (tests/mesh_metrics_reference.py) on hand-computed cases,
the argument checks of the three new C entry points, the grid the wrapper chooses, eval_fl.py's pairing of files, and the
refusal of CPU tensors."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import collide_reference as CR  # noqa: E402
import host_check  # noqa: E402
import mesh_metrics_reference as MR  # noqa: E402


def test_reference_on_two_parallel_unit_squares():
    """Two unit squares over each other, h apart: every sample is h from the other surface, so accuracy = completeness =
    chamfer_l1 = h, chamfer_l2 = 2 h^2, the normals agree, and F = 1 for a threshold above h, 0 below."""
    h = 0.125
    av, af = MR.square(0., n=3)
    bv, bf = MR.square(h, n=2)
    ap, asrc = MR.sample(av, af, 500, 0)
    bp, bsrc = MR.sample(bv, bf, 500, 1)
    m = MR.surface_distance(ap, asrc, av, af, bp, bsrc, bv, bf, (0.5 * h, 2 * h))
    for key in ('accuracy', 'completeness', 'chamfer_l1', 'accuracy_rms', 'completeness_rms', 'accuracy_max'):
        assert abs(m[key] - h) < 1e-12, (key, m[key])
    assert abs(m['chamfer_l2'] - 2 * h * h) < 1e-12
    assert abs(m['normal_consistency'] - 1.) < 1e-12
    assert m['fscore_%g' % (2 * h)] == 1. and m['precision_%g' % (2 * h)] == 1. and m['recall_%g' % (2 * h)] == 1.
    assert m['fscore_%g' % (0.5 * h)] == 0. and m['precision_%g' % (0.5 * h)] == 0.


def test_reference_on_a_tilted_square():
    """A square against the same square turned by theta about its edge y = 0: both are flat, so the normal consistency is
    cos(theta) in both directions; a sample at height y of the turned square is y sin(theta) from the flat one (its foot
    (x, y cos(theta)) lies inside the square), so completeness = sin(theta) / 2 over uniform samples — checked on the
    samples' own mean height."""
    theta = 0.3
    av, af = MR.square(0., n=2)
    bv, bf = MR.square(0., tilt=theta, n=2)
    ap, asrc = MR.sample(av, af, 400, 2)
    bp, bsrc = MR.sample(bv, bf, 400, 3)
    m = MR.surface_distance(ap, asrc, av, af, bp, bsrc, bv, bf, (0.1,))
    for key in ('normal_consistency', 'normal_consistency_pred_to_gt', 'normal_consistency_gt_to_pred'):
        assert abs(m[key] - math.cos(theta)) < 1e-12, (key, m[key])
    assert abs(m['completeness'] - bp[:, 2].mean()) < 1e-12
    # from the flat square, a sample at (x, y) is y sin(theta) from the turned one while its foot y cos(theta) is inside it
    assert abs(m['accuracy'] - (ap[:, 1] * math.sin(theta)).mean()) < 1e-12
    assert abs(m['recall_0.1'] - (bp[:, 2] <= 0.1).mean()) < 1e-12


def test_reference_search_equals_the_brute_force():
    rng = np.random.RandomState(0)
    v = rng.randn(60, 3)
    f = rng.randint(0, 60, (150, 3))
    f[100:110] = f[:10]                                    # duplicates: the lowest index
    p = rng.randn(300, 3) * 1.5
    p[:20] = v[:20]                                        # on vertices: ties between the faces around them
    face, d2 = MR.nearest(p, v, f)
    face0, d20, _, _ = CR.nearest(p, v, f)
    assert np.array_equal(face, face0) and np.array_equal(d2, d20)


ONE = C.c_void_p(16)                                       # a non-NULL pointer that is never followed


def grid_desc(origin=(0., 0., 0.), h=1., dims=(2, 2, 2), offsets=16, entries=16, n_entries=7, tris=16):
    """A recmv_mesh_grid whose pointers are never followed (the argument checks come before any HIP call)."""
    from recmv import _lib
    d = _lib.MeshGridDesc()
    d.origin[:] = origin
    d.cell_size, (d.nx, d.ny, d.nz) = h, dims
    d.offsets, d.entries, d.n_entries, d.tris = offsets, entries, n_entries, tris
    return d


def test_argument_errors_of_the_grid_entry_points_do_not_need_a_gpu():
    """Negative sizes, NULL pointers with non-zero sizes, dims below 1 and a non-positive cell size are found before any HIP
    call and reported through recmv_last_error."""
    from recmv import _lib
    lib = _lib.lib()
    one = ONE
    assert lib.recmv_mesh_grid_workspace_bytes(0) == 0 and lib.recmv_mesh_grid_workspace_bytes(1025) == (1025 + 2) * 4

    def count(*, mesh=(one, 3, one, 1), out=(one, one), null=False, **grid):
        return lib.recmv_mesh_grid_count(*mesh, None if null else C.byref(grid_desc(**{'dims': (1, 1, 1), **grid})), *out, None)
    assert count(mesh=(None, -1, None, 0)) == -1
    assert b"V=-1" in lib.recmv_last_error()
    assert count(dims=(0, 1, 1)) == -1
    assert b"dims=(0,1,1)" in lib.recmv_last_error()
    assert count(h=0.) == -1
    assert b"cell size" in lib.recmv_last_error()
    assert count(h=float("nan")) == -1
    assert count(null=True) == -1
    assert b"grid" in lib.recmv_last_error()
    assert count(out=(None, one)) == -1
    assert b"NULL" in lib.recmv_last_error()
    assert count(mesh=(one, 3, None, 1)) == -1
    assert b"NULL" in lib.recmv_last_error()
    assert count(dims=(1 << 20, 1 << 20, 1)) == -1
    assert b"cells" in lib.recmv_last_error()

    def fill(*, ws=64, **grid):
        d = grid_desc(**{'dims': (1, 1, 1), 'n_entries': 1, **grid})
        return lib.recmv_mesh_grid_fill(one, 3, one, 1, C.byref(d), one, one, ws, None)
    assert fill(n_entries=-1) == -1                        # the capacity of entries
    assert b"entries=-1" in lib.recmv_last_error()
    assert fill(dims=(1, 1, -2)) == -1
    assert b"dims" in lib.recmv_last_error()
    assert fill(h=-1.) == -1
    assert b"cell size" in lib.recmv_last_error()
    assert fill(entries=None) == -1
    assert b"NULL" in lib.recmv_last_error()
    assert fill(ws=4) == -1
    assert b"workspace" in lib.recmv_last_error()

    def query(*, p=one, P=4, F=5, lanes=1, **grid):
        return lib.recmv_closest_point_grid(p, P, one, F, C.byref(grid_desc(**grid)), lanes, one, one, one, None)
    assert query(P=0) == 0                                 # P = 0 is a no-op
    assert query(P=-1) == -1
    assert b"P=-1" in lib.recmv_last_error()
    assert query(F=0) == -1
    assert b"must not be empty" in lib.recmv_last_error()
    assert query(dims=(2, 0, 2)) == -1
    assert b"dims" in lib.recmv_last_error()
    assert query(h=0.) == -1
    assert b"cell size" in lib.recmv_last_error()
    assert query(lanes=3) == -1
    assert b"lanes" in lib.recmv_last_error()
    assert query(p=None) == -1
    assert b"NULL" in lib.recmv_last_error()
    assert query(entries=None) == -1
    assert b"NULL" in lib.recmv_last_error()


# every entry point that takes a recmv_mesh_grid: (call(lib, descriptor or None), whether it reads or writes the tables)
_MESH = (ONE, 3, ONE, 1)
_MESH_B = (C.c_void_p(32), 3, C.c_void_p(32), 1)
GRID_ENTRY_POINTS = {
    "mesh_grid_count": (lambda lib, g: lib.recmv_mesh_grid_count(*_MESH, g, ONE, ONE, None), False),
    "mesh_grid_fill": (lambda lib, g: lib.recmv_mesh_grid_fill(*_MESH, g, ONE, ONE, 1 << 20, None), True),
    "closest_point_grid": (lambda lib, g: lib.recmv_closest_point_grid(ONE, 4, ONE, 5, g, 1, ONE, ONE, ONE, None), True),
    "mesh_intersect_grid_count": (
        lambda lib, g: lib.recmv_mesh_intersect_grid_count(*_MESH, *_MESH_B, g, 1, 0, 0, ONE, ONE, None), True),
    "mesh_intersect_grid_fill": (
        lambda lib, g: lib.recmv_mesh_intersect_grid_fill(*_MESH, *_MESH_B, g, 8, 0, 0, ONE, ONE, 4, ONE, ONE, None), True),
    "segment_mesh_grid": (lambda lib, g: lib.recmv_segment_mesh_grid(ONE, ONE, 4, *_MESH, g, 1, 0, ONE, ONE, None, None), True),
}
MALFORMED_GRIDS = {
    "NULL descriptor": None,
    "ny = 0": dict(dims=(2, 0, 2)),
    "cell size 0": dict(h=0.),
    "cell size NaN": dict(h=float("nan")),
    "cell size inf": dict(h=float("inf")),
    "2^20 x 2^20 x 1 cells": dict(dims=(1 << 20, 1 << 20, 1)),
    "n_entries = -1": dict(n_entries=-1),
    "NULL offsets": dict(offsets=None),
}


@pytest.mark.parametrize("name", sorted(GRID_ENTRY_POINTS))
def test_one_validator_rejects_a_malformed_descriptor_alike_in_every_entry_point(name):
    """Every malformed descriptor is an argument error in every entry point that takes one, found before any HIP call, and the
    message is the same text apart from the entry point's name (compared with recmv_closest_point_grid's, which reads every
    field): the descriptor is checked in one place.  NULL offsets only where the tables are read or written."""
    from recmv import _lib
    lib = _lib.lib()

    def text(entry, grid):
        call, _ = GRID_ENTRY_POINTS[entry]
        rc = call(lib, None if grid is None else C.byref(grid_desc(**grid)))
        msg = lib.recmv_last_error().decode()
        assert rc == -1 and msg.startswith(entry + ": "), (entry, rc, msg)          # RECMV_ERR_ARG
        return msg[len(entry) + 2:]
    for case, grid in MALFORMED_GRIDS.items():
        if case == "NULL offsets" and not GRID_ENTRY_POINTS[name][1]:
            continue
        assert text(name, grid) == text("closest_point_grid", grid), case


def test_host_build_of_the_grid_kernels_returns_the_brute_force_bits(tmp_path):
    """tools/mesh_grid_host_check: csrc/mesh_grid.hip's count, fill and one-lane query kernels compiled for the CPU under the
    address and undefined-behaviour sanitizers against a brute force with the same closest_tri.h and grid_query.h, bit for bit,
    on seven meshes and grids."""
    r = host_check.run("mesh_grid", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(" 0 mismatches") == 7, r.stdout + r.stderr


def test_the_chosen_grid():
    from recmv import metrics
    h, dims = metrics.choose_grid((0, 0, 0), (1, 1, 1), 6000)
    assert dims[0] == dims[1] == dims[2] and abs(h - math.sqrt(6 * metrics.FACES_PER_CELL / 6000)) < 1e-6
    assert all(d * h >= 1. for d in dims)                  # the cells cover the box
    h, dims = metrics.choose_grid((0, 0, 2), (4, 1, 2), 800)                     # a flat mesh: one cell along z
    assert dims[2] == 1 and dims[0] > dims[1] > 1 and dims[0] * h >= 4.
    h, dims = metrics.choose_grid((1, 1, 1), (1, 1, 1), 10)                      # a point
    assert dims == (1, 1, 1) and h > 0
    h, dims = metrics.choose_grid((0, 0, 0), (1, 1, 1), 10 ** 9)                 # capped: the offsets table stays small
    assert dims[0] * dims[1] * dims[2] <= metrics.MAX_CELLS and all(d * h >= 1. for d in dims)
    with pytest.raises(ValueError):
        metrics.choose_grid((0, 0, 0), (float("inf"), 1, 1), 10)
    assert metrics.use_grid('grid', 1, 1) and not metrics.use_grid('brute', 10 ** 9, 10 ** 9)
    assert metrics.use_grid('auto', 1, 1) == (1 >= metrics.AUTO_GRID_MIN_TESTS)
    with pytest.raises(ValueError):
        metrics.use_grid('fast', 1, 1)


def test_eval_fl_pairs_files_by_stem(tmp_path):
    import eval_fl
    pred, gt, empty = tmp_path / "pred", tmp_path / "gt", tmp_path / "empty"
    for d in (pred, gt, empty):
        d.mkdir()
    for name in ("a.obj", "b.obj", "only_pred.obj", "notes.txt"):
        (pred / name).write_text("")
    for name in ("b.obj", "a.obj", "only_gt.obj"):
        (gt / name).write_text("")
    pairs, only_pred, only_gt = eval_fl.pair_files(str(pred), str(gt))
    assert [(s, Path(p).name, Path(g).name) for s, p, g in pairs] == [("a", "a.obj", "a.obj"), ("b", "b.obj", "b.obj")]
    assert [Path(p).name for p in only_pred] == ["only_pred.obj"] and [Path(g).name for g in only_gt] == ["only_gt.obj"]
    with pytest.raises(ValueError):                        # nothing pairs
        eval_fl.pair_files(str(pred), str(empty))
    with pytest.raises(ValueError):                        # a file against a directory
        eval_fl.pair_files(str(pred / "a.obj"), str(gt))
    pairs, _, _ = eval_fl.pair_files(str(pred / "a.obj"), str(gt / "only_gt.obj"))   # two files are one pair
    assert len(pairs) == 1 and pairs[0][0] == "a"
    with pytest.raises(SystemExit):                        # the command reports it as a usage error, before any device work
        eval_fl.main(["--pred", str(pred), "--gt", str(empty)])


def test_metrics_refuse_cpu_tensors():
    from recmv import metrics
    v, f = MR.square(0., n=2)
    v, f = torch.from_numpy(v).float(), torch.from_numpy(f)
    with pytest.raises(RuntimeError):
        metrics.MeshGrid(v, f)
    with pytest.raises(RuntimeError):
        metrics.surface_distance(v, f, v, f, samples=10)
