"""Geodesic distance without a GPU: the numpy restatement (tests/geodesic_reference.py) on hand cases, its bounds (Euclidean from
below, the edge-graph Dijkstra from above, K <= V) and its accuracy against the plane; the plain-torch helpers; every ValueError
of recmv.geodesic; the C entry points (declared, exported, argument errors and empty no-ops before any HIP call); eval_fl.py's
--boundary-bands parser and binning; and the host build of the kernels under the sanitizers.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import geodesic_cases as GC  # noqa: E402
import geodesic_reference as GR  # noqa: E402
import host_check  # noqa: E402

INF = float("inf")
NAMES = ["recmv_geodesic_lds_max_vertices", "recmv_geodesic_auto_max_vertices", "recmv_geodesic_workspace_bytes",
         "recmv_geodesic_check_sources", "recmv_geodesic_sweeps", "recmv_geodesic_lds"]
# The largest relative error of the restatement against the plane on the flat grids with a corner source, measured from the
# restatement alone: it is first-order, set by the vertices next to the source, and the same on all three grids.
MEASURED_PLANE_MAX = 0.05126546140181058
MEASURED_PLANE_MEAN = {9: 0.016706157200426158, 17: 0.012942214873373794, 33: 0.00897256886493427}


# ------------------------------------------------------------------------------------------------------ the restatement
def test_hand_cases():
    D, K = GR.distance(*GC.triangle(), [0])
    assert D.tolist() == [0., 3., 4.] and K == 1
    D, K = GR.distance(*GC.square(False), [0])                                    # the planar update across the diagonal
    assert D[1] == 1. and D[3] == 1. and abs(D[2] - (1. + 2. ** 0.5 / 2.)) <= 1e-15 and K == 2
    D, K = GR.distance(*GC.square(True), [0])
    assert D[2] == np.float64(2.) ** 0.5 and K == 1
    v, f = GC.cylinder()
    assert v.shape == (24 * 9, 3)
    D, K = GR.distance(v, f, list(range(24)))
    assert np.abs(D - v[:, 2].astype(np.float64)).max() <= 1e-12 and K == 8
    D, K = GR.distance(v, f, list(range(24)) + list(range(192, 216)))
    assert D.max() == 1.0 and K == 4


def test_sources_values_duplicates_and_unusable_input():
    v, f = GC.grid(9, jitter=0.3, noise=0.02, seed=3)
    D, _ = GR.distance(v, f, [0, 80, 0, 40], [0.5, 0., 0.25, 3.])
    assert D[0] == 0.25 and D[80] == 0. and D[40] < 3.                            # of duplicates the least; a value can be undercut
    D, K = GR.distance(v, f, [])
    assert np.isinf(D).all() and K == 0
    v, f = GC.two_pieces()
    D, _ = GR.distance(v, f, [3])
    assert np.isfinite(D[:36]).all() and np.isinf(D[36:]).all()
    v, f = GC.broken()
    ok = GR.usable_faces(v, f)                                                    # faces without area are usable: they carry their edges
    assert ok[-7:].tolist() == [False, False, False, False, True, True, False]
    assert (~ok).sum() == 5 + (f[:-7] == 24).any(1).sum() and (f[:-7] == 24).any(1).sum() >= 4               # and the NaN vertex's faces
    D, _ = GR.distance(v, f, [0])
    assert np.isinf(D[24]) and np.isfinite(np.delete(D, 24)).all()
    assert GR.distance(v, f, [24])[0][24] == 0.                                   # a source keeps its value
    with pytest.raises(ValueError):
        GR.distance(*GC.grid(9), [0], max_sweeps=14)
    assert GR.distance(*GC.grid(9), [0], max_sweeps=15)[1] == 15


BOUND_MESHES = {"flat": lambda: GC.grid(17), "jittered": lambda: GC.grid(17, jitter=0.48, noise=0.05, seed=1),
                "icosphere": lambda: GC.icosphere(2)}


@pytest.mark.parametrize("name", sorted(BOUND_MESHES))
def test_bounds_from_a_single_source(name):
    v, f = BOUND_MESHES[name]()
    V = v.shape[0]
    assert V == (162 if name == "icosphere" else 289)
    for s in (0, V // 2):
        D, K = GR.distance(v, f, [s])
        eu = np.sqrt(((v.astype(np.float64) - v[s].astype(np.float64)) ** 2).sum(1))
        dj = GR.dijkstra(v, f, [s])
        print(name, s, "K", K, "min D / euclid", (D[eu > 0] / eu[eu > 0]).min(), "max D / dijkstra", (D[dj > 0] / dj[dj > 0]).max())
        assert (D >= eu * (1. - 1e-12)).all()
        assert (D <= dj * (1. + 1e-12)).all()
        assert K <= V


def test_the_jittered_grid_has_obtuse_angles():
    v, f = GC.grid(17, jitter=0.48, noise=0.05, seed=1)
    p = v.astype(np.float64)[f]
    worst = 0.
    for k in range(3):
        a, b = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
        cos = (a * b).sum(1) / np.sqrt((a * a).sum(1) * (b * b).sum(1))
        worst = max(worst, float(np.degrees(np.arccos(cos.min()))))
    assert worst > 160.                                                           # 163.9 degrees


def test_accuracy_against_the_plane():
    means, maxes = [], []
    for n in (9, 17, 33):
        v, f = GC.grid(n)
        D, K = GR.distance(v, f, [0])
        exact = np.sqrt((v.astype(np.float64) ** 2).sum(1))
        rel = np.abs(D[1:] - exact[1:]) / exact[1:]
        dj = GR.dijkstra(v, f, [0])
        print(n, "K", K, "mean", rel.mean(), "max", rel.max(), "dijkstra max", (np.abs(dj[1:] - exact[1:]) / exact[1:]).max())
        means.append(rel.mean())
        maxes.append(rel.max())
        assert abs(rel.mean() - MEASURED_PLANE_MEAN[n]) <= 1e-9
        assert rel.max() <= MEASURED_PLANE_MAX * 1.1
        assert rel.max() < (np.abs(dj[1:] - exact[1:]) / exact[1:]).max()
        if n == 33:
            assert K == 54
    assert means[0] > means[1] > means[2]
    assert max(maxes) >= MEASURED_PLANE_MAX * 0.999                               # the recorded figure is the measured one
    assert GR.distance(*GC.icosphere(3), [0])[1] == 24


# ------------------------------------------------------------------------------------------------------------ helpers
def test_nearest_source_ties_and_unreached():
    from recmv import geodesic
    fields = torch.tensor([[1., INF, 2., 5.], [1., INF, 1., 7.], [0.5, INF, 1., 5.]], dtype=torch.float64)
    best, label = geodesic.nearest_source(fields)
    assert best.tolist() == [0.5, INF, 1., 5.] and label.tolist() == [2, -1, 1, 0] and label.dtype == torch.int64
    want = GR.nearest_source(fields.numpy())
    assert best.tolist() == want[0].tolist() and label.tolist() == want[1].tolist()
    best, label = geodesic.nearest_source(torch.zeros(0, 3, dtype=torch.float64))
    assert best.tolist() == [INF] * 3 and label.tolist() == [-1] * 3
    with pytest.raises(ValueError):
        geodesic.nearest_source(torch.zeros(3))


def test_interpolate_at_corners_an_edge_midpoint_and_with_an_inf_corner():
    from recmv import geodesic
    v = torch.tensor([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [1, 3, 2]])
    field = torch.tensor([1., 3., 5., INF], dtype=torch.float64)
    pts = torch.tensor([[0, 0, 0], [2, 0, 0], [0, 2, 0], [1, 0, 0], [1, 1, 0], [0.5, 0.5, 0], [1.5, 1.5, 0], [2, 0, 0]],
                       dtype=torch.float32)
    ids = torch.tensor([0, 0, 0, 0, 0, 0, 1, 1])
    got = geodesic.interpolate(field, v, f, ids, pts)
    assert got.dtype == torch.float64
    assert got.tolist() == [1., 3., 5., 2., 4., 2.5, INF, INF]
    with pytest.raises(ValueError):
        geodesic.interpolate(field[:3], v, f, ids, pts)
    with pytest.raises(ValueError):
        geodesic.interpolate(field, v, f, ids[:3], pts)


def test_farthest_points_order_on_a_small_grid():
    v, f = GC.grid(5)
    ids, run = GR.farthest_points(v, f, 5, first=0)
    assert ids[:2] == [0, 24] and set(ids[2:4]) == {4, 20} and ids[2] == 4 and ids[4] == 12       # corners, lowest id first, then the centre
    assert run[ids].tolist() == [0.] * 5 and run.max() <= 0.5
    ids, run = GR.farthest_points(v, f, 100, first=0)
    assert sorted(ids) == list(range(25)) and run.max() == 0.                     # stops when only 0 remains
    ids, run = GR.farthest_points(*GC.two_pieces(), 100, first=40)
    assert sorted(ids) == list(range(36, 52)) and np.isinf(run[:36]).all()        # inf is never a maximum


# ------------------------------------------------------------------------------------------------ recmv.geodesic's arguments
def test_argument_errors_and_cpu_tensors():
    from recmv import geodesic
    assert geodesic.ROUTES == ('auto', 'sweeps', 'lds') and geodesic.lds_max_vertices() == 3640
    assert 0 < geodesic.auto_max_vertices() <= 3640
    v, f = (torch.from_numpy(x) for x in GC.grid(5))
    s = torch.tensor([0])
    bad = [lambda: geodesic.distance(v, f, s, route='fast'),
           lambda: geodesic.distance(v.double(), f, s), lambda: geodesic.distance(v[:, :2], f, s),
           lambda: geodesic.distance(v, f.int(), s), lambda: geodesic.distance(v, f[:, :2], s),
           lambda: geodesic.distance(v, f, torch.tensor([25])), lambda: geodesic.distance(v, f, torch.tensor([-1])),
           lambda: geodesic.distance(v, f, torch.tensor([0, 1]), torch.tensor([0., INF])),
           lambda: geodesic.distance(v, f, torch.tensor([0, 1]), torch.tensor([0., float("nan")])),
           lambda: geodesic.distance(v, f, torch.tensor([0, 1]), torch.tensor([0.])),
           lambda: geodesic.distance(v, f, torch.tensor([0, 1]), torch.tensor([0, 1])),
           lambda: geodesic.distance(v, f, torch.tensor([0], dtype=torch.int32)),
           lambda: geodesic.distance(v, f, torch.tensor([[0]])),
           lambda: geodesic.distance(v, f, [s, s], [torch.tensor([0.])]),
           lambda: geodesic.distance(v, f, [s, torch.tensor([99])]),
           lambda: geodesic.distance(v, f, s, max_sweeps=-1), lambda: geodesic.distance(v, f, s, check_every=0),
           lambda: geodesic.distance(torch.zeros(3641, 3), f, s, route='lds'),
           lambda: geodesic.farthest_points(v, f, -1), lambda: geodesic.farthest_points(v, f, 2, first=25),
           lambda: geodesic.farthest_points(v, f, 2, route='fast'), lambda: geodesic.boundary_distance(v, f, route='fast')]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d raised nothing" % k)
    with pytest.raises(ValueError, match=r"source 1 is vertex 25, outside \[0, 25\)"):
        geodesic.distance(v, f, torch.tensor([3, 25]))
    with pytest.raises(ValueError, match="value of source 0 is not finite"):
        geodesic.distance(v, f, s, torch.tensor([-INF]))
    for call in (lambda: geodesic.distance(v, f, s), lambda: geodesic.distance(v, f, [s, s], route='sweeps'),
                 lambda: geodesic.boundary_distance(v, f), lambda: geodesic.boundary_distance(v, f, per_loop=True),
                 lambda: geodesic.farthest_points(v, f, 3)):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            call()


# ------------------------------------------------------------------------------------------------------------ the C ABI
ONE = C.c_void_p(64)                                                              # a pointer nobody reads: the errors come first


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in NAMES:
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION == 11
    hdr = (REPO / "include" / "recmv_hip.h").read_text()
    note = hdr[:hdr.index("int recmv_abi_version")]
    for n in NAMES:
        assert n in note
    assert "(geodesic distance fields: pure additions, still v11)" in note
    assert lib.recmv_geodesic_lds_max_vertices() == 3640 == (65536 - 16) // 18


def test_a_library_without_the_symbols_is_rejected():
    from recmv import _lib

    class Partial:
        def __getattr__(self, name):
            if name.startswith("recmv_geodesic"):
                raise AttributeError(name)
            return getattr(_lib.lib(), name)
    with pytest.raises(AttributeError, match="recmv_geodesic"):
        _lib._declare(Partial())


def test_c_argument_errors_and_empty_inputs_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    err = lib.recmv_last_error
    wb = lib.recmv_geodesic_workspace_bytes
    assert wb(10, 5, 3) == 16 * 30 + 2 * 32 + 16 and wb(8, 0, 1) == 128 + 16 + 8 and wb(0, 5, 3) == 16 and wb(7, 5, 0) == 0
    assert wb(-1, 5, 3) == -1 and b"V=-1" in err()
    assert wb(1, -5, 3) == -1 and b"F=-5" in err()
    assert wb(1, 5, -3) == -1 and b"B=-3" in err()
    assert wb(1 << 31, 5, 1) == -1 and b"2^31" in err()
    assert wb(1 << 20, 5, 1 << 20) == -1 and b"2^38" in err()

    src, val = (C.c_int64 * 3)(0, 4, 2), (C.c_double * 3)(0., 1., 2.)
    cs = lib.recmv_geodesic_check_sources
    assert cs(src, val, 3, 5) == 0 and cs(src, None, 3, 5) == 0 and cs(None, None, 0, 5) == 0 and cs(None, None, 0, 0) == 0
    assert cs(src, val, 3, 4) == -1 and b"source 1 is vertex 4, outside [0, 4)" in err()
    assert cs((C.c_int64 * 1)(-1), None, 1, 4) == -1 and b"vertex -1" in err()
    for x in (INF, -INF, float("nan")):
        assert cs(src, (C.c_double * 3)(0., 1., x), 3, 5) == -1 and b"value of source 2 is not finite" in err()
    assert cs(src, val, -3, 5) == -1 and b"S=-3" in err()
    assert cs(src, val, 3, -5) == -1 and b"V=-5" in err()
    assert cs(None, None, 2, 5) == -1 and b"NULL sources" in err()

    need = wb(10, 5, 3)

    def sweeps(*, mesh=(ONE, 10, ONE, 5, ONE, ONE), B=3, ws=(ONE, need), k0=0, n=4):
        return lib.recmv_geodesic_sweeps(*mesh, B, *ws, k0, n, None)
    assert sweeps(mesh=(ONE, -10, ONE, 5, ONE, ONE)) == -1 and b"V=-10" in err()
    assert sweeps(mesh=(ONE, 10, ONE, -5, ONE, ONE)) == -1 and b"F=-5" in err()
    assert sweeps(B=-3) == -1 and b"B=-3" in err()
    assert sweeps(k0=-1) == -1 and b"k0=-1" in err()
    assert sweeps(n=-2) == -1 and b"n=-2" in err()
    assert sweeps(n=(1 << 30) + 1) == -1 and b"2^30" in err()
    for k in (0, 2, 4, 5):
        mesh = [ONE, 10, ONE, 5, ONE, ONE]
        mesh[k] = None
        assert sweeps(mesh=tuple(mesh)) == -1 and b"NULL pointer of the mesh" in err()
    assert sweeps(ws=(None, need)) == -1 and b"NULL workspace" in err()
    assert sweeps(ws=(C.c_void_p(20), need)) == -1 and b"aligned" in err()
    assert sweeps(ws=(ONE, need - 1)) == -1 and b"workspace of %d bytes, %d needed" % (need - 1, need) in err()
    assert sweeps(mesh=(None, 0, None, 0, None, None), ws=(None, 0)) == 0        # V = 0: a no-op
    assert sweeps(B=0, ws=(None, 0)) == 0                                         # B = 0: a no-op
    assert sweeps(mesh=(None, 0, None, 0, None, None), B=0, ws=(None, 0), n=0) == 0

    def lds(*, mesh=(ONE, 10, ONE, 5, ONE, ONE), B=3, io=(ONE, ONE, ONE), cap=11):
        return lib.recmv_geodesic_lds(*mesh, B, *io, cap, None)
    assert lds(mesh=(ONE, -10, ONE, 5, ONE, ONE)) == -1 and b"V=-10" in err()
    assert lds(mesh=(ONE, 10, ONE, -5, ONE, ONE)) == -1 and b"F=-5" in err()
    assert lds(B=-3) == -1 and b"B=-3" in err()
    assert lds(cap=-1) == -1 and b"max_sweeps=-1" in err()
    assert lds(mesh=(ONE, 3641, ONE, 5, ONE, ONE)) == -1 and b"V=3641, the lds route takes at most 3640" in err()
    for k in (0, 2, 4, 5):
        mesh = [ONE, 10, ONE, 5, ONE, ONE]
        mesh[k] = None
        assert lds(mesh=tuple(mesh)) == -1 and b"NULL pointer of the mesh" in err()
    assert lds(io=(None, ONE, ONE)) == -1 and b"NULL field" in err()
    assert lds(io=(ONE, None, ONE)) == -1 and b"NULL field" in err()
    assert lds(io=(ONE, ONE, None)) == -1 and b"NULL sweeps" in err()
    assert lds(B=0, io=(None, None, None)) == 0                                   # B = 0: a no-op
    assert lds(mesh=(None, 0, None, 0, None, None), B=0, io=(None, None, None)) == 0


# ------------------------------------------------------------------------------------------------------------- eval_fl
def test_boundary_bands_parser_errors(capsys):
    import eval_fl
    assert eval_fl.parse_bands("0.01") == [0.01] and eval_fl.parse_bands("0.01,0.05, 2") == [0.01, 0.05, 2.]
    for text in ("", "a", "0.1,,0.2", "0", "-1,2", "0.2,0.1", "0.1,0.1", "0.1,inf", "nan", "0.1,nan"):
        with pytest.raises(ValueError):
            eval_fl.parse_bands(text)
        with pytest.raises(SystemExit):                                           # a parser.error, before the meshes are looked for
            eval_fl.main(["--pred", "no_such.obj", "--gt", "no_such.obj", "--boundary-bands=" + text])
        assert "--boundary-bands" in capsys.readouterr().err
    assert "--boundary-bands W1,W2,..." in eval_fl.__doc__ and "--boundary-bands" in eval_fl.build_parser().format_help()


def test_boundary_bands_binning():
    import eval_fl
    g = torch.tensor([0., 0.05, 0.1, 0.1999, 0.2, 0.7, INF, 0.3])
    d = torch.tensor([1., 3., 2., 4., 5., 6., 7., 9.])
    rows = eval_fl.band_stats(g, d, [0.1, 0.2, 0.5])
    assert [(r["lo"], r["hi"], r["count"]) for r in rows] == [(0., 0.1, 2), (0.1, 0.2, 2), (0.2, 0.5, 2), (0.5, None, 2)]
    assert rows[0]["mean"] == 2. and rows[0]["max"] == 3. and abs(rows[0]["rms"] - 5. ** 0.5) < 1e-15
    assert rows[1]["mean"] == 3. and rows[2]["mean"] == 7. and rows[2]["max"] == 9. and rows[3]["mean"] == 6.5 and rows[3]["max"] == 7.
    rows = eval_fl.band_stats(g[:2], d[:2], [0.1, 0.2])
    assert rows[0]["count"] == 2 and rows[1] == {"lo": 0.1, "hi": 0.2, "count": 0, "mean": None, "rms": None, "max": None}
    assert rows[2] == {"lo": 0.2, "hi": None, "count": 0, "mean": None, "rms": None, "max": None}
    assert sum(r["count"] for r in eval_fl.band_stats(g, d, [1e-3])) == 8


# ------------------------------------------------------------------------------------------------------ the host build
def test_host_build_of_the_kernels_equals_the_plain_loops(tmp_path):
    """tools/geodesic_host_check: csrc/geodesic.hip's kernels compiled for the CPU under the address and undefined-behaviour
    sanitizers, both routes against loops that evaluate every face in every sweep, bit for bit, on seven inputs."""
    r = host_check.run("geodesic", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count("-> 0 mismatches") == 7, r.stdout + r.stderr
    for name in ("invalid faces and a NaN vertex: 37 vertices, 56 faces, 1 fields, K 9, 36 values finite",
                 "two pieces, the source in one: 41 vertices, 50 faces, 1 fields, K 6, 25 values finite",
                 "three fields at once: 81 vertices, 128 faces, 3 fields, K 15 8 9", "a fan of valence 70", "a single vertex"):
        assert name in r.stdout
