"""Mesh parameterisation without a GPU: the numpy restatement (tests/param_reference.py) against a dense solve, Tutte's theorem,
the ARAP fixed point on a planar mesh; cut_to_disk; every ValueError of recmv.param and its refusal of CPU tensors; the C entry
points (declared, exported, argument errors and empty no-ops before any HIP call); and the host build of the kernels under the
sanitizers.
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import host_check  # noqa: E402
import param_cases as PC  # noqa: E402
import param_reference as PR  # noqa: E402

NAMES = ["recmv_param_lds_max_vertices", "recmv_param_auto_max_vertices", "recmv_param_solve_workspace_bytes", "recmv_param_solve",
         "recmv_param_solve_lds", "recmv_param_face_frames", "recmv_param_arap_rhs", "recmv_param_distortion"]
DISKS = sorted(PC.DISKS)
TOL = 1e-12
# CG iterations of the restatement to tol = 1e-12 (cotangent, uniform): the GPU runs the same number by construction
ITERATIONS = {"grid5": (2, 2), "grid17": (38, 30), "grid33": (81, 61), "planar": (83, 30), "cap": (38, 30)}


@functools.lru_cache(maxsize=None)
def solved(name, weights):
    v, f = PC.DISKS[name][0]()
    sysm = PR.harmonic_system(v, f, weights)
    return (v, f, sysm) + PR.solve(*sysm, tol=TOL)


# ------------------------------------------------------------------------------------------------------ the restatement
def test_the_cases_are_what_their_reasons_say():
    assert PC.grid(5)[0].shape[0] == 25 and int((PR.harmonic_system(*PC.grid(5))[3] == 0).sum()) == 9
    assert PC.grid(17)[0].shape[0] == 289 and PC.grid(33)[0].shape[0] == 1089 > 1024
    v, f, xy = PC.planar_irregular()
    p = v.astype(np.float64)
    for a, b in ((0, 1), (0, 17), (5, 100), (40, 288)):                           # an isometry of the plane, to the last bit
        assert ((p[a] - p[b]) ** 2).sum() == ((xy[a] - xy[b]) ** 2).sum()
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert np.abs(n / np.linalg.norm(n, axis=1)[:, None] - np.array([0.64, -0.48, 0.6])).max() < 1e-12      # out of the plane z = 0
    assert PC.cap()[0].shape[0] == 289 and np.ptp(PC.cap()[0][:, 2]) > 0.5
    assert PC.cylinder()[0].shape == (144, 3) and PC.shirt()[0].shape[0] == 358 < 600
    assert len(PR.boundary_loop(PC.grid(5)[1])) == 16


def test_the_canonical_sum_is_a_fixed_tree():
    rng = np.random.RandomState(0)
    for n in (1, 63, 64, 255, 256, 257, 1089, 70000):
        x = rng.randn(n) * 10. ** rng.randint(-8, 8, n)
        s = PR.canon_sum(x)
        assert abs(s - float(np.sum(x.astype(np.longdouble)))) <= 1e-13 * np.abs(x).sum()
        assert s == PR.canon_sum(x.copy()) and (n < 256 or PR.canon_partials(x).shape[0] == (n + 255) // 256)
    x = np.zeros(256)
    x[[0, 32, 64]] = [1., 2. ** -53, 2. ** -53]                                   # lane 0 meets lane 32 first: (1 + e) + e = 1
    assert PR.canon_sum(x) == 1.
    x[[0, 32, 64, 128]] = [2. ** -53, 2. ** -53, 1., 0.]                          # (e + e) + 1 > 1: the order matters
    assert PR.canon_sum(x) == 1. + 2. ** -52


@pytest.mark.parametrize("weights", ["cotangent", "uniform"])
@pytest.mark.parametrize("name", DISKS)
def test_the_restated_cg_against_the_dense_solve(name, weights):
    v, f, (off, nbr, w, fixed, rhs, u0), u, it, res, zr = solved(name, weights)
    dense, cond = PR.System(off, nbr, w, fixed).dense(rhs, u0)
    err, bound = np.abs(u - dense).max(), 10 * cond * TOL * np.abs(dense).max()
    print(name, weights, "iterations", it, "residuals", res, "cond", cond, "error", err, "bound", bound)
    assert err <= bound and max(res) <= TOL and zr == 0
    assert it == ITERATIONS[name][weights == "uniform"]
    assert np.array_equal(u[fixed.astype(bool)], u0[fixed.astype(bool)])
    w2 = PR.cotan_weights(v, f, off, nbr)
    i = np.repeat(np.arange(v.shape[0]), np.diff(off))
    back = {(a, b): x for a, b, x in zip(i.tolist(), nbr.tolist(), w2.tolist())}
    assert all(back[(b, a)] == x for (a, b), x in back.items())                   # symmetric bit for bit


@pytest.mark.parametrize("name", DISKS)
def test_uniform_weights_flip_no_face(name):
    """Tutte: a convex combination map onto a strictly convex boundary is an embedding."""
    v, f, _, u, _, _, _ = solved(name, "uniform")
    d = PR.distortion(f, v.shape[0], PR.face_frames(v, f)[0], u)
    assert not np.isnan(d).any() and (d[:, 2] > 0).all() and (d[:, 0] >= d[:, 1]).all() and (d[:, 1] > 0).all()
    assert np.allclose(d[:, 0] * d[:, 1], d[:, 2], rtol=1e-10)


def test_the_isometric_uv_is_a_fixed_point_of_an_arap_iteration():
    v, f, xy = PC.planar_irregular()
    out, rot, rhs, energy, _ = PR.arap_iteration(v, f, xy, TOL)
    assert np.abs(out - xy).max() <= 1e-12 * np.abs(xy).max() and energy <= 1e-24 * (xy.max() ** 2)
    # A rotation takes a face's own flat frame (corner 0 at the origin, corner 1 on the x axis) to uv.  Against the isometric uv
    # that is the direction of the face's first edge there, so the rotation relative to it is the identity:
    e = xy[f[:, 1]] - xy[f[:, 0]]
    e = e / np.sqrt((e * e).sum(1))[:, None]
    ra, rb = rot[:, 0] * e[:, 0] + rot[:, 1] * e[:, 1], rot[:, 1] * e[:, 0] - rot[:, 0] * e[:, 1]
    assert np.abs(ra - 1).max() <= 1e-12 and np.abs(rb).max() <= 1e-12
    S = PR.System(*PR.harmonic_system(v, f)[:3], np.zeros(v.shape[0], np.uint8))
    assert np.abs(S.apply(xy) - rhs).max() <= 1e-12 * np.abs(rhs).max()           # the global system holds at xy
    d = PR.distortion(f, v.shape[0], PR.face_frames(v, f)[0], xy)
    assert np.abs(d - 1).max() <= 1e-12
    moved = xy * 1.3
    out, _, _, e1, _ = PR.arap_iteration(v, f, moved, TOL)                        # a scaled start comes back in one step
    assert e1 > 1 and np.abs((out - out[0]) - (xy - xy[0])).max() <= 1e-9 * np.abs(xy).max()


def test_unusable_faces_and_the_zero_row():
    v, f = PC.flawed()
    frames, cots = PR.face_frames(v, f)
    assert (frames[-1] == 0).all() and (cots[-1] == 0).all() and (frames[:-1, 3] == 0.5).all()
    off, nbr = PR.neighbours_csr(f, 26)
    w = PR.cotan_weights(v, f, off, nbr)
    fixed = np.zeros(26, np.uint8)
    fixed[[i * 5 + j for i in range(5) for j in range(5) if i in (0, 4) or j in (0, 4)]] = 1
    u0 = np.random.RandomState(1).rand(26, 2)
    u, it, res, zr = PR.solve(off, nbr, w, fixed, np.zeros((26, 2)), u0, TOL)
    assert zr == 1 and (u[25] == u0[25]).all() and max(res) <= TOL and off[26] == off[25]
    d = PR.distortion(f, 26, frames, u)
    assert np.isnan(d[-1, :2]).all() and d[-1, 2] == 0 and not np.isnan(d[:-1]).any()
    rot, rhs, part, e = PR.arap_rhs(f, 26, frames, cots, u)
    assert (rot[-1] == [1., 0.]).all() and (rhs[25] == 0).all() and part.shape == (1,) and part[0] == e


# ------------------------------------------------------------------------------------------------------------ the cut
def euler(verts, faces):
    from recmv import connectivity
    used = torch.unique(faces).numel()
    return used - connectivity.EdgeTable(faces, verts.shape[0]).E + faces.shape[0]


@pytest.mark.parametrize("name", ["cylinder", "shirt"])
def test_cut_to_disk(name):
    from recmv import connectivity, param
    v, f = (torch.from_numpy(x) for x in getattr(PC, name)())
    loops = connectivity.boundary_loops(f, v.shape[0])
    cv, cf, origin, seams = param.cut_to_disk(v, f)
    assert len(seams) == len(loops) - 1 == {"cylinder": 1, "shirt": 3}[name]
    assert len(connectivity.boundary_loops(cf, cv.shape[0])) == 1 and euler(cv, cf) == 1 and torch.unique(cf).numel() == cv.shape[0]
    assert cf.shape == f.shape and torch.equal(origin[cf], f) and torch.equal(cv, v[origin]) and origin.dtype == torch.int64
    assert torch.equal(origin[:v.shape[0]], torch.arange(v.shape[0]))
    assert cv.shape[0] == v.shape[0] + sum(len(s["vertices"]) for s in seams)     # every seam vertex is doubled once here
    again = param.cut_to_disk(v, f)
    assert torch.equal(again[1], cf) and torch.equal(again[2], origin) and again[3] == seams
    if name == "cylinder":
        assert seams[0]["vertices"] == [16 * r for r in range(9)] and seams[0]["length"] == 2.0
    else:
        assert all(len(s["vertices"]) >= 2 and s["length"] > 0 for s in seams)
    off, nbr, w, fixed, rhs, u0 = PR.harmonic_system(cv.numpy(), cf.numpy(), "uniform")        # and the disk flattens
    u = PR.solve(off, nbr, w, fixed, rhs, u0, TOL)[0]
    assert (PR.distortion(cf.numpy(), cv.shape[0], PR.face_frames(cv.numpy(), cf.numpy())[0], u)[:, 2] > 0).all()


def test_cut_to_disk_leaves_a_disk_alone_and_names_its_refusals():
    from recmv import param
    v, f = (torch.from_numpy(x) for x in PC.grid(5))
    cv, cf, origin, seams = param.cut_to_disk(v, f)
    assert torch.equal(cv, v) and torch.equal(cf, f) and seams == [] and torch.equal(origin, torch.arange(25))
    for mesh, reason in ((PC.tetrahedron, "closed"), (PC.torus_strip, "genus > 0"), (PC.two_grids, "several pieces"),
                         (PC.fin, "non-manifold")):
        with pytest.raises(ValueError, match=reason):
            param.cut_to_disk(*(torch.from_numpy(x) for x in mesh()))
    with pytest.raises(ValueError, match="not valid"):
        param.cut_to_disk(v, torch.tensor([[0, 1, 25]]))
    with pytest.raises(ValueError, match="no faces"):
        param.cut_to_disk(v, torch.zeros(0, 3, dtype=torch.int64))


def test_circle_boundary():
    from recmv import param
    v, f = PC.grid(5)
    loop = PR.boundary_loop(f)
    got = param.circle_boundary(torch.from_numpy(v), loop)
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), PR.circle_boundary(v, loop))
    assert np.abs((got.numpy() ** 2).sum(1) - 1).max() < 1e-15 and got[0].tolist() == [1., 0.]
    ang = np.unwrap(np.arctan2(got[:, 1].numpy(), got[:, 0].numpy()))
    assert np.allclose(np.diff(ang), 2 * np.pi / 16)                              # unit edges: equal angles, counter-clockwise
    for bad in (lambda: param.circle_boundary(torch.zeros(4, 3), [0, 1, 2]), lambda: param.circle_boundary(torch.zeros(4, 3), []),
                lambda: param.circle_boundary(torch.zeros(4, 3), [0, 4]), lambda: param.circle_boundary(torch.zeros(4, 2), [0, 1])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ recmv.param's arguments
def test_argument_errors_and_cpu_tensors():
    from recmv import param
    assert param.ROUTES == ('auto', 'launch', 'lds') and param.lds_max_vertices() == 2218
    assert 0 < param.auto_max_vertices() <= 2218
    v, f = (torch.from_numpy(x) for x in PC.grid(5))
    uv = torch.zeros(25, 2, dtype=torch.float64)
    off, nbr = (torch.from_numpy(x) for x in PR.neighbours_csr(f.numpy(), 25))
    w, fixed = torch.ones(nbr.shape[0], dtype=torch.float64), torch.zeros(25, dtype=torch.uint8)
    bad = [lambda: param.harmonic(v, f, weights='mean-value'), lambda: param.harmonic(v, f, route='fast'),
           lambda: param.harmonic(v.double(), f), lambda: param.harmonic(v[:, :2], f), lambda: param.harmonic(v, f.int()),
           lambda: param.harmonic(v, f[:, :2]), lambda: param.harmonic(v, f, tol=-1.), lambda: param.harmonic(v, f, tol=float("nan")),
           lambda: param.harmonic(v, f, max_iter=-1), lambda: param.harmonic(torch.zeros(2219, 3), f, route='lds'),
           lambda: param.arap(v, f, route='fast'), lambda: param.arap(v, f, iterations=-1), lambda: param.arap(v, f, tol=-1.),
           lambda: param.arap(v, f, uv0=uv[:24]), lambda: param.arap(v, f, uv0=uv.float()), lambda: param.arap(v.double(), f),
           lambda: param.distortion(v, f, uv[:24]), lambda: param.distortion(v, f, uv.float()), lambda: param.distortion(v, f.int(), uv),
           lambda: param.flatten(v, f, method='lscm'), lambda: param.flatten(v, f, weights='x'), lambda: param.flatten(v, f, route='x'),
           lambda: param.flatten(v, f, iterations=-2), lambda: param.flatten(v, f, tol=-1.), lambda: param.flatten(v[:, :2], f),
           lambda: param.cut_to_disk(v.double(), f), lambda: param.cut_to_disk(v, f.int()),
           lambda: param.solve((off, nbr), w, fixed, uv, uv, route='x'), lambda: param.solve((off.long(), nbr), w, fixed, uv, uv),
           lambda: param.solve((off, nbr), w[:-1], fixed, uv, uv), lambda: param.solve((off, nbr), w.float(), fixed, uv, uv),
           lambda: param.solve((off, nbr), w, fixed[:-1], uv, uv), lambda: param.solve((off, nbr), w, fixed.long(), uv, uv),
           lambda: param.solve((off, nbr), w, fixed, uv[:3], uv), lambda: param.solve((off, nbr), w, fixed, uv, uv.float()),
           lambda: param.solve((off, nbr), w, fixed, uv, uv, tol=-1e-3), lambda: param.solve((off, nbr), w, fixed, uv, uv, max_iter=-1),
           lambda: param.solve((off, nbr), w, fixed, uv, uv, batch=0)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d raised nothing" % k)
    for call in (lambda: param.harmonic(v, f), lambda: param.harmonic(v, f, weights='uniform', route='launch'),
                 lambda: param.arap(v, f), lambda: param.arap(v, f, uv0=uv), lambda: param.distortion(v, f, uv),
                 lambda: param.flatten(v, f), lambda: param.face_frames(v, f), lambda: param.solve((off, nbr), w, fixed, uv, uv)):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            call()


def test_flatten_fl_parser(capsys):
    import flatten_fl
    assert "--arap-iters N" in flatten_fl.__doc__ and "--no-normalise" in flatten_fl.build_parser().format_help()
    for argv in (["--in", "no_such.obj", "--out", "x"], ["--in", ".", "--out", "x", "--arap-iters", "-1"],
                 ["--in", ".", "--out", "x", "--method", "lscm"], ["--in", "."]):
        with pytest.raises(SystemExit):                                           # a parser.error, before any mesh is read
            flatten_fl.main(argv)
        assert "usage:" in capsys.readouterr().err


def test_write_obj_uv(tmp_path):
    import flatten_fl
    from recmv.utils.utils import read_obj
    v, f = (torch.from_numpy(x) for x in PC.grid(3))
    flatten_fl.write_obj_uv(str(tmp_path / "a.obj"), v, v[:, :2].double() * 0.5, f)
    lines = (tmp_path / "a.obj").read_text().splitlines()
    assert [l.split()[0] for l in lines] == ["v"] * 9 + ["vt"] * 9 + ["f"] * 8
    assert lines[9 + 4] == "vt 0.500000 0.500000" and lines[18] == "f 1/1 4/4 5/5"
    rv, rf = read_obj(str(tmp_path / "a.obj"))
    assert torch.equal(rv, v) and torch.equal(rf, f)


# ------------------------------------------------------------------------------------------------------------ the C ABI
ONE = C.c_void_p(256)                                                             # a pointer nobody reads: the errors come first


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in NAMES:
        assert n in declared and hasattr(lib, n)
    assert sorted(n for n in declared if n.startswith("recmv_param_")) == sorted(NAMES)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION == 11
    hdr = (REPO / "include" / "recmv_hip.h").read_text()
    note = hdr[:hdr.index("int recmv_abi_version")]
    for n in NAMES:
        assert n in note
    assert "(mesh parameterisation: pure additions, still v11)" in note
    assert "(geodesic distance fields: pure additions, still v11)" in note       # the earlier phrases stand
    assert lib.recmv_param_lds_max_vertices() == 2218 == (163840 - 4096) // 72
    assert 0 < lib.recmv_param_auto_max_vertices() <= 2218


def test_a_library_without_the_symbols_is_rejected():
    from recmv import _lib

    class Partial:
        def __init__(self, missing):
            self.missing = missing

        def __getattr__(self, name):
            if name == self.missing:
                raise AttributeError(name)
            return getattr(_lib.lib(), name)
    for n in NAMES:
        with pytest.raises(AttributeError, match=n):
            _lib._declare(Partial(n))


def test_c_argument_errors_and_empty_inputs_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    err = lib.recmv_last_error
    wb = lib.recmv_param_solve_workspace_bytes
    assert wb(0) == 0 and wb(1) > 0 and wb(1) % 256 == 0 and wb(1000) > 9 * 8 * 1000 and wb(1000) % 256 == 0
    assert wb(-1) == -1 and b"V=-1" in err() and wb(1 << 31) == -1 and b"2^31" in err()
    need = wb(10)
    it, zr, res = C.c_int32(7), C.c_int32(7), (C.c_double * 2)(7., 7.)
    out = (C.byref(it), res, C.byref(zr))

    def solve(*, csr=(ONE, ONE, ONE), V=10, nnz=40, io=(ONE, ONE, ONE), tol=1e-12, max_iter=5, batch=0, out=out, ws=(ONE, need)):
        return lib.recmv_param_solve(*csr, V, nnz, *io, tol, max_iter, batch, *out, *ws, None)

    def lds(*, csr=(ONE, ONE, ONE), V=10, nnz=40, io=(ONE, ONE, ONE), tol=1e-12, max_iter=5, out=out, report=ONE):
        return lib.recmv_param_solve_lds(*csr, V, nnz, *io, tol, max_iter, *out, report, None)
    for call, who in ((solve, b"param_solve:"), (lds, b"param_solve_lds:")):
        assert call(V=-10) == -1 and b"V=-10" in err() and who in err()
        assert call(nnz=-4) == -1 and b"nnz=-4" in err()
        assert call(V=1 << 31) == -1 and b"2^31" in err()
        assert call(nnz=1 << 31) == -1 and b"2^31" in err()
        assert call(tol=-1e-3) == -1 and b"tol=-0.001" in err()
        assert call(tol=float("nan")) == -1 and b"tol=" in err()
        assert call(max_iter=-1) == -1 and b"max_iter=-1" in err()
        for k in range(3):
            o = list(out)
            o[k] = None
            assert call(out=tuple(o)) == -1 and b"host pointers" in err()
        assert call(csr=(None, ONE, ONE)) == -1 and b"NULL pointer" in err()
        for k in range(3):
            io = [ONE, ONE, ONE]
            io[k] = None
            assert call(io=tuple(io)) == -1 and b"NULL pointer" in err()
        assert call(csr=(ONE, None, ONE)) == -1 and b"NULL neighbour list or weights" in err()
        assert call(csr=(ONE, ONE, None)) == -1 and b"NULL neighbour list or weights" in err()
        it.value, zr.value, res[0] = 7, 7, 7.
        assert call(csr=(None, None, None), V=0, nnz=0, io=(None, None, None)) == 0      # V = 0: a no-op that reports zeros
        assert (it.value, zr.value, res[0], res[1]) == (0, 0, 0., 0.)
    assert solve(ws=(None, need)) == -1 and b"NULL workspace" in err()
    assert solve(ws=(ONE, need - 1)) == -1 and b"workspace of %d bytes, %d needed" % (need - 1, need) in err()
    assert solve(ws=(C.c_void_p(264), need)) == -1 and b"256-byte aligned" in err()
    assert lds(V=2219) == -1 and b"V=2219, the lds route takes at most 2218" in err()
    assert lds(report=None) == -1 and b"NULL report" in err()
    assert lds(report=C.c_void_p(260)) == -1 and b"8-byte aligned" in err()

    frames = lib.recmv_param_face_frames
    assert frames(ONE, -1, ONE, 5, ONE, ONE, None) == -1 and b"V=-1" in err()
    assert frames(ONE, 5, ONE, -2, ONE, ONE, None) == -1 and b"F=-2" in err()
    assert frames(ONE, 1 << 31, ONE, 5, ONE, ONE, None) == -1 and b"2^31" in err()
    for k in (0, 2, 4, 5):
        a = [ONE, 5, ONE, 5, ONE, ONE]
        a[k] = None
        assert frames(*a, None) == -1 and b"NULL pointer" in err()
    assert frames(None, 5, None, 0, None, None, None) == 0 and frames(None, 0, None, 0, None, None, None) == 0

    def rhs(*, faces=ONE, F=5, a=(ONE, ONE, ONE), V=6, b=(ONE, ONE, ONE, ONE, ONE, ONE)):
        return lib.recmv_param_arap_rhs(faces, F, *a, V, *b, None)
    assert rhs(F=-5) == -1 and b"F=-5" in err() and rhs(V=-6) == -1 and b"V=-6" in err()
    assert rhs(F=1 << 31) == -1 and b"2^31" in err()
    assert rhs(b=(ONE, ONE, ONE, ONE, ONE, None)) == -1 and b"NULL energy" in err()
    assert rhs(faces=None) == -1 and b"NULL pointer of the faces" in err()
    assert rhs(a=(None, ONE, ONE)) == -1 and b"of the faces" in err() and rhs(a=(ONE, None, ONE)) == -1 and b"of the faces" in err()
    assert rhs(a=(ONE, ONE, None)) == -1 and b"NULL pointer of the vertices" in err()
    assert rhs(b=(None, ONE, ONE, ONE, ONE, ONE)) == -1 and b"of the vertices" in err()
    assert rhs(b=(ONE, ONE, ONE, None, ONE, ONE)) == -1 and b"of the vertices" in err()
    assert rhs(b=(ONE, ONE, None, ONE, ONE, ONE)) == -1 and b"of the faces" in err()

    dist = lib.recmv_param_distortion
    assert dist(ONE, -5, ONE, ONE, 6, ONE, None) == -1 and b"F=-5" in err()
    assert dist(ONE, 5, ONE, ONE, -6, ONE, None) == -1 and b"V=-6" in err()
    assert dist(ONE, 5, ONE, ONE, 1 << 31, ONE, None) == -1 and b"2^31" in err()
    for k in (0, 2, 3, 5):
        a = [ONE, 5, ONE, ONE, 6, ONE]
        a[k] = None
        assert dist(*a, None) == -1 and b"NULL pointer" in err()
    assert dist(None, 0, None, None, 6, None, None) == 0


# ------------------------------------------------------------------------------------------------------ the host build
def test_host_build_of_the_kernels_equals_the_plain_loops(tmp_path):
    """tools/param_host_check: csrc/mesh_param.hip's kernels compiled for the CPU under the address and undefined-behaviour
    sanitizers — frames, the ARAP step, distortion and the whole lds-route solve against plain loops, bit for bit, on five
    inputs."""
    r = host_check.run("param", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count("-> 0 mismatches") == 5, r.stdout + r.stderr
    for name in ("a jittered 9 x 9 grid, two sides fixed: 81 vertices, 128 faces, 44 iterations, 0 zero rows",
                 "stopped after 7 iterations: 81 vertices, 128 faces, 7 iterations",
                 "a 20 x 30 grid, two sides fixed: 600 vertices, 1102 faces",
                 "an isolated vertex, a face without area, invalid faces, a NaN vertex: 37 vertices, 55 faces, 33 iterations, 2 zero rows",
                 "a single triangle: 3 vertices, 1 faces"):
        assert name in r.stdout
