"""Mesh smoothing without a GPU: the float64 torch path of recmv.smooth on CPU tensors against the numpy restatement
(tests/mesh_smooth_reference.py), the argument checks, the new C entry points (declared, exported, argument errors before any
HIP call), clean_fl.py's new flags, and the quality properties of tests/test_gpu_mesh_smooth.py on the reference and on the
torch path."""
import ctypes as C
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import mesh_smooth_cases as MC  # noqa: E402
import mesh_smooth_reference as MR  # noqa: E402

NEW_SYMBOLS = ("recmv_cotan_weights", "recmv_laplacian_step", "recmv_face_normal_filter", "recmv_vertex_from_normals")


def run(v, f, **kw):
    from recmv import smooth
    x, info = smooth.smooth(torch.from_numpy(v), torch.from_numpy(f), use_kernels=False, **kw)
    assert x.dtype == torch.float32 and x.shape == v.shape
    return x.numpy(), info


def csr(rows, dtype):
    off, idx = MR.Tables.csr(rows, np.int64)
    return torch.from_numpy(off).to(dtype), torch.from_numpy(idx).to(dtype)


@functools.lru_cache(maxsize=None)
def sphere():
    return MC.noisy_sphere()


@functools.lru_cache(maxsize=None)
def cube():
    return MC.noisy_cube()


# ---- the cases and the tables ---------------------------------------------------------------------------------------------------------
def test_the_case_meshes_are_what_the_docstrings_say():
    v, f, clean = sphere()
    assert v.shape == (642, 3) and f.shape == (1280, 3) and abs(MR.volume(clean, f) - 4 * np.pi / 3) < 0.05
    v, f, clean = cube()
    assert v.shape == (386, 3) and f.shape == (768, 3) and abs(MR.volume(clean, f) - 1.) < 1e-6
    assert MC.rms_distance_to_unit_cube(clean) == 0 and MC.rms_radial_error(sphere()[2]) < 1e-6


@pytest.mark.parametrize("mesh", ["tube", "hinged", "pinched", "fan"])
def test_connectivity_tables_equal_the_reference(mesh):
    from recmv import connectivity
    v, f = {"tube": MC.tube, "hinged": MC.hinged_tetrahedra, "pinched": MC.pinched_tetrahedra, "fan": lambda: MC.fan(7)}[mesh]()
    t = MR.Tables(f, len(v))
    table = connectivity.EdgeTable(torch.from_numpy(f), len(v))
    off, idx = connectivity.face_neighbours_csr(table)
    assert off.dtype == idx.dtype == torch.int32
    roff, ridx = MR.Tables.csr(t.ff, np.int32)
    assert np.array_equal(off.numpy(), roff) and np.array_equal(idx.numpy(), ridx)
    assert np.array_equal(connectivity.boundary_neighbours(table).numpy(), t.bnbr)
    if mesh == "hinged":
        assert max(len(r) for r in t.ff) == 5               # across the hinge: the edge's three other faces
    if mesh == "tube":                                      # where iso_remesh builds the same table, it is the same
        from recmv.iso_remesh import _loop_tables
        assert torch.equal(_loop_tables(torch.from_numpy(f), len(v))[1], connectivity.boundary_neighbours(table))


# ---- the torch restatements against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["sphere", "tube", "hinged", "fan"])
def test_torch_restatements_equal_the_reference(mesh):
    """The same sums in the same order in the same arithmetic: within the one-step bounds (in fact the same bits but for exp)."""
    from recmv import smooth
    v, f = {"sphere": lambda: sphere()[:2], "tube": MC.tube, "hinged": MC.hinged_tetrahedra, "fan": lambda: MC.fan(30)}[mesh]()
    t = MR.Tables(f, len(v))
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    nbr, slots, ff = csr(t.nbr, torch.int32), csr(t.slots, torch.int64), csr(t.ff, torch.int32)
    w, invalid, wt, wm = MR.cotan_weights(v, f, t)
    got, n_bad = smooth.cotangent_weights_torch(tv, tf, nbr, slots, return_counts=True)
    flat, bound = np.concatenate(w), np.concatenate([MR.gamma(a + MR.COT_OPS) * m for a, m in zip(wt, wm)])
    assert n_bad == invalid == 0 and (np.abs(got.numpy() - flat) <= bound).all() and (flat >= 0).all()
    pinned = torch.from_numpy(t.boundary)
    for lam, weights, fixed, bnbr in ((0.5, None, None, None), (-0.53, None, pinned, None), (1.0, got, None, torch.from_numpy(t.bnbr))):
        out, ref, terms, mags = MR.laplacian_step(v, t, lam, None if weights is None else w, None if fixed is None else t.boundary,
                                                  None if bnbr is None else t.bnbr)
        res = smooth.laplacian_step_torch(tv, nbr, lam, weights, fixed, bnbr).numpy()
        assert (np.abs(res - ref) <= MR.step_bound(ref, terms, mags, MR.STEP_OPS)).all()
        assert np.array_equal(res, out)
    unit, area, cen, good = MR.face_geometry(v, f)
    gu, ga, gc, gg = smooth.face_geometry(tv, tf)
    close = lambda a, b: np.allclose(a.numpy(), b, rtol=8 * MR.U, atol=8 * MR.U)  # noqa: E731  (a few float64 roundings)
    assert close(gu, unit) and close(ga, area) and close(gc, cen) and gg.all() and good.all()
    n32 = unit.astype(np.float32)
    sc = MR.mean_centroid_distance(cen, t)
    out, ref, terms, rel, _ = MR.normal_filter(n32, area, cen, t, sc, 0.35)
    res = smooth.filter_face_normals_torch(torch.from_numpy(n32), ga, gc, ff, sc, 0.35).numpy()
    assert (np.abs(res - ref) <= MR.ulp32(ref)).all() and rel.min() >= 1 - 1e-6   # one float32 spacing of the component
    out2, ref, terms, mags, _ = MR.vertex_update(v, f, out, t, t.boundary)
    res = smooth.update_vertices_torch(tv, tf, torch.from_numpy(out), slots, pinned).numpy()
    assert (np.abs(res - ref) <= MR.step_bound(ref, terms, mags, MR.UPDATE_OPS)).all() and np.array_equal(res, out2)


@pytest.mark.parametrize("kw", [dict(method="taubin"), dict(method="taubin", weights="cotangent"),
                                dict(method="laplacian", weights="cotangent", reweight=True, iterations=3),
                                dict(method="bilateral", normal_iterations=2, vertex_iterations=3)])
def test_torch_driver_within_the_propagated_bound(kw):
    v, f, _ = sphere()
    x, info = run(v, f, **kw)
    ref, bound, extra = MR.smooth(v, f, sigma_c=info.get("sigma_c"), **kw)
    err = float(np.abs(x - ref).max())
    print("largest error", err, "propagated bound", bound)
    assert err <= bound < 1e-2
    if kw["method"] == "taubin":
        assert info["mu"] == extra["mu"] and abs(info["mu"] + 0.5263157894736842) < 1e-15


def test_info_describes_the_run():
    v, f, _ = sphere()
    x, info = run(v, f)
    assert info["method"] == "taubin" and info["iterations"] == 10 and info["lam"] == 0.5 and info["weights"] == "uniform"
    assert info["boundary"] == "fixed" and info["invalid_faces"] == 0 and info["moved"] == 642
    assert 0 < info["displacement_mean"] <= info["displacement_max"] < 0.2
    assert abs(info["area_before"] - MR.area(v, f)) < 1e-9 and abs(info["area_after"] - MR.area(x, f)) < 1e-9
    assert abs(info["volume_before"] - MR.volume(v, f)) < 1e-9 and abs(info["volume_after"] - MR.volume(x, f)) < 1e-9
    assert abs(info["roughness_before"] - MR.roughness(v, f)) < 1e-9 and abs(info["roughness_after"] - MR.roughness(x, f)) < 1e-9
    tv, tf = MC.tube()
    _, info = run(tv, tf, method="bilateral")
    assert info["volume_before"] is None and info["volume_after"] is None and info["sigma_c"] > 0 and info["sigma_s"] == 0.35
    x0, info = run(tv, tf, iterations=0)
    assert np.array_equal(x0, tv) and info["moved"] == 0
    lines = []
    run(tv, tf, log=lines.append)
    assert len(lines) == 1 and "taubin" in lines[0]


def test_invalid_faces_take_no_part_and_are_counted():
    v, f, nan_at, lonely = MC.with_invalid_faces(sphere()[:2])
    x, info = run(v, f, boundary="free")
    ref, _, _ = MR.smooth(v, f, boundary="free")
    with_nan = (f == nan_at).any(1) & MR.valid_index_faces(f, len(v))
    assert info["invalid_faces"] == 3 + int(with_nan.sum()) and info["volume_before"] is None
    assert np.array_equal(x[lonely], v[lonely]) and np.array_equal(x, ref, equal_nan=True)
    # one bilateral vertex iteration: the faces with the NaN corner are left out, so only that vertex is not finite
    x, _ = run(v, f, method="bilateral", vertex_iterations=1, boundary="free")
    assert np.isfinite(np.delete(x, nan_at, 0)).all() and np.array_equal(x[lonely], v[lonely])


# ---- exact properties on the torch path -----------------------------------------------------------------------------------------------
def check_curve_boundary(smooth_fn, v, f, on):
    """Under 'curve' the vertices of the tube's two loops keep their axial coordinate bit for bit (each moves toward the midpoint
    of two neighbours with the same z) and stay boundary vertices (the faces do not change).  The radius cannot grow under the
    lambda step, a convex combination of points of one circle; Taubin's mu step pushes outward on purpose (a 16-gon's radial
    mode lies inside the pass-band), so the radius is checked for 'laplacian'."""
    for method in ("taubin", "laplacian"):
        x = smooth_fn(method=method, boundary="curve")
        assert np.array_equal(x[on, 2], v[on, 2]) and not np.array_equal(x[on], v[on])
        assert np.array_equal(MR.Tables(f, len(x)).boundary, on)
    assert (np.linalg.norm(x[on, :2].astype(np.float64), axis=1) <= np.linalg.norm(v[on, :2].astype(np.float64), axis=1)).all()


def test_fixed_and_curve_boundaries_of_the_tube():
    v, f = MC.tube()
    t = MR.Tables(f, len(v))
    on = t.boundary
    assert on.sum() == 32
    for kw in (dict(method="taubin"), dict(method="bilateral"), dict(method="taubin", weights="cotangent")):
        x, _ = run(v, f, **kw)
        assert np.array_equal(x[on], v[on]) and not np.array_equal(x[~on], v[~on])
    mask = np.zeros(len(v), bool)
    mask[40:60] = True
    for method in ("taubin", "bilateral"):
        x, _ = run(v, f, method=method, boundary="free", fixed=torch.from_numpy(mask))
        assert np.array_equal(x[mask], v[mask]) and not np.array_equal(x[on], v[on])
    check_curve_boundary(lambda **kw: run(v, f, **kw)[0], v, f, on)
    free, _ = run(v, f, method="laplacian", boundary="free")
    assert not np.array_equal(free[on, 2], v[on, 2])        # why 'free' is not the default: the open ends creep inward


def test_flat_grid_stays_flat():
    v, f = MC.flat_grid()
    t = MR.Tables(f, len(v))
    for kw in (dict(method="taubin", boundary="free"), dict(method="laplacian", weights="cotangent", boundary="curve"),
               dict(method="bilateral", boundary="free")):
        x, info = run(v, f, **kw)
        assert (x[:, 2] == 0).all()
        if kw["method"] == "bilateral":
            assert np.array_equal(x, v) and info["moved"] == 0
    from recmv import smooth
    x = smooth.laplacian_step_torch(torch.from_numpy(v), csr(t.nbr, torch.int32), 0.5).numpy()
    balanced = np.array([not t.boundary[i] and not (v[t.nbr[i]] - v[i]).sum(0).any() for i in range(len(v))])
    assert balanced.sum() == 49 and np.array_equal(x[balanced], v[balanced])


@pytest.mark.parametrize("lam", [0.25, 0.5, 1.0])
def test_a_lambda_step_stays_inside_its_neighbourhood(lam):
    from recmv import smooth
    v, f, _ = sphere()
    t = MR.Tables(f, len(v))
    nbr = csr(t.nbr, torch.int32)
    w = smooth.cotangent_weights_torch(torch.from_numpy(v), torch.from_numpy(f), nbr, csr(t.slots, torch.int64))
    for weights in (None, w):
        x = smooth.laplacian_step_torch(torch.from_numpy(v), nbr, lam, weights).numpy()
        lo = np.array([v[[i] + t.nbr[i]].min(0) for i in range(len(v))])
        hi = np.array([v[[i] + t.nbr[i]].max(0) for i in range(len(v))])
        assert (x >= lo).all() and (x <= hi).all()


# ---- quality --------------------------------------------------------------------------------------------------------------------------
def check_sphere_quality(smooth_fn):
    v, f, _ = sphere()
    taubin, laplacian = smooth_fn(v, f, "taubin"), smooth_fn(v, f, "laplacian")
    before, after = MR.roughness(v, f), MR.roughness(taubin, f)
    vol = MR.volume(v, f)
    lost_t, lost_l = abs(MR.volume(taubin, f) - vol) / vol, abs(MR.volume(laplacian, f) - vol) / vol
    print("roughness %.4f -> %.4f, volume change %.4f (taubin) %.4f (laplacian), radial rms %.4f -> %.4f"
          % (before, after, lost_t, lost_l, MC.rms_radial_error(v), MC.rms_radial_error(taubin)))
    assert after <= 0.5 * before
    assert lost_t <= 0.25 * lost_l
    assert MC.rms_radial_error(taubin) < MC.rms_radial_error(v)


def check_cube_quality(smooth_fn):
    v, f, _ = cube()
    d0 = MC.rms_distance_to_unit_cube(v)
    bilateral, taubin = MC.rms_distance_to_unit_cube(smooth_fn(v, f, "bilateral")), MC.rms_distance_to_unit_cube(smooth_fn(v, f, "taubin"))
    print("rms distance to the cube %.5f; bilateral %.3f x, taubin %.3f x" % (d0, bilateral / d0, taubin / d0))
    assert bilateral <= 0.7 * d0
    assert bilateral < taubin


def test_quality_of_the_reference():
    check_sphere_quality(lambda v, f, m: MR.smooth(v, f, method=m)[0])
    check_cube_quality(lambda v, f, m: MR.smooth(v, f, method=m)[0])


def test_quality_of_the_torch_path():
    check_sphere_quality(lambda v, f, m: run(v, f, method=m)[0])
    check_cube_quality(lambda v, f, m: run(v, f, method=m)[0])


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments():
    from recmv import smooth
    v, f = MC.tube()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    bad = [dict(method="gauss"), dict(weights="area"), dict(boundary="loose"), dict(iterations=-1), dict(lam=float("nan")),
           dict(lam=0.), dict(lam=1.5), dict(lam=-0.5), dict(mu=float("inf")), dict(mu=0.), dict(mu=0.3), dict(sigma_s=0.),
           dict(sigma_s=-1.), dict(sigma_c=0.), dict(sigma_c=float("nan")), dict(fixed=torch.zeros(3, dtype=torch.bool)),
           dict(normal_iterations=-1), dict(vertex_iterations=-2)]
    for kw in bad:
        with pytest.raises(ValueError):
            smooth.smooth(tv, tf, use_kernels=False, **kw)
    for a, b in ((tv, tf.int()), (tv, tf[:, :2]), (tv[:, :2], tf), (tv.long(), tf), (tv.reshape(-1), tf)):
        with pytest.raises(ValueError):
            smooth.smooth(a, b, use_kernels=False)
    smooth.smooth(tv, tf, method="laplacian", mu=0.3, use_kernels=False)            # mu only matters to taubin


def test_kernel_wrappers_refuse_host_tensors():
    from recmv import smooth
    v, f = MC.tube()
    t = MR.Tables(f, len(v))
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    nbr, slots, ff = csr(t.nbr, torch.int32), csr(t.slots, torch.int64), csr(t.ff, torch.int32)
    unit, area, cen, _ = smooth.face_geometry(tv, tf)
    with pytest.raises(RuntimeError):
        smooth.cotangent_weights(tv, tf, nbr, slots)
    with pytest.raises(RuntimeError):
        smooth.laplacian_step(tv, nbr, 0.5)
    with pytest.raises(RuntimeError):
        smooth.filter_face_normals(unit.float(), area, cen, ff, 0.1, 0.35)
    with pytest.raises(RuntimeError):
        smooth.update_vertices(tv, tf, unit.float(), slots)
    with pytest.raises(RuntimeError):
        smooth.smooth(tv, tf)                               # the kernel path is the default


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION


def test_argument_errors_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    one = C.c_void_p(16)                                   # a non-NULL pointer that is never followed
    err = lib.recmv_last_error
    inf, nan = float("inf"), float("nan")

    def cot(V=3, F=1, n_vs=3, nnz=6, mesh=(one, one), vs=(one, one), nbr=(one, one), out=(one, one)):
        return lib.recmv_cotan_weights(mesh[0], V, mesh[1], F, vs[0], vs[1], n_vs, nbr[0], nbr[1], nnz, *out, None)
    assert cot(V=-1) == -1 and b"V=-1" in err()
    assert cot(F=-2) == -1 and b"F=-2" in err()
    assert cot(n_vs=-3) == -1 and b"n_vs=-3" in err()
    assert cot(nnz=-4) == -1 and b"nnz=-4" in err()
    assert cot(V=1 << 31) == -1 and b"2^31" in err()
    assert cot(F=1 << 31) == -1 and b"2^31" in err()
    assert cot(mesh=(None, one)) == -1 and b"NULL" in err()
    assert cot(mesh=(one, None)) == -1 and b"NULL faces" in err()
    assert cot(vs=(one, None)) == -1 and b"slot table" in err()
    assert cot(nbr=(one, None)) == -1 and b"neighbour list" in err()
    assert cot(out=(None, one)) == -1 and b"weights" in err()
    assert cot(out=(one, None)) == -1 and b"NULL" in err()
    assert cot(V=0, F=0, n_vs=0, nnz=0, mesh=(None, None), vs=(None, None), nbr=(None, None), out=(None, None)) == 0

    def lap(V=3, nnz=6, lam=0.5, nbr=(one, one), x=one, opt=(None, None, None), out=C.c_void_p(32)):
        return lib.recmv_laplacian_step(nbr[0], nbr[1], V, nnz, x, *opt, lam, out, None)
    assert lap(V=-1) == -1 and b"V=-1" in err()
    assert lap(nnz=-2) == -1 and b"nnz=-2" in err()
    assert lap(nnz=1 << 31) == -1 and b"2^31" in err()
    assert lap(lam=inf) == -1 and b"lambda" in err()
    assert lap(lam=nan) == -1 and b"lambda" in err()
    assert lap(nbr=(None, one)) == -1 and b"NULL" in err()
    assert lap(nbr=(one, None)) == -1 and b"neighbour list" in err()
    assert lap(x=None) == -1 and b"NULL" in err()
    assert lap(out=None) == -1 and b"NULL" in err()
    assert lap(out=one) == -1 and b"alias" in err()
    assert lap(V=0, nnz=0, lam=-0.53, nbr=(None, None), x=None, out=None) == 0

    def filt(F=2, nnz=2, sc=0.1, ss=0.35, ff=(one, one), ins=(one, one, one), out=C.c_void_p(32)):
        return lib.recmv_face_normal_filter(ff[0], ff[1], F, nnz, *ins, sc, ss, out, None)
    assert filt(F=-1) == -1 and b"F=-1" in err()
    assert filt(nnz=-1) == -1 and b"nnz=-1" in err()
    assert filt(F=1 << 31) == -1 and b"2^31" in err()
    for bad in (0., -1., inf, nan):
        assert filt(sc=bad) == -1 and b"sigma_c" in err()
        assert filt(ss=bad) == -1 and b"sigma_s" in err()
    assert filt(ff=(None, one)) == -1 and b"NULL" in err()
    assert filt(ff=(one, None)) == -1 and b"neighbour list" in err()
    assert filt(ins=(one, None, one)) == -1 and b"NULL" in err()
    assert filt(out=None) == -1 and b"NULL" in err()
    assert filt(out=one) == -1 and b"alias" in err()
    assert filt(F=0, nnz=0, ff=(None, None), ins=(None, None, None), out=None) == 0

    def upd(V=3, F=1, n_vs=3, x=one, faces=one, vs=(one, one), normals=one, out=C.c_void_p(32)):
        return lib.recmv_vertex_from_normals(x, V, faces, F, vs[0], vs[1], n_vs, normals, None, out, None)
    assert upd(V=-1) == -1 and b"V=-1" in err()
    assert upd(F=-1) == -1 and b"F=-1" in err()
    assert upd(n_vs=-5) == -1 and b"n_vs=-5" in err()
    assert upd(V=1 << 31) == -1 and b"2^31" in err()
    assert upd(x=None) == -1 and b"NULL" in err()
    assert upd(faces=None) == -1 and b"slot table" in err()
    assert upd(vs=(None, one)) == -1 and b"slot table" in err()
    assert upd(normals=None) == -1 and b"normals" in err()
    assert upd(out=None) == -1 and b"NULL" in err()
    assert upd(out=one) == -1 and b"alias" in err()
    assert upd(V=0, F=0, n_vs=0, x=None, faces=None, vs=(None, None), normals=None, out=None) == 0


# ---- clean_fl.py ----------------------------------------------------------------------------------------------------------------------
def test_clean_fl_carries_the_new_flags_and_refuses_bad_ones(tmp_path, capsys):
    import clean_fl
    a = clean_fl.build_parser().parse_args(["--in", "x", "--out", "y"])
    assert a.smooth is None and (a.smooth_iters, a.smooth_lambda, a.smooth_mu, a.smooth_weights, a.smooth_boundary) == (
        10, 0.5, None, "uniform", "fixed") and (a.smooth_normal_iters, a.smooth_vertex_iters, a.smooth_sigma_s) == (5, 10, 0.35)
    a = clean_fl.build_parser().parse_args(["--in", "x", "--out", "y", "--smooth", "bilateral", "--smooth-sigma-s", "0.3",
                                            "--smooth-normal-iters", "3", "--smooth-vertex-iters", "4"])
    assert (a.smooth, a.smooth_sigma_s, a.smooth_normal_iters, a.smooth_vertex_iters) == ("bilateral", 0.3, 3, 4)
    me = str(HERE / "mesh_smooth_reference.py")            # any existing file: the usage errors come before it is read
    for bad in (["--smooth", "gauss"], ["--smooth", "taubin", "--smooth-iters", "-1"], ["--smooth", "taubin", "--smooth-lambda", "0"],
                ["--smooth", "taubin", "--smooth-lambda", "1.5"], ["--smooth", "taubin", "--smooth-lambda", "nan"],
                ["--smooth", "taubin", "--smooth-mu", "0.2"], ["--smooth", "taubin", "--smooth-mu", "-inf"],
                ["--smooth", "taubin", "--smooth-weights", "area"], ["--smooth", "taubin", "--smooth-boundary", "loose"],
                ["--smooth", "bilateral", "--smooth-sigma-s", "0"], ["--smooth", "bilateral", "--smooth-normal-iters", "-1"],
                ["--smooth", "bilateral", "--smooth-vertex-iters", "-1"]):
        with pytest.raises(SystemExit):
            clean_fl.main(["--in", me, "--out", str(tmp_path)] + bad)
    with pytest.raises(SystemExit):
        clean_fl.main(["--in", me, "--report-only", "--smooth", "taubin"])          # nothing is written with --report-only
    capsys.readouterr()


def test_topology_json_is_unchanged_without_smooth(tmp_path, monkeypatch):
    """The keys of topology.json with and without --smooth, the GPU work replaced by stand-ins (the file's layout is decided on
    the host): without the flag there is no smooth key at either level."""
    import clean_fl
    from recmv import smooth, topology, utils
    v, f = MC.tube()

    class OnHost:                                           # what read_obj returns, staying on the host
        def __init__(self, t):
            self.t = t

        def to(self, device):
            return self.t
    monkeypatch.setattr(utils, "read_obj", lambda path: (OnHost(torch.from_numpy(v)), OnHost(torch.from_numpy(f))))
    monkeypatch.setattr(utils, "write_obj", lambda path, a, b: None)
    monkeypatch.setattr(topology, "report", lambda a, b: {k: 0 for k in (
        "faces", "components_vertex", "components_edge", "boundary_loops", "euler_characteristic", "watertight")})
    monkeypatch.setattr(topology, "keep_components", lambda a, b, **k: (a, b, {k: 0 for k in (
        "dropped_components", "dropped_faces", "dropped_area", "invalid_faces", "components")}))
    real = smooth.smooth
    monkeypatch.setattr(smooth, "smooth", lambda a, b, **k: real(a, b, use_kernels=False, **k))
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "a.obj").write_text("")
    plain = clean_fl.main(["--in", str(tmp_path / "in"), "--out", str(tmp_path / "plain")])
    assert sorted(plain) == ["connectivity", "files", "largest", "min_area_frac", "min_faces", "report_only"]
    assert sorted(plain["files"]["a.obj"]) == ["after", "before", "dropped"]
    assert json.loads((tmp_path / "plain" / "topology.json").read_text()) == plain
    got = clean_fl.main(["--in", str(tmp_path / "in"), "--out", str(tmp_path / "s"), "--smooth", "taubin", "--smooth-iters", "2"])
    assert got["smooth"] == "taubin" and got["smooth_iters"] == 2 and got["smooth_mu"] is None
    assert sorted(set(got) - set(plain)) == ["smooth", "smooth_boundary", "smooth_iters", "smooth_lambda", "smooth_mu",
                                             "smooth_normal_iters", "smooth_sigma_s", "smooth_vertex_iters", "smooth_weights"]
    entry = got["files"]["a.obj"]["smooth"]
    assert entry["method"] == "taubin" and entry["iterations"] == 2 and entry["moved"] > 0
    assert json.loads((tmp_path / "s" / "topology.json").read_text()) == got
