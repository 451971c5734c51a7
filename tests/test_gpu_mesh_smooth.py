"""Mesh smoothing on the GPU: the four kernels of csrc/mesh_smooth.hip against the numpy restatement
(tests/mesh_smooth_reference.py) within bounds built from the reference's own term counts and magnitudes, the shapes where a
kernel can go wrong, the exact properties (symmetry, repeatability, pinned and curve boundaries, flatness, the convex range of
a lambda step), the driver over many iterations within the propagated bound, the quality properties, and clean_fl.py --smooth."""
import functools
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
import test_mesh_smooth_cpu as CPU  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIGMA_S = 0.35


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr(rows, dtype):
    off, idx = CPU.csr(rows, dtype)
    return off.to(DEV), idx.to(DEV)


def run(v, f, **kw):
    from recmv import smooth
    fixed = kw.pop("fixed", None)
    x, info = smooth.smooth(dev(v), dev(f), fixed=None if fixed is None else dev(fixed), **kw)
    assert x.is_cuda and x.dtype == torch.float32 and x.shape == v.shape
    return x.cpu().numpy(), info


MESHES = {
    "sphere": lambda: MC.noisy_sphere()[:2],
    "cube": lambda: MC.noisy_cube()[:2],
    "fan254": lambda: MC.fan(254),                          # V = 255, 256, 257: the edge of a block of 256 threads
    "fan255": lambda: MC.fan(255),
    "fan256": lambda: MC.fan(256),
    "fan200": lambda: MC.fan(200),                          # a hub row of 200 neighbours
    "hinged": MC.hinged_tetrahedra,                         # an edge with four faces: face rows of five neighbours
    "pinched": MC.pinched_tetrahedra,
    "tube": MC.tube,
    "isolated": lambda: MC.with_isolated_vertex(MC.tube()),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The mesh, its tables and one step of every kernel by the reference — computed once, shared, never changed."""
    v, f = MESHES[name]()
    t = MR.Tables(f, len(v))
    c = {"v": v, "f": f, "t": t, "cot": MR.cotan_weights(v, f, t)}
    unit, area, cen, _ = MR.face_geometry(v, f)
    c.update(n32=unit.astype(np.float32), area=area, cen=cen, sigma_c=MR.mean_centroid_distance(cen, t))
    c["filter"] = MR.normal_filter(c["n32"], area, cen, t, c["sigma_c"], SIGMA_S)
    c["update"] = MR.vertex_update(v, f, c["filter"][0], t, t.boundary)
    return c


def tables(c):
    t = c["t"]
    return csr(t.nbr, torch.int32), csr(t.slots, torch.int64), csr(t.ff, torch.int32)


def ratio(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.


# ---- every kernel against the reference, one step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
def test_kernels_within_the_term_count_bounds(name):
    """One step of each kernel against the float64 reference, which sums the same terms in the same order.

    Vertex outputs (float32): |got - ref| <= 1/2 ulp_f32(ref) + gamma_n * sum |terms|, gamma_n = n u / (1 - n u), u = 2^-53.  The
    first part is the one rounding at the store; the second bounds what two float64 evaluations of a sum of `terms` terms, each
    made by a fixed number of operations (MR.STEP_OPS, MR.UPDATE_OPS), can differ by: n = terms + operations, and sum |terms| is
    |x_i| + |lambda| (sum_j w_ij |x_j| / sum_j w_ij + |x_i|) for a step, |x_i| + 1/|F_i| sum_f |n_f| sum_c |n_f,c| (|c_f,c| + |x_i,c|)
    for the vertex update — each term as the magnitude its rounding error scales with, cancellation included.
    Cotangent weights (float64, nothing is rounded to float32): gamma_n * sum over the edge's faces of 1/2 (sum_c |e1_c e2_c| / |e1 x
    e2| + |cot| * spread), spread >= 1 the cancellation inside the cross product, n = faces + MR.COT_OPS.
    Filtered normals (float32 against the reference's unrounded float64 unit vectors): one float32 spacing of the component.
    The device's exp differs from the host's by a few float64 ulps, far below that; the general form 1/2 ulp + 2 gamma_n sum |w_j
    n_j| / |sum| (the factor 2: the sum and its length; the exp's ulps are counted in MR.FILTER_OPS) is printed beside it."""
    from recmv import smooth
    c = case(name)
    v, f, t = c["v"], c["f"], c["t"]
    tv, tf = dev(v), dev(f)
    nbr, slots, ff = tables(c)
    w, invalid, wt, wm = c["cot"]
    got_w, n_bad = smooth.cotangent_weights(tv, tf, nbr, slots, return_counts=True)
    again = smooth.cotangent_weights(tv, tf, nbr, slots)
    flat = np.concatenate(w) if len(w) else np.zeros(0)
    bound = np.concatenate([MR.gamma(a + MR.COT_OPS) * m for a, m in zip(wt, wm)])
    err = np.abs(got_w.cpu().numpy() - flat)
    print("cotangent weights: largest error / bound", ratio(err, bound))
    assert n_bad == invalid == 0 and (err <= bound).all() and torch.equal(got_w, again)
    # symmetric bit for bit: w[i -> j] == w[j -> i]
    off, idx = (x.cpu().numpy().astype(np.int64) for x in nbr)
    rows = np.repeat(np.arange(len(v)), np.diff(off))
    key, back = rows * len(v) + idx, idx * len(v) + rows
    assert np.array_equal(got_w.cpu().numpy(), got_w.cpu().numpy()[np.searchsorted(key, back)]) and len(key) > 0

    pinned = dev(t.boundary)
    for lam, weights, fixed, bnbr in ((0.5, None, None, None), (MR.default_mu(0.5), None, t.boundary, None),
                                      (1.0, w, None, t.bnbr), (0.5, w, t.boundary, None)):
        out, ref, terms, mags = MR.laplacian_step(v, t, lam, weights, fixed, bnbr)
        args = (tv, nbr, lam, None if weights is None else got_w, None if fixed is None else pinned,
                None if bnbr is None else dev(bnbr))
        got = smooth.laplacian_step(*args)
        bound = MR.step_bound(ref, terms, mags, MR.STEP_OPS)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        print("laplacian step lam=%.3f: largest error / bound" % lam, ratio(err, bound))
        assert (err <= bound).all() and torch.equal(got, smooth.laplacian_step(*args))
        still = terms == 0
        assert np.array_equal(got.cpu().numpy()[still], v[still])                  # copied bit for bit
        if fixed is not None:
            assert still[t.boundary].all()

    out, ref, terms, rel, _ = c["filter"]
    args = (dev(c["n32"]), dev(c["area"]), dev(c["cen"]), ff, c["sigma_c"], SIGMA_S)
    got = smooth.filter_face_normals(*args)
    general = 0.5 * MR.ulp32(ref) + (2 * MR.gamma(terms + MR.FILTER_OPS) * rel)[:, None]
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print("normal filter: largest error / float32 spacing", ratio(err, MR.ulp32(ref)), "largest error / general bound", ratio(err, general))
    assert (err <= MR.ulp32(ref)).all() and torch.equal(got, smooth.filter_face_normals(*args))
    assert np.abs(np.linalg.norm(got.cpu().numpy().astype(np.float64), axis=1) - 1).max() < 1e-6

    out, ref, terms, mags, _ = c["update"]
    args = (tv, tf, dev(c["filter"][0]), slots, pinned)
    got = smooth.update_vertices(*args)
    bound = MR.step_bound(ref, terms, mags, MR.UPDATE_OPS)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print("vertex update: largest error / bound", ratio(err, bound))
    assert (err <= bound).all() and torch.equal(got, smooth.update_vertices(*args))
    assert np.array_equal(got.cpu().numpy()[t.boundary], v[t.boundary])
    if name == "isolated":                                  # no neighbour, no face: every kernel leaves it where it is
        assert len(t.nbr[-1]) == 0 and np.array_equal(got.cpu().numpy()[-1], v[-1])
        assert np.array_equal(smooth.laplacian_step(tv, nbr, 0.5).cpu().numpy()[-1], v[-1])
    if name == "hinged":
        assert max(len(r) for r in t.ff) == 5
    if name == "fan200":
        assert len(t.nbr[0]) == 200 and len(t.slots[0]) == 200


def test_invalid_faces_and_a_nan_corner():
    """Three invalid faces (-1, V + 1, a repeated corner), a corner that is not a number and a vertex whose only face is invalid,
    with the tables of the faces with valid indices: the count is exact (the three and the faces of the NaN corner), the
    weights and the vertex update are finite everywhere but at that corner, and the reference's."""
    from recmv import smooth
    v, f, nan_at, lonely = MC.with_invalid_faces(MC.noisy_sphere()[:2])
    t = MR.Tables(f, len(v))
    nbr, slots = csr(t.nbr, torch.int32), csr(t.slots, torch.int64)
    tv, tf = dev(v), dev(f)
    w, invalid, wt, wm = MR.cotan_weights(v, f, t)
    with_nan = int(((f == nan_at).any(1) & MR.valid_index_faces(f, len(v))).sum())
    got, n_bad = smooth.cotangent_weights(tv, tf, nbr, slots, return_counts=True)
    bound = np.concatenate([MR.gamma(a + MR.COT_OPS) * m for a, m in zip(wt, wm)])
    assert n_bad == invalid == 3 + with_nan and with_nan >= 4
    assert np.isfinite(got.cpu().numpy()).all() and (np.abs(got.cpu().numpy() - np.concatenate(w)) <= bound).all()
    assert len(t.nbr[lonely]) == 0 and len(t.slots[lonely]) == 0
    # a weighted step: the NaN corner's own row has no weight > 0, so it is copied; its neighbours lose only that edge
    out, ref, terms, mags = MR.laplacian_step(v, t, 0.5, w)
    res = smooth.laplacian_step(tv, nbr, 0.5, got).cpu().numpy()
    rest = np.arange(len(v)) != nan_at
    assert np.isfinite(res[rest]).all() and (np.abs(res[rest] - ref[rest]) <= MR.step_bound(ref, terms, mags, MR.STEP_OPS)[rest]).all()
    assert np.array_equal(res[lonely], v[lonely]) and np.array_equal(res[nan_at], v[nan_at], equal_nan=True)
    unit = MR.face_geometry(v, f)[0].astype(np.float32)
    out, ref, terms, mags, _ = MR.vertex_update(v, f, unit, t)
    res = smooth.update_vertices(tv, tf, dev(unit), slots).cpu().numpy()
    assert np.isfinite(res[rest]).all() and (np.abs(res[rest] - ref[rest]) <= MR.step_bound(ref, terms, mags, MR.UPDATE_OPS)[rest]).all()
    assert np.array_equal(res[lonely], v[lonely]) and np.array_equal(res[nan_at], v[nan_at], equal_nan=True)
    # the driver leaves the same faces out
    x, info = run(v, f, method="bilateral", vertex_iterations=1, boundary="free")
    assert info["invalid_faces"] == 3 + with_nan and np.isfinite(x[rest]).all() and np.array_equal(x[lonely], v[lonely])


def test_empty_meshes_are_no_ops():
    from recmv import smooth
    v0, f0 = torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int64, device=DEV)
    e32, e64 = (torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)), \
        (torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    assert smooth.cotangent_weights(v0, f0, e32, e64).shape == (0,)
    assert smooth.laplacian_step(v0, e32, 0.5).shape == (0, 3)
    assert smooth.filter_face_normals(v0, torch.zeros(0, dtype=torch.float64, device=DEV),
                                      torch.zeros(0, 3, dtype=torch.float64, device=DEV), e32, 0.1, 0.35).shape == (0, 3)
    assert smooth.update_vertices(v0, f0, v0, e64).shape == (0, 3)
    for method in ("taubin", "bilateral"):
        x, info = smooth.smooth(v0, f0, method=method)
        assert x.shape == (0, 3) and info["moved"] == 0
    v = dev(MC.tube()[0])                                   # vertices without faces: nothing moves
    x, info = smooth.smooth(v, f0, weights="cotangent")
    assert torch.equal(x, v) and info["moved"] == 0 and info["area_before"] == 0


# ---- exact properties -------------------------------------------------------------------------------------------------------------------
def test_two_runs_of_the_driver_have_the_same_bits():
    v, f = case("sphere")["v"], case("sphere")["f"]
    for kw in (dict(method="taubin", weights="cotangent", reweight=True), dict(method="bilateral")):
        a, ia = run(v, f, **kw)
        b, ib = run(v, f, **kw)
        assert np.array_equal(a, b) and ia == ib


def test_fixed_and_curve_boundaries_of_the_tube():
    v, f = MC.tube()
    on = MR.Tables(f, len(v)).boundary
    for kw in (dict(method="taubin"), dict(method="bilateral"), dict(method="taubin", weights="cotangent")):
        x, info = run(v, f, **kw)
        assert np.array_equal(x[on], v[on]) and not np.array_equal(x[~on], v[~on]) and info["moved"] == int((~on).sum())
    mask = np.zeros(len(v), bool)
    mask[40:60] = True
    for method in ("taubin", "bilateral"):
        x, _ = run(v, f, method=method, boundary="free", fixed=mask)
        assert np.array_equal(x[mask], v[mask]) and not np.array_equal(x[on], v[on])
    CPU.check_curve_boundary(lambda **kw: run(v, f, **kw)[0], v, f, on)


def test_flat_grid_stays_flat():
    from recmv import smooth
    v, f = MC.flat_grid()
    t = MR.Tables(f, len(v))
    for kw in (dict(method="taubin", boundary="free"), dict(method="laplacian", weights="cotangent", boundary="curve"),
               dict(method="taubin", weights="cotangent", boundary="free"), dict(method="bilateral", boundary="free")):
        x, info = run(v, f, **kw)
        assert (x[:, 2] == 0).all()
        if kw["method"] == "bilateral":
            assert np.array_equal(x, v) and info["moved"] == 0
    x = smooth.laplacian_step(dev(v), csr(t.nbr, torch.int32), 0.5).cpu().numpy()
    balanced = np.array([not t.boundary[i] and not (v[t.nbr[i]] - v[i]).sum(0).any() for i in range(len(v))])
    assert balanced.sum() == 49 and np.array_equal(x[balanced], v[balanced]) and not np.array_equal(x, v)


@pytest.mark.parametrize("lam", [0.25, 0.5, 1.0])
def test_a_lambda_step_stays_inside_its_neighbourhood(lam):
    """For 0 < lam <= 1 the step is a convex combination of the vertex and its neighbours, and rounding is monotone: every output
    coordinate lies in the closed range of those inputs' coordinates, exactly."""
    from recmv import smooth
    c = case("sphere")
    v, t = c["v"], c["t"]
    nbr, slots, _ = tables(c)
    w = smooth.cotangent_weights(dev(v), dev(c["f"]), nbr, slots)
    lo = np.array([v[[i] + t.nbr[i]].min(0) for i in range(len(v))])
    hi = np.array([v[[i] + t.nbr[i]].max(0) for i in range(len(v))])
    for weights in (None, w):
        x = smooth.laplacian_step(dev(v), nbr, lam, weights).cpu().numpy()
        assert (x >= lo).all() and (x <= hi).all() and not np.array_equal(x, v)


# ---- the driver over many steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(method="taubin"), dict(method="taubin", weights="cotangent"),
                                dict(method="bilateral", normal_iterations=2, vertex_iterations=3)],
                         ids=["taubin-uniform", "taubin-cotangent", "bilateral"])
def test_driver_within_the_propagated_bound(kw):
    """10 Taubin iterations (20 steps) and a bilateral run against the reference driver, which rounds to float32 after every step
    too.  MR.smooth propagates the one-step bounds: a difference D before a step is at most gain * D + b after it; lam step:
    gain |1 - lam| + |lam| = 1, mu step: 1 + 2 |mu|; b = the step's largest one-step bound plus half a float32 spacing, for two
    float64 results on either side of a rounding boundary.  The bilateral run is kept short (2 + 3 iterations): the normal
    filter's gain, taken from its own sums, is above 10 per iteration, and a bound grown over 5 + 10 would say nothing."""
    v, f = case("sphere")["v"], case("sphere")["f"]
    x, info = run(v, f, **kw)
    ref, bound, _ = MR.smooth(v, f, sigma_c=info.get("sigma_c"), **kw)
    err = float(np.abs(x.astype(np.float64) - ref).max())
    print("largest error %.3g, propagated bound %.3g, ratio %.3g" % (err, bound, err / bound))
    assert err <= bound < 1e-3                             # (below 1 % of what the run moves: the bound says something)


# ---- quality ------------------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_noisy_sphere():
    """10 uniform Taubin iterations: roughness at most half, |dV| / V at most a quarter of 10 Laplacian iterations', the radial
    error falls — on the reference first (a failing input shows without the kernels), then on the kernel path."""
    CPU.check_sphere_quality(lambda v, f, m: MR.smooth(v, f, method=m)[0])
    CPU.check_sphere_quality(lambda v, f, m: run(v, f, method=m)[0])
    v, f = case("sphere")["v"], case("sphere")["f"]
    x, info = run(v, f)
    assert abs(info["roughness_after"] - MR.roughness(x, f)) < 1e-9 and abs(info["volume_after"] - MR.volume(x, f)) < 1e-9
    assert abs(info["area_after"] - MR.area(x, f)) < 1e-9 and info["moved"] == len(v)


def test_quality_on_the_noisy_cube():
    """bilateral with the defaults: the rms distance to the cube's surface at most 0.7 x the input's and below 10 Taubin
    iterations', which round the edges off."""
    CPU.check_cube_quality(lambda v, f, m: MR.smooth(v, f, method=m)[0])
    CPU.check_cube_quality(lambda v, f, m: run(v, f, method=m)[0])


# ---- clean_fl.py --------------------------------------------------------------------------------------------------------------------------
def test_clean_fl_smooths_before_it_simplifies(tmp_path, capsys):
    import json
    import clean_fl
    from recmv.utils import read_obj, write_obj
    src = tmp_path / "in"
    src.mkdir()
    meshes = {"sphere.obj": MC.noisy_sphere()[:2], "tube.obj": MC.tube()}
    for name, (v, f) in meshes.items():
        write_obj(str(src / name), torch.from_numpy(v), torch.from_numpy(f))
    out = clean_fl.main(["--in", str(src), "--out", str(tmp_path / "out"), "--smooth", "taubin", "--simplify-ratio", "0.5"])
    capsys.readouterr()
    assert out["smooth"] == "taubin" and out["simplify_ratio"] == 0.5
    assert json.loads((tmp_path / "out" / "topology.json").read_text()) == json.loads(json.dumps(out))
    for name, (v, f) in meshes.items():
        e = out["files"][name]
        order = list(e)
        assert order.index("smooth") < order.index("simplify") < order.index("after")
        assert e["smooth"]["method"] == "taubin" and e["smooth"]["moved"] > 0
        assert e["simplify"]["faces_before"] == len(f) == e["before"]["faces"]
        assert e["after"]["boundary_loops"] == e["before"]["boundary_loops"] and e["after"]["faces"] in (len(f) // 2, len(f) // 2 + 1)
        nv, nf = read_obj(str(tmp_path / "out" / name))
        assert nf.shape[0] == e["after"]["faces"] and torch.isfinite(nv).all()
    assert out["files"]["tube.obj"]["before"]["boundary_loops"] == 2
    plain = clean_fl.main(["--in", str(src), "--out", str(tmp_path / "plain")])
    capsys.readouterr()
    assert not [k for k in plain if k.startswith("smooth")] and "smooth" not in plain["files"]["tube.obj"]
