"""recmv.geodesic on the GPU: D and the sweep count K of both routes and of route='auto' are BIT EQUAL to the numpy restatement
(tests/geodesic_reference.py, which recomputes every candidate in every sweep), whatever the cadence of the convergence check;
the lds capacity; the helpers; eval_fl.py --boundary-bands.
"""
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
import geodesic_cases as GC  # noqa: E402
import geodesic_reference as GR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROUTES = ("sweeps", "lds", "auto")


def _square_values():
    v, f = GC.grid(9, jitter=0.3, noise=0.02, seed=3)
    return v, f


# name -> (mesh, list of source lists, list of value lists or None)
CASES = {
    "one_vertex": lambda: ((np.array([[1, 2, 3]], np.float32), np.zeros((0, 3), np.int64)), [[0]], None),
    "triangle": lambda: (GC.triangle(), [[0]], None),
    "square_other_diagonal": lambda: (GC.square(False), [[0]], None),
    "square_through_source": lambda: (GC.square(True), [[0]], None),
    "cylinder_bottom": lambda: (GC.cylinder(), [list(range(24))], None),
    "cylinder_both": lambda: (GC.cylinder(), [list(range(24)) + list(range(192, 216))], None),
    "grid17": lambda: (GC.grid(17), [[0]], None),
    "grid17_jittered": lambda: (GC.grid(17, jitter=0.48, noise=0.05, seed=1), [[0]], None),
    "icosphere162": lambda: (GC.icosphere(2), [[0]], None),
    "fan70": lambda: (GC.fan(70), [[5]], None),
    "two_pieces": lambda: (GC.two_pieces(), [[3]], None),
    "broken": lambda: (GC.broken(), [[0]], None),
    "values_and_duplicate": lambda: (_square_values(), [[0, 80, 0, 40]], [[0.5, 0., 0.25, 3.]]),
    "three_fields": lambda: (GC.grid(17, jitter=0.3, seed=2), [[0], [144], list(range(0, 289, 3))], None),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    (v, f), sources, values = CASES[name]()
    want = [GR.distance(v, f, s, None if values is None else values[b]) for b, s in enumerate(sources)]
    D = np.stack([w[0] for w in want])
    D.setflags(write=False)
    return v, f, sources, values, D, [w[1] for w in want]


def _dev(v, f):
    return torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int64)


def _solve(name, route, **kw):
    from recmv import geodesic
    v, f, sources, values, D, K = _case(name)
    tv, tf = _dev(v, f)
    src = [torch.tensor(s, dtype=torch.int64) for s in sources]
    val = None if values is None else [torch.tensor(x, dtype=torch.float64) for x in values]
    if len(src) == 1:
        got, k = geodesic.distance(tv, tf, src[0], None if val is None else val[0], route=route, return_sweeps=True, **kw)
        return got[None], [k]
    got, k = geodesic.distance(tv, tf, src, val, route=route, return_sweeps=True, **kw)
    return got, k.tolist()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_both_routes_give_the_bits_and_the_sweep_count_of_the_restatement(name, route):
    D, K = _case(name)[4:]
    got, k = _solve(name, route)
    print(name, route, "K", k, "want", K)
    assert got.dtype == torch.float64 and tuple(got.shape) == D.shape
    assert np.array_equal(_bits(got), D.view(np.int64))
    assert k == K


def test_the_cases_are_what_their_names_say():
    K = _case("three_fields")[5]
    assert K[0] > 1.5 * K[1] > 4 * K[2] > 0
    assert np.isinf(_case("two_pieces")[4][0]).sum() == 16
    D = _case("broken")[4][0]
    assert np.isinf(D[24]) and np.isinf(D).sum() == 1
    assert _case("grid17")[0].shape[0] == 289
    assert abs(_case("square_other_diagonal")[4][0][2] - (1. + 2. ** 0.5 / 2.)) < 1e-15


# ------------------------------------------------------------------------------------------------------------- cadence
@functools.lru_cache(maxsize=None)
def _grid33():
    v, f = GC.grid(33)
    D, K = GR.distance(v, f, [0])
    return v, f, D, K


@pytest.mark.parametrize("route", ("sweeps", "lds"))
def test_check_every_and_the_sweep_cap_change_nothing(route):
    from recmv import geodesic
    assert 17 < geodesic.DEFAULT_CHECK_EVERY < 54
    for v, f, D, K in (_grid33(), (*GC.grid(9), *GR.distance(*GC.grid(9), [0]))):
        assert (K > geodesic.DEFAULT_CHECK_EVERY) == (v.shape[0] == 33 * 33)
        tv, tf = _dev(v, f)
        src = torch.tensor([0])
        for every in (1, 7, None):
            got, k = geodesic.distance(tv, tf, src, route=route, check_every=every, return_sweeps=True)
            assert np.array_equal(_bits(got), D.view(np.int64)) and k == K
            got, k = geodesic.distance(tv, tf, src, route=route, check_every=every, max_sweeps=K, return_sweeps=True)
            assert np.array_equal(_bits(got), D.view(np.int64)) and k == K
            with pytest.raises(RuntimeError, match="not converged"):
                geodesic.distance(tv, tf, src, route=route, check_every=every, max_sweeps=K - 1)


# ------------------------------------------------------------------------------------------------------------ capacity
def test_the_lds_capacity_is_accepted_and_one_more_vertex_is_refused():
    from recmv import geodesic
    cap = geodesic.lds_max_vertices()
    assert cap == 3640 and 0 < geodesic.auto_max_vertices() <= cap
    for V in (cap, cap + 1):
        v, f = GC.with_count(V)
        D, K = GR.distance(v, f, [0])
        assert np.isfinite(D).all()
        tv, tf = _dev(v, f)
        for route in ("sweeps", "auto") + (("lds",) if V == cap else ()):
            got, k = geodesic.distance(tv, tf, torch.tensor([0]), route=route, return_sweeps=True)
            assert np.array_equal(_bits(got), D.view(np.int64)) and k == K, (V, route)
        if V > cap:
            with pytest.raises(ValueError, match="at most 3640"):
                geodesic.distance(tv, tf, torch.tensor([0]), route="lds")


# ------------------------------------------------------------------------------------------------------------- helpers
def test_per_loop_boundary_fields_and_their_labels_on_the_cylinder():
    from recmv import geodesic
    v, f = GC.cylinder()
    tv, tf = _dev(v, f)
    fields, loops = geodesic.boundary_distance(tv, tf, per_loop=True)
    assert [sorted(l) for l in loops] == [list(range(24)), list(range(192, 216))] and tuple(fields.shape) == (2, 216)
    for b, loop in enumerate(loops):
        single = geodesic.distance(tv, tf, torch.tensor(loop))
        assert np.array_equal(_bits(fields[b]), _bits(single))
        assert np.array_equal(_bits(single), GR.distance(v, f, loop)[0].view(np.int64))
    both = geodesic.boundary_distance(tv, tf)
    best, label = geodesic.nearest_source(fields)
    assert np.array_equal(_bits(best), _bits(both)) and float(both.max()) == 1.0
    ring = np.arange(216) // 24
    assert label.cpu().tolist() == np.where(ring <= 4, 0, 1).tolist()          # the tie ring (4, mid-height) goes to loop 0
    assert bool((fields[0][96:120] == fields[1][96:120]).all())
    sv, sf = _dev(*GC.icosphere(1))
    assert bool(torch.isinf(geodesic.boundary_distance(sv, sf)).all())
    fields, loops = geodesic.boundary_distance(sv, sf, per_loop=True)
    assert loops == [] and tuple(fields.shape) == (0, 42)


def test_farthest_points_are_those_of_the_restatement():
    from recmv import geodesic
    v, f = GC.icosphere(3)
    want_ids, want_run = GR.farthest_points(v, f, 6, first=7)
    ids, run = geodesic.farthest_points(*_dev(v, f), 6, first=7)
    assert ids == want_ids and len(set(ids)) == 6
    assert np.array_equal(_bits(run), want_run.view(np.int64))
    v, f = GC.two_pieces()                                                        # the other piece is never reached: inf is not a maximum
    ids, run = geodesic.farthest_points(*_dev(v, f), 40, first=0)
    assert ids == GR.farthest_points(v, f, 40, first=0)[0] and len(ids) == 36 and max(ids) < 36


# ------------------------------------------------------------------------------------------------------------- eval_fl
def _write_obj(path, v, f):
    with open(path, "w") as out:
        for p in v:
            out.write("v %.9g %.9g %.9g\n" % tuple(p))
        for t in f:
            out.write("f %d %d %d\n" % tuple(t + 1))


def test_eval_fl_boundary_bands(tmp_path):
    import eval_fl
    gv, gf = GC.cylinder()
    pv = gv.copy()
    pv[:, :2] *= (1. + 0.02 * gv[:, 2:3])                                         # wider towards the top
    _write_obj(tmp_path / "pred.obj", pv, gf)
    _write_obj(tmp_path / "gt.obj", gv, gf)
    _write_obj(tmp_path / "closed.obj", *GC.icosphere(2))
    common = ["--gpu-ids", "0", "--gt", str(tmp_path / "gt.obj"), "--samples", "4000", "--seed", "3"]
    eval_fl.main(common + ["--pred", str(tmp_path / "pred.obj"), "--out", str(tmp_path / "plain.json")])
    eval_fl.main(common + ["--pred", str(tmp_path / "pred.obj"), "--out", str(tmp_path / "bands.json"), "--boundary-bands", "0.2,0.5,5"])
    plain = json.loads((tmp_path / "plain.json").read_text())
    bands = json.loads((tmp_path / "bands.json").read_text())
    pair = bands["pairs"]["pred"]
    bb = pair.pop("boundary_bands")
    assert pair == plain["pairs"]["pred"] and bands["mean"] == plain["mean"]     # json round-trips a float exactly
    assert bb["widths"] == [0.2, 0.5, 5.] and bb["pred_reason"] is None and bb["gt_reason"] is None
    for side, key in (("pred", "accuracy"), ("gt", "completeness")):
        rows = bb[side]
        assert [(r["lo"], r["hi"]) for r in rows] == [(0., 0.2), (0.2, 0.5), (0.5, 5.), (5., None)]
        assert sum(r["count"] for r in rows) == 4000
        assert rows[3] == {"lo": 5., "hi": None, "count": 0, "mean": None, "rms": None, "max": None}
        assert all(r["count"] > 0 and 0. <= r["mean"] <= r["rms"] <= r["max"] for r in rows[:3])
        total = sum(r["count"] * r["mean"] for r in rows[:3]) / 4000.
        assert abs(total - pair[key]) <= 1e-12 * pair[key]
        assert max(r["max"] for r in rows[:3]) == pair[key + "_max"]
    eval_fl.main(common + ["--pred", str(tmp_path / "closed.obj"), "--out", str(tmp_path / "closed.json"), "--boundary-bands", "0.2"])
    bb = json.loads((tmp_path / "closed.json").read_text())["pairs"]["closed"]["boundary_bands"]
    assert bb["pred"] is None and bb["pred_reason"] == "closed" and bb["gt"] is not None and bb["gt_reason"] is None
