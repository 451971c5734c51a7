"""recmv.topology on the GPU against tests/mesh_topology_reference.py (numpy float64 + scipy's connected components).

Integers (labels, ids, counts, orders, genus) are compared for equality.  Tolerances, derived and not tuned:
  * a sum of n per-face figures (a piece's area, the mesh's area, a mean): the per-face formula is the same float64 sequence
    with contraction off on both sides, so only the order of the summation differs — n 2^-53 relative per order, doubled — plus
    16 eps for the sqrt and atan2 of two maths libraries: (n + 16) 2^-52 times the value (mesh_topology_reference.area_tolerance);
  * one per-face figure (an area, an edge length, an edge ratio): 16 eps relative; an angle: 1e-12 rad;
  * minima, maxima and bounding boxes of float32 coordinates: exact.
"""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import mesh_topology_cases as TC  # noqa: E402
import mesh_topology_reference as TR  # noqa: E402

DEV = "cuda:0"
EPS64 = TR.EPS64
ANGLE_TOL = 1e-12                                          # rad


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def body():
    from test_gpu_animation import _irregular_body
    v, f = _irregular_body(level=3)                        # 1280 faces, closed
    return v.numpy(), f.numpy()


def body_with_floaters(count=40):
    return TC.merge(body(), TC.floaters(count))


def check_graph(n, links):
    """Both runs (the second with a read-back after every round) give the reference's labels, the same round count within the
    cap, and the exact number of rows that join nothing."""
    from recmv import topology
    links = np.asarray(links, np.int64)
    want, invalid = TR.graph_components(n, links)
    a, ia = topology.graph_components(n, dev(links), return_info=True)
    b, ib = topology.graph_components(n, dev(links), return_info=True, rounds_per_readback=1)
    print("n %d, %d rows of %d: %d rounds (cap %d), %d invalid" % (n, links.shape[0], links.shape[1], ia['rounds'], ia['cap'],
                                                                  ia['invalid']))
    assert a.dtype == torch.int64 and a.shape == (n,)
    assert torch.equal(a, b) and ia == ib
    assert torch.equal(a.cpu(), torch.from_numpy(want))
    assert ia['invalid'] == invalid
    assert 1 <= ia['rounds'] <= ia['cap'] == 2 * max(n - 1, 0).bit_length() + 2
    return ia


@pytest.mark.parametrize("K", [3, 2])
@pytest.mark.parametrize("numbering", ["random", "ascending", "descending"])
def test_graph_components_on_a_deep_strip(numbering, K):
    f, n = TC.strip_faces(4097, numbering)
    info = check_graph(n, f if K == 3 else TC.face_edges(f))
    if numbering != "random":
        assert info['rounds'] == 2                         # every vertex hangs under its neighbour: one round, and one to see it


@pytest.mark.parametrize("hub", [None, 0, 5000])
def test_graph_components_under_contention(hub):
    f, n = TC.hub_faces(5000, hub)
    check_graph(n, f)
    check_graph(n, TC.face_edges(f))


def test_graph_components_on_isolated_triangles_and_the_body():
    bv, bf = body()
    iso = len(bv) + np.arange(9000, dtype=np.int64).reshape(3000, 3)
    check_graph(len(bv) + 9000 + 5, np.concatenate([bf, iso]))                    # (5 nodes that no row touches)
    check_graph(len(bv) + 9000 + 5, TC.face_edges(np.concatenate([iso, bf])))


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 255, 257])
def test_graph_components_on_few_rows(M):
    f, n = TC.strip_faces(4097, "random")
    check_graph(n, TC.face_edges(f)[:M])
    check_graph(n, f[:M])


@pytest.mark.parametrize("K", [2, 3])
def test_graph_components_rows_that_join_nothing(K):
    f, n = TC.strip_faces(600, "random")
    links = TC.with_invalid_rows(f if K == 3 else TC.face_edges(f), n)
    info = check_graph(n, links)
    assert info['invalid'] == len(range(0, len(links), 7))


def test_graph_components_without_nodes():
    from recmv import topology
    label, info = topology.graph_components(0, torch.zeros(0, 2, dtype=torch.int64, device=DEV), return_info=True)
    assert label.shape == (0,) and info['rounds'] == 1 and info['invalid'] == 0
    label = topology.graph_components(7, torch.zeros(0, 3, dtype=torch.int64, device=DEV))
    assert label.tolist() == list(range(7))


def test_segment_sums_are_exact_enough_and_reproducible():
    from recmv import _lib, topology
    chunk = int(_lib.lib().recmv_segment_sums_chunk())
    lens = [0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 0, 3 * chunk + 5, 300001, 0]
    g = np.random.default_rng(2)
    x = np.concatenate([g.normal(size=(sum(lens), 2)), g.random((sum(lens), 1)) * 1e-3 + 1.], 1)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    s, lo, hi = topology.segment_sums(dev(x), dev(off))
    s2, lo2, hi2 = topology.segment_sums(dev(x), dev(off))
    assert torch.equal(s, s2) and torch.equal(lo, lo2) and torch.equal(hi, hi2)   # bit for bit
    s, lo, hi = s.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
    for k, n in enumerate(lens):
        seg = x[off[k]:off[k + 1]]
        for c in range(3):
            want = math.fsum(seg[:, c])                    # exactly rounded
            assert abs(s[k, c] - want) <= n * 2.0 ** -53 * math.fsum(np.abs(seg[:, c])), (k, c)   # any order of n additions
        if n:
            assert np.array_equal(lo[k], seg.min(0)) and np.array_equal(hi[k], seg.max(0))
        else:
            assert np.all(lo[k] == np.inf) and np.all(hi[k] == -np.inf) and np.all(s[k] == 0)


def test_face_stats_equal_the_reference():
    from recmv import topology
    v, f = body()
    v = np.concatenate([v, [[np.nan, 0, 0], [np.inf, 1, 1]], v[:1]]).astype(np.float32)
    V = len(v)
    f = np.concatenate([f, [[0, 1, V], [2, 2, 3], [-1, 0, 1], [0, 1, V - 3], [V - 2, 5, 6], [0, V - 1, 1], [7, 7, 7]]]).astype(np.int64)
    area, ang, ratio, counts = topology.face_stats(dev(v), dev(f))
    r_area, r_ang, r_ratio, r_nonfinite = TR.face_stats(v, f)
    area, ang, ratio = area.cpu().numpy(), ang.cpu().numpy(), ratio.cpu().numpy()
    assert counts.tolist() == [4, r_nonfinite] and r_nonfinite == 2
    for got, want, tol in ((area, r_area, 16 * EPS64 * np.abs(r_area)), (ang, r_ang, ANGLE_TOL), (ratio, r_ratio, 16 * EPS64 * np.abs(r_ratio))):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
        ok = np.isfinite(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= np.broadcast_to(tol, want.shape)[ok])
    assert np.isinf(ratio[-2]) and area[-2] == 0 and ang[-2] == 0                  # a valid face with an edge of length 0


def compare_components(got, want, n_faces_total):
    assert got['count'] == want['count']
    assert torch.equal(got['face_component'].cpu(), torch.from_numpy(want['face_component']))
    if want['vertex_component'] is None:
        assert got['vertex_component'] is None
    else:
        assert torch.equal(got['vertex_component'].cpu(), torch.from_numpy(want['vertex_component']))
    assert torch.equal(got['faces_per_component'].cpu(), torch.from_numpy(want['faces_per_component']))
    assert torch.equal(got['by_area'].cpu(), torch.from_numpy(want['by_area']))
    assert got['invalid_faces'] == want['invalid_faces']
    area = got['area'].cpu().numpy()
    for c in range(want['count']):
        n = int(want['faces_per_component'][c])
        assert abs(area[c] - want['area'][c]) <= TR.area_tolerance(n, want['area'][c]), (c, area[c], want['area'][c])
    assert np.array_equal(got['bbox_min'].cpu().numpy().astype(np.float64), want['bbox_min'])
    assert np.array_equal(got['bbox_max'].cpu().numpy().astype(np.float64), want['bbox_max'])


@pytest.mark.parametrize("connectivity", ["vertex", "edge"])
@pytest.mark.parametrize("mesh", ["pinched", "hinged", "with invalid faces"])
def test_components_on_hand_cases(mesh, connectivity):
    from recmv import topology
    if mesh == "pinched":
        v, f = TC.pinched_tetrahedra()
    elif mesh == "hinged":
        v, f = TC.hinged_tetrahedra()
    else:
        v, f = TC.merge(TC.tetrahedron(), TC.tetrahedron(0.5, (3, 0, 0)))
        v = np.concatenate([v, [[9, 9, 9]]]).astype(np.float32)                    # an unreferenced vertex
        f = np.concatenate([[[0, 1, 9]], f[:3], [[2, 2, 3]], f[3:], [[-1, 0, 1]]]).astype(np.int64)
    got = topology.components(dev(v), dev(f), connectivity)
    compare_components(got, TR.components(v, f, connectivity), len(f))
    if mesh == "pinched":
        assert got['count'] == (1 if connectivity == 'vertex' else 2)
    if mesh == "hinged":
        assert got['count'] == 1


@pytest.mark.parametrize("connectivity", ["vertex", "edge"])
def test_components_of_the_body_with_floaters(connectivity):
    from recmv import topology
    v, f = body_with_floaters(40)
    got = topology.components(dev(v), dev(f), connectivity)
    again = topology.components(dev(v), dev(f), connectivity)
    compare_components(got, TR.components(v, f, connectivity), len(f))
    assert got['count'] == 41 and got['faces_per_component'].tolist() == [1280] + [4] * 40
    assert got['by_area'].tolist() == [0] + list(range(40, 0, -1))                 # every floater larger than the one before
    assert torch.equal(got['area'], again['area'])                                 # bit for bit
    assert got['rounds'] == again['rounds']


def compare_reports(got, want):
    assert set(got) == set(want)
    json.dumps(got)
    for k, w in want.items():
        if isinstance(w, (bool, int)):
            assert got[k] == w and type(got[k]) is type(w), k
    F = want['faces']
    assert abs(got['area'] - want['area']) <= TR.area_tolerance(F, want['area'])
    to_deg = 180. / math.pi
    assert abs(got['min_angle_deg']['min'] - want['min_angle_deg']['min']) <= ANGLE_TOL * to_deg
    assert abs(got['min_angle_deg']['mean'] - want['min_angle_deg']['mean']) <= (ANGLE_TOL + TR.area_tolerance(F, math.pi / 3)) * to_deg
    assert got['min_angle_deg']['below_10_deg'] == want['min_angle_deg']['below_10_deg']
    for k in ('min', 'max'):
        assert abs(got['edge_length'][k] - want['edge_length'][k]) <= 16 * EPS64 * want['edge_length'][k]
    assert abs(got['edge_length']['mean'] - want['edge_length']['mean']) <= TR.area_tolerance(want['edges'], want['edge_length']['mean'])
    assert len(got['components']) == len(want['components'])
    for g, w in zip(got['components'], want['components']):
        for k in ('id', 'faces', 'boundary_loops', 'euler_characteristic', 'genus', 'bbox_min', 'bbox_max'):
            assert g[k] == w[k], k
        assert abs(g['area'] - w['area']) <= TR.area_tolerance(w['faces'], w['area'])
        assert abs(g['area_share'] - w['area_share']) <= TR.area_tolerance(w['faces'] + F + 16, w['area_share'])


@pytest.mark.parametrize("mesh", ["body", "body with floaters and a flipped face", "tube"])
def test_report(mesh):
    from recmv import topology
    if mesh == "body":
        v, f = body()
    elif mesh == "tube":
        v, f = TC.tube(17, 6)
    else:
        v, f = TC.flipped(body_with_floaters(40), 77)
    got = topology.report(dev(v), dev(f))
    want = TR.report(v, f)
    print(json.dumps(got)[:600])
    compare_reports(got, want)
    if mesh == "body":
        assert got['watertight'] and got['euler_characteristic'] == 2 and got['components'][0]['genus'] == 0
    elif mesh == "tube":
        assert got['boundary_loops'] == 2 and got['euler_characteristic'] == 0 and got['components'][0]['genus'] == 0
        assert not got['watertight'] and got['components_vertex'] == 1
    else:
        assert got['orientation_conflicts'] == 3 and got['components_vertex'] == 41 and len(got['components']) == 8
        assert got['components'][0]['genus'] is None and got['components'][1]['genus'] == 0 and not got['watertight']
        assert got['euler_characteristic'] == 2 * 41


def test_report_of_meshes_without_valid_faces():
    from recmv import topology
    v = torch.zeros(3, 3, device=DEV)
    for f in (torch.zeros(0, 3, dtype=torch.int64, device=DEV), torch.tensor([[0, 0, 1], [0, 1, 5]], device=DEV)):
        got = topology.report(v, f)
        compare = TR.report(v.cpu().numpy(), f.cpu().numpy())
        assert got == compare and not got['watertight'] and got['components'] == [] and got['unreferenced_vertices'] == 3


RULES = [dict(), dict(min_area_frac=0.01), dict(largest=3), dict(min_faces=5), dict(largest=5, min_faces=4, min_area_frac=2e-4),
         dict(largest=1, connectivity='edge'), dict(min_area_frac=1.0), dict(largest=0)]


@pytest.mark.parametrize("rules", RULES, ids=[",".join("%s=%s" % kv for kv in r.items()) or "none" for r in RULES])
def test_keep_components(rules):
    from recmv import topology
    v, f = body_with_floaters(12)
    v = np.concatenate([v[:100], [[7, 7, 7]], v[100:]]).astype(np.float32)        # an unreferenced vertex in the middle
    f = np.where(f >= 100, f + 1, f)
    f = np.concatenate([f[:10], [[0, 0, 1]], f[10:], [[0, 1, len(v)]]]).astype(np.int64)                 # two invalid faces
    kv, kf, info = topology.keep_components(dev(v), dev(f), **rules)
    r_v, r_f, r_kept, r_map, r_dropped, r_dropped_faces = TR.keep_components(v, f, **rules)
    assert torch.equal(kf.cpu(), torch.from_numpy(r_f)) and torch.equal(info['kept_faces'].cpu(), torch.from_numpy(r_kept))
    assert torch.equal(info['vertex_map'].cpu(), torch.from_numpy(r_map))
    assert kv.dtype == torch.float32 and torch.equal(kv.cpu().view(torch.int32), torch.from_numpy(r_v).view(torch.int32))   # the rows' bits
    assert info['dropped_components'] == r_dropped and info['dropped_faces'] == r_dropped_faces and info['invalid_faces'] == 2
    assert info['components'] == 13 and len(info['kept_components']) == 13 - r_dropped
    if not rules:
        assert len(r_kept) == len(f) - 2 and len(r_v) == len(v) - 1
    if rules == dict(min_area_frac=0.01):
        assert len(r_kept) == 1280 and r_dropped == 12
    if rules == dict(largest=0):
        assert kv.shape == (0, 3) and kf.shape == (0, 3)


def floater_scene():
    """The prediction: the body and one small far floater appended after it; the ground truth: the body.  Also a lower bound
    of the distance from any point of the floater to the body."""
    bv, bf = body()
    shift, size = np.array([2., -1.5, 1.]), 0.05
    pv, pf = TC.merge((bv, bf), TC.tetrahedron(size, shift))
    gap = float(np.linalg.norm(shift)) - 2 * size - float(np.linalg.norm(bv.astype(np.float64), axis=1).max())
    return pv, pf, bv, bf, gap


def test_dropping_a_floater_gives_the_bodys_metrics_exactly():
    from recmv import metrics, topology
    pv, pf, bv, bf, gap = floater_scene()
    kv, kf, info = topology.keep_components(dev(pv), dev(pf), min_area_frac=0.01)
    assert info['dropped_components'] == 1 and info['dropped_faces'] == 4
    assert torch.equal(kv.cpu(), torch.from_numpy(bv)) and torch.equal(kf.cpu(), torch.from_numpy(bf))
    kw = dict(samples=20000, seed=0)
    clean = metrics.surface_distance(kv, kf, dev(bv), dev(bf), **kw)
    bare = metrics.surface_distance(dev(bv), dev(bf), dev(bv), dev(bf), **kw)
    dirty = metrics.surface_distance(dev(pv), dev(pf), dev(bv), dev(bf), **kw)
    assert clean == bare                                   # every figure, exactly
    print("gap %.4f: accuracy_max %.6g with the floater, %.6g without" % (gap, dirty['accuracy_max'], clean['accuracy_max']))
    assert gap > 1. and dirty['accuracy_max'] >= gap > 100 * bare['accuracy_max']
    assert dirty['precision_0.005'] < clean['precision_0.005']


def test_eval_fl_drops_floaters_and_reports_topology(tmp_path):
    import eval_fl
    from recmv import metrics
    from recmv.utils import read_obj, write_obj
    pv, pf, bv, bf, gap = floater_scene()
    (tmp_path / "pred").mkdir()
    (tmp_path / "gt").mkdir()
    write_obj(str(tmp_path / "pred" / "a.obj"), pv, pf)
    write_obj(str(tmp_path / "gt" / "a.obj"), bv, bf)
    common = ["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt"), "--samples", "20000"]
    out = tmp_path / "m.json"
    res = eval_fl.main(common + ["--drop-floaters", "0.01", "--topology", "--out", str(out)])
    gv, gf = read_obj(str(tmp_path / "gt" / "a.obj"))
    bare = metrics.surface_distance(gv.to(DEV), gf.to(DEV), gv.to(DEV), gf.to(DEV), samples=20000, seed=0)
    entry = res['pairs']['a']
    assert {k: entry[k] for k in bare} == bare             # the body's metrics, exactly
    assert set(entry) == set(bare) | {'floaters', 'topology_pred', 'topology_gt'}
    assert entry['floaters']['dropped_components'] == 1 and entry['floaters']['dropped_faces'] == 4
    assert entry['floaters']['components'] == 2 and entry['floaters']['faces'] == 1280
    assert entry['topology_pred'] == entry['topology_gt'] and entry['topology_gt']['watertight']
    assert entry['topology_gt']['components_vertex'] == 1 and entry['topology_gt']['components'][0]['genus'] == 0
    assert set(res['mean']) == set(bare) and res['mean'] == bare
    assert json.loads(out.read_text())['pairs']['a']['floaters'] == entry['floaters']
    plain = eval_fl.main(common)
    assert set(plain['pairs']['a']) == set(bare) and set(plain) == set(res)
    assert plain['pairs']['a']['accuracy_max'] >= gap - 1e-5                       # (the files hold six decimals)
    only = eval_fl.main(common + ["--topology"])
    assert only['pairs']['a']['topology_pred']['components_vertex'] == 2 and 'floaters' not in only['pairs']['a']


def test_clean_fl_reports_and_cleans(tmp_path, capsys):
    import clean_fl
    from recmv.utils import read_obj, write_obj
    pv, pf, bv, bf, _ = floater_scene()
    src = tmp_path / "in"
    src.mkdir()
    write_obj(str(src / "a.obj"), pv, pf)
    write_obj(str(src / "b.obj"), *TC.tube(17, 6))
    res = clean_fl.main(["--in", str(src), "--report-only"])
    printed = capsys.readouterr().out
    assert printed.count("boundary loops") == 2 and "a.obj: 1284 faces, 2 pieces" in printed and "b.obj" in printed
    assert set(res['files']) == {"a.obj", "b.obj"} and set(res['files']['a.obj']) == {"before"}
    assert res['files']['b.obj']['before']['boundary_loops'] == 2 and res['files']['b.obj']['before']['components_vertex'] == 1
    out = tmp_path / "out"
    res = clean_fl.main(["--in", str(src), "--out", str(out), "--min-area-frac", "0.01"])
    saved = json.loads((out / "topology.json").read_text())
    assert saved['files']['a.obj']['dropped'] == {'components': 1, 'faces': 4, 'area': res['files']['a.obj']['dropped']['area'],
                                                  'invalid_faces': 0, 'vertices': 4}
    assert saved['files']['a.obj']['before']['components_vertex'] == 2 and saved['files']['a.obj']['after']['components_vertex'] == 1
    assert saved['files']['a.obj']['after']['watertight'] and saved['files']['b.obj']['dropped']['components'] == 0
    kv, kf = read_obj(str(out / "a.obj"))
    gv, gf = read_obj(str(src / "a.obj"))
    assert torch.equal(kf, torch.from_numpy(bf)) and torch.equal(kv, gv[:len(bv)])
