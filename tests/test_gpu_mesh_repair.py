"""Mesh repair on the GPU: the pair search of csrc/point_grid.hip against the O(V^2) loop of tests/mesh_repair_reference.py (the
pair SET must be equal, the array the same on a second run) on the shapes where it can go wrong, the five stages of
recmv.repair against the numpy restatement on every case of tests/mesh_repair_cases.py (faces, maps and counts equal, vertices
bit-equal), the properties of the result read through recmv.topology.report, and simplify, clean_fl.py and eval_fl.py on
repaired meshes."""
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
import mesh_repair_cases as RC  # noqa: E402
import mesh_repair_reference as RR  # noqa: E402
import mesh_topology_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLOUDS = RC.clouds()
MESHES = RC.meshes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def bits(v):
    return np.ascontiguousarray(host(v), np.float32).view(np.uint32)


def same_info(got, want):
    """Every entry of the reference's info is in the module's, equal: tensors as arrays, numbers as numbers, dicts likewise."""
    for k, w in want.items():
        g = got[k]
        if isinstance(w, dict):
            same_info(g, w)
        elif isinstance(w, np.ndarray):
            assert np.array_equal(host(g), w), k
        else:
            assert g == w and type(g) in (int, float, bool), (k, g, w)


def same_mesh(got, want):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[0].is_cuda and got[1].is_cuda
    assert np.array_equal(host(got[1]), want[1])
    assert bits(got[0]).shape == bits(want[0]).shape and np.array_equal(bits(got[0]), bits(want[0]))
    same_info(got[2], want[2])


@functools.lru_cache(maxsize=None)
def reference_pairs(name):
    v, eps, _ = CLOUDS[name]
    return RR.points_within(v, eps)


@functools.lru_cache(maxsize=None)
def reference_repair(name):
    v, f, eps, _ = MESHES[name]
    return RR.repair(v, f, weld_eps=eps)


@functools.lru_cache(maxsize=None)
def gpu_repair(name):
    from recmv import repair
    v, f, eps, _ = MESHES[name]
    return repair.repair(dev(v), dev(f), weld_eps=eps)


# ---- the pair search --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CLOUDS))
def test_pairs_equal_the_plain_loop_and_come_out_the_same_twice(name):
    from recmv import repair
    v, eps, max_pairs = CLOUDS[name]
    want, nonfinite = reference_pairs(name)
    got, info = repair.points_within(dev(v), eps, max_pairs=max_pairs, return_info=True)
    again = repair.points_within(dev(v), eps, max_pairs=max_pairs)
    assert got.dtype == torch.int64 and got.is_cuda and got.shape == (len(want), 2)
    assert torch.equal(got, again)
    g = host(got)
    assert (g[:, 0] < g[:, 1]).all() and (np.diff(g[:, 0]) >= 0).all()
    assert np.array_equal(g[np.lexsort((g[:, 1], g[:, 0]))], want)
    assert info['pairs'] == len(want) and info['nonfinite_vertices'] == nonfinite
    if info['dims'] is not None:
        assert info['dims'][0] * info['dims'][1] * info['dims'][2] <= max(4 * (len(v) - nonfinite), 64) and info['cell'] >= eps


def test_the_written_out_counts():
    assert len(reference_pairs('300 coincident')[0]) == 44850
    for name in ('lattice', 'lattice negative', 'lattice straddling 0'):
        assert len(reference_pairs(name)[0]) == 3 * 6 * 6 * 5      # the axis neighbours at exactly d2 == eps^2, no diagonal
    assert len(reference_pairs('signed zeros')[0]) == 4
    assert len(reference_pairs('eps beyond the box')[0]) == 64 * 63 // 2
    assert reference_pairs('nan and inf')[1] == 4
    both = reference_pairs('two clusters 1e6 apart')[0]
    assert len(both) > 0 and ((both[:, 0] < 30) == (both[:, 1] < 30)).all()


def test_the_default_max_pairs_refuses_the_coincident_cloud():
    from recmv import repair
    v = CLOUDS['300 coincident'][0]
    with pytest.raises(ValueError, match="too large for this mesh"):
        repair.points_within(dev(v), 0.)
    with pytest.raises(ValueError, match="too large for this mesh"):
        repair.points_within(dev(v), 0., max_pairs=44849)
    assert repair.points_within(dev(v), 0., max_pairs=44850).shape == (44850, 2)


# ---- the stages against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
def test_weld_equals_the_reference(name):
    from recmv import repair
    v, f, eps, _ = MESHES[name]
    for e in {0., RC.WELD_EPS, eps or 0.}:
        same_mesh(repair.weld(dev(v), dev(f), e), RR.weld(v, f, e))


@pytest.mark.parametrize("name", sorted(MESHES))
def test_drop_degenerate_equals_the_reference(name):
    from recmv import repair
    v, f = MESHES[name][:2]
    same_mesh(repair.drop_degenerate(dev(v), dev(f)), RR.drop_degenerate(v, f))


@pytest.mark.parametrize("name", sorted(MESHES))
def test_split_nonmanifold_equals_the_reference(name):
    from recmv import repair
    v, f = MESHES[name][:2]
    if name == 'defects':
        with pytest.raises(ValueError, match="invalid faces"):
            repair.split_nonmanifold(dev(v), dev(f))
        v, f, _ = RR.drop_degenerate(v, f)
    same_mesh(repair.split_nonmanifold(dev(v), dev(f)), RR.split_nonmanifold(v, f))


@pytest.mark.parametrize("name", sorted(MESHES))
def test_orient_equals_the_reference(name):
    from recmv import repair
    v, f = MESHES[name][:2]
    same_mesh(repair.orient(dev(v), dev(f)), RR.orient(v, f))


@pytest.mark.parametrize("name", sorted(MESHES))
def test_repair_equals_the_reference(name):
    same_mesh(gpu_repair(name), reference_repair(name))


def test_welding_a_chain_shows_in_the_radius():
    """Points 0.6 apart along a line with eps = 1: every neighbour pair and no other joins, the chain collapses into vertex 0,
    and cluster_radius_max is the chain's length — exactly, on both sides."""
    from recmv import repair
    v = np.zeros((9, 3), np.float32)
    v[:, 0] = np.arange(9, dtype=np.float32) * np.float32(0.6)
    f = np.array([[0, 4, 8]], np.int64)
    got, want = repair.weld(dev(v), dev(f), 1.), RR.weld(v, f, 1.)
    same_mesh(got, want)
    assert got[2]['clusters'] == 1 and got[2]['merged_vertices'] == 8 and got[2]['cluster_radius_max'] == float(v[8, 0]) > 1.
    assert host(got[1]).tolist() == [[0, 0, 0]]


# ---- the properties of the result -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
def test_repair_leaves_no_defect(name):
    from recmv import topology
    v, f, info = gpu_repair(name)
    rep = topology.report(v, f)
    for key in ('invalid_faces', 'zero_area_faces', 'duplicate_faces', 'nonmanifold_edges', 'boundary_pinch_vertices',
                'unreferenced_vertices', 'nonfinite_faces'):
        assert rep[key] == 0, key
    if MESHES[name][3]:
        assert rep['orientation_conflicts'] == 0 and info['orient']['non_orientable_pieces'] == 0
    else:
        assert rep['orientation_conflicts'] > 0 and info['orient']['non_orientable_pieces'] == 1
    assert np.array_equal(bits(v), bits(MESHES[name][0][host(info['origin'])]))       # rows are copies, bit for bit


@pytest.mark.parametrize("name", ['soup', 'jittered_soup'])
def test_the_welded_soup_is_the_icosphere(name):
    from recmv import topology
    ico = RC.icosphere()
    v, f, info = gpu_repair(name)
    assert np.array_equal(host(f), ico[1]) and topology.report(v, f)['watertight']
    assert topology.report(dev(MESHES[name][0]), dev(MESHES[name][1]))['components_vertex'] == 320
    assert info['weld']['merged_vertices'] == 960 - 162 and info['weld']['cluster_radius_max'] <= MESHES[name][2]
    if name == 'soup':
        assert np.array_equal(bits(v), bits(ico[0]))


@pytest.mark.parametrize("name", sorted(MESHES))
def test_repair_is_idempotent(name):
    from recmv import repair
    v, f, _ = gpu_repair(name)
    v2, f2, info = repair.repair(v, f, weld_eps=MESHES[name][2])
    assert torch.equal(f2, f) and np.array_equal(bits(v2), bits(v))
    assert info['split_nonmanifold']['added_vertices'] == 0 or MESHES[name][2] is not None
    assert info['orient']['flipped_faces'] == 0 and len(info['kept_faces']) == f.shape[0]


def test_the_moebius_strip_keeps_its_conflicts():
    from recmv import topology
    v, f = MESHES['moebius'][:2]
    before = topology.report(dev(v), dev(f))
    rv, rf, info = gpu_repair('moebius')
    assert np.array_equal(host(rf), f) and info['orient']['flipped_faces'] == 0 and info['orient']['non_orientable_pieces'] == 1
    assert topology.report(rv, rf)['orientation_conflicts'] == before['orientation_conflicts'] == info['orient']['conflicts_before'] > 0


def test_the_tie_flips_the_side_without_the_lowest_face():
    flipped = host(gpu_repair('tied_strip')[2]['orient']['flipped'])
    assert flipped.sum() == 6 and not flipped[0] and flipped[1::2].all()


# ---- integration ------------------------------------------------------------------------------------------------------------------
def test_simplify_refuses_the_hinge_and_takes_its_repair():
    from recmv import simplify, topology
    v, f = TC.hinged_tetrahedra()
    with pytest.raises(ValueError, match="edge-manifold"):
        simplify.simplify(dev(v), dev(f), target_faces=6)
    rv, rf, _ = gpu_repair('hinged_tetrahedra')
    rep = topology.report(rv, rf)
    assert rep['components_vertex'] == 2 and rep['watertight']
    nv, nf, info = simplify.simplify(rv, rf, target_faces=6)
    assert nf.shape[0] <= 8 and torch.isfinite(nv).all()


def test_clean_fl_repairs_first_of_all(tmp_path, capsys):
    import clean_fl
    from recmv.utils import read_obj, write_obj
    src = tmp_path / "in"
    src.mkdir()
    cases = {"soup.obj": 'jittered_soup', "hinge.obj": 'hinged_tetrahedra', "third.obj": 'every_third_flipped'}
    for file, name in cases.items():
        write_obj(str(src / file), torch.from_numpy(MESHES[name][0]), torch.from_numpy(MESHES[name][1]))
    out = clean_fl.main(["--in", str(src), "--out", str(tmp_path / "out"), "--repair", "--weld-eps", str(RC.WELD_EPS)])
    printed = capsys.readouterr().out
    assert out["repair"] is True and out["weld_eps"] == RC.WELD_EPS
    assert json.loads((tmp_path / "out" / "topology.json").read_text()) == json.loads(json.dumps(out))
    for file in cases:
        e = out["files"][file]
        assert file + ": repaired, " in printed and json.dumps(e["repair"])
        assert e["after"]["nonmanifold_edges"] == e["after"]["orientation_conflicts"] == e["after"]["boundary_pinch_vertices"] == 0
        nv, nf = read_obj(str(tmp_path / "out" / file))
        assert nf.shape[0] == e["after"]["faces"] and nv.shape[0] == e["after"]["vertices"]
    soup, hinge, third = (out["files"][k] for k in cases)
    assert soup["before"]["components_vertex"] == 320 and soup["after"]["components_vertex"] == 1 and soup["after"]["watertight"]
    assert soup["repair"]["weld"]["merged_vertices"] == 960 - 162 and soup["after"]["vertices"] == 162
    assert torch.equal(read_obj(str(tmp_path / "out" / "soup.obj"))[1], torch.from_numpy(RC.icosphere()[1]))
    assert hinge["before"]["nonmanifold_edges"] == 1 and hinge["repair"]["split_nonmanifold"]["added_vertices"] == 2
    assert hinge["after"]["components_vertex"] == 2 and hinge["after"]["watertight"]
    assert third["before"]["orientation_conflicts"] > 0 and third["repair"]["orient"]["flipped_faces"] == 107
    plain = clean_fl.main(["--in", str(src), "--out", str(tmp_path / "plain")])
    capsys.readouterr()
    assert "repair" not in plain and "weld_eps" not in plain and "repair" not in plain["files"]["hinge.obj"]
    assert plain["files"]["hinge.obj"]["after"]["nonmanifold_edges"] == 1


def test_eval_fl_repairs_both_meshes_before_anything_else(tmp_path, capsys):
    import eval_fl
    from recmv import topology
    from recmv.utils import read_obj, write_obj
    ico = RC.icosphere()
    write_obj(str(tmp_path / "pred.obj"), torch.from_numpy(MESHES['soup'][0]), torch.from_numpy(MESHES['soup'][1]))
    write_obj(str(tmp_path / "gt.obj"), torch.from_numpy(ico[0]), torch.from_numpy(ico[1]))
    args = ["--pred", str(tmp_path / "pred.obj"), "--gt", str(tmp_path / "gt.obj"), "--samples", "2000", "--topology"]
    res = eval_fl.main(args + ["--repair", "--weld-eps", "0", "--out", str(tmp_path / "m.json")])
    capsys.readouterr()
    e = res["pairs"]["pred"]
    want = topology.report(*(x.to(DEV) for x in read_obj(str(tmp_path / "gt.obj"))))
    assert want["watertight"] and want["faces"] == 320
    assert e["topology_pred"] == want and e["topology_gt"] == want
    assert e["repair_pred"]["weld"]["merged_vertices"] == 960 - 162 and e["repair_gt"]["weld"]["merged_vertices"] == 0
    assert res["repair"] == {"weld_eps": 0.} and e["chamfer_l1"] < 1e-6
    assert json.loads((tmp_path / "m.json").read_text()) == json.loads(json.dumps(res))
    plain = eval_fl.main(args)
    capsys.readouterr()
    assert "repair" not in plain and "repair_pred" not in plain["pairs"]["pred"]
    assert plain["pairs"]["pred"]["topology_pred"]["components_vertex"] == 320
