"""Hole filling on the GPU: recmv_hole_triangulate on both routes against the numpy restatement bit for bit, recmv.holes.fill
against the restatement's fill, the properties of the closed results, refinement and fairing, and the commands."""
import json
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import hole_fill_cases as HC  # noqa: E402
import hole_fill_reference as HR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOOPS = HC.loop_cases()
MESHES = HC.mesh_cases()
NAMES = list(LOOPS)
SMALL = [k for k in NAMES if len(LOOPS[k]) <= HC.LDS_MAX]


@lru_cache(maxsize=None)
def packed(names):
    """The loops `names` (or the 200 small ones) in one vertex table, with the restatement's answer."""
    sets = HC.many_small_loops() if names == 'many' else [LOOPS[k] for k in names]
    verts, lv, lo = HC.pack(sets)
    faces, weight = HR.triangulate_loops(verts, lv, lo)
    return verts, lv, lo, faces, weight


def run(names, route, offsets_on_device=True):
    from recmv import holes
    verts, lv, lo, faces, weight = packed(names)
    args = (torch.from_numpy(verts).to(DEV), torch.from_numpy(lv).to(DEV),
            torch.from_numpy(lo).to(DEV) if offsets_on_device else torch.from_numpy(lo))
    got_f, got_w = holes.triangulate_loops(*args, route=route)
    again_f, again_w = holes.triangulate_loops(*args, route=route)
    assert got_f.is_cuda and got_w.is_cuda and got_f.dtype == torch.int64 and got_w.dtype == torch.float64
    assert torch.equal(got_f, again_f) and torch.equal(got_w.view(torch.int64), again_w.view(torch.int64))      # the same bits
    assert got_f.shape == faces.shape
    assert np.array_equal(got_f.cpu().numpy(), faces)
    assert np.array_equal(got_w.cpu().numpy().view(np.uint64), weight.view(np.uint64))
    return got_f, got_w


@pytest.mark.parametrize("route", ["auto", "lds", "global"])
@pytest.mark.parametrize("name", NAMES)
def test_one_loop_against_the_restatement(name, route):
    if route == "lds" and name not in SMALL:
        from recmv import holes
        verts, lv, lo, _, _ = packed((name,))
        with pytest.raises(ValueError, match="lds route"):
            holes.triangulate_loops(torch.from_numpy(verts).to(DEV), torch.from_numpy(lv).to(DEV), torch.from_numpy(lo), route="lds")
        return
    run((name,), route)


@pytest.mark.parametrize("route", ["auto", "lds", "global"])
def test_mixed_sizes_in_one_call(route):
    names = tuple(SMALL if route == "lds" else NAMES)
    _, w = run(names, route, offsets_on_device=(route != "global"))
    w = w.cpu().numpy()
    nan = names.index('n10_nan')
    assert w[nan] == np.inf and np.isfinite(np.delete(w, nan)).all()                         # the other loops are untouched


@pytest.mark.parametrize("route", ["auto", "lds", "global"])
def test_two_hundred_small_loops(route):
    f, w = run('many', route)
    assert w.shape[0] == 200 and bool(torch.isfinite(w).all())


def test_an_id_outside_the_vertex_table_reads_as_nan():
    from recmv import holes
    verts, lv, lo, _, _ = packed(('n7', 'n5'))
    lv = lv.copy()
    lv[2] = len(verts) + 5
    f, w = holes.triangulate_loops(torch.from_numpy(verts).to(DEV), torch.from_numpy(lv).to(DEV), torch.from_numpy(lo))
    assert w[0].item() == np.inf and w[1].item() == packed(('n7', 'n5'))[4][1]


# ------------------------------------------------------------------------------------------------- fill
def _fill(name, **extra):
    from recmv import holes
    v, f, kw = MESHES[name]
    return holes.fill(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), **dict(kw, **extra))


@lru_cache(maxsize=None)
def reference_fill(name):
    v, f, kw = MESHES[name]
    return HR.fill(v, f, **kw)


@pytest.mark.parametrize("route", ["auto", "global"])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_fill_against_the_restatement(name, route):
    from recmv import holes
    v, f, _ = MESHES[name]
    rv, rf, rinfo = reference_fill(name)
    ov, of, info = _fill(name, route=route)
    assert np.array_equal(of.cpu().numpy(), rf)
    assert np.array_equal(ov.cpu().numpy().view(np.uint32), rv.view(np.uint32))
    assert info == rinfo
    assert json.loads(json.dumps(holes.info_json(info))) == rinfo
    if info['filled'] == 0:                                                                  # the input, the same shapes and bits
        assert ov.shape == (len(v), 3) and of.shape == (len(f), 3)


def test_fill_refuses_meshes_that_need_a_repair():
    from recmv import holes
    v = torch.zeros((5, 3), device=DEV)
    fan = torch.tensor([[0, 1, 2], [0, 1, 3], [0, 1, 4]], device=DEV)                          # three faces on one edge
    flipped = torch.tensor([[0, 1, 2], [0, 1, 3]], device=DEV)                                 # both run 0 -> 1
    for faces in (fan, flipped):
        with pytest.raises(ValueError, match="repair.repair"):
            holes.fill(v, faces)


def signed_volume(v, f):
    p = np.asarray(v, np.float64)[np.asarray(f)]
    return float(np.einsum('ij,ij->i', p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.)


CLOSED = {'icosphere_one_hole': HC.icosphere(1), 'icosphere_two_holes': HC.icosphere(1), 'tetrahedron_minus_one': HC.tetrahedron(),
          'cylinder_keep_0': None}


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_filled_meshes_are_closed_and_oriented(name):
    from recmv import repair, topology
    ov, of, info = _fill(name)
    rep = topology.report(ov, of)
    assert rep['boundary_loops'] == 0 and rep['watertight'] and rep['nonmanifold_edges'] == 0
    assert rep['orientation_conflicts'] == 0
    assert repair.orient(ov, of)[2]['flipped_faces'] == 0
    if CLOSED[name] is not None:                                                             # as before the faces were removed
        wv, wf = CLOSED[name]
        whole = topology.report(torch.from_numpy(wv).to(DEV), torch.from_numpy(wf).to(DEV))
        assert rep['euler_characteristic'] == whole['euler_characteristic'] == 2
        assert signed_volume(ov.cpu(), of.cpu()) * signed_volume(wv, wf) > 0
    else:
        assert rep['euler_characteristic'] == 2 and signed_volume(ov.cpu(), of.cpu()) > 0    # the cylinder faces outwards


# ------------------------------------------------------------------------------------------------- refine and fair
@pytest.fixture(scope="module", params=["hole12", "cylinder"])
def refined(request):
    from recmv import holes
    v, f = HC.icosphere_hole12() if request.param == "hole12" else HC.cylinder()
    v, f = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    plain = holes.fill(v, f)
    fine = holes.fill(v, f, refine=True)
    fair = holes.fill(v, f, refine=True, fair_iterations=5)
    return v, f, plain, fine, fair


def test_refine_keeps_the_mesh_closed_and_the_borders(refined):
    from recmv import topology
    from recmv.connectivity import EdgeTable
    v, f, plain, (ov, of, info), _ = refined
    V, F = v.shape[0], f.shape[0]
    assert not info['refine_capped'] and 0 < info['refine_rounds']
    rep = topology.report(ov, of)
    assert rep['watertight'] and rep['nonmanifold_edges'] == 0 and rep['boundary_loops'] == 0 and rep['orientation_conflicts'] == 0
    assert torch.equal(ov[:V].view(torch.int32), v.view(torch.int32)) and torch.equal(of[:F], f)
    assert sum(info['verts_added']) == ov.shape[0] - V > 0 and sum(info['faces_added']) == of.shape[0] - F
    at_v = V
    for l in range(info['loops']):                                                           # loop by loop
        start, count = info['face_start'][l], info['faces_added'][l]
        patch = of[start:start + count]
        table = EdgeTable(patch, ov.shape[0])
        border = table.edges[table.count == 1]
        first = plain[1][plain[2]['face_start'][l]:plain[2]['face_start'][l] + plain[2]['faces_added'][l]]
        t0 = EdgeTable(first, V)
        assert torch.equal(border, t0.edges[t0.count == 1])                                  # every border edge is still one
        new = patch[patch >= V]
        assert int(new.min()) == at_v and int(new.max()) == at_v + info['verts_added'][l] - 1
        at_v += info['verts_added'][l]
        inner = table.edges[table.count == 2]
        length = (ov[inner[:, 0]].double() - ov[inner[:, 1]].double()).norm(dim=1)
        lbar = info['perimeter'][l] / info['edges'][l]
        assert float(length.max()) <= 4. / 3. * lbar * (1 + 1e-12)


def test_fairing_moves_only_the_new_vertices(refined):
    from recmv import holes, topology
    v, f, _, (ov, of, info), (fv, ff, finfo) = refined
    V = v.shape[0]
    assert torch.equal(ff, of) and finfo == info
    assert torch.equal(fv[:V].view(torch.int32), v.view(torch.int32))
    assert not torch.equal(fv[V:], ov[V:]) and bool(torch.isfinite(fv).all())
    assert topology.report(fv, ff)['watertight']
    with pytest.raises(ValueError, match="refine"):
        holes.fill(v, f, fair_iterations=3)


# ------------------------------------------------------------------------------------------------- end to end
def holed_sphere_facing_x():
    """Level 2 without the faces at the vertices with x > 0.7: one hole of 18 edges and radius 0.8, far wider than the band,
    that faces along +x.  The lattice columns run along x: those through the hole meet the wall once and end inside."""
    v, f = HC.icosphere(2)
    return v, HC.without_vertices(f, np.nonzero(v[:, 0] > 0.7)[0].tolist())


def test_voxel_remesh_needs_the_fill():
    from recmv import holes, voxelize
    v, f = (torch.from_numpy(x).to(DEV) for x in holed_sphere_facing_x())
    before = voxelize.remesh(v, f, step=0.08)[2]
    ov, of, info = holes.fill(v, f)
    after = voxelize.remesh(ov, of, step=0.08)[2]
    print("open_columns %d -> %d" % (before['open_columns'], after['open_columns']))
    assert info['filled'] == 1 and before['open_columns'] > 0 and after['open_columns'] == 0 and after['sign_conflicts'] == 0


def _write(path, v, f):
    from recmv.utils import write_obj
    write_obj(str(path), torch.as_tensor(np.asarray(v)).float(), torch.as_tensor(np.asarray(f)).long())


def test_clean_fl_fill_holes_then_voxel_remesh(tmp_path, capsys):
    import clean_fl
    _write(tmp_path / "holed.obj", *holed_sphere_facing_x())
    with pytest.raises(SystemExit):
        clean_fl.main(["--in", str(tmp_path / "holed.obj"), "--out", str(tmp_path / "a"), "--voxel-remesh", "0.08"])
    assert "not closed" in capsys.readouterr().err
    out = clean_fl.main(["--in", str(tmp_path / "holed.obj"), "--out", str(tmp_path / "b"), "--fill-holes", "--voxel-remesh", "0.08"])
    saved = json.loads((tmp_path / "b" / "topology.json").read_text())
    entry = saved['files']['holed.obj']
    assert entry['holes'] == out['files']['holed.obj']['holes'] and entry['holes']['filled'] == 1 == entry['holes']['loops']
    assert entry['holes']['status'] == ['filled'] and saved['fill_holes'] is True
    assert entry['voxel']['open_columns'] == 0 and entry['before']['boundary_loops'] == 1 and entry['after']['watertight']
    assert (tmp_path / "b" / "holed.obj").exists()
    assert "1 boundary loops, 1 filled" in capsys.readouterr().out
    plain = clean_fl.main(["--in", str(tmp_path / "holed.obj"), "--out", str(tmp_path / "c")])
    assert 'holes' not in plain['files']['holed.obj'] and 'fill_holes' not in plain
    kept = clean_fl.main(["--in", str(tmp_path / "holed.obj"), "--out", str(tmp_path / "d"), "--fill-holes", "--fill-keep-largest",
                          "1", "--fill-refine"])
    assert kept['files']['holed.obj']['holes']['status'] == ['keep_largest']
    assert kept['files']['holed.obj']['after']['boundary_loops'] == 1


def test_eval_fl_volume_with_fill_holes(tmp_path):
    import eval_fl
    v, f = holed_sphere_facing_x()
    _write(tmp_path / "pred.obj", v, f)
    _write(tmp_path / "gt.obj", *HC.icosphere(2))
    argv = ["--pred", str(tmp_path / "pred.obj"), "--gt", str(tmp_path / "gt.obj"), "--samples", "2000", "--volume",
            "--volume-step", "0.08"]
    res = eval_fl.main(argv)['pairs']['pred']
    assert res['volume_iou'] is None and 'holes_pred' not in res
    res = eval_fl.main(argv + ["--fill-holes", "--fill-max-edges", "18"])
    got = res['pairs']['pred']
    assert got['holes_pred']['filled'] == 1 and got['holes_gt']['loops'] == 0
    assert got['volume_iou'] is not None and 0.8 < got['volume_iou'] < 1. and got['volume_pred'] > 0
    assert res['fill_holes'] == {'max_edges': 18, 'keep_largest': None}
