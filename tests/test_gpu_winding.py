"""Generalized winding numbers on the GPU: recmv_winding_exact, the pyramid route (recmv_winding_tree_*), recmv.winding, the
winding sign of recmv.voxelize and the new flags of clean_fl.py and eval_fl.py.

Judges.
  exact           tests/winding_reference.py's float64 sum on every node of the small lattices, within TOL_EXACT (8 x the error of
                  the reference's own f32-term sum) where the node is at least 1e-3 box diagonals from the surface; integers on
                  the closed meshes.
  bits            the header's reduction: partial sums of chunks of recmv_winding_chunk_faces() faces, added in ascending order
                  and divided by 4 pi in float64 — recomputed here from the workspace, and each partial from a call on the chunk's
                  faces alone.  The same bits twice, for one query alone, for a slice and for the whole batch.
  tree            exact float64 within TOL_TREE[beta] (2 x the float64 pyramid rule's own error + TOL_EXACT); the flags of the
                  float64 judge wherever ||w64| - 1/2| exceeds that tolerance, at most 3 % of the nodes left out (pinned on the
                  CPU: tests/test_winding_cpu.py).
  voxelisation    the parity sign on a closed mesh, derived bounds on the capped hole, the union of two parity occupancies.
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
import winding_reference as WR  # noqa: E402

DEV = "cuda:0"
STEP = 0.06                                                # the small lattices' step


def _t(v, f):
    return torch.as_tensor(np.asarray(v), dtype=torch.float32).to(DEV).contiguous(), torch.as_tensor(np.asarray(f)).long().to(DEV).contiguous()


def _bits(x):
    return x.contiguous().view(torch.int64)


@pytest.fixture(scope="module")
def cases():
    """name -> (verts, faces on the device, queries [N,3] on the device, w64 [N], far [N]) — the reference is computed once."""
    out = {}
    for name in WR.NAMES:
        v, f, _ = WR.case(name)
        pts, w64, far = WR.case_reference(name)
        out[name] = (*_t(v, f), torch.from_numpy(np.array(pts)).to(DEV), w64, far)
    return out


# -------------------------------------------------------------------------------------------- 1. exact against float64
@pytest.mark.parametrize("name", WR.NAMES)
def test_exact_against_float64(cases, name):
    from recmv import winding
    v, f, pts, w64, far = cases[name]
    w = winding.winding_number(pts, v, f)
    assert w.dtype == torch.float64 and w.shape == (pts.shape[0],)
    w = w.cpu().numpy()
    err = np.abs(w - w64)
    print("%s: %d nodes, %d far enough, max |w - w64| = %.3g there (TOL_EXACT %.3g), %.3g anywhere" % (
        name, len(w), far.sum(), err[far].max(), WR.TOL_EXACT, err.max()))
    assert err[far].max() <= WR.TOL_EXACT
    if name in WR.CLOSED:
        assert np.abs(w - np.round(w))[far].max() <= WR.TOL_EXACT
    inside = winding.points_inside(pts, v, f).cpu().numpy()
    decided = WR.decided(w64, WR.TOL_EXACT)
    assert inside.dtype == bool and np.array_equal(inside[decided], WR.inside(w64)[decided])
    assert (~decided).mean() <= WR.UNDECIDED_CAP


def test_inward_orientation_special_queries_and_broken_faces(cases):
    from recmv import winding
    v, f, pts, w64, far = cases['body']
    flipped = winding.winding_number(pts, v, f.flip(1).contiguous()).cpu().numpy()
    assert np.abs(flipped + w64)[far].max() <= WR.TOL_EXACT and flipped.min() < -0.99
    assert torch.equal(winding.points_inside(pts, v, f.flip(1).contiguous()), winding.points_inside(pts, v, f))   # two-sided
    # queries that are not finite give NaN (outside); a query on a vertex is no error
    q = torch.cat([pts[:3], torch.tensor([[float("nan"), 0., 0.], [0., float("inf"), 0.], [0., 0., -float("inf")]], device=DEV), v[:2]])
    w = winding.winding_number(q, v, f)
    assert torch.equal(_bits(w[:3]), _bits(winding.winding_number(pts, v, f)[:3])) and bool(torch.isnan(w[3:6]).all())
    assert bool(torch.isfinite(w[6:]).all()) and not bool(winding.points_inside(q, v, f)[3:6].any())
    # faces with an index out of range contribute nothing, faces without area nothing; a corner that is not finite: NaN
    V = v.shape[0]
    extra = torch.tensor([[0, 1, V], [-1, 2, 3], [5, 5, 5], [7, 8, 8], [1 << 40, 0, 1]], device=DEV)
    want = winding.winding_number(pts[:500], v, f)
    for faces in (torch.cat([f, extra]), torch.cat([extra, f]), torch.cat([f[:640], extra, f[640:]])):
        assert torch.equal(_bits(winding.winding_number(pts[:500], v, faces)), _bits(want))
    bad = v.clone()
    bad[int(f[17, 1])] = float("inf")
    assert bool(torch.isnan(winding.winding_number(pts[:500], bad, f)).all())
    assert bool(torch.isnan(winding.winding_number(pts[:500], bad, f, method='tree')).all())
    # P = 0 and F = 0
    none_f = f[:0]
    assert winding.winding_number(pts[:0], v, f).shape == (0,) and winding.winding_number(pts[:0], v, f, method='tree').shape == (0,)
    for method in winding.METHODS:
        w = winding.winding_number(pts[:300], v, none_f, method=method)
        assert w.dtype == torch.float64 and bool((w == 0).all())


# ------------------------------------------------------------------------- 2. determinism and launch-shape independence
def test_exact_bits_do_not_depend_on_the_launch(cases):
    from recmv import winding
    v, f, pts, _, _ = cases['body']
    w = winding.winding_number(pts, v, f)
    assert torch.equal(_bits(w), _bits(winding.winding_number(pts, v, f)))
    assert torch.equal(_bits(winding.winding_number(pts[4321:4322], v, f)), _bits(w[4321:4322]))
    assert torch.equal(_bits(winding.winding_number(pts[5000:5100], v, f)), _bits(w[5000:5100]))
    # a mesh of more than two chunks: copies of the body side by side; the header's reduction from the workspace's partials,
    # and each partial from a call on that chunk's faces alone
    K = winding.chunk_faces()
    copies = 2 * K // f.shape[0] + 1
    vs = torch.cat([v + torch.tensor([0.05 * c, 0., 0.], device=DEV) for c in range(copies)])
    fs = torch.cat([f + c * v.shape[0] for c in range(copies)])
    assert fs.shape[0] > 2 * K
    q = pts[::7].contiguous()
    w, partial = winding.exact_partials(q, vs, fs)
    chunks = -(-fs.shape[0] // K)
    assert partial.shape == (chunks, q.shape[0]) and chunks == 3
    total = np.zeros(q.shape[0])
    for c in range(chunks):
        total = total + partial[c].cpu().numpy()
    assert np.array_equal((total / (4. * math.pi)).view(np.int64), w.cpu().numpy().view(np.int64))
    for c in range(chunks):
        alone, part = winding.exact_partials(q, vs, fs[c * K:(c + 1) * K].contiguous())
        assert torch.equal(_bits(part[0]), _bits(partial[c]))
        assert np.array_equal((part[0].cpu().numpy() / (4. * math.pi)).view(np.int64), alone.cpu().numpy().view(np.int64))
    assert torch.equal(_bits(winding.winding_number(q[100:101], vs, fs)), _bits(w[100:101]))
    old, winding.WORKSPACE_BYTES = winding.WORKSPACE_BYTES, 8 * chunks * 1024             # slices of 1024 queries: the same bits
    try:
        assert torch.equal(_bits(winding.winding_number(q, vs, fs)), _bits(w))
    finally:
        winding.WORKSPACE_BYTES = old


# ------------------------------------------------------------------------------- 3. cross-check with the parity test
@pytest.mark.parametrize("name", ["body", "torus"])
def test_winding_inside_equals_the_parity_inside_on_closed_meshes(cases, name):
    from recmv import metrics, winding
    v, f, pts, w64, _ = cases[name]
    parity = metrics.points_inside(pts, v, f)
    assert torch.equal(winding.points_inside(pts, v, f), parity) and int(parity.sum()) >= 2000
    assert torch.equal(metrics.points_inside(pts, v, f, rule='winding'), parity)
    pen_p, pen_w = metrics.penetration(pts, v, f), metrics.penetration(pts, v, f, rule='winding')
    assert pen_p['count'] == pen_w['count'] and torch.equal(pen_p['depth'], pen_w['depth'])


# ------------------------------------------------------------------------------------ 4. the tree against float64
@pytest.mark.parametrize("name", WR.NAMES)
def test_tree_against_float64(cases, name):
    from recmv import winding
    v, f, pts, w64, far = cases[name]
    tree = winding.WindingTree(v, f)
    origin, side = WR.cube(*WR.case(name)[:2])
    pyr = WR.Pyramid(*WR.case(name)[:2])
    assert tree.levels == pyr.levels and tree.origin == tuple(float(x) for x in origin) and tree.side == float(side)
    assert tree.n_faces == f.shape[0]
    for beta in (2., None):
        tol = WR.TOL_TREE[winding.DEFAULT_BETA if beta is None else beta]
        w = tree.query(pts, beta)
        assert w.dtype == torch.float64
        err = np.abs(w.cpu().numpy() - w64)
        decided = WR.decided(w64, tol)
        print("%s, beta %s, levels %d: max |w - w64| = %.4f on the far nodes (TOL_TREE %.4f), %.2f %% undecided" % (
            name, beta, tree.levels, err[far].max(), tol, 100. * (~decided).mean()))
        assert err[far].max() <= tol
        assert np.array_equal(winding.inside_from_winding(w).cpu().numpy()[decided], WR.inside(w64)[decided])
        assert (~decided).mean() <= WR.UNDECIDED_CAP
        # the same queries in another order, unsorted, alone: the same bits per query
        perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
        assert torch.equal(_bits(tree.query(pts[perm].contiguous(), beta)), _bits(w[perm]))
        assert torch.equal(_bits(tree.query(pts, beta, sort=False)), _bits(w))
        assert torch.equal(_bits(tree.query(pts[777:778], beta)), _bits(w[777:778]))
    assert torch.equal(_bits(winding.winding_number(pts, v, f, method='tree')), _bits(w))


# ------------------------------------------------------------------------------------------------- 5. tree edge cases
def test_tree_edge_cases_against_the_exact_kernel(cases):
    from recmv import winding
    v, f, pts, w64, far = cases['cap_z']
    exact = winding.winding_number(pts, v, f)
    tol = WR.TOL_TREE[WR.DEFAULT_BETA] + WR.TOL_EXACT
    far_t = torch.from_numpy(np.array(far)).to(DEV)
    for levels in (1, 7):
        tree = winding.WindingTree(v, f, levels=levels)
        assert tree.levels == levels and tree.nodes.shape == ((8 ** (levels + 1) - 1) // 7, 16)
        err = (tree.query(pts) - exact).abs()[far_t].max().item()
        print("levels %d: max |tree - exact| = %.4f" % (levels, err))
        assert err <= tol
    with pytest.raises(ValueError):
        winding.WindingTree(v, f, levels=8)
    with pytest.raises(ValueError):
        winding.WindingTree(v, f).query(pts, beta=0.5)
    # a mesh that fits in one finest cell: the body at 1 / 100 beside one far triangle that sets the cube
    small_v = torch.cat([v * 0.01, torch.tensor([[5., 5., 5.], [5.1, 5., 5.], [5., 5.1, 5.]], device=DEV)])
    small_f = torch.cat([f, torch.tensor([[0, 1, 2]], device=DEV) + v.shape[0]])
    tree = winding.WindingTree(small_v, small_f, levels=3)
    start = tree.cell_start
    assert int(((start[1:] - start[:-1]) > 0).sum()) == 2
    q = torch.cat([pts * 0.01, pts[::50] * 0.01 + 5.])
    away = torch.cat([far_t, torch.ones(q.shape[0] - pts.shape[0], dtype=torch.bool, device=DEV)])
    err = (tree.query(q) - winding.winding_number(q, small_v, small_f)).abs()
    assert err[away].max().item() <= tol
    # queries far outside the cube
    g = torch.Generator().manual_seed(5)
    out_q = ((torch.rand(2000, 3, generator=g) - 0.5) * 200.).to(DEV)
    out_q = out_q[out_q.abs().amax(1) > 2.]
    tree = winding.WindingTree(v, f)
    err = (tree.query(out_q) - winding.winding_number(out_q, v, f)).abs().max().item()
    print("queries outside the cube: max |tree - exact| = %.3g" % err)
    assert err <= tol
    # faces with invalid indices: the tree of the mesh without them, bit for bit
    extra = torch.tensor([[0, 1, v.shape[0]], [-1, 2, 3]], device=DEV)
    broken = winding.WindingTree(v, torch.cat([f[:300], extra, f[300:]]))
    assert broken.n_faces == f.shape[0] and broken.levels == tree.levels
    assert torch.equal(_bits(broken.query(pts)), _bits(tree.query(pts)))


# --------------------------------------------------------------------------------------------------- 6. voxelisation
def test_voxel_sign_winding_equals_parity_on_a_closed_mesh(cases):
    from recmv import voxelize
    v, f, pts, w64, _ = cases['body']
    lat = WR.case('body')[2]
    parity = voxelize.distance_field(v, f, lat)
    assert parity['sign'] == 'parity'
    for method, tol in (('tree', WR.TOL_TREE[WR.DEFAULT_BETA]), ('exact', WR.TOL_EXACT)):
        field = voxelize.distance_field(v, f, lat, sign='winding', winding_method=method)
        decided = torch.from_numpy(WR.decided(w64, tol)).to(DEV).view(lat.dims)
        assert field['sign'] == 'winding' and field['inside'].dtype == torch.bool
        assert torch.equal(field['inside'][decided], parity['inside'][decided]) and float((~decided).float().mean()) <= WR.UNDECIDED_CAP
        assert torch.equal(field['dist2'].view(torch.int32), parity['dist2'].view(torch.int32)) and torch.equal(field['face'], parity['face'])
        assert field['band_nodes'] == parity['band_nodes'] and field['open_columns'] == 0 and field['sign_conflicts'] == 0
        band = torch.tensor(field['band'], dtype=torch.float32, device=DEV)
        want = torch.where(field['inside'], -1., 1.) * torch.minimum(field['dist2'].sqrt(), band)
        assert torch.equal(field['sdf'], want) and field['sdf'].dtype == torch.float32
    assert torch.equal(voxelize.distance_field(v, f, lat, sign='winding')['inside'],
                       voxelize.distance_field(v, f, lat, sign='winding', winding_method=voxelize.DEFAULT_WINDING_METHOD)['inside'])


def test_voxel_remesh_of_a_holed_body_caps_the_hole(cases):
    from recmv import iso_remesh, topology, voxelize
    v, f, _, _, _ = cases['cap_z']
    parity = voxelize.remesh(v, f, step=STEP)
    assert parity[2]['open_columns'] > 0 or parity[2]['sign_conflicts'] > 0        # the gap: a lost parity, the existing behaviour
    ov, of, info = voxelize.remesh(v, f, step=STEP, sign='winding')
    rep = topology.report(ov, of)
    print("holed body: %d -> %d faces, open_columns %d, sign_conflicts %d, watertight %s, %d piece(s)" % (
        info['faces_in'], info['faces_out'], info['open_columns'], info['sign_conflicts'], rep['watertight'], rep['components_vertex']))
    assert info['sign'] == 'winding' and rep['watertight'] and rep['components_vertex'] == 1 and rep['boundary_edges'] == 0
    # a vertex lies on a lattice edge whose ends differ in sign: either the surface crosses that edge (within one step of the
    # input) or the ends are clamped nodes on either side of w = 1/2, which happens only where the cap is missing
    step = info['lattice'].step
    _, _, d2 = iso_remesh.closest_point(ov.contiguous(), v, f)
    near = d2.sqrt() <= step * (1. + 1e-5)
    in_cap = ov[:, 2] >= WR.CAP - step
    assert bool((near | in_cap).all()) and int((~near).sum()) > 0 and int(near.sum()) > 0.8 * ov.shape[0]
    exact = voxelize.remesh(v, f, step=STEP, sign='winding', winding_method='exact')
    assert topology.report(exact[0], exact[1])['watertight']


def test_occupancy_of_two_overlapping_bodies_is_their_union(cases):
    from recmv import voxelize
    v, f, pts, w64, _ = cases['two_bodies']
    lat = WR.case('two_bodies')[2]
    n, F = v.shape[0] // 2, f.shape[0] // 2
    a = voxelize.occupancy(v[:n].contiguous(), f[:F].contiguous(), lat)
    b = voxelize.occupancy(v[n:].contiguous(), (f[F:] - n).contiguous(), lat)
    both = voxelize.occupancy(v, f, lat, sign='winding')
    decided = torch.from_numpy(WR.decided(w64, WR.TOL_TREE[WR.DEFAULT_BETA])).to(DEV).view(lat.dims)
    assert torch.equal(both[decided], (a | b)[decided]) and float((~decided).float().mean()) <= WR.UNDECIDED_CAP
    overlap = a & b
    assert int(overlap.sum()) > 500 and not bool(voxelize.occupancy(v, f, lat)[overlap].any())             # parity: the XOR
    assert bool(both[overlap & decided].all())
    vol = voxelize.volume(v, f, lat, sign='winding')
    assert vol == int(both.sum()) * lat.step ** 3
    iou = voxelize.volume_iou(v[:n].contiguous(), f[:F].contiguous(), v, f, step=STEP, sign='winding')
    assert iou['sign'] == 'winding' and iou['intersection'] <= iou['union'] and 0.5 < iou['iou'] < 1.


# ------------------------------------------------------------------------------------------------------- 7. commands
def _write(path, v, f):
    from recmv.utils import write_obj
    write_obj(str(path), torch.as_tensor(np.asarray(v)).float(), torch.as_tensor(np.asarray(f)).long())


def test_clean_fl_voxel_sign_winding_takes_a_holed_body(tmp_path, capsys):
    import clean_fl
    from recmv import topology
    from recmv.utils import read_obj
    v, f, _ = WR.case('cap_z')
    _write(tmp_path / "holed.obj", v, f)
    with pytest.raises(SystemExit):                        # the parity sign refuses it
        clean_fl.main(["--in", str(tmp_path / "holed.obj"), "--out", str(tmp_path / "p"), "--voxel-remesh", "0.06"])
    capsys.readouterr()
    out = clean_fl.main(["--in", str(tmp_path / "holed.obj"), "--out", str(tmp_path / "w"), "--voxel-remesh", "0.06",
                         "--voxel-sign", "winding"])
    vox = json.load(open(tmp_path / "w" / "topology.json"))['files']['holed.obj']['voxel']
    assert vox == out['files']['holed.obj']['voxel'] and vox['sign'] == 'winding' and vox['mode'] == 'remesh'
    assert vox['open_columns'] > 0 or vox['sign_conflicts'] > 0                     # information, not a refusal
    ov, of = read_obj(str(tmp_path / "w" / "holed.obj"))
    assert of.shape[0] == vox['faces_after'] and topology.report(ov.to(DEV), of.to(DEV))['watertight']
    assert out['files']['holed.obj']['after']['watertight'] and not out['files']['holed.obj']['before']['watertight']


def test_eval_fl_inside_rule_winding_takes_a_holed_body(tmp_path):
    import eval_fl
    from recmv.utils import read_obj
    bv, bf, _ = WR.case('body')
    hv, hf, _ = WR.case('cap_z')
    pred = bv.copy()
    pred[:, 2] -= np.float32(0.3)                          # a copy of the body 0.3 lower: its top lies under the hole
    _write(tmp_path / "pred.obj", pred, bf)
    _write(tmp_path / "body.obj", bv, bf)
    _write(tmp_path / "holed.obj", hv, hf)
    base = ["--pred", str(tmp_path / "pred.obj"), "--gt", str(tmp_path / "pred.obj"), "--samples", "2000", "--intersections", "--penetration"]
    closed = eval_fl.main(base + ["--body", str(tmp_path / "body.obj")])['pairs']['pred']
    holed = eval_fl.main(base + ["--body", str(tmp_path / "holed.obj"), "--inside-rule", "winding"])['pairs']['pred']
    pv, _ = read_obj(str(tmp_path / "pred.obj"))           # what the command read
    w64 = WR.winding(pv.numpy(), hv, hf)
    undecided = int((~WR.decided(w64, WR.DECISION_MARGIN)).sum())
    print("inside the closed body (parity) %d, inside the holed body (winding) %d, %d of %d vertices undecided" % (
        closed['body_inside_vertices'], holed['body_inside_vertices'], undecided, len(w64)))
    assert closed['body_inside_vertices'] > 50 and undecided <= WR.UNDECIDED_CAP * len(w64)
    assert abs(holed['body_inside_vertices'] - closed['body_inside_vertices']) <= undecided
    assert holed['body_inside'] == {'rule': 'winding'} and 'body_inside' not in closed
