"""Mesh voxelisation on the GPU: recmv_voxel_band_distance and recmv_voxel_sign_fill (recmv.voxelize.distance_field), the voxel
remesh, solidify, the volumes, and the new flags of clean_fl.py and eval_fl.py.

Judges.
  band distance   the brute force iso_remesh.closest_point on ALL nodes, bit for bit: where its dist2 <= band^2 (the product
                  formed once in f32) dist2 and face are equal, elsewhere dist2 = +inf and face = -1.  Both run closest_tri.h's
                  closest_st on load_tri's corners, and the scatter reaches every node of the band (csrc/mesh_voxelize.hip).
  sign, primary   metrics.points_inside on ALL nodes, an exact bool comparison: the band nodes take its answer, and the column
                  rule carries it on (in float64 the rule reproduces the per-node test on both meshes:
                  tests/test_voxelize_cpu.py).
  sign, float64   tests/voxelize_reference.py on 1 500 drawn nodes, where it decides; at most 3 % may be undecided.
  sdf             where(inside, -1, 1) * minimum(sqrt(dist2), band) formed with torch from the pinned outputs, within 1 ulp of
                  f32 (the square root's rounding and nothing else); exactly +-band outside the band.
  remesh          derived bounds.  A marching-cubes vertex lies on a lattice edge whose ends have opposite signs, so the surface
                  crosses that edge: every output vertex is within one step of the input.  For a body with no feature thinner
                  than a cell, a cell the surface only grazes has a cut neighbour: every input point is within 2 sqrt(3) steps
                  of the output.  The volumes differ by at most the input's area times one step.
  solidify        the unsigned distance is 1-Lipschitz along the cut lattice edge: every output vertex's distance to the input
                  lies in [t/2 - step, t/2 + step].
  volume          the error lies in the cells within half a cell diagonal of the surface: |count step^3 - V| <= sqrt(3) area step.
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
import mesh_metrics_reference as MR  # noqa: E402
import mesh_topology_cases as TC  # noqa: E402
from test_voxelize_cpu import (BODY_STEP, UNDECIDED_CAP, body, body_lattice, sample_reference, sign_cases, torus)  # noqa: E402

DEV = "cuda:0"
REMESH_STEP = 0.04


def _t(v, f):
    return torch.as_tensor(np.asarray(v), dtype=torch.float32).to(DEV).contiguous(), torch.as_tensor(np.asarray(f)).long().to(DEV).contiguous()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _pin(v, f, lattice, band_steps):
    """distance_field(signed=False) against the brute force on all nodes; returns (field, number of band nodes)."""
    from recmv import iso_remesh, voxelize
    band = band_steps * lattice.step
    field = voxelize.distance_field(v, f, lattice, band=band, signed=False)
    nodes = lattice.nodes(DEV).reshape(-1, 3).contiguous()
    face, _, dist2 = iso_remesh.closest_point(nodes, v, f)
    b = torch.tensor(field['band'], dtype=torch.float32, device=DEV)
    assert field['band'] == float(np.float32(band))
    in_band = dist2 <= b * b
    got_d, got_f = field['dist2'].reshape(-1), field['face'].reshape(-1)
    assert field['dist2'].shape == lattice.dims and got_d.dtype == torch.float32 and got_f.dtype == torch.int64
    assert torch.equal(_bits(got_d[in_band]), _bits(dist2[in_band])) and torch.equal(got_f[in_band], face[in_band])
    assert bool(torch.isposinf(got_d[~in_band]).all()) and bool((got_f[~in_band] == -1).all())
    n = int(in_band.sum())
    assert field['band_nodes'] == n and field['open_columns'] == 0 and not bool(field['inside'].any())
    return field, n


@pytest.fixture(scope="module")
def meshes():
    bv, bf = body()
    tv, tf = torus()
    return {'body': _t(bv, bf), 'torus': _t(tv, tf), 'body_cpu': (bv, bf)}


@pytest.fixture(scope="module")
def fields(meshes):
    """The signed fields of the two sign meshes at bands of 2 and 3 steps, and points_inside on all their nodes: computed once."""
    from recmv import metrics, voxelize
    out = {}
    for name, (_, _, lat) in sign_cases().items():
        v, f = meshes[name]
        want = metrics.points_inside(lat.nodes(DEV).reshape(-1, 3).contiguous(), v, f)
        out[name] = {'lattice': lat, 'inside_all': want,
                     'field': {s: voxelize.distance_field(v, f, lat, band=s * lat.step) for s in (2, 3)}}
    return out


# ------------------------------------------------------------------------------------------------------------ 1. band
@pytest.mark.parametrize("steps", [2, 3])
def test_band_equals_the_brute_force_on_the_body(meshes, steps):
    v, f = meshes['body']
    assert f.shape[0] == 1280
    _, n = _pin(v, f, body_lattice(meshes['body_cpu'][0]), steps)
    assert 3000 <= n <= 8000                               # (float64: 3 515 and 5 409 nodes)


def test_band_on_a_lattice_that_covers_half_of_the_mesh(meshes):
    """The lattice starts in the middle of the body: faces on the far side have negative node indices, faces across the border
    a clipped box; and it ends inside the body on the other axes."""
    from recmv import voxelize
    v, f = meshes['body']
    full = body_lattice(meshes['body_cpu'][0])
    half = voxelize.Lattice((0.013, full.origin[1], -0.2), BODY_STEP, (25, 13, 12))
    _, n = _pin(v, f, half, 3)
    assert n >= 300


def test_band_with_faces_far_larger_than_cells(meshes):
    from recmv import voxelize
    v, f = _t(*TC.tetrahedron(scale=1.))
    lat = voxelize.Lattice((-0.475, -0.475, -0.475), 0.05, (40, 40, 40))
    _, n = _pin(v, f, lat, 3)
    assert n >= 4000                                       # every face's box holds thousands of nodes: the lane-strided loop


def test_band_on_a_single_node_axis_and_a_long_z_row(meshes):
    from recmv import voxelize
    v, f = meshes['body']
    lat = voxelize.Lattice((0.3, -0.08, -0.69), 0.02, (1, 9, 70))
    _, n = _pin(v, f, lat, 3)
    assert n >= 30


def test_band_with_invalid_degenerate_and_nan_faces(meshes):
    v, f = meshes['body']
    V = v.shape[0]
    v2 = torch.cat([v, torch.tensor([[float("nan"), 0.1, 0.2]], device=DEV)]).contiguous()
    extra = torch.tensor([[0, 1, V + 5], [7, 7, 30], [3, V, 4]], device=DEV)       # out of range, no area, a NaN corner
    f2 = torch.cat([f[:500], extra, f[500:]]).contiguous()
    field, n = _pin(v2, f2, body_lattice(meshes['body_cpu'][0]), 3)
    won = field['face'][field['face'] >= 0]
    assert n >= 3000 and not bool(((won >= 500) & (won < 503)).any())


def test_two_runs_give_identical_bits(meshes):
    from recmv import voxelize
    v, f = meshes['body']
    lat = body_lattice(meshes['body_cpu'][0])
    a = voxelize.distance_field(v, f, lat, band=3 * lat.step, signed=False)
    b = voxelize.distance_field(v, f, lat, band=3 * lat.step, signed=False)
    assert torch.equal(_bits(a['dist2']), _bits(b['dist2'])) and torch.equal(a['face'], b['face'])
    assert torch.equal(_bits(a['sdf']), _bits(b['sdf']))


# ------------------------------------------------------------------------------------------------------------ 2.-4. sign
@pytest.mark.parametrize("name", ["body", "torus"])
@pytest.mark.parametrize("steps", [2, 3])
def test_inside_equals_points_inside_on_all_nodes(fields, name, steps):
    c = fields[name]
    field = c['field'][steps]
    assert field['inside'].dtype == torch.bool and field['inside'].shape == c['lattice'].dims
    assert torch.equal(field['inside'].reshape(-1), c['inside_all'])
    assert field['open_columns'] == 0 and field['sign_conflicts'] == 0 and int(c['inside_all'].sum()) >= 2000
    assert 0 < field['band_nodes'] < c['lattice'].n_nodes


def test_an_open_mesh_shows_in_the_diagnostics():
    """The open cylinder (radius 0.3, axis z).  open_columns > 0 on the lattice of step 0.05 and pad 3, and no other claim is
    made for that count: the holes face along z, the columns run along x, and at other steps every column ends outside.
    sign_conflicts > 0 on every lattice whose band is below the radius — derived: the nodes near the axis are farther than the
    band from the surface all the way from deep inside the cylinder (inside: every ray leaves through the wall) out through the
    hole to where no column holds a band node (outside), so their flag flips between two nodes outside the band."""
    from recmv import voxelize
    v, f = _t(*TC.tube())
    field = voxelize.distance_field(v, f, voxelize.lattice_for(v, step=0.05, pad_steps=3))
    print("step 0.05: open_columns %d, sign_conflicts %d" % (field['open_columns'], field['sign_conflicts']))
    assert field['open_columns'] > 0 and field['sign_conflicts'] > 0
    _, _, info = voxelize.remesh(v, f, step=0.04)
    print("step 0.04: open_columns %d, sign_conflicts %d" % (info['open_columns'], info['sign_conflicts']))
    assert info['sign_conflicts'] > 0


@pytest.mark.parametrize("name", ["body", "torus"])
def test_inside_against_the_float64_reference_on_drawn_nodes(fields, name):
    v, f, lat = sign_cases()[name]
    idx, inside, decided = sample_reference(v, f, lat)
    print("%s: %d nodes drawn, %.2f %% undecided" % (name, len(idx), 100. * (~decided).mean()))
    assert (~decided).mean() <= UNDECIDED_CAP
    for steps in (2, 3):
        got = fields[name]['field'][steps]['inside'].reshape(-1)[idx.to(DEV)].cpu().numpy()
        assert np.array_equal(got[decided], inside[decided])


@pytest.mark.parametrize("name", ["body", "torus"])
@pytest.mark.parametrize("steps", [2, 3])
def test_sdf_is_the_clamped_signed_root(fields, name, steps):
    field = fields[name]['field'][steps]
    band = torch.tensor(field['band'], dtype=torch.float32, device=DEV)
    sign = torch.where(field['inside'], -torch.ones_like(band), torch.ones_like(band))
    want = sign * torch.minimum(field['dist2'].sqrt(), band)
    ulp = torch.maximum(want.abs(), torch.tensor(2. ** -126, device=DEV)) * 2. ** -23              # an upper bound of one ulp
    assert field['sdf'].dtype == torch.float32 and bool(((field['sdf'] - want).abs() <= ulp).all())
    out = torch.isinf(field['dist2'])
    assert bool((field['sdf'][out] == sign[out] * band).all()) and bool((field['sdf'].abs() <= band).all())
    assert int(out.sum()) == fields[name]['lattice'].n_nodes - field['band_nodes']


# ------------------------------------------------------------------------------------------------------------ 5. remesh
def _volume_area(v, f):
    tri = v.double()[f]
    vol = (tri[:, 0] * torch.linalg.cross(tri[:, 1], tri[:, 2], dim=-1)).sum() / 6.
    area = 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1).norm(dim=-1).sum()
    return float(vol), float(area)


@pytest.fixture(scope="module")
def sphere_orientation():
    """The sign of the signed volume MCGpu.mc_gpu gives an analytic sphere SDF that is negative inside."""
    from recmv import MCGpu
    ax = torch.linspace(-1., 1., 24, device=DEV)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing='ij')
    sdf = ((x * x + y * y + z * z).sqrt() - 0.6).contiguous()
    v, f = MCGpu.mc_gpu(sdf, 2. / 23, 2. / 23, 2. / 23, -1., -1., -1., 0.)
    vol, _ = _volume_area(v, f)
    assert abs(abs(vol) - 4. / 3. * math.pi * 0.6 ** 3) < 0.05
    return math.copysign(1., vol)


@pytest.mark.parametrize("name,euler", [("body", 2), ("torus", 0)])
def test_remesh_is_watertight_close_and_keeps_the_volume(meshes, sphere_orientation, name, euler):
    from recmv import iso_remesh, metrics, topology, voxelize
    v, f = meshes[name]
    ov, of, info = voxelize.remesh(v, f, step=REMESH_STEP)
    step = info['lattice'].step
    assert info['open_columns'] == 0 and info['sign_conflicts'] == 0 and info['faces_in'] == f.shape[0] and info['faces_out'] == of.shape[0] > 0
    assert info['band'] == float(np.float32(3 * step)) and info['band_nodes'] > 0
    lo, hi = v.amin(0).cpu(), v.amax(0).cpu()              # padded by at least band + 1 step
    for a in range(3):
        last = info['lattice'].origin[a] + (info['lattice'].dims[a] - 1) * step
        assert info['lattice'].origin[a] <= float(lo[a]) - 3.999 * step and last >= float(hi[a]) + 3.999 * step
    r = topology.report(ov, of)
    assert r['watertight'] and r['components_vertex'] == 1 and r['components_edge'] == 1 and r['nonmanifold_edges'] == 0
    assert r['boundary_edges'] == 0 and r['euler_characteristic'] == euler
    d_out = iso_remesh.closest_point(ov, v, f)[2].sqrt()
    gen = torch.Generator(device=DEV).manual_seed(11)
    pts, _ = metrics.sample_surface(v, f, 2000, gen)
    d_in = iso_remesh.closest_point(pts.contiguous(), ov, of)[2].sqrt()
    vol_in, area_in = _volume_area(v, f)
    vol_out, _ = _volume_area(ov, of)
    print("%s: %d -> %d faces, output to input %.4f (bound %.4f), input to output %.4f (bound %.4f), volume %.4f -> %.4f" % (
        name, f.shape[0], of.shape[0], float(d_out.max()), step, float(d_in.max()), 2 * math.sqrt(3) * step, vol_in, vol_out))
    assert float(d_out.max()) <= step * (1 + 1e-4)
    assert float(d_in.max()) <= 2. * math.sqrt(3.) * step
    assert abs(abs(vol_out) - abs(vol_in)) <= area_in * step
    assert math.copysign(1., vol_out) == sphere_orientation


# ------------------------------------------------------------------------------------------------------------ 6. solidify
@pytest.mark.parametrize("name,euler", [("square", 2), ("tube", 0)])
def test_solidify_gives_a_closed_shell_at_half_the_thickness(name, euler):
    from recmv import iso_remesh, topology, voxelize
    v, f = _t(*(MR.square(n=8) if name == "square" else TC.tube()))
    t, step = 0.2, 0.04
    ov, of, info = voxelize.solidify(v, f, t, step=step)
    step = info['lattice'].step
    r = topology.report(ov, of)
    assert r['watertight'] and r['components_vertex'] == 1 and r['nonmanifold_edges'] == 0 and r['euler_characteristic'] == euler
    d = iso_remesh.closest_point(ov, v, f)[2].sqrt()
    print("%s: %d faces, distances %.4f .. %.4f" % (name, of.shape[0], float(d.min()), float(d.max())))
    assert float(d.min()) >= 0.5 * t - step and float(d.max()) <= 0.5 * t + step
    assert info['open_columns'] == 0 and info['faces_out'] == of.shape[0]
    with pytest.raises(ValueError):
        voxelize.solidify(v, f, 0.1, step=0.04)


# ------------------------------------------------------------------------------------------------------------ 7. volumes
@pytest.fixture(scope="module")
def shifted_pair(meshes):
    from recmv import voxelize
    v, f = meshes['body']
    w = (v + torch.tensor([0.1, 0., 0.], device=DEV)).contiguous()
    return v, f, w, voxelize.volume_iou(v, f, w, f, step=REMESH_STEP)


def test_volume_iou_of_identical_disjoint_and_shifted_bodies(meshes, shifted_pair):
    from recmv import metrics, voxelize
    v, f = meshes['body']
    same = voxelize.volume_iou(v, f, v, f, step=0.06)
    assert same['iou'] == 1. and same['intersection'] == same['union'] > 0 and same['volume_a'] == same['volume_b']
    far = (v + torch.tensor([2., 0., 0.], device=DEV)).contiguous()
    apart = voxelize.volume_iou(v, f, far, f, step=0.06)
    assert apart['iou'] == 0. and apart['intersection'] == 0 and apart['union'] > 0
    _, _, w, r = shifted_pair
    nodes = r['lattice'].nodes(DEV).reshape(-1, 3).contiguous()
    a, b = metrics.points_inside(nodes, v, f), metrics.points_inside(nodes, w, f)
    assert isinstance(r['intersection'], int) and isinstance(r['union'], int)
    assert r['intersection'] == int((a & b).sum()) and r['union'] == int((a | b).sum())
    assert r['iou'] == r['intersection'] / r['union'] and 0.5 < r['iou'] < 1.
    assert r['step'] == float(np.float32(REMESH_STEP)) and r['open_columns_a'] == 0 and r['open_columns_b'] == 0
    assert r['sign_conflicts_a'] == 0 and r['sign_conflicts_b'] == 0
    assert r['volume_a'] == int(a.sum()) * r['step'] ** 3 and r['volume_b'] == int(b.sum()) * r['step'] ** 3


def test_volume_against_the_signed_volume(meshes):
    from recmv import voxelize
    v, f = meshes['body']
    lat = voxelize.lattice_for(v, step=REMESH_STEP, pad_steps=3)
    vol, area = _volume_area(v, f)
    got = voxelize.volume(v, f, lat)
    print("volume %.5f against %.5f, bound %.5f" % (got, abs(vol), math.sqrt(3.) * area * lat.step))
    assert abs(got - abs(vol)) <= math.sqrt(3.) * area * lat.step
    occ = voxelize.occupancy(v, f, lat)
    assert occ.dtype == torch.bool and occ.shape == lat.dims and got == int(occ.sum()) * lat.step ** 3
    pts = lat.nodes(DEV).reshape(-1, 3)[::7].contiguous()
    sd = voxelize.signed_distance(pts, v, f)
    assert torch.equal(sd < 0, occ.reshape(-1)[::7]) and sd.dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------ 8. commands
def _write(path, v, f):
    from recmv.utils import write_obj
    write_obj(str(path), torch.as_tensor(np.asarray(v)).float(), torch.as_tensor(np.asarray(f)).long())


def test_clean_fl_voxel_remesh_solidify_and_refusal(tmp_path, capsys, meshes):
    import clean_fl
    from recmv import topology
    from recmv.utils import read_obj
    _write(tmp_path / "body.obj", *meshes['body_cpu'])
    _write(tmp_path / "square.obj", *MR.square(n=8))
    _write(tmp_path / "tube.obj", *TC.tube())
    out = clean_fl.main(["--in", str(tmp_path / "body.obj"), "--out", str(tmp_path / "a"), "--voxel-remesh", "0.04"])
    vox = json.load(open(tmp_path / "a" / "topology.json"))['files']['body.obj']['voxel']
    assert vox == out['files']['body.obj']['voxel'] and vox['mode'] == 'remesh' and vox['open_columns'] == 0
    assert vox['faces_before'] == 1280 and vox['band_nodes'] > 0 and len(vox['lattice']['dims']) == 3
    v, f = read_obj(str(tmp_path / "a" / "body.obj"))
    assert f.shape[0] == vox['faces_after'] and topology.report(v.to(DEV), f.to(DEV))['watertight']
    out = clean_fl.main(["--in", str(tmp_path / "square.obj"), "--out", str(tmp_path / "b"), "--voxel-remesh", "0.04",
                         "--solidify", "0.2"])
    vox = out['files']['square.obj']['voxel']
    assert vox['mode'] == 'solidify' and out['solidify'] == 0.2 and out['files']['square.obj']['after']['watertight']
    v, f = read_obj(str(tmp_path / "b" / "square.obj"))
    assert f.shape[0] == vox['faces_after'] > 0
    capsys.readouterr()
    with pytest.raises(SystemExit):
        clean_fl.main(["--in", str(tmp_path / "tube.obj"), "--out", str(tmp_path / "c"), "--voxel-remesh", "0.04"])
    err = capsys.readouterr().err
    assert "open_columns" in err and "not closed" in err and not (tmp_path / "c").exists()
    out = clean_fl.main(["--in", str(tmp_path / "tube.obj"), "--out", str(tmp_path / "c"), "--voxel-remesh", "0.04", "--voxel-force"])
    assert out['files']['tube.obj']['voxel']['sign_conflicts'] > 0 and (tmp_path / "c" / "tube.obj").exists()


def test_clean_fl_without_the_new_flags_writes_what_it_wrote_before(tmp_path, meshes):
    """The command without the new flags against the calls it has always made (keep_components, write_obj) on one small mesh
    with a floater: the same bytes of the mesh, and a topology.json with the keys it always had and no others."""
    import clean_fl
    from recmv import topology
    from recmv.utils import read_obj
    v, f = TC.merge(TC.tetrahedron(scale=1.), TC.tetrahedron(scale=0.1, shift=(3., 0., 0.)))
    _write(tmp_path / "m.obj", v, f)
    out = clean_fl.main(["--in", str(tmp_path / "m.obj"), "--out", str(tmp_path / "o"), "--largest", "1"])
    rv, rf = read_obj(str(tmp_path / "m.obj"))
    kv, kf, _ = topology.keep_components(rv.to(DEV), rf.to(DEV), largest=1, min_area_frac=None, min_faces=None,
                                         connectivity='vertex')
    _write(tmp_path / "want.obj", kv.cpu(), kf.cpu())
    assert (tmp_path / "o" / "m.obj").read_bytes() == (tmp_path / "want.obj").read_bytes()
    assert set(out) == {'files', 'connectivity', 'largest', 'min_area_frac', 'min_faces', 'report_only'}
    assert set(out['files']['m.obj']) == {'before', 'after', 'dropped'}
    assert json.load(open(tmp_path / "o" / "topology.json")) == json.loads(json.dumps(out))
    assert (tmp_path / "o" / "topology.json").read_text() == json.dumps(out, indent=1, sort_keys=True)


def test_eval_fl_volume_reports_the_iou(tmp_path, shifted_pair):
    import eval_fl
    from recmv import voxelize
    from recmv.utils import read_obj
    v, f, w, _ = shifted_pair
    _write(tmp_path / "pred.obj", v.cpu(), f.cpu())
    _write(tmp_path / "gt.obj", w.cpu(), f.cpu())
    res = eval_fl.main(["--pred", str(tmp_path / "pred.obj"), "--gt", str(tmp_path / "gt.obj"), "--samples", "2000", "--volume",
                        "--volume-step", "0.04"])
    (pv, pf), (gv, gf) = read_obj(str(tmp_path / "pred.obj")), read_obj(str(tmp_path / "gt.obj"))   # what the command read
    want = voxelize.volume_iou(pv.to(DEV), pf.to(DEV), gv.to(DEV), gf.to(DEV), step=0.04)
    got = res['pairs']['pred']
    assert got['volume_iou'] == want['iou'] and got['volume_pred'] == want['volume_a'] and got['volume_gt'] == want['volume_b']
    assert got['volume']['intersection'] == want['intersection'] and got['volume']['reason'] is None
    assert res['mean']['volume_iou'] == want['iou'] and 0.5 < want['iou'] < 1.
    plain = eval_fl.main(["--pred", str(tmp_path / "pred.obj"), "--gt", str(tmp_path / "gt.obj"), "--samples", "2000"])
    assert not any(k.startswith('volume') for k in plain['pairs']['pred']) and set(plain['mean']) == set(res['mean']) - {
        'volume_iou', 'volume_pred', 'volume_gt'}
    _write(tmp_path / "open.obj", *TC.tube())
    res = eval_fl.main(["--pred", str(tmp_path / "open.obj"), "--gt", str(tmp_path / "gt.obj"), "--samples", "2000", "--volume",
                        "--volume-step", "0.04"])
    got = res['pairs']['open']
    assert got['volume_iou'] is None and got['volume_pred'] is None and 'not closed' in got['volume']['reason']
    assert 'volume_iou' not in res['mean'] and 'chamfer_l1' in res['mean']
