"""Segment queries on the GPU: recmv_segment_mesh_grid and recmv_segment_mesh_brute (recmv.metrics.segment_hits), the inside
test and the penetration depth built on them, Surface_Intesection and the penetration option of the intersection report.

Primary judge: the brute-force kernel, exactly — face, the bits of t and count of the grid query equal the brute force's for
every launch shape (1, 8, 64 lanes per segment), both modes and every grid: both run csrc/seg_tri.h's seg_face_hit on the same
corners, and the grid's walk reaches every face that passes its gate (derivation in csrc/segment_mesh.hip).

Second judge: the float64 restatement tests/segment_mesh_reference.py, on what it DECIDES (tests/test_segment_mesh_cpu.py): the
hit sets' sizes and first faces are the reference's, and |t - t64| <= 2 * 20 eps32 L^3 / |sp - sq| + 2 eps32.  Derivation of
that tolerance: t = sp / (sp - sq); the f32 determinants err by at most B = 20 eps32 L^3 each (csrc/tri_tri.h), so with
D = sp - sq, to first order, t' - t = (e_p (1 - t) + e_q t) / D, at most B / |D| in magnitude as 0 < t < 1; the rounded
difference and the rounded quotient add t eps32 together.  The tolerance is twice that sum — from the determinant bound and
the one division, not tuned.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import segment_mesh_reference as SR  # noqa: E402
from test_segment_mesh_cpu import (FLAT, RADIUS, UNDECIDED_CAP, body, inside_points, normal_casts, radial_band,  # noqa: E402
                                   random_segments, references)  # noqa: F401  (references: the module-scoped fixture)

DEV = "cuda:0"
LANES = (1, 8, 64)


def _same(a, b, count):
    assert torch.equal(a['face'], b['face'])
    assert torch.equal(a['t'].view(torch.int32), b['t'].view(torch.int32))
    if count:
        assert a['count'].dtype == torch.int32 and torch.equal(a['count'], b['count'])
    else:
        assert a['count'] is None


def _check(p, q, v, f, grids=({},), lanes=LANES):
    """The grid query on every grid, launch shape and mode against the brute force; returns the brute force's answer."""
    from recmv import metrics
    p, q, v, f = (x.to(DEV).contiguous() for x in (p, q, v, f))
    want = metrics.segment_hits(p, q, v, f, count=True, method='brute')
    S = p.shape[0]
    assert want['face'].dtype == torch.int64 and want['face'].shape == (S,) and want['t'].shape == (S,)
    assert want['point'].shape == (S, 3) and want['count'].shape == (S,)
    none = want['face'] < 0
    assert bool(torch.isnan(want['t'][none]).all()) and bool((want['count'][none] == 0).all())
    assert bool((want['count'][~none] > 0).all()) and bool(torch.isnan(want['point'][none]).all())
    for kw in grids:
        g = metrics.MeshGrid(v, f, **kw)
        for n in lanes:
            _same(g.segment_hits(p, q, count=True, lanes=n), want, True)
            _same(g.segment_hits(p, q, count=False, lanes=n), want, False)
    return want


@pytest.fixture(scope="module")
def inputs():
    v, f = body()
    p, q = random_segments(v)
    cp, cq, w = normal_casts(v, f)
    return {'v': v, 'f': f, 'random': (p, q), 'casts': (cp, cq), 'w': w}


def test_grid_equals_brute_force_on_every_grid_launch_shape_and_mode(inputs):
    v, f = inputs['v'], inputs['f']
    assert f.shape[0] == 1280
    grids = ({}, {"dims": (1, 1, 1)}, {"dims": (1, 1, 17)}, {"dims": (37, 41, 29)})
    p, q = inputs['random']
    want = _check(p, q, v, f, grids=grids)
    assert int((want['face'] >= 0).sum()) >= 500 and int((want['count'] > 1).sum()) >= 500
    want = _check(*inputs['casts'], v, f, grids=grids)
    assert int((want['face'] >= 0).sum()) >= 400


@pytest.mark.parametrize("S", [0, 1, 63, 65])
def test_segment_counts_around_the_group_and_wave_sizes(inputs, S):
    p, q = inputs['random']
    want = _check(p[:S], q[:S], inputs['v'], inputs['f'], grids=({}, {"dims": (1, 1, 17)}))
    assert want['face'].shape == (S,)


def test_a_grid_that_does_not_cover_its_mesh_and_segments_outside_it(inputs):
    """A forced grid of 8^3 small cells around the mesh's lower corner: most faces are clamped into its edge cells; and
    segments that start, end or lie outside the mesh's box, along the axes, in cell-boundary planes, and without length."""
    from recmv import metrics
    v, f = inputs['v'].to(DEV), inputs['f'].to(DEV)
    p, q = (x.clone() for x in inputs['random'])
    p[::5] *= 4.                                           # far outside
    q[1::7, 0] = p[1::7, 0]                                # direction components exactly 0
    q[2::7, 1:] = p[2::7, 1:]
    q[3::11] = p[3::11]                                    # no length
    g = metrics.MeshGrid(v, f, dims=(8, 8, 8), cell_size=0.05)
    lo = torch.tensor(list(g.origin))
    k = torch.arange(p.shape[0]) % 9
    p[4::13, 2] = (lo[2] + k[4::13] * g.cell_size)         # in cell-boundary planes
    q[4::13, 2] = p[4::13, 2]
    p, q = p.to(DEV), q.to(DEV)
    want = metrics.segment_hits(p, q, v, f, count=True, method='brute')
    for n in LANES:
        _same(g.segment_hits(p, q, count=True, lanes=n), want, True)
        _same(g.segment_hits(p, q, count=False, lanes=n), want, False)
    assert int((want['face'] >= 0).sum()) >= 300 and bool((want['face'][3::11] < 0).all())


def test_degenerate_invalid_and_nan_input(inputs):
    v, f = inputs['v'], inputs['f']
    V = v.shape[0]
    flat = torch.tensor([[5, 5, 9], [7, 11, 11], [4, 4, 4]])
    bad = torch.tensor([[0, 1, V + 1], [-1, 2, 3], [V + 7, V + 8, V + 9]])
    faces = torch.cat([f[:100], flat, bad, f[100:]]).contiguous()
    p, q = (x[:1024].clone() for x in inputs['random'])
    p[::9, 1] = float("nan")
    q[4::9, 2] = float("inf")
    want = _check(p, q, v, faces, lanes=(1, 64))
    plain = _check(inputs['random'][0][:1024], inputs['random'][1][:1024], v, f, lanes=(8,))
    assert bool((want['face'][::9] < 0).all()) and bool((want['face'][4::9] < 0).all())
    ok = torch.ones(1024, dtype=torch.bool)
    ok[::9] = False
    ok[4::9] = False
    assert torch.equal(want['count'][ok.to(DEV)], plain['count'][ok.to(DEV)])     # the six extra faces are hit by nothing
    hit = want['face'] >= 0
    assert not bool(((want['face'][hit] >= 100) & (want['face'][hit] < 106)).any())
    nan_v = v.clone()
    nan_v[::7] = float("nan")
    from recmv import metrics                              # (a grid refuses vertices that are not finite: the brute force)
    with pytest.raises(ValueError):
        metrics.MeshGrid(nan_v.to(DEV), f.to(DEV))
    want = metrics.segment_hits(inputs['random'][0][:1024].to(DEV), inputs['random'][1][:1024].to(DEV), nan_v.to(DEV), f.to(DEV),
                                count=True, method='brute')
    touched = torch.isnan(nan_v[f]).any(2).any(1).to(DEV)
    hit = want['face'] >= 0
    assert int(hit.sum()) > 50 and not bool(touched[want['face'][hit]].any())


@pytest.mark.parametrize("name", ["random", "casts"])
def test_against_the_float64_reference(inputs, references, name):
    from recmv import metrics
    p, q = inputs[name]
    r = references[name]
    got = metrics.segment_hits(p.to(DEV), q.to(DEV), inputs['v'].to(DEV), inputs['f'].to(DEV), count=True, method='grid')
    face, t, count = got['face'].cpu().numpy(), got['t'].cpu().numpy().astype(np.float64), got['count'].cpu().numpy()
    pd, fd = r['pairs_decided'], r['first_decided']
    hitting = r['count'] > 0
    err = np.abs(t - r['t'])
    print("%s: %d segments hit (reference %d); decided: %d hit sets, %d first hits; worst |t - t64| / tolerance %.3g" % (
        name, (face >= 0).sum(), hitting.sum(), pd.sum(), (fd & hitting).sum(), np.nanmax((err / r['t_tol'])[fd & hitting])))
    assert np.array_equal(count[pd], r['count'][pd])       # the hit sets' sizes, where every pair is decided
    assert np.array_equal(face[fd], r['face'][fd])         # the first faces (-1 where the reference hits nothing)
    assert np.all(err[fd & hitting] <= r['t_tol'][fd & hitting])
    assert (hitting & ~fd).sum() <= UNDECIDED_CAP * hitting.sum()
    decided_pair = r['margin'] > SR.BOUND_C * SR.EPS32
    first = {int(s): int(j) for s, j in enumerate(face) if j >= 0}
    ref_miss = {(int(s), int(j)) for (s, j), h, d in zip(r['cand'].tolist(), r['hit'], decided_pair) if d and not h}
    assert not [(s, j) for s, j in first.items() if (s, j) in ref_miss]            # no first hit on a decided miss
    point = got['point'].cpu()
    want = p + got['t'].cpu()[:, None] * (q - p)
    assert torch.equal(torch.nan_to_num(point, nan=7.), torch.nan_to_num(want, nan=7.))
    # the hit sets themselves, pair by pair: the 16 faces with the most decided hits, each cast as a mesh of that one face —
    # `count` is then the pair's own decision, and `t` its own parameter.  A pair that is not among the reference's
    # candidates has boxes that do not meet: no hit, by the same exact comparisons in the kernel.
    cand, ref_hit = r['cand'], r['hit'] & decided_pair
    busiest = np.argsort(-np.bincount(cand[ref_hit, 1], minlength=inputs['f'].shape[0]), kind='stable')[:16]
    checked = hits = 0
    for j in busiest.tolist():
        one = metrics.segment_hits(p.to(DEV), q.to(DEV), inputs['v'].to(DEV), inputs['f'][j:j + 1].to(DEV).contiguous(), count=True,
                                   method='brute')
        c1, t1 = one['count'].cpu().numpy(), one['t'].cpu().numpy().astype(np.float64)
        mine = cand[:, 1] == j
        want_hit = np.zeros(len(c1), bool)
        want_hit[cand[mine & r['hit'], 0]] = True
        known = np.ones(len(c1), bool)                      # decided, or not a candidate at all
        known[cand[mine & ~decided_pair, 0]] = False
        assert np.array_equal((c1 == 1)[known], want_hit[known]) and set(np.unique(c1)) <= {0, 1}, j
        sel = mine & ref_hit
        assert np.all(np.abs(t1[cand[sel, 0]] - r['t_pair'][sel]) <= r['t_tol_pair'][sel]), j
        checked += int(known.sum())
        hits += int(sel.sum())
    print("%s: %d pairs of 16 one-face meshes checked against the reference, %d of them decided hits" % (name, checked, hits))
    assert hits >= 16


def _coplanar_scenes(n_side=10, seed=11):
    """n_side^3 scenes in one mesh, 3 apart, each under a random rigid motion of its own (float64, rounded to f32 at the end):
    two faces that hold the segment's line at 0.7 to 0.95 of its length — their sp and sq are rounding noise, the f32
    predicate accepts a good part of them, and the bare quotient sp / (sp - sq) of such a pair can land anywhere in (0, 1) —
    behind a clean face crossed at t = 0.21; three segments along the line per scene.  tools/segment_mesh_host_check runs the
    same scenes one by one; there about 1 in 170 segments had a noise quotient in front of the clean hit."""
    g = torch.Generator().manual_seed(seed)
    n = n_side ** 3
    w = torch.rand(n, generator=g, dtype=torch.float64) * 2 * np.pi
    cy, cz, o = torch.cos(w), torch.sin(w), torch.zeros(n, dtype=torch.float64)
    def pt(x, s):
        return torch.stack([o + x, s * cy, s * cz], 1)
    verts = torch.stack([pt(0.4, -0.2), pt(0.9, -0.1), pt(0.65, 0.3), pt(0.95, 0.25),
                         torch.tensor([-0.58, -0.3, -0.3], dtype=torch.float64).expand(n, 3),
                         torch.tensor([-0.58, 0.4, -0.2], dtype=torch.float64).expand(n, 3),
                         torch.tensor([-0.58, 0., 0.5], dtype=torch.float64).expand(n, 3)], 1)          # [n,7,3]
    ends = torch.tensor([[-1, 0, 0], [1, 0, 0], [-0.8, 0, 0], [0.97, 0, 0], [-1, 0, 0], [0.8, 0, 0]], dtype=torch.float64).expand(n, 6, 3)
    rot = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))[0]
    k = torch.arange(n)
    shift = 3. * torch.stack([k % n_side, (k // n_side) % n_side, k // n_side ** 2], 1).double() + 0.3 * torch.rand(n, 3, generator=g, dtype=torch.float64)
    verts = (verts @ rot.transpose(1, 2) + shift[:, None]).float()
    ends = (ends @ rot.transpose(1, 2) + shift[:, None]).float()
    faces = (torch.tensor([[0, 1, 2], [1, 3, 2], [4, 5, 6]])[None] + 7 * k[:, None, None]).reshape(-1, 3)
    return ends[:, 0::2].reshape(-1, 3).contiguous(), ends[:, 1::2].reshape(-1, 3).contiguous(), verts.reshape(-1, 3).contiguous(), faces


def test_a_face_that_holds_the_segments_line_behind_an_earlier_hit():
    """The first hit with the early stop is the brute force's where a face late in the walk has determinants that are noise:
    every launch shape, both modes, two grids.  Every segment crosses its scene's clean face (3 n + 2); a tenth of them at
    least must be judged to hit a coplanar face as well, or the scenes show nothing."""
    p, q, v, f = _coplanar_scenes()
    want = _check(p, q, v, f, grids=({}, {"dims": (48, 48, 48)}))
    S = p.shape[0]
    count, face, t = want['count'].cpu(), want['face'].cpu(), want['t'].cpu()
    assert S == 3000 and bool((count >= 1).all())
    noisy = count > 1
    early = noisy & (face % 3 != 2)
    print("%d segments, %d judged to hit a coplanar face, %d of those in front of the clean hit" % (S, noisy.sum(), early.sum()))
    assert int(noisy.sum()) >= S // 10
    clean = face % 3 == 2
    expect = torch.tensor([0.21, 0.22 / 1.77, 0.21 / 0.9]).repeat(S // 3)
    assert bool(((t - expect)[clean].abs() < 1e-4).all())
    # a coplanar face's reported t lies where the face is: between 0.7 and 0.95 of the first segment's length, and so never
    # in front of the clean hit (the bare quotient of the same pairs lands there now and then)
    assert int(early.sum()) == 0


def test_the_contract_on_hand_cases_on_the_device():
    from recmv import metrics
    v = torch.tensor(FLAT + FLAT + [[0, 0, -1], [1, 0, -1], [0, 1, -1], [9, 9, 9]], dtype=torch.float32)
    f = torch.tensor([[3, 4, 5], [0, 1, 2], [0, 1, 99], [-1, 1, 2], [6, 7, 8], [9, 9, 0], [0, 0, 1]])
    nan = float("nan")
    cases = [  # p, q, count, face, t
        ([0.2, 0.2, 1], [0.2, 0.2, -3], 3, 0, 0.25),       # two faces at equal t: the lowest id wins; then a third
        ([0.2, 0.2, -3], [0.2, 0.2, 1], 3, 4, 0.5),
        ([0.2, 0.2, 1], [0.2, 0.2, -0.5], 2, 0, 2. / 3.),
        ([2, 2, 1], [2, 2, -1], 0, -1, nan),               # beside
        ([0.1, -0.2, 2], [0.1, -0.2, 0.5], 0, -1, nan),    # ends before the plane
        ([0.1, -0.2, 1], [0.1, -0.2, 0], 0, -1, nan),      # an endpoint exactly in the plane
        ([0, 1, 1], [0, 1, -0.5], 0, -1, nan),             # through a vertex
        ([-1, -1, 0.5], [1, -1, -0.5], 0, -1, nan),        # through an edge
        ([-1, -1, 0], [1, -1, 0], 0, -1, nan),             # along an edge
        ([-0.5, -0.5, 0], [0.5, 0, 0], 0, -1, nan),        # in the plane
        ([0.1, -0.2, 1], [0.1, -0.2, 1], 0, -1, nan),      # no length
        ([0.1, nan, 1], [0.1, -0.2, -3], 0, -1, nan),
        ([0.1, -0.2, 1], [0.1, float("inf"), -3], 0, -1, nan),
    ]
    p = torch.tensor([c[0] for c in cases], dtype=torch.float32)
    q = torch.tensor([c[1] for c in cases], dtype=torch.float32)
    want_t = torch.tensor([c[4] for c in cases], dtype=torch.float32)
    for method in ('brute', 'grid'):
        got = metrics.segment_hits(p.to(DEV), q.to(DEV), v.to(DEV), f.to(DEV), count=True, method=method)
        assert got['count'].tolist() == [c[2] for c in cases], method
        assert got['face'].tolist() == [c[3] for c in cases], method
        t = got['t'].cpu()
        assert torch.equal(torch.isnan(t), torch.isnan(want_t)) and torch.allclose(t[:3], want_t[:3], rtol=0, atol=4 * 2.0 ** -23)
        first = metrics.segment_hits(p.to(DEV), q.to(DEV), v.to(DEV), f.to(DEV), method=method)
        assert first['count'] is None and torch.equal(first['face'], got['face'])
    with pytest.raises(ValueError):
        metrics.segment_hits(p.to(DEV), q[:3].to(DEV), v.to(DEV), f.to(DEV))
    with pytest.raises(ValueError):
        metrics.segment_hits(p.to(DEV).double(), q.to(DEV).double(), v.to(DEV), f.to(DEV))
    with pytest.raises(ValueError):
        metrics.segment_hits(p.to(DEV), q.to(DEV), v.to(DEV), f.to(DEV), method='fast')
    with pytest.raises(ValueError):
        metrics.MeshGrid(v[:9].to(DEV), f[:2].to(DEV)).segment_hits(p.to(DEV), q.to(DEV), lanes=3)


def test_points_inside_agrees_with_the_ground_truth_outside_the_band(inputs):
    from recmv import metrics
    v, f = inputs['v'], inputs['f']
    pts = inside_points(v)
    r_in, r_out = radial_band(v, f)
    r = pts.double().norm(dim=1)
    clear = (r < r_in) | (r > r_out)
    for method in ('grid', 'brute'):
        got = metrics.points_inside(pts.to(DEV), v.to(DEV), f.to(DEV), method=method).cpu()
        assert got.dtype == torch.bool and got.shape == (2000,)
        assert torch.equal(got[clear], (r < r_in)[clear]), method
    assert int((r < r_in).sum()) >= 100 and metrics.points_inside(pts[:0].to(DEV), v.to(DEV), f.to(DEV)).shape == (0,)
    bad = pts[:4].clone()
    bad[0, 0] = float("nan")
    assert not bool(metrics.points_inside(bad.to(DEV), v.to(DEV), f.to(DEV))[0])


def test_penetration_depths_are_the_closest_point_distances(inputs):
    from recmv import metrics
    v, f = inputs['v'].to(DEV), inputs['f'].to(DEV)
    pts = inside_points(inputs['v']).to(DEV)
    m = metrics.penetration(pts, v, f, method='grid')
    inside = metrics.points_inside(pts, v, f, method='grid')
    _, _, d2 = metrics.MeshGrid(v, f).closest_point(pts)
    assert torch.equal(m['inside'], inside) and m['depth'].dtype == torch.float32
    assert torch.equal(m['depth'][inside], d2.sqrt()[inside]) and bool((m['depth'][~inside] == 0).all())
    assert m['count'] == int(inside.sum()) >= 100 and m['max_depth'] == float(m['depth'].max())
    assert abs(m['mean_depth'] - float(m['depth'][inside].double().mean())) < 1e-9
    assert 0.3 * RADIUS < m['max_depth'] < RADIUS
    out = metrics.penetration(pts[~inside], v, f)
    assert out['count'] == 0 and out['max_depth'] == 0. and out['mean_depth'] == 0.


def test_surface_intesection_on_the_two_bodies(inputs):
    from recmv import metrics, shading
    from recmv.engineer.optimizer import Surface_Intesection, TriMesh
    v, f, w = inputs['v'].to(DEV), inputs['f'].to(DEV), inputs['w'].to(DEV)
    max_dist = 0.2 * RADIUS
    out = Surface_Intesection(max_dist=max_dist, method='grid')(smpl_slice=TriMesh(w, f), cano_meshes=(v, f))
    V = w.shape[0]
    valid, face, loc, dist = out['valid'], out['face'], out['location'], out['distance']
    assert valid.shape == (V,) and face.shape == (V,) and loc.shape == (V, 3) and dist.shape == (V,)
    assert int(valid.sum()) >= 300 and bool((face[~valid] < 0).all()) and bool(torch.isnan(dist[~valid]).all())
    assert bool((dist[valid].abs() <= max_dist).all()) and bool((dist[valid] > 0).any()) and bool((dist[valid] < 0).any())
    # the reference on the very segments the class casts (its normals are the device's)
    n = shading.verts_normals(w, f)
    p = torch.cat([w, w])
    q = torch.cat([w + max_dist * n, w - max_dist * n])
    r = SR.segment_hits(p.cpu().numpy(), q.cpu().numpy(), inputs['v'].numpy(), inputs['f'].numpy())
    ref_valid = (r['face'].reshape(2, V) >= 0).any(0)
    decided = r['first_decided'].reshape(2, V).all(0)
    assert np.array_equal(valid.cpu().numpy()[decided], ref_valid[decided]) and decided.mean() >= 1 - UNDECIDED_CAP
    # every valid location lies on its face: barycentric residual within the t tolerance times the segment length
    tri = v[f[face[valid]]].double()                       # the corners of the hit faces [n,3,3]
    x = loc[valid].double()
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    sol = torch.linalg.lstsq(torch.stack([e1, e2], 2), (x - tri[:, 0])[:, :, None]).solution[:, :, 0]
    res = (tri[:, 0] + sol[:, 0:1] * e1 + sol[:, 1:2] * e2 - x).norm(dim=1)
    back = (dist[valid] < 0).cpu().numpy()
    idx = np.nonzero(valid.cpu().numpy())[0] + np.where(back, V, 0)
    tol = torch.from_numpy(r['t_tol'][idx]).to(DEV) * max_dist + 4 * 2.0 ** -23 * RADIUS      # (+ the rounding of p + t (q - p))
    dec = torch.from_numpy(r['first_decided'][idx]).to(DEV)
    assert bool((res[dec] <= tol[dec]).all()) and bool((sol[dec] > -1e-3).all()) and bool((sol[dec].sum(1) < 1 + 1e-3).all())
    # the nearer of the two hits
    both = metrics.segment_hits(p, q, v, f, method='brute')
    t2 = torch.where(both['face'] >= 0, both['t'], torch.full_like(both['t'], float("inf"))).view(2, V)
    assert torch.equal(dist[valid].abs(), t2.min(0)[0][valid] * max_dist)
    fixed = Surface_Intesection(ray_dirs=[0., 0., -1.], use_normal=False, max_dist=3 * RADIUS)(smpl_slice=(w, f), cano_meshes=(v, f))
    assert int(fixed['valid'].sum()) >= 300 and bool((fixed['location'][fixed['valid']][:, :2] - w[fixed['valid']][:, :2]).abs().max() < 1e-5)


def test_intersection_report_with_penetration_sees_a_patch_sunk_wholly_inside():
    from recmv import collide
    from test_gpu_animation import _irregular_body
    body_v, body_f = _irregular_body(level=2)
    gv, gf = _irregular_body(level=2, seed=5)
    clean = (1.15 * gv).contiguous()
    # a small separate patch of the garment (its own faces and vertices) floating deep inside the body: no face crosses
    patch_v = 0.1 * gv[gf[:6].reshape(-1)] + torch.tensor([0.05, 0.02, -0.03])
    patch_f = torch.arange(18).reshape(6, 3) + gv.shape[0]
    sunk_v = torch.cat([clean, patch_v]).contiguous()
    sunk_f = torch.cat([gf, patch_f]).contiguous()
    garments = {'shirt': (torch.stack([sunk_v, sunk_v]).to(DEV), sunk_f.to(DEV))}
    body = (torch.stack([body_v, body_v]).to(DEV), body_f.to(DEV))
    plain = collide.intersection_report(garments, *body)
    full = collide.intersection_report(garments, *body, penetration=True)
    assert set(plain[0]['shirt']) == {'body_faces', 'self_faces', 'faces'} and set(plain[0]) == {'shirt', 'between'}
    assert set(full[0]['shirt']) == {'body_faces', 'self_faces', 'faces', 'inside_vertices', 'max_depth'}
    assert {k: full[0]['shirt'][k] for k in plain[0]['shirt']} == plain[0]['shirt'] and full[0]['between'] == plain[0]['between']
    assert full[0]['shirt']['body_faces'] == 0 and full[0]['shirt']['inside_vertices'] == 18
    assert 0.2 * RADIUS < full[0]['shirt']['max_depth'] < RADIUS and full[1] == full[0]
    clean_rep = collide.intersection_report({'shirt': (clean[None].to(DEV), gf.to(DEV))}, body_v[None].to(DEV), body_f.to(DEV),
                                            penetration=True)
    assert clean_rep[0]['shirt']['inside_vertices'] == 0 and clean_rep[0]['shirt']['max_depth'] == 0.
