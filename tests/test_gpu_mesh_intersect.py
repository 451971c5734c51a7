"""Crossing faces on the GPU: recmv_mesh_intersect_grid_count / _fill and recmv_mesh_intersect_brute (recmv.metrics).

Primary judge: the brute-force kernel, exactly — the sorted pairs and the per-face counts of the grid query equal the brute
force's as integers, for every launch shape (1, 8, 64 lanes per face) and on every grid: both kernels run the one predicate
of csrc/tri_tri.h on the same corners behind the same box test.

Second judge: the float64 restatement tests/mesh_intersect_reference.py.  Every pair the reference DECIDES (all deciding
determinants above BOUND(L) = 20 eps32 L^3, derived in tests/test_mesh_intersect_cpu.py) must get the reference's answer; the
share of undecided crossing pairs stays under that file's cap.
"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import mesh_intersect_reference as XR  # noqa: E402
from test_mesh_intersect_cpu import (BOUND_C, EPS32, UNDECIDED_CAP, pulled_sphere, two_bodies, undecided_share,  # noqa: E402
                                     unwelded)
from test_nricp_cpu import icosphere  # noqa: E402

DEV = "cuda:0"
LANES = (1, 8, 64)


def _brute(av, af, bv=None, bf=None):
    from recmv import metrics
    if bv is None:
        return metrics._brute_crossings(av, af, av, af, True)
    return metrics._brute_crossings(av, af, bv, bf, False)


def _check(av, af, bv, bf, grids=({},), lanes=LANES):
    """The grid query of B on every grid and launch shape against the brute force; returns the brute force's (pairs, counts).
    bv None: self mode."""
    from recmv import metrics
    av, af = av.to(DEV).contiguous(), af.to(DEV).contiguous()
    own = bv is None
    if not own:
        bv, bf = bv.to(DEV).contiguous(), bf.to(DEV).contiguous()
    pairs, counts = _brute(av, af, bv, bf)
    assert pairs.dtype == torch.int64 and counts.dtype == torch.int32 and counts.shape == (af.shape[0],)
    assert int(counts.sum()) == pairs.shape[0]
    for kw in grids:
        g = metrics.MeshGrid(av, af, **kw) if own else metrics.MeshGrid(bv, bf, **kw)
        for n in lanes:
            got, cnt = g.self_intersections(lanes=n) if own else g.intersections(av, af, lanes=n)
            assert torch.equal(got, pairs) and torch.equal(cnt, counts), (kw, n, got.shape, pairs.shape)
    return pairs, counts


def _against_reference(pairs, av, af, bv, bf, self_mode=False, capped=True):
    ref, cand, cross, margin = XR.intersections(av.numpy(), af.numpy(), bv.numpy(), bf.numpy(), self_mode=self_mode)
    decided = margin > BOUND_C * EPS32
    key = lambda p: set(map(tuple, np.asarray(p).tolist()))  # noqa: E731
    got = key(pairs.cpu().numpy())
    tested = key(cand)
    assert got <= tested                                   # nothing outside the pairs whose boxes meet
    wrong = [tuple(p) for p, c, d in zip(cand.tolist(), cross, decided) if d and ((tuple(p) in got) != bool(c))]
    und_cross, und_all = undecided_share(cross, margin)
    print("%d pairs (reference %d), %d tested, undecided %d crossing / %d tested, wrong among the decided: %d" % (
        len(got), len(ref), len(cand), und_cross, und_all, len(wrong)))
    assert not wrong, wrong[:5]
    assert not capped or und_cross <= UNDECIDED_CAP * max(len(ref), 1)
    return ref


@pytest.fixture(scope="module")
def bodies():
    return two_bodies()


def test_grid_equals_brute_force_on_every_grid_and_launch_shape(bodies):
    av, af, bv, bf = bodies
    assert af.shape[0] == 1280
    pairs, counts = _check(av, af, bv, bf, grids=({}, {"dims": (1, 1, 1)}, {"dims": (37, 41, 29)}))
    assert pairs.shape[0] >= 100 and bool((pairs[1:, 0] * 2 ** 31 + pairs[1:, 1] > pairs[:-1, 0] * 2 ** 31 + pairs[:-1, 1]).all())


def test_against_the_float64_reference(bodies):
    from recmv import metrics
    av, af, bv, bf = bodies
    m = metrics.mesh_intersections(av.to(DEV), af.to(DEV), bv.to(DEV), bf.to(DEV), method='grid')
    ref = _against_reference(m['pairs'], av, af, bv, bf)
    assert m['n_pairs'] == m['pairs'].shape[0]
    assert torch.equal(m['faces_a'].cpu(), torch.unique(m['pairs'][:, 0]).cpu())
    assert m['ratio_a'] == m['faces_a'].shape[0] / 1280 and m['ratio_b'] == m['faces_b'].shape[0] / 1280 and len(ref) >= 100


def test_symmetry(bodies):
    from recmv import metrics
    av, af, bv, bf = (t.to(DEV) for t in bodies)
    ab, _ = metrics.MeshGrid(bv, bf).intersections(av, af)
    ba, _ = metrics.MeshGrid(av, af).intersections(bv, bf)
    swapped = ab[:, [1, 0]]
    swapped = swapped[torch.sort(swapped[:, 0] * 2 ** 31 + swapped[:, 1])[1]]
    assert torch.equal(swapped, ba) and ab.shape[0] > 0


def test_self_mode_clean_pulled_and_unwelded():
    from recmv import metrics
    from test_gpu_animation import _irregular_body
    v, f = _irregular_body(level=3)
    pairs, _ = _check(v, f, None, None, grids=({}, {"dims": (1, 1, 1)}))
    assert pairs.shape[0] == 0                             # a clean closed surface: neighbours touch, nothing crosses
    v, f = pulled_sphere()
    pairs, _ = _check(v, f, None, None, grids=({}, {"dims": (1, 1, 1)}, {"dims": (23, 19, 31)}))
    ref = _against_reference(pairs, v, f, v, f, self_mode=True)
    assert len(ref) >= 10 and bool((pairs[:, 0] < pairs[:, 1]).all())
    shared = (f[pairs[:, 0].cpu()][:, :, None] == f[pairs[:, 1].cpu()][:, None, :]).any(2).any(1)
    assert not bool(shared.any())
    m = metrics.self_intersections(v.to(DEV), f.to(DEV), method='brute')
    assert torch.equal(m['pairs'], pairs) and m['ratio'] == m['faces'].shape[0] / f.shape[0]
    # unwelded: every face has its own corners, no index is shared, the seams are bit-identical positions
    uv, uf = unwelded(v, f)
    _, cand, cross, _ = XR.intersections(uv.numpy(), uf.numpy(), uv.numpy(), uf.numpy(), self_mode=True)
    touching = (f[cand[:, 0]][:, :, None] == f[cand[:, 1]][:, None, :]).any(2).any(1).numpy()
    assert touching.sum() > 1000 and not cross[touching].any()                    # the reference: no seam pair crosses
    upairs, _ = _check(uv, uf, None, None)
    assert torch.equal(upairs, pairs)


def test_dedup_two_large_triangles_in_a_fine_grid():
    """Their boxes share hundreds of cells of a forced 24^3 grid; the pair is reported once."""
    bv = torch.tensor([[-1., -1., 0.02], [1., -0.9, -0.03], [0.1, 1., 0.01], [-1., -1., -1.], [1., 1., 1.]])
    bf = torch.tensor([[0, 1, 2]])
    av = torch.tensor([[0.05, -0.9, -0.8], [-0.03, 0.9, -0.7], [0.02, 0.1, 0.9]])
    af = torch.tensor([[0, 1, 2]])
    pairs, counts = _check(av, af, bv, bf, grids=({"dims": (24, 24, 24)}, {}))
    assert pairs.tolist() == [[0, 0]] and counts.tolist() == [1]


def test_one_huge_triangle_through_many_tiny_ones():
    sv, sf = icosphere(2)
    tiny_v, tiny_f = (0.15 * sv + torch.tensor([0.1, 0.05, 0.])).contiguous(), sf
    huge_v = torch.tensor([[-1., -1., -0.2], [1.5, -1., 0.1], [-1., 1.5, 0.15]])       # z = 0.08 at the sphere's centre
    huge_f = torch.tensor([[0, 1, 2], [0, 1, 2]])
    pairs, counts = _check(huge_v, huge_f, tiny_v, tiny_f, grids=({}, {"dims": (12, 12, 12)}))    # huge against a fine grid
    assert pairs.shape[0] >= 8 and counts[0] == counts[1]
    back, _ = _check(tiny_v, tiny_f, huge_v, huge_f, grids=({}, {"dims": (12, 12, 12)}))          # the huge one in every cell
    assert back.shape[0] == pairs.shape[0]
    # (L is the huge face's extent, the tiny faces' determinants are small against L^3: more pairs are undecided here, and
    # the cap is a statement about the main inputs; every decided pair must still agree)
    _against_reference(pairs, huge_v, huge_f, tiny_v, tiny_f, capped=False)


def test_degenerate_invalid_and_nan_input(bodies):
    av, af, bv, bf = bodies
    V = av.shape[0]
    flat = torch.tensor([[5, 5, 9], [7, 11, 11], [4, 4, 4]])
    bad = torch.tensor([[0, 1, V + 1], [-1, 2, 3], [V + 7, V + 8, V + 9]])
    faces = torch.cat([af[:100], flat, bad, af[100:]]).contiguous()
    pairs, counts = _check(av, faces, bv, bf, lanes=(1, 64))
    assert int(counts[100:106].sum()) == 0                 # faces without area and invalid faces: no pair
    back, _ = _check(bv, bf, av, faces, lanes=(8,))        # and none as faces of B
    assert not bool(((back[:, 1] >= 100) & (back[:, 1] < 106)).any())
    plain, _ = _brute(av.to(DEV), af.to(DEV), bv.to(DEV), bf.to(DEV))
    assert pairs.shape[0] == plain.shape[0] == back.shape[0]
    nan_v = av.clone()
    nan_v[::7] = float("nan")
    pairs, counts = _check(nan_v, af, bv, bf, lanes=(1, 8))
    touched = torch.isnan(nan_v[af]).any(2).any(1)
    assert touched.sum() > 100 and int(counts[touched.to(DEV)].sum()) == 0       # a face with a NaN corner crosses nothing
    all_nan = torch.full_like(av, float("nan"))
    pairs, counts = _check(all_nan, af, bv, bf, lanes=(8,))
    assert pairs.shape[0] == 0


def test_fill_with_too_small_a_capacity_stays_inside_its_buffer(bodies):
    """Guard regions around the pair buffer; capacity below the count: only slots below capacity are written, the rest is
    counted in `dropped`."""
    import ctypes as C
    from recmv import _lib as L
    from recmv import metrics
    av, af, bv, bf = (t.to(DEV).contiguous() for t in bodies)
    g = metrics.MeshGrid(bv, bf)
    pairs, counts = g.intersections(av, af)
    K, FA = pairs.shape[0], af.shape[0]
    offsets = torch.zeros(FA + 1, dtype=torch.int32, device=DEV)
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
    cap, guard = K // 2, 64
    buf = torch.full((guard + 2 * K + guard,), -7, dtype=torch.int32, device=DEV)
    cursor = torch.empty(FA, dtype=torch.int32, device=DEV)
    dropped = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    mesh = (L.ptr(av), av.shape[0], L.ptr(af), FA, L.ptr(bv), bv.shape[0], L.ptr(bf), bf.shape[0])
    grid = (C.byref(g.desc),)
    out = (L.ptr(offsets), C.c_void_p(buf.data_ptr() + 4 * guard), cap, L.ptr(cursor), L.ptr(dropped))
    for lanes in LANES:
        buf.fill_(-7)
        L.check(L.lib().recmv_mesh_intersect_grid_fill(*mesh, *grid, lanes, 0, 0, *out, L.stream_ptr(torch.device(DEV))))
        torch.cuda.synchronize()
        assert bool((buf[:guard] == -7).all()) and bool((buf[guard + 2 * cap:] == -7).all())
        written = buf[guard:guard + 2 * cap].view(-1, 2)
        kept = int((offsets[1:].clamp(max=cap) - offsets[:-1].clamp(max=cap)).sum())
        assert int((written[:, 0] >= 0).sum()) == kept == cap and int(dropped) == K - cap
    buf.fill_(-7)
    L.check(L.lib().recmv_mesh_intersect_brute(*mesh, 0, 0, None, None, *out, L.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert bool((buf[:guard] == -7).all()) and bool((buf[guard + 2 * cap:] == -7).all()) and int(dropped) == K - cap
    # offsets that disagree with what the pass finds (all zero): nothing is written, everything is reported
    buf.fill_(-7)
    offsets.zero_()
    L.check(L.lib().recmv_mesh_intersect_grid_fill(*mesh, *grid, 8, 0, 0, *out, L.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert bool((buf == -7).all()) and int(dropped) == K


def test_empty_and_tiny_meshes(bodies):
    from recmv import metrics
    av, af, bv, bf = (t.to(DEV) for t in bodies)
    g = metrics.MeshGrid(bv, bf)
    pairs, counts = g.intersections(av, af[:0])
    assert pairs.shape == (0, 2) and counts.shape == (0,)
    one = metrics.mesh_intersections(av, af[:1], bv, bf, method='grid')
    assert torch.equal(one['pairs'], metrics.mesh_intersections(av, af[:1], bv, bf, method='brute')['pairs'])
    with pytest.raises(ValueError):
        metrics.mesh_intersections(av, af[:0], bv, bf)
    with pytest.raises(ValueError):
        metrics.self_intersections(av, af, method='fast')


def _garment_over_body():
    """A body sphere and a 'garment': a slightly larger sphere, one vertex of which is pushed deep inside the body — the
    faces around it cut through the body — and one vertex pulled through the garment's far side."""
    from test_gpu_animation import _irregular_body
    body_v, body_f = _irregular_body(level=2)
    gv, gf = _irregular_body(level=2, seed=5)
    gv = (1.15 * gv).contiguous()
    k = int(gv[:, 0].argmax())
    gv[k] = 0.5 * gv[k]
    return body_v, body_f, gv, gf, k


def test_intersection_report_on_a_garment_over_a_body():
    from recmv import collide, metrics
    body_v, body_f, gv, gf, k = _garment_over_body()
    clean = (1.15 * body_v).contiguous()                   # frame 1: nothing crosses
    garments = {'shirt': (torch.stack([gv, 1.15 * _clean_garment()]).to(DEV), gf.to(DEV)),
                'coat': (torch.stack([1.4 * clean, 1.4 * clean]).to(DEV), body_f.to(DEV))}
    rep = collide.intersection_report(garments, torch.stack([body_v, body_v]).to(DEV), body_f.to(DEV))
    assert len(rep) == 2 and set(rep[0]) == {'shirt', 'coat', 'between'}
    around = int((gf == k).any(1).sum())
    want = metrics.mesh_intersections(gv.to(DEV), gf.to(DEV), body_v.to(DEV), body_f.to(DEV), method='brute')
    assert rep[0]['shirt']['body_faces'] == want['faces_a'].shape[0] >= around - 1 and rep[0]['shirt']['faces'] == gf.shape[0]
    assert set(want['faces_a'].tolist()) <= set(torch.nonzero((gf == k).any(1)).reshape(-1).tolist())
    assert rep[0]['shirt']['self_faces'] == 0 and rep[0]['coat'] == {'body_faces': 0, 'self_faces': 0, 'faces': body_f.shape[0]}
    assert rep[0]['between'] == {'shirt|coat': {'faces_a': 0, 'faces_b': 0}}
    assert rep[1]['shirt']['body_faces'] == 0 and rep[1]['between']['shirt|coat'] == {'faces_a': 0, 'faces_b': 0}


def _clean_garment():
    from test_gpu_animation import _irregular_body
    return _irregular_body(level=2, seed=5)[0]


def _write_obj(path, v, f):
    with open(path, "w") as fh:
        for p in v.tolist():
            fh.write("v %r %r %r\n" % tuple(p))
        for t in (f + 1).tolist():
            fh.write("f %d %d %d\n" % tuple(t))


def test_eval_fl_intersections_end_to_end(tmp_path):
    import eval_fl
    from recmv import metrics
    from recmv.utils import read_obj
    body_v, body_f, gv, gf, _ = _garment_over_body()
    pv, pf = pulled_sphere()
    _write_obj(tmp_path / "pred.obj", pv, pf)
    _write_obj(tmp_path / "gt.obj", gv, gf)
    _write_obj(tmp_path / "body.obj", body_v, body_f)
    base = ["--pred", str(tmp_path / "pred.obj"), "--gt", str(tmp_path / "gt.obj"), "--samples", "2000"]
    plain = eval_fl.main(base + ["--out", str(tmp_path / "plain.json")])
    full = eval_fl.main(base + ["--intersections", "--body", str(tmp_path / "body.obj"), "--out", str(tmp_path / "full.json")])
    new = {'self_intersecting_faces', 'self_intersection_ratio', 'self_intersecting_faces_gt', 'self_intersection_ratio_gt',
           'body_intersecting_faces', 'body_intersection_ratio'}
    assert set(full['pairs']['pred']) - set(plain['pairs']['pred']) == new and set(full['mean']) - set(plain['mean']) == new
    assert set(plain) == set(full) and not any('intersect' in k for k in plain['pairs']['pred'])
    assert {k: v for k, v in full['pairs']['pred'].items() if k not in new} == plain['pairs']['pred']
    assert json.load(open(tmp_path / "full.json"))['pairs']['pred'] == full['pairs']['pred']
    v, f = read_obj(str(tmp_path / "pred.obj"))
    own = metrics.self_intersections(v.to(DEV), f.to(DEV))
    got = full['pairs']['pred']
    assert got['self_intersecting_faces'] == own['faces'].shape[0] > 0 and got['self_intersection_ratio'] == own['ratio']
    assert got['self_intersecting_faces_gt'] == 0 and got['self_intersection_ratio_gt'] == 0.
    bv, bf = read_obj(str(tmp_path / "body.obj"))
    hit = metrics.mesh_intersections(v.to(DEV), f.to(DEV), bv.to(DEV), bf.to(DEV))
    assert got['body_intersecting_faces'] == hit['faces_a'].shape[0] > 0 and got['body_intersection_ratio'] == hit['ratio_a']
