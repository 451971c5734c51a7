"""ICP alignment on the GPU (csrc/icp.hip, recmv/align.py, eval_fl.py --align) against the float64 / longdouble restatement of
tests/icp_reference.py.

The sums: every entry but the count within (n + 64) 2^-53 M of the longdouble sum over the same accepted pairs, M the same sum
with every factor replaced by its magnitude and every difference u - w by |u| + |w| — the bound of recursive summation plus
at most 64 roundings per term, valid for any summation order; the count exactly.  Which pairs are accepted is known by
construction (`planted`, `border_cases`), not by running the point-triangle test again.

The iteration: maxres = max over the potato's vertices |T_est(T_applied(v)) - v|.  The float64 restatement reaches 4e-9 on
these points (the float32 rounding of the source); the device path is limited by the float32 closest point, a few eps32 of
coordinates of order 1, and has to reach 1e-5 x diagonal (about 150 ulp) within 10 iterations.  The first iterate is at
3e-2, and a wrong sign, composition order or centre misses by more than 1e-3.  Measured on an MI355X: profiles/icp_check.txt.
"""
import ctypes as C
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
import icp_reference as IR  # noqa: E402
import mesh_metrics_reference as MR  # noqa: E402

DEV = "cuda:0"
U53 = 2. ** -53
N_POINTS = 1500
BOUND = 1e-5                                               # x diagonal: the iteration's residual
POINT_AGREE = 1e-4                                         # x diagonal: device against restatement, point metric


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def accumulate(x, q, face, dist2, verts, faces, border, limit, centre, plane, sums, workspace=None):
    """recmv_icp_accumulate into the caller's `sums` (and workspace): what align.icp_sums does, on buffers the test filled."""
    from recmv import _lib as L
    lib = L.lib()
    P = x.shape[0]
    nbytes = int(lib.recmv_icp_accumulate_workspace_bytes(P))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=DEV) if workspace is None else workspace
    assert ws.numel() >= nbytes
    c = (C.c_double * 3)(*centre)
    L.check(lib.recmv_icp_accumulate(L.ptr(x), L.ptr(q), L.ptr(face), L.ptr(dist2), P, L.ptr(verts), verts.shape[0],
                                     L.ptr(faces), faces.shape[0], L.ptr(border), L.ptr(limit), c, int(plane), L.ptr(sums),
                                     L.ptr(ws), nbytes, L.stream_ptr(torch.device(DEV))), "icp_accumulate")
    return sums


def closest(x, verts, faces):
    from recmv import iso_remesh
    return iso_remesh.closest_point(x, verts, faces)


def check_sums(got, S, M, what):
    """Entry 0 exactly, every other entry within (n + 64) 2^-53 M; prints the largest error in units of the bound."""
    got = got.cpu().numpy().astype(IR.LD)
    n = float(S[0])
    assert got[0] == S[0], "%s: count %r, expected %r" % (what, got[0], S[0])
    tol = (n + 64.) * IR.LD(U53) * M
    err = np.abs(got - S)
    worst = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0.))))
    print("%s: n = %d, largest |error| / bound = %.3g" % (what, n, worst))
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, "%s: entries %s off by %s (bound %s)" % (what, bad.tolist(), err[bad], tol[bad])


@pytest.fixture(scope="module")
def small():
    """Level-2 potato (320 faces), 1000 points beside it with their correspondences from the device, and the planted pairs.
    The face list the sums see has two more faces than the one searched: a face without area and one with an index outside
    the mesh (a search never returns them; the pairs that name them are planted)."""
    v, f = IR.potato(2)
    rng = np.random.RandomState(11)
    pts, pick = MR.sample(v, f, 1000, 12)
    x = (pts + 0.03 * rng.randn(1000, 3)).astype(np.float32)
    vd, fd = dev(v), dev(f)
    face, q, d2 = closest(dev(x), vd, fd)
    face, q, d2 = face.cpu().numpy().copy(), q.cpu().numpy().copy(), d2.cpu().numpy().copy()
    assert np.all((face >= 0) & (face < len(f))) and np.all(np.isfinite(d2)) and np.all(d2 > 0)
    F = len(f)
    f_ext = np.concatenate([f, [[f[0, 0], f[0, 0], f[0, 1]], [0, 1, len(v) + 5]]]).astype(np.int64)
    limit = np.float32(np.median(d2[8:]))
    above = np.nextafter(limit, np.float32(np.inf), dtype=np.float32)
    assert above > limit
    # the planted pairs, at the front so that every P from 63 on holds them all; pair 0 is an ordinary one
    face[1] = -1
    x[2, 1] = np.nan
    d2[3] = np.inf
    d2[4], d2[5] = limit, above
    face[6], face[7] = F, F + 1
    d2[0] = d2[6] = d2[7] = np.float32(0.5) * limit        # below the threshold: the rule under test decides, not the distance
    assert d2[4] <= limit and not d2[5] <= limit           # pairs 4 and 5: the threshold's own comparison decides
    fate = {1: False, 2: False, 3: False, 7: False}        # pair 6: accepted unless the plane part is asked for
    return {'v': v, 'f': f, 'f_ext': f_ext, 'x': x, 'q': q, 'face': face, 'd2': d2, 'limit': limit, 'fate': fate,
            'centre': (0.5 * (v.min(0).astype(np.float64) + v.max(0))).tolist()}


def accepted(s, P, plane, limit):
    """The mask of the first P pairs of `small`: the planted fates, and for every other pair the threshold alone (equality
    is accepted, one ulp above is not: pairs 4 and 5)."""
    acc = np.ones(P, bool) if limit is None else (s['d2'][:P] <= limit)            # the same float32 comparison; NaN: nothing
    for i, ok in s['fate'].items():
        if i < P:
            acc[i] = ok and acc[i]
    if P > 6 and plane:
        acc[6] = False
    return acc


@pytest.mark.parametrize("P", [1, 63, 257, 1000])
def test_sums_against_the_longdouble_reference(small, P):
    s = small
    vd, fd = dev(s['v']), dev(s['f_ext'])
    x, q, face, d2 = dev(s['x'][:P]), dev(s['q'][:P]), dev(s['face'][:P]), dev(s['d2'][:P])
    for plane in (1, 0):
        for limit in (s['limit'], None):
            out = torch.full((56,), float("nan"), dtype=torch.float64, device=DEV)
            lim = None if limit is None else dev(np.array([limit], np.float32))
            accumulate(x, q, face, d2, vd, fd, None, lim, s['centre'], plane, out)
            acc = accepted(s, P, plane, limit)
            S, M = IR.sums(s['x'][:P], s['q'][:P], s['face'][:P], acc, s['v'], s['f_ext'], s['centre'], bool(plane))
            check_sums(out, S, M, "P=%d plane=%d limit=%s" % (P, plane, limit is not None))
            if not plane:
                assert bool((out[19:] == 0).all())         # exact zeros, not small numbers
            assert float(out[55]) == 0.
    if P >= 63:
        assert accepted(s, P, 1, s['limit'])[:8].tolist() == [True, False, False, False, True, False, False, False]
        assert accepted(s, P, 0, None)[:8].tolist() == [True, False, False, False, True, True, True, False]
    # nothing accepted — a NaN threshold — gives 56 zeros, from a buffer that held NaN
    out = torch.full((56,), float("nan"), dtype=torch.float64, device=DEV)
    accumulate(x, q, face, d2, vd, fd, None, dev(np.array([np.nan], np.float32)), s['centre'], 1, out)
    assert bool((out == 0).all())


def test_the_wrapper_gives_the_same_sums_and_p_zero_gives_zeros(small):
    from recmv import align
    s = small
    vd, fd = dev(s['v']), dev(s['f_ext'])
    x, q, face, d2 = dev(s['x']), dev(s['q']), dev(s['face']), dev(s['d2'])
    raw = accumulate(x, q, face, d2, vd, fd, None, dev(np.array([s['limit']], np.float32)), s['centre'], 1,
                     torch.empty(56, dtype=torch.float64, device=DEV))
    for limit in (float(s['limit']), dev(np.array([s['limit']], np.float32))):    # a number or a device scalar
        got = align.icp_sums(x, q, face, d2, vd, fd, max_dist2=limit, centre=s['centre'], plane=True)
        assert got.dtype == torch.float64 and torch.equal(got.view(torch.int64), raw.view(torch.int64))
    out = torch.full((56,), float("nan"), dtype=torch.float64, device=DEV)
    accumulate(x[:0], q[:0], face[:0], d2[:0], vd, fd, None, None, s['centre'], 1, out)
    assert bool((out == 0).all())
    assert bool((align.icp_sums(x[:0], q[:0], face[:0], d2[:0], vd, fd) == 0).all())


def border_cases(v, f_open):
    """Points whose fate under the border rule follows from how they are built, on an open mesh: (points float32 [N,3],
    accepted [N] bool, kind [N]: 0 beyond the midpoint of a border edge, 1 beyond a border corner, 2 over a border face).
      0: the midpoint of a border edge, moved by a quarter of the edge's length away from the face in the face's plane (at a
         right angle to the edge) and a twentieth along the face normal: the nearest point of the face is on that edge, and
         of the faces around it none comes nearer than the edge they would have to reach across.
      1: a border vertex at which the faces of the mesh span less than 120 degrees, moved by a quarter of the shortest edge
         there against the mean direction of those faces' edges: the point lies behind both border edges, the vertex is the
         nearest point of every face that has it.
      2: a point of a border face with every barycentric weight >= 0.15, moved by a twentieth of the shortest edge along the
         face normal: its nearest point is the point it was moved from, inside the face."""
    v = np.asarray(v, np.float64)
    flags = IR.border_flags(f_open, len(v))
    rng = np.random.RandomState(21)
    pts, ok, kind = [], [], []
    normal = np.cross(v[f_open[:, 1]] - v[f_open[:, 0]], v[f_open[:, 2]] - v[f_open[:, 0]])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    for k, face in enumerate(f_open):
        for bit, (i, j, o) in enumerate(((0, 1, 2), (0, 2, 1), (1, 2, 0))):
            if not (flags[k] >> bit) & 1:
                continue
            a, b, c = v[face[i]], v[face[j]], v[face[o]]
            mid, t = 0.5 * (a + b), (b - a) / np.linalg.norm(b - a)
            out = (mid - c) - ((mid - c) @ t) * t
            out /= np.linalg.norm(out)
            L = np.linalg.norm(b - a)
            pts.append(mid + 0.25 * L * out + 0.05 * L * normal[k])
            ok.append(False)
            kind.append(0)
        if flags[k] & 7:
            w = 0.15 + 0.55 * rng.dirichlet([1., 1., 1.])
            tri = v[face]
            L = min(np.linalg.norm(tri[i] - tri[(i + 1) % 3]) for i in range(3))
            pts.append(w @ tri + 0.05 * L * normal[k])
            ok.append(True)
            kind.append(2)
    on_border = sorted({int(face[c]) for k, face in enumerate(f_open) for c in range(3) if (flags[k] >> (3 + c)) & 1})
    for vi in on_border:
        angle, mean, shortest, nrm = 0., np.zeros(3), np.inf, np.zeros(3)
        for k, face in enumerate(f_open):
            if vi not in face:
                continue
            c = list(face).index(vi)
            e1, e2 = v[face[(c + 1) % 3]] - v[vi], v[face[(c + 2) % 3]] - v[vi]
            angle += math.acos(np.clip(e1 @ e2 / np.linalg.norm(e1) / np.linalg.norm(e2), -1., 1.))
            mean += e1 / np.linalg.norm(e1) + e2 / np.linalg.norm(e2)
            shortest = min(shortest, np.linalg.norm(e1), np.linalg.norm(e2))
            nrm += normal[k]
        if angle < math.radians(120.):
            pts.append(v[vi] - 0.25 * shortest * mean / np.linalg.norm(mean) + 0.05 * shortest * nrm / np.linalg.norm(nrm))
            ok.append(False)
            kind.append(1)
    return np.array(pts).astype(np.float32), np.array(ok), np.array(kind)


def test_the_border_rule_on_an_open_mesh():
    from recmv import align
    v, f = IR.potato(2)
    f_open = IR.open_copy(v, f)
    pts, ok, kind = border_cases(v, f_open)
    print("open level-2 potato: %d of %d faces; %d points beyond an edge, %d beyond a corner, %d over a border face" % (
        len(f_open), len(f), (kind == 0).sum(), (kind == 1).sum(), (kind == 2).sum()))
    assert (kind == 0).sum() >= 20 and (kind == 1).sum() >= 3 and (kind == 2).sum() >= 20
    vd, fd = dev(v), dev(f_open)
    x = dev(pts)
    face, q, d2 = closest(x, vd, fd)
    border = align.border_flags(fd, len(v))
    assert border.is_cuda and np.array_equal(border.cpu().numpy(), IR.border_flags(f_open, len(v)))
    centre = (0.5 * (v.min(0).astype(np.float64) + v.max(0))).tolist()
    for plane in (True, False):
        got = align.icp_sums(x, q, face, d2, vd, fd, border=border, centre=centre, plane=plane)
        S, M = IR.sums(pts, q.cpu().numpy(), face.cpu().numpy(), ok, v, f_open, centre, plane)
        check_sums(got, S, M, "border rule, plane=%d" % plane)
        every = align.icp_sums(x, q, face, d2, vd, fd, border=None, centre=centre, plane=plane)
        assert float(every[0]) == len(pts)                 # without the flags nobody is rejected


def test_the_same_call_gives_the_same_bits(small):
    s = small
    vd, fd = dev(s['v']), dev(s['f_ext'])
    x, q, face, d2 = dev(s['x']), dev(s['q']), dev(s['face']), dev(s['d2'])
    lim = dev(np.array([s['limit']], np.float32))
    from recmv import _lib as L
    nbytes = int(L.lib().recmv_icp_accumulate_workspace_bytes(1000))
    assert nbytes == 4 * 56 * 8                            # several slabs
    for plane in (1, 0):
        a = accumulate(x, q, face, d2, vd, fd, None, lim, s['centre'], plane,
                       torch.full((56,), float("nan"), dtype=torch.float64, device=DEV),
                       torch.full((nbytes,), 0xff, dtype=torch.uint8, device=DEV))
        b = accumulate(x, q, face, d2, vd, fd, None, lim, s['centre'], plane,
                       torch.full((56,), 1e300, dtype=torch.float64, device=DEV),
                       torch.zeros(nbytes, dtype=torch.uint8, device=DEV))
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        assert float(a[0]) > 400


@pytest.fixture(scope="module")
def scene():
    """Level-3 potato (1280 faces), 1500 samples of it, and per motion the samples and the vertices under it (float32)."""
    v, f = IR.potato(3)
    pts, _ = MR.sample(v, f, N_POINTS, 7)
    out = {'v': v, 'f': f, 'diag': IR.diagonal(v), 'f_open': IR.open_copy(v, f)}
    for mode in ('rigid', 'similarity'):
        T = IR.applied(mode == 'similarity')
        out[mode] = {'T': T, 'points': IR.transform_points(T, pts).astype(np.float32),
                     'verts': IR.transform_points(T, v).astype(np.float32)}
    assert abs(out['diag'] - 1.27) < 0.01 and len(out['f_open']) == 847
    return out


def estimate(r):
    return r['scale'], np.array(r['R']), np.array(r['t'])


@pytest.mark.parametrize("method", ["brute", "grid"])
@pytest.mark.parametrize("mode", ["rigid", "similarity"])
def test_the_plane_metric_recovers_the_motion(scene, mode, method):
    from recmv import align
    m = scene[mode]
    r = align.icp(dev(m['verts']), dev(scene['f']), dev(scene['v']), dev(scene['f']), mode=mode, metric='plane',
                  points=dev(m['points']), iters=10, method=method)
    res = IR.maxres(estimate(r), m['T'], scene['v'])
    print("plane, %s, %s: maxres %.3e = %.3e x diagonal after %d steps (rms %.3e -> %.3e, %d pairs)" % (
        mode, method, res, res / scene['diag'], r['iterations'], r['rms_before'], r['rms_after'], r['pairs']))
    assert r['iterations'] <= 10 and r['points'] == N_POINTS and r['pairs'] == N_POINTS and 'reason' not in r
    assert len(r['rms']) == r['iterations'] + 1 and r['rms'][0] == r['rms_before'] and r['rms'][-1] == r['rms_after']
    assert res <= BOUND * scene['diag']
    R = np.array(r['R'])
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0
    if mode == 'rigid':
        assert r['scale'] == 1.
    else:
        assert abs(r['scale'] - 1. / IR.SCALE) <= 1e-5
    M = np.array(r['matrix'])
    assert np.abs(M[:3, :3] - r['scale'] * R).max() <= 1e-15 and M[:3, 3].tolist() == r['t'] and M[3].tolist() == [0, 0, 0, 1]
    moved = align.apply(r, dev(m['verts'])).cpu().numpy()
    assert moved.dtype == np.float32 and np.abs(moved - scene['v']).max() <= 2 * BOUND * scene['diag']
    json.dumps(r)                                          # python numbers throughout


def test_an_open_target_needs_the_border_rule(scene):
    from recmv import align
    m = scene['rigid']
    args = (dev(m['verts']), dev(scene['f']), dev(scene['v']), dev(scene['f_open']))
    beyond = float((IR.transform_points((1., np.eye(3), np.zeros(3)), MR.sample(scene['v'], scene['f'], N_POINTS, 7)[0])[:, 0] >= 0.2).mean())
    r = align.icp(*args, mode='rigid', metric='plane', points=dev(m['points']), iters=10, reject_border=True, method='brute')
    res = IR.maxres(estimate(r), m['T'], scene['v'])
    print("open target (%.0f %% of the samples beyond the cut), border rule: maxres %.3e = %.3e x diagonal, %d of %d pairs" % (
        100 * beyond, res, res / scene['diag'], r['pairs'], r['points']))
    assert res <= BOUND * scene['diag'] and r['pairs'] >= N_POINTS // 2
    r = align.icp(*args, mode='rigid', metric='plane', points=dev(m['points']), iters=10, reject_border=False, trim=1.,
                  method='brute')
    res = IR.maxres(estimate(r), m['T'], scene['v'])
    print("open target, no border rule: maxres %.3e, %d pairs" % (res, r['pairs']))
    assert res >= 1e-2 and r['pairs'] == N_POINTS


def test_trimming_a_distance_limit_an_initial_guess_and_too_few_pairs(scene):
    from recmv import align
    m = scene['similarity']
    args = (dev(m['verts']), dev(scene['f']), dev(scene['v']), dev(scene['f']))
    kw = dict(mode='similarity', metric='plane', points=dev(m['points']), iters=10, method='brute')
    # half of the pairs, by a threshold found on the device: ceil(0.5 P) of them, more only where distances tie
    r = align.icp(*args, trim=0.5, max_dist=0.5, **kw)
    res = IR.maxres(estimate(r), m['T'], scene['v'])
    print("trim 0.5: maxres %.3e x diagonal, %d of %d pairs" % (res / scene['diag'], r['pairs'], r['points']))
    assert N_POINTS // 2 <= r['pairs'] <= N_POINTS // 2 + 8 and res <= BOUND * scene['diag']
    # a limit below every distance: nothing to fit, the transform stays the initial one and the result says why
    none = align.icp(*args, max_dist=1e-6, **kw)
    assert none['pairs'] < 3 and not none['converged'] and none['iterations'] == 0 and 'pairs accepted' in none['reason']
    assert none['scale'] == 1. and none['R'] == [[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]] and none['t'] == [0., 0., 0.]
    # the same limit combined with the trim threshold by minimum
    assert align.icp(*args, trim=0.5, max_dist=1e-6, **kw)['pairs'] < 3
    # from the solution: one search, no step worth taking, the transform kept (a result or a 4x4 matrix as the guess)
    for init in (r, r['matrix']):
        again = align.icp(*args, init=init, **dict(kw, iters=0))
        assert again['iterations'] == 0 and len(again['rms']) == 1 and again['rms_before'] <= 1e-6
        assert np.abs(np.array(again['matrix']) - np.array(r['matrix'])).max() <= 1e-12
    # the seeded samples of the source mesh, and its vertices
    by_samples = align.icp(*args[:2], *args[2:], mode='similarity', samples=2000, seed=3, iters=10, method='brute')
    by_verts = align.icp(*args[:2], *args[2:], mode='similarity', samples=0, iters=10, method='brute')
    assert by_samples['points'] == 2000 and by_verts['points'] == len(scene['v'])
    assert by_samples == align.icp(*args[:2], *args[2:], mode='similarity', samples=2000, seed=3, iters=10, method='brute')
    for fit in (by_samples, by_verts):
        assert IR.maxres(estimate(fit), m['T'], scene['v']) <= BOUND * scene['diag']


def test_the_point_metric_follows_the_restatement(scene):
    from recmv import align
    m = scene['rigid']
    r = align.icp(dev(m['verts']), dev(scene['f']), dev(scene['v']), dev(scene['f']), mode='rigid', metric='point',
                  points=dev(m['points']), iters=10, tol=0., method='brute')
    ref = IR.icp(m['points'], scene['v'], scene['f'], mode='rigid', metric='point', iters=10)
    assert r['iterations'] == 10 and len(r['rms']) == 11 and not r['converged']
    for a, b in zip(r['rms'][:-1], r['rms'][1:]):
        assert b <= a * (1 + 1e-5)
    src = m['verts'].astype(np.float64)
    diff = float(np.linalg.norm(IR.transform_points(estimate(r), src) - IR.transform_points(ref['T'], src), axis=1).max())
    print("point metric, 10 steps: device against restatement %.3e = %.3e x diagonal; rms %.4e -> %.4e (restatement %.4e -> %.4e)" % (
        diff, diff / scene['diag'], r['rms'][0], r['rms'][-1], ref['rms'][0], ref['rms'][-1]))
    assert diff <= POINT_AGREE * scene['diag']
    assert r['rms'][-1] < 0.5 * r['rms'][0]


def write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(r) for r in np.asarray(v, np.float64).tolist()))
        fh.write("".join("f %d %d %d\n" % tuple(r) for r in (np.asarray(f) + 1).tolist()))


def test_eval_fl_aligns_before_it_measures(tmp_path):
    import eval_fl
    v, f = IR.potato(2)
    T = IR.applied(True)
    moved = IR.transform_points(T, v).astype(np.float32)
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    pred.mkdir()
    gt.mkdir()
    write_obj(pred / "a.obj", moved, f)
    write_obj(gt / "a.obj", v, f)
    common = ["--samples", "4000", "--method", "brute"]
    out = tmp_path / "aligned"
    res = eval_fl.main(["--pred", str(pred / "a.obj"), "--gt", str(gt / "a.obj"), "--align", "similarity", "--align-out", str(out),
                        "--out", str(tmp_path / "m.json")] + common)
    rec = res['alignment']['a']
    print("eval_fl --align similarity: chamfer_l1 %.3e, scale %.7f (1 / 1.08 = %.7f), %d steps" % (
        res['pairs']['a']['chamfer_l1'], rec['scale'], 1 / IR.SCALE, rec['iterations']))
    assert res['pairs']['a']['chamfer_l1'] < 1e-4 and abs(rec['scale'] - 1. / IR.SCALE) <= 1e-4
    assert sorted(rec) == ['R', 'converged', 'iterations', 'pairs', 'rms_after', 'rms_before', 'scale', 't']
    assert res['align'] == {'mode': 'similarity', 'metric': 'plane', 'trim': 1.0, 'iters': 50, 'from': 'each'}
    assert 'alignment' not in res['pairs']['a'] and 'scale' in res and all(isinstance(x, float) for x in res['mean'].values())
    saved = json.loads((tmp_path / "m.json").read_text())
    assert saved['alignment']['a']['scale'] == rec['scale']
    from recmv.utils import read_obj
    av, af = read_obj(str(out / "a.obj"))
    assert torch.equal(af, torch.from_numpy(f)) and float((av - torch.from_numpy(v)).abs().max()) < 1e-4
    plain = eval_fl.main(["--pred", str(pred / "a.obj"), "--gt", str(gt / "a.obj"), "--align", "none"] + common)
    default = eval_fl.main(["--pred", str(pred / "a.obj"), "--gt", str(gt / "a.obj")] + common)
    assert plain['pairs']['a']['chamfer_l1'] > 1e-2 and 'alignment' not in plain and 'align' not in plain
    assert plain == default and sorted(plain) == ['mean', 'method', 'pairs', 'samples', 'scale', 'seed', 'thresholds',
                                                  'unmatched_gt', 'unmatched_pred']
    # two pairs, one transform: the second ground truth is shifted, so a fit of its own would differ
    write_obj(pred / "b.obj", moved, f)
    write_obj(gt / "b.obj", v + np.float32(0.05), f)
    common += ["--align-iters", "12"]
    first = eval_fl.main(["--pred", str(pred), "--gt", str(gt), "--align", "similarity", "--align-from", "first"] + common)
    assert first['alignment']['b'] == first['alignment']['a'] and first['align']['from'] == 'first'
    assert first['pairs']['a']['chamfer_l1'] < 1e-4 and first['pairs']['b']['chamfer_l1'] > 1e-2
    each = eval_fl.main(["--pred", str(pred), "--gt", str(gt), "--align", "similarity"] + common)
    assert each['alignment']['b'] != each['alignment']['a'] and each['pairs']['b']['chamfer_l1'] < 1e-4


def test_icp_optimizer_fitting_moves_the_source_onto_the_target():
    from recmv.engineer.optimizer import ICP_Optimizer
    from test_icp_cpu import _Boundary
    rng = np.random.RandomState(4)
    ring = lambda c, r, n: np.stack([c[0] + r * np.cos(np.linspace(0, 2 * np.pi, n, endpoint=False)),   # noqa: E731
                                     c[1] + 0.6 * r * np.sin(np.linspace(0, 2 * np.pi, n, endpoint=False)),
                                     np.full(n, c[2])], 1)
    target = {'neck': ring((0., 0., 0.5), 0.1, 60), 'hem': ring((0.02, 0.01, -0.3), 0.25, 90)}
    T = (1., IR.rotation([0.2, 1., 0.1], math.radians(3.)), np.array([0.01, -0.005, 0.008]))
    inv = lambda x: (x - T[2]) @ T[1]                      # noqa: E731  (T^-1: the source that T brings onto the target)
    source = {k: inv(p) for k, p in target.items()}
    a = _Boundary({k: dev(p, torch.float32) for k, p in source.items()})
    b = _Boundary({k: dev(p, torch.float32) for k, p in target.items()})
    loss = ICP_Optimizer(0)(smpl_slice=a, target_polygon=b)
    R, t = a.moved
    assert R.is_cuda and R.dtype == torch.float32 and R.shape == (3, 3) and t.shape == (1, 3)
    # the same step in float64: nearest neighbours by a distance matrix, the restatement's solver on those pairs
    S = np.concatenate([source[k] for k in target]).astype(np.float32).astype(np.float64)
    W = np.concatenate([target[k] for k in target]).astype(np.float32).astype(np.float64)
    near = ((S[:, None, :] - W[None, :, :]) ** 2).sum(-1).argmin(1)
    _, R_ref, t_ref = IR.solve_point(IR.pair_sums(S, W[near]), False)
    after = float(((IR.transform_points((1., R_ref, t_ref), S) - W[near]) ** 2).sum())
    before = float(((S - W) ** 2).sum())
    print("ICP_Optimizer.fitting: sum of squares %.3e -> %.3e (float64: %.3e)" % (before, float(loss), after))
    assert np.abs(R.cpu().numpy() - R_ref).max() <= 1e-5 and np.abs(t.cpu().numpy()[0] - t_ref).max() <= 1e-5
    assert abs(float(loss) - after) <= 1e-3 * after and after < before   # the best motion for pairs no farther apart than the given ones
