"""Segment queries without a GPU: the float64 restatement (tests/segment_mesh_reference.py) on hand cases, the new C entry
points (declared, exported, argument errors before any HIP call), the refusal of CPU tensors, the commands' new flag, the host
build of the grid kernel under the sanitizers, and the decidability of the GPU test's inputs.

A (segment, face) pair is DECIDED when its margin (segment_mesh_reference's: the smallest deciding |determinant| / L^3)
exceeds 20 eps32 — csrc/tri_tri.h's derived bound on a determinant's f32 error, BOUND(L) = 20 eps32 L^3 (derivation repeated in
tests/test_mesh_intersect_cpu.py) — so the f32 kernels take every deciding sign as the reference does.  A segment's hit set and
count are decided when all its tested pairs are; its first hit when the first hit's pair is decided, no other hit's t lies
within the sum of the two t tolerances (segment_mesh_reference.T_TOL: 2 * 20 eps32 L^3 / |sp - sq| + 2 eps32, derived there)
and no undecided pair could be reported in front of it (segment_mesh_reference.segment_hits).
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import host_check  # noqa: E402
import segment_mesh_reference as SR  # noqa: E402

EPS32 = SR.EPS32
BOUND_C = SR.BOUND_C                                       # csrc/tri_tri.h: a determinant errs by at most 20 eps32 L^3
UNDECIDED_CAP = 0.01                                       # of the hitting segments
MIN_HITTING = 500
BAND_CAP = 0.20                                            # of the inside-test points
RADIUS = 0.5


def body():
    from test_gpu_animation import _irregular_body
    return _irregular_body(level=3)                        # 1280 faces, radius 0.5 +- 9 %


def vertex_normals(v, f):
    """Area-weighted unit vertex normals in torch on the host (the test's own; any direction would do for a cast)."""
    tri = v[f]
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1)
    out = torch.zeros_like(v)
    for k in range(3):
        out.index_add_(0, f[:, k], n)
    return out / out.norm(dim=1, keepdim=True)


def random_segments(v, n=4096, seed=3):
    """Endpoints uniform in the bounding box scaled 1.5 about its centre.  (Of the seeds 1 .. 15 the reference alone leaves
    0.2 % .. 1.1 % of the hitting segments undecided, silhouette grazes mostly; seed 11 breaks the cap, 3 does not.)"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = v.amin(0), v.amax(0)
    c, e = 0.5 * (lo + hi), 0.75 * (hi - lo)
    pq = c + e * (2 * torch.rand(2, n, 3, generator=g) - 1)
    return pq[0].float().contiguous(), pq[1].float().contiguous()


def normal_casts(v, f, length=0.2 * RADIUS):
    """The +-normal casts from the vertices of the copy scaled 0.9 and shifted 0.3 radius (the crossing-faces test's second body)."""
    w = (0.9 * v + torch.tensor([0.3 * RADIUS, 0., 0.])).float().contiguous()
    n = vertex_normals(w, f)
    p = torch.cat([w, w])
    q = torch.cat([w + length * n, w - length * n]).float()
    return p.contiguous(), q.contiguous(), w


def inside_points(v, n=2000, seed=5):
    """Uniform in the bounding box scaled 1.5 about its centre (the box of the random segments)."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = v.amin(0), v.amax(0)
    c, e = 0.5 * (lo + hi), 0.75 * (hi - lo)
    return (c + e * (2 * torch.rand(n, 3, generator=g) - 1)).float().contiguous()


def radial_band(v, f):
    """[r_in, r_out]: every point of the surface has a distance to the origin in it.  A point of a face is a convex combination
    of its corners, so its distance is at most the largest corner radius r_max; and at least r_min - sag with sag the largest
    sagitta of a face against the sphere through its corners' radius: for a chord of length e on a sphere of radius r the
    midpoint lies r - sqrt(r^2 - e^2 / 4) below it; a point of a face is no farther from its nearest corner than the longest
    edge e_max, which bounds the drop by r_max - sqrt(r_max^2 - e_max^2) (the whole edge as half chord: generous)."""
    r = v.double().norm(dim=1)
    tri = v.double()[f]
    e_max = float(max((tri[:, i] - tri[:, (i + 1) % 3]).norm(dim=1).max() for i in range(3)))
    r_min, r_max = float(r.min()), float(r.max())
    sag = r_max - (r_max ** 2 - e_max ** 2) ** 0.5
    return r_min - sag, r_max


def reach_of(points, v):
    """recmv.metrics.points_inside's segment length, in float64 (any length beyond the box would do for the reference)."""
    lo, hi = v.double().amin(0), v.double().amax(0)
    return (1.5 * (hi - lo).norm() + (points.double() - 0.5 * (lo + hi)).norm(dim=1)).numpy()


@pytest.fixture(scope="module")
def references():
    """The float64 answers for the GPU test's two segment sets, computed once."""
    v, f = body()
    p, q = random_segments(v)
    cp, cq, _ = normal_casts(v, f)
    return {'random': SR.segment_hits(p.numpy(), q.numpy(), v.numpy(), f.numpy()),
            'casts': SR.segment_hits(cp.numpy(), cq.numpy(), v.numpy(), f.numpy())}


def _one(p, q, tri):
    hit, t, margin, tol, _ = SR.seg_tri(np.array([p], float), np.array([q], float), np.array([tri], float))
    return bool(hit[0]), float(t[0]), float(margin[0])


FLAT = [[-1, -1, 0], [1, -1, 0], [0, 1, 0]]                # in z = 0, the origin inside


def test_reference_on_hand_cases():
    hit, t, margin = _one([0.1, -0.2, 1], [0.1, -0.2, -3], FLAT)
    assert hit and t == 0.25 and margin > 1e-3             # a clean hit with its t
    hit, t, _ = _one([0.1, -0.2, -3], [0.1, -0.2, 1], FLAT)
    assert hit and t == 0.75                               # the other way round
    assert not _one([2, 2, 1], [2, 2, -1], FLAT)[0]        # beside the triangle
    assert not _one([0.1, -0.2, 2], [0.1, -0.2, 0.5], FLAT)[0]                     # ends before the plane
    assert not _one([0.1, -0.2, 1], [0.1, -0.2, 0], FLAT)[0]                       # an endpoint exactly in the plane
    assert not _one([0.1, -0.2, 0], [0.1, -0.2, -1], FLAT)[0]
    assert not _one([0, 1, 1], [0, 1, -1], FLAT)[0]        # through a vertex
    assert not _one([-1, -1, 0.5], [1, -1, -0.5], FLAT)[0]                         # crosses the plane on the edge ab
    assert not _one([-1, -1, 0], [1, -1, 0], FLAT)[0]      # along an edge
    assert not _one([-0.5, -0.5, 0], [0.5, 0, 0], FLAT)[0]                         # in the plane, through the inside
    assert not _one([0.1, -0.2, 1], [0.1, -0.2, 1], FLAT)[0]                       # no length
    assert not _one([0.1, -0.2, 0], [0.1, -0.2, 0], FLAT)[0]
    assert not _one([0.1, 0, 1], [0.1, 0, -1], [[0, 0, 0], [0, 0, 0], [1, 1, 0]])[0]            # a repeated corner
    assert not _one([0, 0.5, 1], [0, 0.5, -1], [[0, 0, 0], [0, 0.5, 0], [0, 1, 0]])[0]          # three corners in a line
    nan = float("nan")
    assert not _one([0.1, nan, 1], [0.1, -0.2, -3], FLAT)[0]
    assert not _one([0.1, -0.2, 1], [0.1, -0.2, -3], [[-1, -1, 0], [1, nan, 0], [0, 1, 0]])[0]
    assert not _one([0.1, -0.2, 1], [0.1, float("inf"), -3], FLAT)[0]


def test_reference_mesh_level():
    """An out-of-range face index is hit by nothing; of two faces at equal t the lowest id wins; counts."""
    v = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0], [-1, -1, 0], [1, -1, 0], [0, 1, 0], [0, 0, -1], [1, 0, -1], [0, 1, -1]], float)
    f = np.array([[3, 4, 5], [0, 1, 2], [0, 1, 99], [-1, 1, 2], [6, 7, 8]])
    p = np.array([[0.2, 0.2, 1], [0.2, 0.2, 1], [5, 5, 1]], float)
    q = np.array([[0.2, 0.2, -3], [0.2, 0.2, -0.5], [5, 5, -1]], float)
    r = SR.segment_hits(p, q, v, f)
    assert r['count'].tolist() == [3, 2, 0] and r['face'].tolist() == [0, 0, -1]
    assert r['t'][0] == 0.25 and np.isnan(r['t'][2])
    assert not r['first_decided'][0] and r['pairs_decided'][0]                     # two faces at one t: the tie is not "decided"
    assert set(r['cand'][:, 1]) <= {0, 1, 4}               # the invalid faces are never tested


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in ("recmv_segment_mesh_brute", "recmv_segment_mesh_grid"):
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION == 11


def test_argument_errors_do_not_need_a_gpu():
    from recmv import _lib
    from test_mesh_metrics_cpu import grid_desc
    lib = _lib.lib()
    one = C.c_void_p(16)                                   # a non-NULL pointer that is never followed
    err = lib.recmv_last_error

    def brute(*, seg=(one, one, 4), mesh=(one, 3, one, 1), out=(one, one, one)):
        return lib.recmv_segment_mesh_brute(*seg, *mesh, *out, None)
    assert brute(seg=(one, one, -1)) == -1 and b"S=-1" in err()
    assert brute(mesh=(one, -3, one, 1)) == -1 and b"V=-3" in err()
    assert brute(mesh=(one, 3, one, -2)) == -1 and b"F=-2" in err()
    assert brute(seg=(None, one, 4)) == -1 and b"NULL segment" in err()
    assert brute(seg=(one, None, 4)) == -1 and b"NULL segment" in err()
    assert brute(mesh=(one, 3, None, 1)) == -1 and b"NULL pointer of the mesh" in err()
    assert brute(mesh=(None, 3, one, 1)) == -1 and b"NULL pointer of the mesh" in err()
    assert brute(out=(None, one, one)) == -1 and b"NULL output" in err()
    assert brute(out=(one, None, one)) == -1 and b"NULL output" in err()
    assert brute(out=(one, one, None)) == -1 and b"NULL count" in err()
    assert brute(mesh=(one, 3, one, 1 << 31)) == -1 and b"faces" in err()
    assert brute(seg=(None, None, 0), out=(None, None, None)) == 0                 # S = 0: a no-op

    def grid(*, seg=(one, one, 4), mesh=(one, 3, one, 1), null=False, lanes=1, want=0, out=(one, one, None), **desc):
        g = None if null else C.byref(grid_desc(**desc))
        return lib.recmv_segment_mesh_grid(*seg, *mesh, g, lanes, want, *out, None)
    assert grid(seg=(one, one, -5)) == -1 and b"S=-5" in err()
    assert grid(mesh=(one, 3, one, -2)) == -1 and b"F=-2" in err()
    assert grid(seg=(None, one, 4)) == -1 and b"NULL segment" in err()
    assert grid(out=(None, one, None)) == -1 and b"NULL output" in err()
    assert grid(want=1) == -1 and b"want_count=1 needs count" in err()
    assert grid(want=2, out=(one, one, one)) == -1 and b"want_count=2" in err()
    assert grid(lanes=3) == -1 and b"lanes=3" in err()
    assert grid(lanes=0) == -1 and b"lanes" in err()
    assert grid(h=0.) == -1 and b"cell size" in err()
    assert grid(h=float("nan")) == -1 and b"cell size" in err()
    assert grid(h=float("inf")) == -1 and b"cell size" in err()
    assert grid(null=True) == -1 and b"grid" in err()
    assert grid(dims=(2, 0, 2)) == -1 and b"dims=(2,0,2)" in err()
    assert grid(dims=(1 << 20, 1 << 20, 1)) == -1 and b"cells" in err()
    assert grid(n_entries=-1) == -1 and b"entries=-1" in err()
    assert grid(offsets=None) == -1 and b"NULL pointer of the grid" in err()
    assert grid(entries=None) == -1 and b"NULL pointer of the grid" in err()
    assert grid(seg=(None, None, 0), out=(None, None, None)) == 0


def test_segment_queries_refuse_cpu_tensors_and_bad_arguments():
    from recmv import collide, metrics
    from recmv.engineer.optimizer import Surface_Intesection
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])
    f = torch.tensor([[0, 1, 2]])
    p = torch.zeros(2, 3)
    with pytest.raises(RuntimeError):
        metrics.segment_hits(p, p, v, f)
    with pytest.raises(RuntimeError):
        metrics.segment_hits(p, p, v, f, method='brute', count=True)
    with pytest.raises(RuntimeError):
        metrics.points_inside(p, v, f)
    with pytest.raises(RuntimeError):
        metrics.penetration(p, v, f)
    with pytest.raises(RuntimeError):
        Surface_Intesection()(smpl_slice=(v, f), cano_meshes=(v, f))
    with pytest.raises(RuntimeError):
        collide.intersection_report({'shirt': (v[None], f)}, v[None], f, penetration=True)
    with pytest.raises(ValueError):
        metrics.use_grid_for_segments('fast', 1, 1)
    with pytest.raises(ValueError):
        Surface_Intesection(max_dist=0.)
    with pytest.raises(ValueError):
        Surface_Intesection(method='fast')
    assert metrics.use_grid_for_segments('grid', 1, 1) and not metrics.use_grid_for_segments('brute', 10 ** 6, 10 ** 6)
    assert metrics.use_grid_for_segments('auto', 1, metrics.AUTO_GRID_MIN_SEGMENT_TESTS)
    assert not metrics.use_grid_for_segments('auto', 1, metrics.AUTO_GRID_MIN_SEGMENT_TESTS - 1)
    assert metrics.SEGMENT_LANES in (1, 8, 64)
    d = torch.tensor(metrics.INSIDE_DIRECTIONS, dtype=torch.float64)
    assert d.shape == (3, 3) and torch.allclose(d.norm(dim=1), torch.ones(3, dtype=torch.float64), atol=1e-12)
    assert float(d.abs().max()) < 0.9 and float(d.abs().min()) > 0.2               # none along an axis or in a coordinate plane
    for i in range(3):
        for j in range(i + 1, 3):
            assert abs(float(d[i] @ d[j])) < 0.5           # mutually far from parallel
    import recmv.engineer.optimizer as O
    assert O.Surface_Intesection is Surface_Intesection and Surface_Intesection().name == 'Surface_Intesection'


def test_the_commands_carry_the_new_flag_and_it_defaults_to_off(tmp_path):
    import eval_fl
    import infer_fl_animation
    me = str(HERE / "segment_mesh_reference.py")           # any existing file: the usage errors come before it is read
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g"])
    assert a.penetration is False and a.intersections is False and a.body is None
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g", "--intersections", "--body", "b", "--penetration"])
    assert a.penetration is True
    with pytest.raises(SystemExit):                        # before any device work
        eval_fl.main(["--pred", me, "--gt", me, "--penetration"])
    with pytest.raises(SystemExit):
        eval_fl.main(["--pred", me, "--gt", me, "--intersections", "--penetration"])
    a = infer_fl_animation.build_parser().parse_args(["--data-type", "snug"])
    assert a.penetration is False and a.report_intersections is False
    a = infer_fl_animation.build_parser().parse_args(["--data-type", "snug", "--report-intersections", "--penetration"])
    assert a.penetration and a.report_intersections
    with pytest.raises(SystemExit):
        infer_fl_animation.main(["--data-type", "snug", "--motion", "m.npz", "--penetration"])


def test_host_build_of_the_grid_kernel_equals_the_brute_loop(tmp_path):
    """tools/segment_mesh_host_check: csrc/segment_mesh.hip's one-lane grid kernel, both modes, compiled for the CPU under the
    address and undefined-behaviour sanitizers, against a loop over seg_face_hit on nine meshes and grids, and on two
    families of scenes the f32 determinants cannot decide: a face that holds the segment's line behind a clean hit (the first
    hit with the early stop must still be the brute loop's), and tiny segments in the plane of a huge face far away (the
    program fails unless the box gate alone refused pairs there that the bare predicate accepts)."""
    r = host_check.run("segment_mesh", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(" 0 mismatches") == 11, r.stdout + r.stderr
    for name in ("single cell", "column 1x1x17", "two faces 40^3", "grid does not cover", "planar", "a face in every cell",
                 "icosphere 11^3", "coplanar face behind a hit", "tiny segments far from a huge face"):
        assert name in r.stdout


def test_the_gpu_tests_segments_are_decidable(references):
    """The float64 reference alone: at least 500 segments hit over the two segment sets, and in each set at most 1 % of the
    hitting segments are undecided."""
    total = 0
    for name, r in references.items():
        hitting = r['count'] > 0
        und = hitting & ~r['first_decided']
        und_pairs = int((~(r['margin'] > BOUND_C * EPS32)).sum())
        print("%s: %d segments, %d hit (%d more than one face), %d tested pairs (%d undecided), undecided hitting segments %d" % (
            name, len(hitting), hitting.sum(), (r['count'] > 1).sum(), len(r['cand']), und_pairs, und.sum()))
        total += int(hitting.sum())
        assert hitting.sum() >= 400
        assert und.sum() <= UNDECIDED_CAP * hitting.sum()
        ok = r['hit']
        assert np.all((r['t_pair'][ok] > 0) & (r['t_pair'][ok] < 1))
    assert total >= MIN_HITTING


def test_the_inside_tests_points_are_decidable():
    """2 000 points in the box: ground truth |x| < r outside a band that covers the surface's radial spread; at most 20 % of
    the points fall in the band, and the float64 majority parity agrees with the ground truth on all the others."""
    from recmv import metrics
    v, f = body()
    pts = inside_points(v)
    r_in, r_out = radial_band(v, f)
    r = pts.double().norm(dim=1).numpy()
    clear = (r < r_in) | (r > r_out)
    print("band [%.4f, %.4f] of radius %.2f: %d of %d points excluded, %d inside" % (r_in, r_out, RADIUS, (~clear).sum(), len(r),
                                                                                     (r < r_in).sum()))
    assert (~clear).mean() <= BAND_CAP and (r < r_in).sum() >= 100
    inside, decided = SR.points_inside(pts.numpy(), v.numpy(), f.numpy(), metrics.INSIDE_DIRECTIONS, reach_of(pts, v))
    assert np.array_equal(inside[clear], (r < r_in)[clear])
    assert (~decided[clear]).mean() <= UNDECIDED_CAP
