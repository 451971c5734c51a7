"""Crossing faces without a GPU: the float64 restatement (tests/mesh_intersect_reference.py) on hand cases, the new C entry
points (declared, exported, argument errors before any HIP call), the refusal of CPU tensors, the commands' new flags, and
the decidability of the GPU test's inputs.

BOUND(L) = 20 eps32 L^3 on a determinant of the f32 predicate (csrc/tri_tri.h), L the largest coordinate difference among
the points involved, u = eps32 / 2 = 2^-24, to first order in u:
  * rows: each element is one rounded difference, relative error u, magnitude <= L;
  * cofactor m = fmaf(r1y, r2z, -fl(r1z r2y)): the rounded product errs by u L^2, the fused result by u |m| <= 2 u L^2, the
    four row elements in its two products carry (|r1y r2z| + |r1z r2y|) 2 u <= 4 u L^2: 7 u L^2 per cofactor, |m| <= 2 L^2;
  * expansion fmaf(r0x, m0, fmaf(r0y, m1, fl(r0z m2))): three roundings of partial sums of at most 2, 4 and 6 L^3 (12 u L^3),
    the cofactors' errors times |r0| <= L (21 u L^3), r0's own rounding on |r0 . m| <= 6 L^3 (6 u L^3);
  * sum 39 u L^3 = 19.5 eps32 L^3, below 20 eps32 L^3 with the second-order terms; a determinant the kernel replaces by 0
    because two rows rounded to the same bits was at most 6 L^2 (2 u L) = 12 u L^3 — inside the bound.
A pair is DECIDED when every determinant that decides it exceeds BOUND(L) in float64 (the reference's margin, in units of
L^3, exceeds 20 eps32): the f32 kernel then takes every sign as the reference does.  Derived, not tuned.
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
import mesh_intersect_reference as XR  # noqa: E402

EPS32 = 2.0 ** -23
BOUND_C = 20.0                                             # BOUND(L) = BOUND_C * EPS32 * L^3
UNDECIDED_CAP = 0.01                                       # of the crossing pairs


def two_bodies():
    """The GPU test's main input: the irregular level-3 icosphere (1280 faces) and a copy scaled 0.9, shifted 0.3 radius."""
    from test_gpu_animation import _irregular_body
    v, f = _irregular_body(level=3)
    radius = 0.5
    w = (0.9 * v + torch.tensor([0.3 * radius, 0., 0.])).float().contiguous()
    return v, f, w, f.clone()


def pulled_sphere():
    """The level-3 icosphere with one vertex pulled through the opposite side: folds over itself."""
    from test_gpu_animation import _irregular_body
    v, f = _irregular_body(level=3)
    v = v.clone()
    k = int(v[:, 2].argmax())
    v[k] = torch.tensor([0.013, -0.021, -1.7]) * 0.5
    return v.contiguous(), f


def unwelded(v, f):
    """Every face with its own three vertices, bit-identical positions."""
    return v[f.reshape(-1)].contiguous(), torch.arange(3 * f.shape[0]).reshape(-1, 3)


def undecided_share(cross, margin):
    und = margin <= BOUND_C * EPS32
    return int((und & cross).sum()), int(und.sum())


def _one(a, b):
    cross, margin = XR.tri_tri(np.array([a], float), np.array([b], float))
    return bool(cross[0]), float(margin[0])


def test_reference_on_hand_cases():
    flat = [[-1, -1, 0], [1, -1, 0], [0, 1, 0]]                        # in z = 0, the origin inside
    # like an X: the second stands in x = 0.1 through the first
    cross, margin = _one(flat, [[0.1, -0.2, -1], [0.1, -0.2, 1], [0.1, 0.6, 0.3]])
    assert cross and margin > 1e-3
    assert _one([[0.1, -0.2, -1], [0.1, -0.2, 1], [0.1, 0.6, 0.3]], flat)[0]                    # symmetric
    # disjoint: boxes meet, the triangle stays above the plane
    assert not _one(flat, [[0, 0, 0.5], [1, 0, 1], [0, 1, 2]])[0]
    # touching at a vertex: a corner of the second is a corner of the first
    assert not _one(flat, [[0, 1, 0], [0, 2, 1], [1, 2, -1]])[0]
    # a corner of the second at a corner of the first, its opposite edge elsewhere: still only touching
    assert not _one(flat, [[-1, -1, 0], [-1, -1, 1], [-2, -1, 1]])[0]
    # sharing an edge (a hinge)
    assert not _one(flat, [[-1, -1, 0], [1, -1, 0], [0, 0, 1]])[0]
    # coplanar overlapping
    assert not _one(flat, [[-0.5, -0.5, 0], [2, -0.5, 0], [0, 3, 0]])[0]
    # one vertex exactly in the other's plane (inside it), the rest above: touching, no crossing
    assert not _one(flat, [[0, 0, 0], [1, 0, 1], [0, 1, 1]])[0]
    # zero area: a repeated corner whose edge passes through the first; three collinear corners
    assert not _one(flat, [[0, 0, -1], [0, 0, -1], [0, 0, 1]])[0]
    assert not _one([[0, 0, -1], [0, 0, -1], [0, 0, 1]], flat)[0]
    assert not _one(flat, [[0, 0, -1], [0, 0, 0.5], [0, 0, 1]])[0]
    # NaN anywhere
    assert not _one(flat, [[0.1, -0.2, -1], [0.1, float("nan"), 1], [0.1, 0.6, 0.3]])[0]


def test_reference_mesh_level():
    """Pairs, self mode and invalid faces on a tiny mesh: two quads crossing like a plus sign."""
    v = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1], [0, -1, -0.5], [0, 1, -0.5], [0, 1, 0.5], [0, -1, 0.5]], float)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [0, 1, 99], [-1, 2, 3]])
    pairs, cand, cross, margin = XR.intersections(v, f[:2], v, f[2:])
    assert len(pairs) >= 2 and set(pairs[:, 0]) == {0, 1} and pairs[:, 1].max() <= 1     # the invalid faces cross nothing
    own, cand, _, _ = XR.intersections(v, f, v, f, self_mode=True)
    assert (own[:, 0] < own[:, 1]).all() and len(own) == len(pairs)
    assert {(i, j - 2) for i, j in own.tolist()} == {tuple(p) for p in pairs.tolist()}
    assert not any(set(f[i]) & set(f[j]) for i, j in cand.tolist())                      # no tested pair shares an index


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    names = ("recmv_mesh_intersect_brute", "recmv_mesh_intersect_grid_count", "recmv_mesh_intersect_grid_fill")
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in names:
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION


def test_argument_errors_do_not_need_a_gpu():
    from recmv import _lib
    from test_mesh_metrics_cpu import grid_desc
    lib = _lib.lib()
    one = C.c_void_p(16)                                   # a non-NULL pointer that is never followed
    two = C.c_void_p(32)
    err = lib.recmv_last_error

    def brute(*, a=(one, 3, one, 1), b=(two, 3, two, 1), flags=(0, 0), out=(one, one), fill=(None, None, 0, None, None)):
        return lib.recmv_mesh_intersect_brute(*a, *b, *flags, *out, *fill, None)
    assert brute(a=(one, -1, one, 1)) == -1 and b"VA=-1" in err()
    assert brute(flags=(0, 1)) == -1 and b"skip_shared" in err()                  # meaningless for two meshes
    assert brute(flags=(1, 1)) == -1 and b"same mesh" in err()                    # self mode on two meshes
    assert brute(flags=(2, 0)) == -1 and b"self_mode=2" in err()
    assert brute(a=(one, 3, None, 1)) == -1 and b"NULL" in err()
    assert brute(out=(None, one)) == -1 and b"NULL" in err()
    assert brute(out=(None, None), fill=(one, one, -1, one, one)) == -1 and b"capacity=-1" in err()
    assert brute(out=(None, None), fill=(one, None, 4, one, one)) == -1 and b"NULL" in err()
    assert brute(fill=(one, one, 4, one, one)) == -1 and b"no counts" in err()

    def count(*, a=(one, 3, one, 1), b=(two, 3, two, 1), null=False, lanes=1, flags=(0, 0), out=(one, one), **grid):
        g = None if null else C.byref(grid_desc(**grid))
        return lib.recmv_mesh_intersect_grid_count(*a, *b, g, lanes, *flags, *out, None)
    assert count(b=(two, 3, two, -2)) == -1 and b"FB=-2" in err()
    assert count(dims=(2, 0, 2)) == -1 and b"dims=(2,0,2)" in err()
    assert count(h=0.) == -1 and b"cell size" in err()
    assert count(h=float("nan")) == -1
    assert count(null=True) == -1 and b"grid" in err()
    assert count(lanes=3) == -1 and b"lanes" in err()
    assert count(n_entries=-1) == -1 and b"entries=-1" in err()
    assert count(offsets=None) == -1 and b"NULL" in err()
    assert count(out=(one, None)) == -1 and b"NULL" in err()
    assert count(flags=(0, 1)) == -1 and b"skip_shared" in err()
    assert count(dims=(1 << 20, 1 << 20, 1)) == -1 and b"cells" in err()

    def fill(*, a=(one, 3, one, 1), lanes=8, flags=(0, 0), tail=(one, one, 4, one, one)):
        return lib.recmv_mesh_intersect_grid_fill(*a, two, 3, two, 1, C.byref(grid_desc()), lanes, *flags, *tail, None)
    assert fill(tail=(None, one, 4, one, one)) == -1 and b"offsets" in err()
    assert fill(tail=(one, one, 1 << 31, one, one)) == -1 and b"capacity" in err()
    assert fill(tail=(one, one, 4, None, one)) == -1 and b"NULL" in err()
    assert fill(tail=(one, one, 4, one, C.c_void_p(20))) == -1 and b"aligned" in err()
    assert fill(lanes=0) == -1 and b"lanes" in err()
    assert fill(a=(one, 3, one, 1 << 31)) == -1 and b"faces" in err()


def test_crossing_queries_refuse_cpu_tensors_and_bad_arguments():
    from recmv import collide, metrics
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])
    f = torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError):
        metrics.mesh_intersections(v, f, v, f)
    with pytest.raises(RuntimeError):
        metrics.self_intersections(v, f)
    with pytest.raises(RuntimeError):
        metrics.self_intersections(v, f, method='brute')
    with pytest.raises(RuntimeError):
        collide.intersection_report({'shirt': (v[None], f)}, v[None], f)
    with pytest.raises(ValueError):
        metrics.use_grid_for_pairs('fast', 1, 1)
    assert metrics.use_grid_for_pairs('grid', 1, 1) and not metrics.use_grid_for_pairs('brute', 10 ** 6, 10 ** 6)
    assert metrics.use_grid_for_pairs('auto', 1, metrics.AUTO_GRID_MIN_PAIRS)
    assert not metrics.use_grid_for_pairs('auto', 1, metrics.AUTO_GRID_MIN_PAIRS - 1)
    assert metrics.INTERSECT_LANES in (1, 8, 64)


def test_the_commands_carry_the_new_flags_and_they_default_to_off():
    import eval_fl
    import infer_fl_animation
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g"])
    assert a.intersections is False and a.body is None
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g", "--intersections", "--body", "b"])
    assert a.intersections is True and a.body == "b"
    with pytest.raises(SystemExit):                        # --body alone is a usage error, before any device work
        eval_fl.main(["--pred", str(HERE / "mesh_intersect_reference.py"), "--gt", str(HERE / "mesh_intersect_reference.py"),
                      "--body", "b"])
    a = infer_fl_animation.build_parser().parse_args(["--data-type", "snug"])
    assert a.report_intersections is False and a.fix_collisions is False
    assert infer_fl_animation.build_parser().parse_args(["--data-type", "snug", "--report-intersections"]).report_intersections


def test_host_build_of_the_grid_kernel_equals_the_pair_loop(tmp_path):
    """tools/mesh_intersect_host_check: csrc/mesh_intersect.hip's one-lane grid kernel (count, fill, a fill with half the
    capacity) compiled for the CPU under the address and undefined-behaviour sanitizers, against a double loop over the pair
    test of the brute force, on eight meshes and grids."""
    r = host_check.run("mesh_intersect", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(" 0 mismatches") == 8, r.stdout + r.stderr


def test_the_gpu_tests_inputs_are_decidable():
    """The float64 reference alone: on the two bodies at least 100 crossing pairs, and on every input the GPU test compares
    with the reference at most 1 % of the crossing pairs are undecided (margin <= BOUND)."""
    av, af, bv, bf = two_bodies()
    pairs, cand, cross, margin = XR.intersections(av.numpy(), af.numpy(), bv.numpy(), bf.numpy())
    und_cross, und_all = undecided_share(cross, margin)
    print("two bodies: %d crossing of %d tested pairs, undecided %d crossing / %d tested, smallest margin %.3g (bound %.3g)" % (
        len(pairs), len(cand), und_cross, und_all, margin.min(), BOUND_C * EPS32))
    assert len(pairs) >= 100
    assert und_cross <= UNDECIDED_CAP * len(pairs)
    v, f = pulled_sphere()
    pairs, cand, cross, margin = XR.intersections(v.numpy(), f.numpy(), v.numpy(), f.numpy(), self_mode=True)
    und_cross, und_all = undecided_share(cross, margin)
    print("pulled sphere: %d crossing of %d tested pairs, undecided %d / %d" % (len(pairs), len(cand), und_cross, und_all))
    assert len(pairs) >= 10 and und_cross <= UNDECIDED_CAP * len(pairs)
