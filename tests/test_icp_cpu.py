"""ICP alignment without a GPU: recmv.align's border flags and the two host solvers on hand cases and against the restatement
(tests/icp_reference.py), the port of the reference's ICP_Optimizer.solver against the reference's own output
(tests/golden/icp_solver.npz, tests/golden/make_golden_icp.py), the new C entry points (declared, exported, every argument
error before any HIP call) and eval_fl.py's new flags.
"""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import icp_reference as IR  # noqa: E402

GOLDEN = HERE / "golden" / "icp_solver.npz"


def _cloud(n=40, seed=2):
    rng = np.random.RandomState(seed)
    return (rng.rand(n, 3) - 0.5) * np.array([1.0, 0.6, 0.3]) + np.array([0.1, -0.2, 0.05])


def test_border_flags_on_hand_built_meshes():
    from recmv import align
    # a strip of four triangles over the vertices 0 2 4 / 1 3 5:   1-3-5
    #                                                              |/|/|
    #                                                              0-2-4
    strip = torch.tensor([[0, 2, 1], [2, 3, 1], [2, 4, 3], [4, 5, 3]])
    flags = align.border_flags(strip, 6)
    assert flags.dtype == torch.uint8 and flags.shape == (4,)
    # face 0 (a=0, b=2, c=1): ab 0-2 border, ac 0-1 border, bc 2-1 shared; every vertex of the strip lies on the border
    # face 1 (2, 3, 1): ab 2-3 shared, ac 2-1 shared, bc 3-1 border
    # face 2 (2, 4, 3): ab 2-4 border, ac 2-3 shared, bc 4-3 shared
    # face 3 (4, 5, 3): ab 4-5 border, ac 4-3 shared, bc 5-3 border
    assert flags.tolist() == [56 | 1 | 2, 56 | 4, 56 | 1, 56 | 1 | 4]
    assert np.array_equal(flags.numpy(), IR.border_flags(strip.numpy(), 6))
    tetra = torch.tensor([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    assert align.border_flags(tetra, 4).tolist() == [0, 0, 0, 0]
    assert align.border_flags(torch.tensor([[0, 1, 2]]), 3).tolist() == [63]
    # a fan around an interior vertex 0: the spokes are shared, the rim is the border, vertex 0 is not on it
    fan = torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]])
    assert align.border_flags(fan, 5).tolist() == [4 | 16 | 32] * 4
    assert align.border_flags(torch.zeros(0, 3, dtype=torch.int64), 5).shape == (0,)
    with pytest.raises(ValueError):
        align.border_flags(torch.tensor([[0, 1, 7]]), 3)
    with pytest.raises(ValueError):
        align.border_flags(torch.tensor([[0, 1, 2]], dtype=torch.int32), 3)
    v, f = IR.potato(2)
    cut = IR.open_copy(v, f)
    assert 0 < len(cut) < len(f)
    assert np.array_equal(align.border_flags(torch.from_numpy(cut), len(v)).numpy(), IR.border_flags(cut, len(v)))


@pytest.mark.parametrize("scale", [False, True])
def test_solve_point_recovers_a_known_motion(scale):
    from recmv import align
    u = _cloud()
    T = (1.3 if scale else 1., IR.rotation([0.3, -1., 0.5], 0.7), np.array([0.2, -0.1, 0.3]))
    S = IR.pair_sums(u, IR.transform_points(T, u))
    ds, dR, dt = align.solve_point(S, scale)
    assert isinstance(ds, float) and dR.dtype == np.float64 and dt.dtype == np.float64
    assert abs(ds - T[0]) <= 1e-12 and np.abs(dR - T[1]).max() <= 1e-12 and np.abs(dt - T[2]).max() <= 1e-12
    rs, rR, rt = IR.solve_point(S, scale)                  # the restatement from Umeyama's paper agrees
    assert abs(ds - rs) <= 1e-12 and np.abs(dR - rR).max() <= 1e-12 and np.abs(dt - rt).max() <= 1e-12
    if not scale:                                          # a rigid fit of scaled data leaves ds alone
        assert align.solve_point(IR.pair_sums(u, 1.3 * u), False)[0] == 1.
    assert align.solve_point(torch.from_numpy(S), scale)[0] == ds                  # a tensor of sums is taken too


def test_solve_point_guards_against_reflections_and_degenerate_pairs():
    from recmv import align
    u = _cloud()
    w = u * np.array([1., 1., -1.])                        # mirrored: the best orthogonal map is a reflection
    _, R, _ = align.solve_point(IR.pair_sums(u, w), False)
    assert abs(np.linalg.det(R) - 1.) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
    line = np.outer(np.linspace(-1., 1., 20), [1., 2., -0.5]) + [0.3, 0., 0.1]
    with pytest.raises(ValueError):
        align.solve_point(IR.pair_sums(line, line + 0.1), False)
    with pytest.raises(ValueError):
        align.solve_point(IR.pair_sums(u[:2], w[:2]), False)
    with pytest.raises(ValueError):
        align.solve_point(np.zeros(56), False)
    with pytest.raises(ValueError):
        align.solve_point(np.zeros(55), False)
    bad = IR.pair_sums(u, w)
    bad[9] = float("nan")
    with pytest.raises(ValueError):
        align.solve_point(bad, False)


def _planes(count=3, n=30, seed=5):
    """Points on the planes x = 0.4, y = -0.3 and x + y + z = 0.2 — three non-parallel planes: they fix a rigid motion, but
    meet in one point, and a scaling about it keeps all three — and with `count` = 4 on z = -0.35 besides, which does not
    pass through that point and so fixes the scale: (points, unit normals)."""
    rng = np.random.RandomState(seed)
    pts, nrm = [], []
    for normal, offset in (([1., 0., 0.], 0.4), ([0., 1., 0.], -0.3), ([1., 1., 1.], 0.2), ([0., 0., 1.], -0.35))[:count]:
        m = np.array(normal) / np.linalg.norm(normal)
        p = rng.rand(n, 3) - 0.5
        pts.append(p - np.outer(p @ m - offset / np.linalg.norm(normal), m))
        nrm.append(np.tile(m, (n, 1)))
    return np.concatenate(pts), np.concatenate(nrm)


def _plane_sums(x, w, m):
    """The closest point of x on the plane of w with normal m is x - ((x - w) . m) m: the pairs a search would give."""
    q = x - ((x - w) * m).sum(1, keepdims=True) * m
    return IR.pair_sums(x, q, m)


@pytest.mark.parametrize("scale", [False, True])
def test_solve_plane_recovers_a_small_motion_to_second_order_then_to_rounding(scale):
    from recmv import align
    w, m = _planes(4 if scale else 3)
    # the source is the surface moved by T^-1, so the step to find is T
    T = (1.002 if scale else 1., IR.rotation([0.5, 1., -0.7], 1e-3), np.array([2e-3, -1e-3, 1.5e-3]))
    x0 = (w - T[2]) @ T[1] / T[0]
    assert np.abs(IR.transform_points(T, x0) - w).max() < 1e-15
    ds, dR, dt = align.solve_plane(_plane_sums(x0, w, m), scale)
    assert np.abs(dR @ dR.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(dR) - 1.) <= 1e-15
    x1 = IR.transform_points((ds, dR, dt), x0)
    assert np.abs(x1 - w).max() <= 1e-5 and abs(ds - T[0]) <= 1e-5 and np.abs(dR - T[1]).max() <= 1e-5
    rs, rR, rt = IR.solve_plane(_plane_sums(x0, w, m), scale)
    assert abs(ds - rs) <= 1e-12 and np.abs(dR - rR).max() <= 1e-12 and np.abs(dt - rt).max() <= 1e-12
    ds2, dR2, dt2 = align.solve_plane(_plane_sums(x1, w, m), scale)
    x2 = IR.transform_points((ds2, dR2, dt2), x1)
    assert np.abs(((x2 - w) * m).sum(1)).max() <= 1e-10    # on the planes again
    total = (ds2 * ds, dR2 @ dR, ds2 * (dR2 @ dt) + dt2)
    assert abs(total[0] - T[0]) <= 1e-10 and np.abs(total[1] - T[1]).max() <= 1e-10 and np.abs(total[2] - T[2]).max() <= 1e-10
    if not scale:
        assert ds == 1. and ds2 == 1.


def test_solve_plane_refuses_what_does_not_determine_the_motion():
    from recmv import align
    w, m = _planes()
    with pytest.raises(ValueError):                        # three planes through one point leave the scale free
        align.solve_plane(_plane_sums(w * 1.001, w, m), True)
    assert align.solve_plane(_plane_sums(w + 1e-3, w, m), False)[0] == 1.
    one = slice(0, 30)                                     # one plane only: three of the six unknowns are free
    with pytest.raises(ValueError):
        align.solve_plane(_plane_sums(w[one] + 1e-3, w[one], m[one]), False)
    with pytest.raises(ValueError):
        align.solve_plane(_plane_sums(w[one] + 1e-3, w[one], m[one]), True)
    with pytest.raises(ValueError):
        align.solve_plane(np.zeros(56), False)
    with pytest.raises(ValueError):                        # point-mode sums carry no plane part
        align.solve_plane(IR.pair_sums(w, w + 1e-3), False)


def test_the_restatement_of_the_sums_on_a_hand_case():
    """Two pairs about the centre (1, 0, 0) on the face z = 0 of a single triangle, one of them not accepted."""
    verts = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    faces = np.array([[0, 1, 2]])
    x = np.array([[2, 1, 3], [1, 1, 5]], np.float32)
    q = np.array([[2, 1, 0], [1, 1, 0]], np.float32)
    S, M = IR.sums(x, q, np.array([0, 0]), [True, False], verts, faces, [1., 0., 0.], True)
    u, w = np.array([1., 1., 3.]), np.array([1., 1., 0.])
    assert S[0] == 1 and S[1:4].tolist() == u.tolist() and S[4:7].tolist() == w.tolist()
    assert S[7:16].tolist() == np.outer(u, w).reshape(-1).tolist()
    assert (S[16], S[17], S[18]) == (11., 2., 9.)
    J = np.array([1., -1., 0., 0., 0., 1., 3.])            # u x m = (1, -1, 0) with m = (0, 0, 1); u . m = 3
    assert S[19:47].tolist() == np.outer(J, J)[np.triu_indices(7)].tolist()
    assert S[47:54].tolist() == (3. * J).tolist() and S[54] == 9. and S[55] == 0.
    assert M[18] == 2 ** 2 + 2 ** 2 + 3 ** 2               # (|u| + |w|)^2 per axis: (1 + 1, 1 + 1, 3 + 0)
    assert np.all(M >= np.abs(S))
    S0, _ = IR.sums(x, q, np.array([0, 0]), [True, True], verts, faces, [1., 0., 0.], False)
    assert S0[0] == 2 and np.all(S0[19:] == 0)


def test_icp_optimizer_solver_equals_the_reference():
    from recmv import align
    from recmv.engineer.optimizer import ICP_Optimizer
    import recmv.engineer.optimizer.icp_optimzier as mod
    g = np.load(GOLDEN)
    source, target = torch.from_numpy(g["source"]), torch.from_numpy(g["target"])
    assert source.dtype == torch.float32 and source.shape == (50, 3)
    opt = ICP_Optimizer(3)
    assert opt.name == "ICP_Optimizer" and opt.epoch == 3 and mod.ICP_Optimizer is ICP_Optimizer
    keep_s, keep_t = source.clone(), target.clone()
    R, t = opt.solver(source, target)
    assert torch.equal(source, keep_s) and torch.equal(target, keep_t)             # unlike the reference: arguments unchanged
    assert R.dtype == torch.float32 and R.shape == (3, 3) and t.shape == (1, 3)
    err_R, err_t = float(np.abs(R.numpy() - g["R"]).max()), float(np.abs(t.numpy() - g["t"]).max())
    print("ICP_Optimizer.solver against the reference: |dR| %.3e, |dt| %.3e" % (err_R, err_t))
    assert err_R <= 1e-5 and err_t <= 1e-5
    R64, t64 = opt.solver(source.double(), target.double())                        # (the reference fails on float64)
    assert R64.dtype == torch.float64 and float((R64 - R.double()).abs().max()) <= 1e-6
    new_source = (R64 @ source.double().T).T + t64
    assert float(opt.energy_func(new_source, target.double())) < float(opt.energy_func(source.double(), target.double()))
    sums = mod.pair_sums(source, target)
    assert sums.dtype == torch.float64 and sums.shape == (align.N_SUMS,)
    assert np.abs(sums.numpy() - IR.pair_sums(source.numpy(), target.numpy())).max() <= 1e-12


class _Boundary:
    """The reference's interface of a garment with boundary fields: get_fields / get_boundary / transform_R_t."""

    def __init__(self, fields):
        self.fields = dict(fields)
        self.moved = None

    def get_fields(self):
        return list(self.fields)

    def get_boundary(self, *names):
        return [self.fields[n] for n in names]

    def transform_R_t(self, R, t):
        self.moved = (R, t)


def test_icp_optimizer_fitting_refuses_cpu_tensors():
    from recmv.engineer.optimizer import ICP_Optimizer
    a = _Boundary({'neck': torch.rand(5, 3), 'hem': torch.rand(6, 3)})
    with pytest.raises(RuntimeError):
        ICP_Optimizer(0)(smpl_slice=a, target_polygon=a)


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in ("recmv_icp_accumulate", "recmv_icp_accumulate_workspace_bytes"):
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION == 11
    hdr = (REPO / "include" / "recmv_hip.h").read_text()
    assert "#define RECMV_ICP_SUMS 56" in hdr
    ws = lib.recmv_icp_accumulate_workspace_bytes
    assert ws(0) == 0 and ws(-5) == 0 and ws(1) == 56 * 8 and ws(256) == 56 * 8 and ws(257) == 2 * 56 * 8
    assert ws(10 ** 5) == ws(10 ** 9) == 256 * 56 * 8      # a fixed cap: a function of P alone


def test_argument_errors_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    one = C.c_void_p(64)                                   # a non-NULL aligned pointer that is never followed
    centre = (C.c_double * 3)(0., 0., 0.)
    err = lib.recmv_last_error
    need = lib.recmv_icp_accumulate_workspace_bytes(4)

    def call(*, pairs=(one, one, one, one, 4), mesh=(one, 3, one, 1), border=None, limit=None, c=centre, plane=1, sums=one,
             ws=(one, need)):
        return lib.recmv_icp_accumulate(*pairs, *mesh, border, limit, c, plane, sums, *ws, None)
    ARG, WS = -1, -4
    assert call(pairs=(one, one, one, one, -1)) == ARG and b"icp_accumulate" in err() and b"P=-1" in err()
    assert call(mesh=(one, -3, one, 1)) == ARG and b"V=-3" in err()
    assert call(mesh=(one, 3, one, -2)) == ARG and b"F=-2" in err()
    for k in range(4):
        p = [one] * 4 + [4]
        p[k] = None
        assert call(pairs=tuple(p)) == ARG and b"icp_accumulate: NULL pointer of the pairs" in err()
    assert call(mesh=(None, 3, one, 1)) == ARG and b"NULL pointer of the mesh" in err()
    assert call(mesh=(one, 3, None, 1)) == ARG and b"NULL pointer of the mesh" in err()
    assert call(mesh=(one, 0, one, 1)) == ARG and b"must not be empty" in err()
    assert call(mesh=(one, 3, one, 0)) == ARG and b"must not be empty" in err()
    assert call(c=None) == ARG and b"NULL centre" in err()
    assert call(sums=None) == ARG and b"sums" in err()
    assert call(sums=C.c_void_p(68)) == ARG and b"8-byte aligned" in err()
    assert call(plane=2) == ARG and b"with_plane=2" in err()
    assert call(plane=-1) == ARG and b"with_plane=-1" in err()
    assert call(ws=(one, need - 1)) == WS and b"icp_accumulate: workspace" in err()
    assert call(ws=(None, need)) == WS and b"workspace" in err()
    assert call(ws=(C.c_void_p(68), need)) == WS and b"8-byte aligned" in err()
    # P = 0 is checked like every other size: the errors that do not depend on the pairs are still found ...
    empty = (None, None, None, None, 0)
    assert call(pairs=empty, mesh=(None, 0, None, 0), sums=None, ws=(None, 0)) == ARG and b"sums" in err()
    assert call(pairs=empty, mesh=(None, 0, None, 0), c=None, ws=(None, 0)) == ARG and b"NULL centre" in err()
    assert call(pairs=empty, mesh=(None, 0, None, 0), plane=3, ws=(None, 0)) == ARG
    # ... and a valid call needs neither pairs, mesh nor workspace.  It writes the 56 zeros, so it needs a device: where there
    # is one, RECMV_OK and zeros from a buffer filled with NaN; where there is none, the launch fails as a HIP error, not
    # as an argument error.
    if torch.cuda.is_available():
        out = torch.full((56,), float("nan"), dtype=torch.float64, device="cuda:0")
        rc = call(pairs=empty, mesh=(None, 0, None, 0), sums=C.c_void_p(out.data_ptr()), ws=(None, 0))
        torch.cuda.synchronize()
        assert rc == 0 and bool((out == 0).all())
    else:
        assert call(pairs=empty, mesh=(None, 0, None, 0), ws=(None, 0)) == -2 and b"icp_accumulate" in err()


def test_the_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from recmv import align
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])
    f = torch.tensor([[0, 1, 2]])
    p = torch.zeros(4, 3)
    with pytest.raises(RuntimeError):
        align.icp_sums(p, p, torch.zeros(4, dtype=torch.int64), torch.zeros(4), v, f)
    with pytest.raises(RuntimeError):
        align.icp(v, f, v, f)
    for bad in (dict(mode='affine'), dict(metric='line'), dict(trim=0.), dict(trim=1.5), dict(max_dist=0.), dict(iters=-1),
                dict(method='fast')):
        with pytest.raises(ValueError):
            align.icp(v, f, v, f, **bad)
    r = {'matrix': [[0., -2., 0., 1.], [2., 0., 0., 2.], [0., 0., 2., 3.], [0., 0., 0., 1.]]}
    out = align.apply(r, torch.tensor([[1., 0., 0.], [0., 1., 1.]]))
    assert out.dtype == torch.float32 and out.tolist() == [[1., 4., 3.], [-1., 2., 5.]]
    s, R, t = align._initial(r['matrix'])
    assert abs(s - 2.) < 1e-15 and np.abs(R - np.array([[0., -1., 0.], [1., 0., 0.], [0., 0., 1.]])).max() < 1e-15
    assert t.tolist() == [1., 2., 3.]
    with pytest.raises(ValueError):
        align._initial(np.diag([1., 1., -1., 1.]))


def test_eval_fl_carries_the_align_flags_and_they_default_to_off():
    import eval_fl
    me = str(HERE / "icp_reference.py")                    # any existing file: the usage errors come before it is read
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g"])
    assert a.align == 'none' and a.align_metric == 'plane' and a.align_from == 'each' and a.align_out is None
    assert a.align_trim == 1.0 and a.align_iters == 50
    for mode in ('none', 'rigid', 'similarity'):
        assert eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g", "--align", mode]).align == mode
    with pytest.raises(SystemExit):
        eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g", "--align", "affine"])
    with pytest.raises(SystemExit):
        eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g", "--align-metric", "line"])
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g", "--align", "similarity", "--align-from", "first",
                                           "--align-metric", "point", "--align-trim", "0.8", "--align-iters", "7",
                                           "--align-out", "d"])
    assert (a.align_from, a.align_metric, a.align_trim, a.align_iters, a.align_out) == ('first', 'point', 0.8, 7, 'd')
    with pytest.raises(SystemExit):                        # before any device work
        eval_fl.main(["--pred", me, "--gt", me, "--align-out", "d"])
    with pytest.raises(SystemExit):
        eval_fl.main(["--pred", me, "--gt", me, "--align", "rigid", "--align-trim", "0"])
    with pytest.raises(SystemExit):
        eval_fl.main(["--pred", me, "--gt", me, "--align", "rigid", "--align-iters", "-2"])
