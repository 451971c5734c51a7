"""Laplacian alignment without a GPU: boundary loops, the loop -> field assignment, best_match against a restatement of the
reference's code, the dense solve against the reference's f32 pseudo-inverse, argument checks of the new C entry points and
the register_fl.py flags."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from recmv import lap_align as LA  # noqa: E402
from recmv import nricp as K  # noqa: E402
from test_nricp_cpu import icosphere  # noqa: E402

CAPS = {'neck': (1, 1.), 'upper_bottom': (1, -1.), 'left_cuff': (0, 1.), 'right_cuff': (0, -1.)}


def cut_sphere(level, caps=tuple(CAPS), h=0.8):
    """An icosphere with the caps |coordinate| > h cut off (axis and sign per CAPS) and unused vertices dropped."""
    v, f = icosphere(level)
    drop = torch.zeros(v.shape[0], dtype=torch.bool)
    for name in caps:
        ax, sg = CAPS[name]
        drop |= v[:, ax] * sg > h
    f = f[~drop[f].any(1)]
    used = torch.unique(f)
    remap = torch.full((v.shape[0],), -1, dtype=torch.int64)
    remap[used] = torch.arange(used.shape[0])
    return v[used].contiguous(), remap[f].contiguous()


def ring(name, h=0.8, dy=0., S=200):
    """The feature curve of a cap: a circle of S samples in the cut plane, shifted by dy along y."""
    ax, sg = CAPS[name]
    t = torch.linspace(0, 2 * np.pi, S + 1)[:-1]
    rho = (1 - h * h) ** .5
    a, b = rho * torch.cos(t), rho * torch.sin(t)
    c = torch.full_like(t, sg * h)
    p = torch.stack([a, c, b], -1) if ax == 1 else torch.stack([c, a, b], -1)
    return (p + torch.tensor([0., dy, 0.])).float()


def test_boundary_loops_of_a_cut_sphere():
    v, f = cut_sphere(3)
    loops = LA.boundary_loops(f, v.shape[0])
    assert len(loops) == 4
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    uniq, cnt = np.unique(edges, axis=0, return_counts=True)
    border = {tuple(e) for e in uniq[cnt == 1].tolist()}
    walked = set()
    for loop in loops:
        assert len(loop) >= 3 and len(set(loop)) == len(loop)
        for a, b in zip(loop, loop[1:] + loop[:1]):                     # closed: the last vertex returns to the first
            walked.add((min(a, b), max(a, b)))
    assert walked == border
    bnd = K.mesh_boundary(f, v.shape[0])
    assert sorted(i for l in loops for i in l) == sorted(torch.nonzero(bnd)[:, 0].tolist())
    assert LA.boundary_loops(icosphere(2)[1]) == []                     # closed mesh: no loop


def test_assign_loops_picks_the_nearest_loop_and_skips_what_is_missing():
    v, f = cut_sphere(3)
    loops = LA.boundary_loops(f)
    curves = {n: ring(n, dy=0.05) for n in CAPS}
    got = LA.assign_loops(loops, v, curves, ['neck', 'left_cuff', 'right_cuff', 'upper_bottom'], log=lambda s: None)
    for name, li in got.items():
        cen = v[sorted(set(loops[li]))].mean(0)
        ax, sg = CAPS[name]
        assert cen[ax] * sg > 0.7                                       # the loop of that cap
    assert len(set(got.values())) == 4
    # two loops for four fields: two fields are logged and skipped; a field without a curve is logged too
    v2, f2 = cut_sphere(3, caps=('neck', 'upper_bottom'))
    logs = []
    got2 = LA.assign_loops(LA.boundary_loops(f2), v2, {n: curves[n] for n in ('neck', 'left_cuff', 'upper_bottom')},
                           ['neck', 'left_cuff', 'right_cuff', 'upper_bottom'], log=logs.append)
    assert sorted(got2) == ['neck', 'upper_bottom']
    assert any('right_cuff' in s and 'no curve' in s for s in logs)
    assert any('left_cuff' in s and 'no loop left' in s for s in logs)


def _best_match_reference(vertices, source_idx, target_bo):
    """Garment_Mesh.best_match (garment_structure.py:667-715) for one field, ot.dist restated as squared distances."""
    from scipy.optimize import linear_sum_assignment
    source_bo = vertices[source_idx]
    idx = torch.arange(0, target_bo.shape[0], (target_bo.shape[0] - 1) / source_bo.shape[0]).long()
    target_bo = target_bo[idx]
    source_bo = source_bo.detach().cpu().numpy()
    target_bo = target_bo.detach().cpu().numpy()
    distance = ((source_bo[:, None, :].astype(np.float64) - target_bo[None].astype(np.float64)) ** 2).sum(-1)
    source_match_idx, target_match_idx = linear_sum_assignment(distance)
    source_c = source_bo.mean(axis=0)
    target_c = target_bo.mean(axis=0)
    source_n = source_bo - source_c
    target_n = (target_bo - target_c)[target_match_idx]
    source_n_norm = np.linalg.norm(source_n, axis=1, keepdims=True)
    target_n_norm = np.linalg.norm(target_n, axis=1, keepdims=True)
    similiarity = ((source_n * target_n) / (source_n_norm * target_n_norm)).sum(axis=-1)
    norm_mask = (similiarity > 0.5)
    source_match_idx = source_match_idx[norm_mask]
    target_match_idx = target_match_idx[norm_mask]
    return source_idx[source_match_idx], target_bo[target_match_idx]


def test_best_match_equals_the_reference_restatement():
    g = torch.Generator().manual_seed(0)
    verts = torch.randn(40, 3, generator=g)
    t = torch.linspace(0, 2 * np.pi, 27)[:-1]
    ids = torch.tensor([1, 4, 5, 9, 12, 13, 20, 22, 30, 33, 38])
    verts[ids] = torch.stack([torch.cos(t[::2][:11]), 0.1 * torch.randn(11, generator=g), torch.sin(t[::2][:11])], -1)
    curve = torch.stack([1.2 * torch.cos(t), torch.full_like(t, 0.3), 1.2 * torch.sin(t)], -1)
    curve[5] = torch.tensor([-3., 0.3, 0.])                             # an outlier the direction filter drops
    i, tg = LA.best_match(verts, ids, curve)
    ri, rt = _best_match_reference(verts, ids, curve)
    assert torch.equal(i, ri) and np.array_equal(tg.numpy(), rt)
    assert 0 < i.shape[0] <= ids.shape[0]
    n = ids.shape[0]
    assert torch.equal(LA.resample_curve(curve, n), curve[torch.arange(0, 26, 25 / n).long()])


def test_constraint_weights_count_repeated_vertices():
    idx = torch.tensor([4, 1, 4, 0])
    t = torch.tensor([[1., 2., 3.], [0., 0., 1.], [3., 2., 1.], [5., 5., 5.]])
    cw, cwt = LA.constraint_weights(idx, t, 6, 2.)
    assert cw.dtype == torch.float64 and cw.tolist() == [2., 2., 0., 0., 4., 0.]
    assert cwt[4].tolist() == [8., 8., 8.] and cwt[1].tolist() == [0., 0., 2.] and cwt[5].abs().sum() == 0


def _problem(level=2, dy=0.15):
    v, f = cut_sphere(level)
    loops = LA.boundary_loops(f)
    curves = {n: ring(n, dy=dy) for n in CAPS}
    fl = LA.assign_loops(loops, v, curves, list(CAPS), log=lambda s: None)
    idx, tgt, _ = LA.match(v, loops, fl, curves)
    topo = LA.Topology(f, v.shape[0], 'cpu')
    return v, f, topo, idx, tgt


def test_solve_torch_equals_the_reference_inverse_and_solves_the_normal_equations():
    v, f, topo, idx, tgt = _problem()
    V, w = v.shape[0], 1.
    cw, cwt = LA.constraint_weights(idx, tgt, V, w)
    u = LA.solve_torch(topo, v, cw, cwt)
    # the reference (lap_deform_optimizer.py:150-186) in f32: inv(L^T W L) L^T W [L v; t]
    Lm = LA.laplacian_dense(topo.edges, V, dtype=torch.float32)
    Cm = torch.zeros(idx.shape[0], V)
    Cm[torch.arange(idx.shape[0]), idx] = 1.
    W = torch.diag(torch.cat([torch.ones(V), torch.full((idx.shape[0],), w)]))
    Lb = torch.cat([Lm, Cm])
    t = torch.cat([Lm @ v, tgt])
    ref = torch.linalg.inv(Lb.T @ W @ Lb) @ Lb.T @ W @ t
    diag = float((v.max(0).values - v.min(0).values).norm())
    assert (u - ref).abs().max() < 1e-3 * diag
    # f64 normal equations
    L64 = LA.laplacian_dense(topo.edges, V)
    A = L64.T @ L64 + torch.diag(cw)
    b = L64.T @ (L64 @ v.double()) + cwt
    u64 = torch.linalg.solve(A, b)
    assert (A @ u64 - b).norm() <= 1e-10 * b.norm()
    assert torch.equal(u, u64.float())
    # the constraint moved the boundary toward the curves
    assert ((u[idx] - tgt).norm(dim=1).mean() < 0.5 * (v[idx] - tgt).norm(dim=1).mean())


def test_the_restated_cg_solve_agrees_with_solve_torch():
    """tests/cg_reference.py's lap_solve, which tests/test_gpu_lap_align.py holds the kernels to bit for bit, against the dense
    solve, to the tolerance that file uses for the kernel path."""
    import cg_reference as CR
    v, f, topo, idx, tgt = _problem(level=3)
    cw, cwt = LA.constraint_weights(idx, tgt, v.shape[0], 1.)
    off, nbr = (x.numpy() for x in topo.nbr)
    u, iters, res, _ = CR.lap_solve(off, nbr, v.numpy(), cw.numpy(), cwt.numpy(), 1e-12, 100000)
    assert u.dtype == np.float32 and 0 < iters < 100000 and max(res) <= 1e-12
    diag = float((v.max(0).values - v.min(0).values).norm())
    assert (torch.from_numpy(u).double() - LA.solve_torch(topo, v, cw, cwt).double()).abs().max() <= 1e-5 * diag
    assert not np.array_equal(u, v.numpy())


def test_solve_torch_refuses_large_templates():
    class T:
        V = LA.DENSE_MAX_V + 1
    try:
        LA.solve_torch(T(), torch.zeros(T.V, 3), None, None)
    except ValueError as e:
        assert "kernel path" in str(e)
    else:
        raise AssertionError("expected a ValueError")


def test_laplacian_optimizer_on_the_cpu_runs_the_torch_path():
    from recmv.engineer.optimizer import Laplacian_Optimizer
    v, f = cut_sphere(2)
    mesh = K.TriMesh(v.clone(), f)
    logs = []
    names = list(CAPS)
    out = Laplacian_Optimizer(log=logs.append)(source_fl_meshes=[mesh], target_meshes=[ring(n, dy=0.15) for n in names],
                                               source_type=['long_sleeve_upper'], target_fl_type=names, outlayer=True)
    assert out['source_fl_meshes'][0] is mesh and not torch.equal(mesh.verts, v)
    assert sum('Laplacian align long_sleeve_upper epoch' in s for s in logs) == 3
    closed = K.TriMesh(*icosphere(1))
    try:
        Laplacian_Optimizer(log=logs.append)(source_fl_meshes=[closed], target_meshes=[ring('neck')],
                                             source_type=['long_sleeve_upper'], target_fl_type=['neck'], outlayer=True)
    except ValueError as e:
        assert "nothing to constrain" in str(e)
    else:
        raise AssertionError("expected a ValueError")


def test_new_entry_points_reject_bad_arguments():
    from recmv import _lib as L
    lib = L.lib()
    assert {"recmv_lap_align_solve", "recmv_lap_align_workspace_bytes", "recmv_lap_smooth"} <= set(L.exported_symbols())
    n = C.c_void_p(0)
    it = C.c_int32(-5)
    res = (C.c_double * 3)(1., 1., 1.)
    buf = (C.c_byte * 512)()
    p = C.cast(buf, C.c_void_p)
    assert lib.recmv_lap_align_solve(n, n, 0, 0, n, n, n, 1e-10, 10, n, C.byref(it), res, n, 0, n) == 0   # V = 0: no-op
    assert it.value == 0 and list(res) == [0., 0., 0.]
    assert lib.recmv_lap_align_solve(n, n, -1, 0, n, n, n, 1e-10, 10, n, C.byref(it), res, n, 0, n) == -1
    assert lib.recmv_lap_align_solve(p, p, 4, 6, p, p, p, -1., 10, p, C.byref(it), res, p, 512, n) == -1   # tol < 0
    assert lib.recmv_lap_align_solve(p, p, 4, 6, p, p, p, 1e-10, -1, p, C.byref(it), res, p, 512, n) == -1  # max_iter < 0
    assert lib.recmv_lap_align_solve(p, p, 4, 6, p, p, p, 1e-10, 10, p, n, res, p, 512, n) == -1           # NULL host out
    assert lib.recmv_lap_align_solve(p, n, 4, 6, p, p, p, 1e-10, 10, p, C.byref(it), res, p, 1 << 20, n) == -1
    assert b"neighbour" in lib.recmv_last_error()
    assert lib.recmv_lap_align_solve(p, p, 4, 6, p, n, p, 1e-10, 10, p, C.byref(it), res, p, 1 << 20, n) == -1
    assert b"NULL" in lib.recmv_last_error()
    assert lib.recmv_lap_align_solve(p, p, 4, 6, p, p, p, 1e-10, 10, p, C.byref(it), res, p, 8, n) == -1
    assert b"workspace" in lib.recmv_last_error()
    assert lib.recmv_lap_align_workspace_bytes(0) == 0 < lib.recmv_lap_align_workspace_bytes(4)
    assert lib.recmv_lap_smooth(n, n, 0, 0, n, n, n) == 0                                                  # V = 0: no-op
    assert lib.recmv_lap_smooth(n, n, -2, 0, n, n, n) == -1
    assert lib.recmv_lap_smooth(p, p, 4, 6, p, n, n) == -1
    assert lib.recmv_lap_smooth(p, p, 4, 6, p, p, n) == -1                                                 # out aliases u
    assert b"alias" in lib.recmv_last_error()


def test_register_fl_help_lists_the_alignment_flags():
    out = subprocess.run([sys.executable, str(REPO / "rec-mv_amd" / "register_fl.py"), "--help"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0
    assert "--align-curves" in out.stdout and "--align-epochs" in out.stdout and "--torch-path" in out.stdout
