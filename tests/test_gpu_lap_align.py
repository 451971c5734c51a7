"""Laplacian alignment on the GPU: recmv_lap_align_solve against a float64 dense solve (and bit for bit against itself) and
against the numpy restatement of its recurrence and summation order (tests/cg_reference.py) bit for bit, recmv_lap_smooth against its f64 restatement, Laplacian_Optimizer's kernel path against its torch path and its effect on
displaced rings, the 40962-vertex template, and register_fl.py --align-curves end to end on a run trained with curves."""
import functools
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
DEV = "cuda:0"

import cg_reference as CR  # noqa: E402
import param_cases as PC  # noqa: E402
from test_lap_align_cpu import CAPS, cut_sphere, ring  # noqa: E402


def _diag(v):
    return float((v.max(0).values - v.min(0).values).norm())


def _constraints(v, f, dy=0.15):
    from recmv import lap_align as LA
    loops = LA.boundary_loops(f)
    curves = {n: ring(n, dy=dy) for n in CAPS}
    fl = LA.assign_loops(loops, v, curves, list(CAPS), log=lambda s: None)
    idx, tgt, _ = LA.match(v, loops, fl, curves)
    return LA.constraint_weights(idx, tgt, v.shape[0], 1.)


def test_solve_matches_a_dense_float64_solve_and_is_reproducible():
    from recmv import lap_align as LA
    v, f = cut_sphere(4)
    assert v.shape[0] < 2562                                                  # level 4 minus the caps
    cw, cwt = _constraints(v, f)
    topo = LA.Topology(f, v.shape[0], DEV)
    vd = v.to(DEV)
    u, iters, res = LA.solve(topo, vd, cw, cwt, tol=1e-12, max_iter=100000)
    u2, iters2, res2 = LA.solve(topo, vd, cw, cwt, tol=1e-12, max_iter=100000)
    assert torch.equal(u, u2) and iters == iters2 and res == res2             # bit for bit
    assert 0 < iters < 100000 and max(res) <= 1e-12
    L64 = LA.laplacian_dense(topo.edges.cpu(), v.shape[0])
    A = L64.T @ L64 + torch.diag(cw)
    ref = torch.linalg.solve(A, L64.T @ (L64 @ v.double()) + cwt)
    assert (u.cpu().double() - ref).abs().max() <= 1e-5 * _diag(v)


def test_constraint_free_component_is_unchanged():
    from recmv import lap_align as LA
    v, f = cut_sphere(3)
    w, g = cut_sphere(2)
    w = w * 0.5 + torch.tensor([3., 0., 0.])                                   # a second, unconstrained component
    V = v.shape[0]
    verts = torch.cat([v, w])
    faces = torch.cat([f, g + V])
    cw, cwt = _constraints(v, f)
    cw = torch.cat([cw, torch.zeros(w.shape[0], dtype=torch.float64)])
    cwt = torch.cat([cwt, torch.zeros(w.shape[0], 3, dtype=torch.float64)])
    topo = LA.Topology(faces, verts.shape[0], DEV)
    u, iters, res = LA.solve(topo, verts.to(DEV), cw, cwt, tol=1e-12, max_iter=100000)
    assert iters > 0
    assert torch.equal(u[V:].cpu(), w)
    assert not torch.equal(u[:V].cpu(), v)


# ---------------------------------------------------------------------------------------- the solve against its restatement
def _lifted(rows, cols):
    """PC.grid(rows, cols) lifted out of its plane, so that no column of the solve is trivial."""
    v, f = PC.grid(rows, cols)
    v[:, 2] = (0.25 * np.sin(0.7 * v[:, 0]) * np.cos(0.4 * v[:, 1])).astype(np.float32)
    return v, f


def _sides(v, rows, cols):
    """The sides j = 0 and j = cols - 1 of the first `rows` grid rows, drawn apart: (cw [V], cwt [V,3]) with weight 1."""
    side = np.array([r * cols + c for r in range(rows) for c in (0, cols - 1)])
    cw, cwt = np.zeros(v.shape[0]), np.zeros((v.shape[0], 3))
    cw[side] = 1.
    cwt[side] = v[side].astype(np.float64) + np.array([[0.5, -0.3, 0.2]]) * np.where(v[side][:, 1:2] == 0, 1., -1.)
    return cw, cwt


def _triangle():
    v = np.array([[0., 0., 0.], [1., 0., 0.25], [0., 1., -0.5]], np.float32)
    cw, cwt = np.array([0., 1., 0.]), np.array([[0., 0., 0.], [1.5, -0.25, 0.5], [0., 0., 0.]])
    return v, np.array([[0, 1, 2]], np.int64), cw, cwt


def _grid300():
    """15 x 20 vertices: grid rows 0 .. 11 with two constrained sides, rows 12 .. 14 a component of their own without a
    constraint, and vertex 299 without a face."""
    v, f = _lifted(15, 20)
    f = f[(f // 20 <= 11).all(1) | ((f // 20 >= 12).all(1) & (f != 299).all(1))]
    return (v, f) + _sides(v, 12, 20)


def _grid257():
    v, f = _lifted(257, 257)
    return (v, f) + _sides(v, 257, 257)


# name -> (mesh and constraints, tol, max_iter): the smallest shapes at which the state machine or the reductions can go wrong
RESTATED = {
    "one triangle, one slot, a partly filled wave": (_triangle, 1e-12, 100000),
    "300 vertices, two slots": (_grid300, 1e-12, 100000),
    "66049 vertices, 259 slots, stopped at the cap": (_grid257, 1e-12, 6),
    "300 vertices, a column frozen early": (_grid300, 1e-3, 100000),
}


@functools.lru_cache(maxsize=None)
def restated(name):
    """(v, f, cw, cwt, offsets, neighbours, restated u, iterations, residuals, where each column froze); computed once."""
    from recmv import lap_align as LA
    build, tol, max_iter = RESTATED[name]
    v, f, cw, cwt = build()
    off, nbr = (x.numpy() for x in LA.Topology(torch.from_numpy(f), v.shape[0], "cpu").nbr)
    out = (v, f, cw, cwt, off, nbr) + CR.lap_solve(off, nbr, v, cw, cwt, tol, max_iter)
    for a in out[:7]:
        a.setflags(write=False)                                                 # (the tests copy what they hand to torch)
    return out


@pytest.mark.parametrize("name", list(RESTATED))
def test_solve_has_the_restatements_bits(name):
    from recmv import lap_align as LA
    build, tol, max_iter = RESTATED[name]
    v, f, cw, cwt, off, nbr, want, it, res, frozen = restated(name)
    V = v.shape[0]
    topo = LA.Topology(torch.tensor(f), V, DEV)
    assert np.array_equal(topo.nbr[0].cpu().numpy(), off) and np.array_equal(topo.nbr[1].cpu().numpy(), nbr)
    vd, cwd, cwtd = torch.tensor(v, device=DEV), torch.tensor(cw), torch.tensor(cwt)
    u, iters, residuals = LA.solve(topo, vd, cwd, cwtd, tol=tol, max_iter=max_iter)
    print(name, "iterations", iters, "residuals", residuals, "restatement", it, res, "frozen at", frozen)
    assert iters == it and residuals == res
    assert torch.equal(u.cpu(), torch.tensor(want))
    assert it > 0 and not np.array_equal(want, v)
    if build is _triangle:
        assert V == 3 and it < 10 and max(res) <= tol
    if build is _grid300:
        assert V == 300 and off[300] == off[299] and max(res) <= tol
        assert np.array_equal(want[240:], v[240:]) and not np.array_equal(want[:240], v[:240])       # the free component's bits
    if build is _grid257:
        assert (V + 255) // 256 == 259 and it == max_iter == 6 and min(res) > tol             # the cap is what is reported
    if tol == 1e-3:
        first = int(np.argmin(frozen))
        assert 0 < frozen[first] and frozen[first] + 2 <= min(k for c, k in enumerate(frozen) if c != first) and max(frozen) == it
        early = LA.solve(topo, vd, cwd, cwtd, tol=tol, max_iter=frozen[first])[0]
        assert torch.equal(early[:, first], u[:, first])                          # frozen: the later iterations left it alone
        assert not torch.equal(early, u)


def test_smooth_matches_an_f64_restatement():
    from recmv import lap_align as LA
    v, f = cut_sphere(4)
    iso = torch.tensor([[0.3, -0.2, 0.9], [1.5, 2.5, -3.]])
    verts = torch.cat([v, iso])                                               # two isolated vertices
    V = verts.shape[0]
    topo = LA.Topology(f, V, DEV)
    out = LA.smooth(topo, verts.to(DEV)).cpu()
    off, nbr = topo.nbr[0].cpu().long(), topo.nbr[1].cpu().long()
    ref = torch.zeros(V, 3, dtype=torch.float64)
    for i in range(V):
        row = nbr[off[i]:off[i + 1]]
        if row.numel():
            s = torch.zeros(3, dtype=torch.float64)
            for j in row.tolist():
                s = s + verts[j].double()
            ref[i] = s * (1. / row.numel())
    assert torch.equal(out, ref.float())
    assert torch.equal(out[-2:], torch.zeros(2, 3))
    assert torch.equal(LA.smooth_torch(LA.Topology(f, V, 'cpu'), verts), ref.float())


def _align(v, f, use_kernels, epoch=3, dy=0.15):
    from recmv import nricp as K
    from recmv.engineer.optimizer import Laplacian_Optimizer
    mesh = K.TriMesh(v.to(DEV).clone(), f.to(DEV))
    names = list(CAPS)
    opt = Laplacian_Optimizer(epoch=epoch, use_kernels=use_kernels, log=lambda s: None)
    opt(source_fl_meshes=[mesh], target_meshes=[ring(n, dy=dy).to(DEV) for n in names], source_type=['long_sleeve_upper'],
        target_fl_type=names, outlayer=True)
    return mesh.verts, opt.history


def test_optimizer_kernel_path_matches_torch_path_and_reaches_the_curves():
    v, f = cut_sphere(4)
    uk, hk = _align(v, f, True)
    ut, ht = _align(v, f, False)
    assert (uk - ut).abs().max().item() <= 1e-5 * _diag(v)
    assert [h['pairs'] for h in hk] == [h['pairs'] for h in ht]
    assert all(h['iters'] > 0 and max(h['residual']) <= 1e-10 for h in hk)
    start, end = hk[0]['before'], hk[-1]['after']
    assert end < start / 5, (start, end)


def test_largest_template_converges():
    from recmv import lap_align as LA
    v, f = cut_sphere(6)
    assert v.shape[0] > 20000                                                 # level 6: 40962 vertices before the cut
    cw, cwt = _constraints(v, f)
    topo = LA.Topology(f, v.shape[0], DEV)
    u, iters, res = LA.solve(topo, v.to(DEV), cw, cwt)
    assert iters < LA.MAX_ITER and max(res) <= LA.TOL
    assert torch.isfinite(u).all()


# load_run(args, curves=True) in a child process (a loaded loop keeps device memory cached in the process that built it), saving
# the curve state it restored and the curves it evaluates
_LOAD_CURVES = """
import sys, torch
sys.path.insert(0, sys.argv[1])
from infer_fl import build_parser, load_run
optNet = load_run(build_parser().parse_args(['--gpu-ids', '0', '--rec-root', sys.argv[2], '--data-type', 'scene']),
                  curves=True)[0]
torch.save({'state': {k: v.cpu() for k, v in optNet.inter_free_curve.state_dict().items()},
            'curves': optNet.inter_free_curve.inference().cpu()}, sys.argv[3])
"""


def test_register_fl_align_curves_end_to_end(tmp_path):
    from recmv import utils
    import capture_fixture as cf
    from recmv.utils.constant import TEMPLATE_GARMENT
    env = dict(os.environ)
    subprocess.run([sys.executable, str(REPO / "tools" / "make_infer_run.py"), str(tmp_path / "a"), "--size", "128",
                    "--curves"], check=True, timeout=600, env=env)
    run = str(tmp_path / "a" / "capture" / "result")
    # the curves load_run restores equal the checkpoint's
    got = str(tmp_path / "curves.pt")
    out = subprocess.run([sys.executable, "-c", _LOAD_CURVES, str(REPO / "rec-mv_amd"), run, got], capture_output=True,
                         text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    loaded = torch.load(got, map_location="cpu")
    saved = torch.load(os.path.join(run, "latest.pth"), map_location="cpu")["model_state_dict"]
    keys = [k for k in saved if k.startswith("inter_free_curve.")]
    assert keys and all(torch.equal(loaded["state"][k[len("inter_free_curve."):]], saved[k]) for k in keys)
    s = {k[len("inter_free_curve."):]: saved[k] for k in keys}
    expect = s["cano_verts_center"] + s["cano_v_dirs"] * s["init_scale"] * torch.relu(s["scale"]) + s["nx_scale"] * s["cano_nx"]
    assert torch.allclose(loaded["curves"], expect, rtol=1e-6, atol=0.)
    shutil.copytree(str(tmp_path / "a"), str(tmp_path / "b"))
    run_b = str(tmp_path / "b" / "capture" / "result")
    v, f = cut_sphere(3)
    tpl = str(tmp_path / "template.obj")
    utils.write_obj(tpl, v * 0.3, f)
    names = TEMPLATE_GARMENT[cf.GARMENT_TYPE]

    def cmd(root):
        c = [sys.executable, str(REPO / "rec-mv_amd" / "register_fl.py"), "--gpu-ids", "0", "--rec-root", root,
             "--data-type", "scene", "--fit-epochs", "3", "--refine-epochs", "2", "--inner-iter", "10", "--dense-pcl", "600"]
        for n in names:
            c += ["--template", "%s=%s" % (n, tpl)]
        return c

    # a checkpoint without the curve keys is refused with a clear message
    shutil.copytree(str(tmp_path / "a"), str(tmp_path / "c"))
    run_c = str(tmp_path / "c" / "capture" / "result")
    ck = torch.load(os.path.join(run_c, "latest.pth"), map_location="cpu")
    ck["model_state_dict"] = {k: v for k, v in ck["model_state_dict"].items() if not k.startswith("inter_free_curve.")}
    torch.save(ck, os.path.join(run_c, "latest.pth"))
    out_c = subprocess.run(cmd(run_c) + ["--align-curves"], capture_output=True, text=True, timeout=600, env=env)
    assert out_c.returncode != 0 and "no feature curves" in out_c.stderr, out_c.stdout[-3000:] + out_c.stderr[-3000:]
    assert not any(os.path.exists(os.path.join(run_c, "registry_%s.obj" % n)) for n in names)
    out = subprocess.run(cmd(run) + ["--align-curves"], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    for n in names:
        assert "Laplacian align %s epoch 3/3" % n in out.stdout, out.stdout[-3000:]
    out_b = subprocess.run(cmd(run_b), capture_output=True, text=True, timeout=600, env=env)
    assert out_b.returncode == 0, out_b.stdout[-3000:] + out_b.stderr[-3000:]
    assert "Laplacian align" not in out_b.stdout
    for n in names:
        va, fa = utils.read_obj(os.path.join(run, "registry_%s.obj" % n))
        vb, fb = utils.read_obj(os.path.join(run_b, "registry_%s.obj" % n))
        assert torch.isfinite(va).all() and torch.equal(fa, fb)
        assert not torch.equal(va, vb)
