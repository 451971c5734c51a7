"""Feature-curve tubes without a GPU: the new entry points of librecmv_hip.so are exported and check their arguments before any
HIP call, `curve_to_mesh` refuses host tensors, the golden tube faces form a closed manifold, and infer_fl_curve.py carries the
reference's arguments."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(REPO / "rec-mv_amd"))


def edge_use_counts(faces):
    """How many faces use every undirected edge of a face table [F,3]."""
    f = np.asarray(faces).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


def test_new_entry_points_are_exported():
    from recmv import _lib
    lib = _lib.lib()                                            # _declare fails on a library without the two symbols
    assert lib.recmv_abi_version() == _lib.ABI_VERSION
    assert {"recmv_curve_tubes", "recmv_curve_fit_step"} <= set(_lib.exported_symbols())
    assert lib.recmv_curve_tubes.restype is C.c_int and lib.recmv_curve_fit_step.restype is C.c_int


def test_curve_tubes_checks_its_arguments_without_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    n, p = None, C.c_void_p(16)
    tubes = lib.recmv_curve_tubes
    for L_, S, J in ((0, 24, 6), (4, 0, 6), (4, 24, 0), (-1, 24, 6)):
        assert tubes(p, p, 0.002, L_, S, J, p, p, n) == -1
        assert b"must be at least 1" in lib.recmv_last_error()
    for J in (7, 11, 361, 720):
        assert tubes(p, p, 0.002, 4, 24, J, p, p, n) == -1
        assert b"must divide 360" in lib.recmv_last_error()
    assert tubes(p, p, 0.002, 1 << 19, 1 << 19, 6, p, p, n) == -1
    assert b"too many" in lib.recmv_last_error()
    assert tubes(p, p, float("nan"), 4, 24, 6, p, p, n) == -1
    assert b"NaN" in lib.recmv_last_error()
    for args in ((n, p, p, p), (p, n, p, p), (p, p, n, p), (p, p, p, n)):
        assert tubes(args[0], args[1], 0.002, 4, 24, 6, args[2], args[3], n) == -1
        assert b"NULL" in lib.recmv_last_error()


def test_curve_fit_step_checks_its_arguments_without_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    n, p = None, C.c_void_p(16)
    step = lib.recmv_curve_fit_step

    def call(L_=4, S=200, P=4, M=2000, w=(1000., 0.1), ptrs=None):
        q = ptrs or [p] * 11
        return step(*q[:8], L_, S, P, M, w[0], w[1], *q[8:], n)

    for kw in (dict(L_=0), dict(S=0), dict(P=0), dict(M=0), dict(S=-3)):
        assert call(**kw) == -1
        assert b"must be at least 1" in lib.recmv_last_error()
    assert call(S=200, M=5000) == -1                                   # (12 * 200 + 4 * 5000) * 4 bytes > 64 KiB
    assert b"LDS" in lib.recmv_last_error()
    assert call(S=2000, M=2000) == -1
    assert b"LDS" in lib.recmv_last_error()
    assert call(L_=70000) == -1                                        # more curves than a grid axis holds
    assert call(w=(float("nan"), 0.1)) == -1
    assert b"NaN" in lib.recmv_last_error()
    for k in range(11):
        assert call(ptrs=[n if i == k else p for i in range(11)]) == -1
        assert b"NULL" in lib.recmv_last_error()


def test_curve_ops_refuse_host_tensors():
    from recmv import curves as fl
    t = torch.linspace(0, 2 * np.pi, 25)[:-1]
    ring = torch.stack([torch.cos(t), 0.1 * torch.sin(2 * t), torch.sin(t)], -1)
    curve = fl.Intersect_Free_Curve([ring, 0.5 * ring + 1, 0.7 * ring - 1, 0.3 * ring], [ring] * 4, ['a', 'b', 'c', 'd'])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        curve.curve_to_mesh()
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        fl.curve_tubes(curve.inference(), curve.cano_nx[:, 0])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        fl.fit_step(curve, torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        fl.fit_curves_to_loops(curve, [ring], [0], iters=1)
    # the torch statement of the objective runs anywhere and is differentiable in the two parameters
    loss = fl.fit_step_torch(curve, [1.1 * ring, 0.4 * ring], [0, 3])
    g = torch.autograd.grad(loss.sum(), [curve.scale, curve.nx_scale])
    assert loss.shape == (2,) and all(torch.isfinite(x).all() for x in g)
    assert g[0][1].abs().max() == 0 and g[0][0].abs().max() > 0        # only the targeted curves move


@pytest.mark.parametrize("J", [6, 4])
def test_golden_tube_faces_are_a_closed_manifold(J):
    g = np.load(GOLD / "curve_tubes.npz")
    verts, faces = g["tube_verts_j%d" % J], g["tube_faces_j%d" % J]
    S = g["tube_curves"].shape[1]
    assert verts.shape == (4, S * J, 3) and faces.shape == (4, 2 * S * J, 3) and faces.dtype == np.int64
    for f in faces:
        assert f.min() == 0 and f.max() == S * J - 1                   # indices local to the curve
        assert (edge_use_counts(f) == 2).all()                          # every edge is used by exactly two faces
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    merged = g["fl_faces"]
    assert merged.min() == 0 and merged.max() == g["fl_verts"].shape[0] - 1 and (edge_use_counts(merged) == 2).all()


def test_infer_fl_curve_help_lists_the_reference_arguments():
    out = subprocess.run([sys.executable, str(REPO / "rec-mv_amd" / "infer_fl_curve.py"), "--help"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for flag in ("--gpu-ids", "--batch-size", "--rec-root", "--frames", "--nV", "--nI", "--C", "--nColor", "--data-type",
                 "--a_pose", "--fit-registry", "--fit-iters", "--curve-radius", "--curve-joints"):
        assert flag in out.stdout, flag
