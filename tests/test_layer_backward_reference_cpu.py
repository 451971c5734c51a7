"""The float64 references of tests/layer_backward_reference.py against float64 autograd, and every condition on the test
inputs that the bounds of that module rely on (the GPU tests of tests/test_gpu_layer_backward.py use the same inputs)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import layer_backward_reference as R  # noqa: E402

SHAPES = [(7, 5, 3), (33, 12, 9)]


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_layer_backward_reference_equals_autograd(act, M, N, K):
    g = torch.Generator().manual_seed(M + act)
    p = 3.0 if act == R.ACT_SOFTPLUS else 0.0
    x = torch.randn(M, K, generator=g, dtype=torch.float64, requires_grad=True)
    W = torch.randn(N, K, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(N, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(M, N, generator=g, dtype=torch.float64)
    z = x @ W.t() + b
    y = R.act_fn(z, act, p)
    gx, gW, gb = torch.autograd.grad(y, [x, W, b], gy)
    ref = R.layer_backward(gy, y, x, W, act, p)
    _close(ref["gx"], gx)
    _close(ref["gW"], gW)
    _close(ref["gb"], gb)
    # act'(z) through y, and its derivative: act''(z) = d(act')/dy * dy/dz
    z1 = z.detach().requires_grad_(True)
    y1 = R.act_fn(z1, act, p)
    d1, = torch.autograd.grad(y1.sum(), z1, create_graph=True)
    _close(R.dact(y1, act, p), d1.detach())
    if d1.requires_grad:
        d2, = torch.autograd.grad(d1.sum(), z1)
    else:
        d2 = torch.zeros_like(z1)
    _close(R.d2act(y1, act, p) * R.dact(y1, act, p), d2)


@pytest.mark.parametrize("rows,cols", [(5, 3), (17, 40)])
def test_weight_norm_reference_equals_autograd(rows, cols):
    g = torch.Generator().manual_seed(rows)
    v = torch.randn(rows, cols, generator=g, dtype=torch.float64, requires_grad=True)
    gg = (torch.rand(rows, 1, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
    gW = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    W = gg * v / v.norm(dim=1, keepdim=True)
    a_v, a_g = torch.autograd.grad(W, [v, gg], gW)
    Wr, n = R.weight_norm(v, gg)
    gv, ggr, T = R.weight_norm_backward(v, gg, gW)
    _close(Wr, W.detach())
    _close(n, v.detach().norm(dim=1))
    _close(gv, a_v)
    _close(ggr, a_g.reshape(-1))
    assert (T >= ggr.abs() - 1e-12).all()


def test_gather_and_add_scaled_references():
    t = torch.arange(12.).reshape(4, 3)
    idx = torch.tensor([3, 0, 3, 1, 1])
    out = R.gather_rows(t, idx, 5, 2, 4)
    assert torch.equal(out[:, :2], t.index_select(0, idx)[:, :2]) and torch.equal(out[:, 2:], torch.zeros(5, 2))
    assert torch.equal(R.gather_rows(t, None, 3, 3, 3), t[:1].expand(3, 3))
    assert torch.equal(R.gather_rows(t, None, 3, 0, 2), torch.zeros(3, 2))
    a, b = torch.tensor([1., 2.]), torch.tensor([4., -8.])
    assert torch.equal(R.add_scaled(a, 0.5, b), torch.tensor([3., -2.], dtype=torch.float64))


@pytest.mark.parametrize("M,N,K,act", R.LINEAR_CASES)
def test_exact_integer_inputs_stay_below_2_to_24(M, N, K, act):
    c = R.int_case(M, N, K, act)
    assert c["act"] in (R.ACT_NONE, R.ACT_RELU)
    assert set(c["gy"].unique().tolist()) <= {-3., -2., -1., 0., 1., 2., 3.}
    assert set(c["y"].unique().tolist()) <= {-1., 0., 1., 2.}
    for k in ("x", "W"):
        assert set(c[k].unique().tolist()) <= {-2., -1., 0., 1., 2.}
    # sum |gz| |B| bounds every partial sum of every summation order
    assert c["integral"] and c["peak"] < 2 ** 24
    if M >= 255 and N >= 5:
        assert c["want"]["gb"].abs().max() > 0 and c["want"]["gx"].abs().max() > 0 and c["want"]["gW"].abs().max() > 0


def _check_activation_outputs(y, act, p):
    if act == R.ACT_SOFTPLUS:
        t = p * y.double()
        assert (y >= 0).all()
        if y.numel() >= 64:
            assert (y == 0).any()
            assert t[t > 0].min() <= 1.0001e-5, "beta y must reach down to 1e-5, where 1 - exp(-beta y) cancels"
            assert (t > 104).any()
            assert ((t > 1e-3) & (t < 10)).any()
    if act == R.ACT_TANH:
        assert (y.abs() <= 1).all()


@pytest.mark.parametrize("M,N,K,act", R.BOUNDED_CASES)
def test_rounding_inputs_meet_the_conditions_of_the_bounds(M, N, K, act):
    c = R.float_case(M, N, K, act)
    _check_activation_outputs(c["y"], act, c["p"])
    if M >= 255:
        rows = c["gy"].abs().double().mean(1)
        assert rows[-1] / rows[0] > 1e4, "the rows of gy span several decades"
    for k in ("gz", "gb", "gx", "gW"):
        assert c["bound"][k].shape == c["ref"][k].shape and (c["bound"][k] >= 0).all() and torch.isfinite(c["bound"][k]).all()
    # the any-order sum bound is the maintainer's first-order form plus second-order terms only
    gza = c["ref"]["gz"].abs()
    first_order = c["bound"]["gz"].sum(0) + (M - 1) * R.U * gza.sum(0)
    assert (c["bound"]["gb"] >= first_order).all() and (c["bound"]["gb"] <= first_order * 1.01 + 1e-300).all()


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("n", R.ACT_GRAD_N)
def test_flat_activation_inputs_meet_the_conditions(n, act):
    gy, b, y = R.act_inputs(n, act)
    assert gy.shape == b.shape == y.shape == (n,)
    _check_activation_outputs(y, act, R.act_param(act))
    assert torch.isfinite(R.bound_act_grad2(gy, b, y, act, R.act_param(act))).all()


@pytest.mark.parametrize("rows", R.WN_ROWS)
@pytest.mark.parametrize("cols", R.WN_COLS)
def test_weight_norm_inputs_have_norms_away_from_one(rows, cols):
    v, g, gW = R.wn_inputs(rows, cols)
    n = v.double().norm(dim=1)
    away = ((n - 1).abs() > 0.05).double().mean()
    assert (n > 0).all() and away >= 0.9, "a dropped 1/|v| must change most rows"
    if rows > 1:
        assert n.max() / n.min() > 1e3 and (g > 0).any() and (g < 0).any()


def test_softplus_bound_separates_expm1_from_one_minus_exp():
    """A float32 evaluation with expm1 meets the dZ bound on the test's own inputs; the cancelling form 1 - exp(-beta y) does not."""
    c = R.float_case(255, 64, 39, R.ACT_SOFTPLUS)
    gy, y = c["gy"].numpy(), c["y"].numpy()
    t = np.float32(-R.BETA) * y
    good = torch.from_numpy(gy * -np.expm1(t))
    bad = torch.from_numpy(gy * (np.float32(1) - np.exp(t)))
    assert good.dtype == bad.dtype == torch.float32
    assert R.ratio((good.double() - c["ref"]["gz"]).abs(), c["bound"]["gz"]) <= 1.0
    assert R.ratio((bad.double() - c["ref"]["gz"]).abs(), c["bound"]["gz"]) > 100.0


@pytest.mark.parametrize("M,N,K,act", R.NEAR_ZERO_CASES)
def test_near_zero_case_shows_one_minus_exp_in_the_layer_outputs(M, N, K, act):
    """The near-zero inputs keep beta y in [1e-5, 1e-4]; with dZ from the cancelling form, evaluated in float32 and multiplied in
    float64 (no other error), gb, gx and gW all leave their bounds, and with expm1 they stay inside."""
    c = R.float_case(M, N, K, act, True)
    t = c["p"] * c["y"].double()
    assert (t >= 0.99e-5).all() and (t <= 1.01e-4).all()
    gy, y = c["gy"].numpy(), c["y"].numpy()
    tf = np.float32(-R.BETA) * y
    for dz, inside in ((gy * -np.expm1(tf), True), (gy * (np.float32(1) - np.exp(tf)), False)):
        gz = torch.from_numpy(dz).double()
        got = {"gb": gz.sum(0), "gx": gz @ c["W"].double(), "gW": gz.t() @ c["x"].double()}
        for k in got:
            r = R.ratio((got[k] - c["ref"][k]).abs(), c["bound"][k])
            assert (r <= 1.0) if inside else (r > 10.0), (k, r)


def test_ratio_counts_an_error_at_a_zero_bound_as_a_failure():
    assert R.ratio(torch.tensor([0., 1.]), torch.tensor([0., 2.])) == 0.5
    assert R.ratio(torch.tensor([1e-30]), torch.tensor([0.])) == float("inf")
