"""Plain float64 references, descriptors, test inputs and error bounds for the whole-MLP passes: the per-layer chain
(csrc/mlp_chain.hip), the row-tile kernels (csrc/mlp_rows.hip) and the jet pass (csrc/mlp_jet.hip).

Everything here runs on the host in float64 from float32 inputs and imports nothing from recmv: only the value-with-bound class E and
the positional encoding of tests/skinning_reference.py and the float64 activations and the product bound of
tests/layer_backward_reference.py.  tests/test_mlp_reference_cpu.py checks the references against float64 autograd of a plain torch
composition; tests/test_gpu_mlp_passes.py judges the kernels.

The network, as include/recmv_hip.h states it:
  input   = [gamma_L(x) * pe_weights | cond[cond_index[p]]]
  layer l = act(h W[l]^T + b[l]);  [h | gamma] / sqrt2 in front of skip_layer;  the last layer is linear and only its first n_out rows
  are evaluated;  residual nets: out = x + out;  a second weight set serves the rows >= split_row.
  VJP     = J(x)^T g, a NULL cotangent meaning ones on output 0.
  jet     : y and tang[k*P + p, j] = dy_j / dx_k (without the residual's identity); its reverse sweep, as the header of mlp_jet.hip writes
            it: zbar = ybar phi' + phi'' sum_k sbar_k u_k, ubar_k = sbar_k phi', Wbar = [zbar; ubar]^T [h; t], bbar = colsum(zbar), down
            through gamma with the second-derivative form for the tangent rows.

How the bounds are formed.  Every quantity travels as an E pair (v, e) of skinning_reference: v is the exact float64 value of the
network above for the exact float32 inputs, e bounds the distance of ANY float32 evaluation that uses the family's operations.
  matrix products   the project's own product bound (test_gemm_nt_vs_fp64, bound_product): 4e-7 sum |a||b| + 1e-6, with the errors of
                    BOTH operands carried linearly: 4e-7 (|a|+e_a).(|b|+e_b) + e_a.(|b|+e_b) + |a|.e_b + 1e-6.  No gamma_(K-1) rule is
                    substituted for an MFMA product.
  element-wise sums the esum rule (any order): the encoding's VJP, colsum, the jet's sum over the three tangents, and the sum of the
                    eight waves' partial products of the last layer in mlp_rows_fwd_kernel (gamma_7 on top of the product bound).
  constants         1/sqrt2, sqrt2, log2 e, ln 2, 1/3, 1/6, 1/24 and 1/beta enter as E(true value, |float32 constant - true value|).
  activations       each family's formulas are WRITTEN OUT in E arithmetic, operation by operation as the kernel has them, so every
                    rounding, every cancellation (1 - exp(-beta y) next to the 1/64 switch; 1 - sig in the jet's phi'') and the error
                    of the argument (beta e^(-beta y) e_y for softplus' act' through y) is counted by the rules of E and not by hand:
                      chain   forward: the GEMM epilogue (gemm_f32.hip apply_act): zb = z beta, t = __expf(-|zb|) = exp2(-|zb| log2e),
                              log1p(t) by t(1 - t(1/2 - t(1/3 - t/4))) below 1/64 and __logf(1 + t) = log2(1 + t) ln2 above,
                              (max(zb,0) + l) / beta, z itself for zb > 20; tanhf.  act' through y: recmv_act_grad_2d
                              (-expm1f(-beta y); 1 - y y) for the first dZ of a run and the epilogue of recmv_gemm_nt_mulgrad (dact_y:
                              t(1 - t(1/2 - t(1/6 - t/24))) below 1/64, 1 - __expf(-t) above) where the chain fuses it.
                      rows    softplus_fwd / softplus_grad of mlp_rows.hip: the same two formulas on the hardware units.
                      jet     act_jet: expf, log1pf, tanhf and a division; sig = 1/(1+e) or e/(1+e), phi'' = beta sig (1 - sig).
                    The value of a formula in float64 differs from the exact activation by its truncation (the series) or its step
                    (e^-20 / beta in the beta z > 20 branch): |formula - exact| is added to e.  Where the argument lies within its own
                    error of a switch point (t = 1/64, beta z = 20) the kernel may take either branch: the larger of the two bounds.
                    The error e_z of the argument goes through the activation's own Lipschitz constant over [z - e_z, z + e_z] and
                    the formula's error is taken at the ends and the centre of that interval (_through).
  underflow         softplus(100) drives exp(-beta |z|) below the normal range for z < -0.87, which the nets here reach: every softplus
                    output and derivative carries 16 beta 2^-126 for it.  Nothing else in the passes leaves the normal range
                    (pre-activations, products and outputs are checked on the host).
  ReLU              act' flips where a hidden |z| is within its own bound: those rows are left out of the bounded comparison (at most
                    1 % per case, checked on the host) and are still checked for finiteness.

Function accuracies (ulp).  expm1f, expf, sinf, cosf, sincosf: the allowances of the two earlier reference modules as they stand.
The hardware exp2 and log2 (v_exp_f32, v_log_f32) are specified to 1 ulp; log1pf and tanhf of the device library to 2 ulp (OpenCL
full-profile figures, which the ROCm device library is built to).  test_gpu_mlp_passes.py::test_activation_sweep runs a one-unit net
(n = 2, multires 0, W0 = [1,0,0], W1 = [1]: out = act(x_0), gx_0 = act'(.), the jet's tang = phi' and its gx under a one-hot gtang =
phi'') over log-spaced |z| of both signs across every switch point, judges every sample with the bound BUILT FROM these per-function
allowances and the formula's roundings (not with an allowance for the activation as a whole: a changed series coefficient fails it),
and prints the largest error in units of u.  Allowances: the specified figure plus one ulp, because a sweep is finite:
HWEXP2_ULP = HWLOG2_ULP = 2, LOG1PF_ULP = TANHF_ULP = 3.
Measured on an MI355X (gfx950, ROCm 7.2), largest relative error over the samples whose exact value is a normal float32, in u = 2^-24
(1 ulp is between 1 and 2 u):
  tanhf                          2.08 u (1.04 ulp; rounded up 2, allowance 3) in all three families
  softplus(100), chain and rows  82.4 u, at beta |z| near 87, where rounding beta z alone moves exp(-beta |z|) by beta |z| u
  act' through y, chain          1.88 u (expm1f form);   tanh 0.96 u
  act' through y, rows           24.1 u (1 - exp(-t) just above t = 1/64: the cancellation the bound carries)
  jet softplus                   phi 40.5 u, phi' 60 u (both at large beta |z|), phi'' 1.36 u beta absolute
  jet tanh                       phi' 106 u relative (1 - t^2 next to |t| = 1), phi'' 1.99 u absolute
Largest error / bound of the sweeps below the beta z = 20 step: 0.74 (softplus, chain and rows), 0.72 (act' through y, rows), 0.78
(the jet's softplus, all three outputs), 0.50 at the most for tanh; beyond the step the bound is the step itself.  The hardware exp2
and log2 cannot be isolated further through the ABI: they are judged inside these formulas.

Exact-integer cases: x in {-2..2}, weights in {-1, 0, 1}, biases in {-1..1}, codes in {-2..2}, cotangents in {-3..3}, multires 0, ReLU,
no skip: every product and partial sum is an integer below 2^24 (int_peak, asserted on the host): torch.equal in every summation
order, and one dropped, doubled or misplaced column, row or code index changes the result.
"""
import functools
import math

import numpy as np
import torch

import layer_backward_reference as LB
import skinning_reference as R
from layer_backward_reference import ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_TANH, EXPF_ULP, EXPM1F_ULP, _gen
from skinning_reference import E, U, ecat, esum, f64, gamma, ratio  # noqa: F401

HWEXP2_ULP = 2.0
HWLOG2_ULP = 2.0
LOG1PF_ULP = 3.0
TANHF_ULP = 3.0
TINY = 2.0 ** -126
MAX_LAYERS = 12
FAMILIES = ("chain", "rows", "jet")


def _const(true, f32):
    return E(torch.tensor(true, dtype=torch.float64), torch.tensor(abs(float(np.float32(f32)) - true), dtype=torch.float64))


C_INV = _const(math.sqrt(0.5), 0.70710678118654752440)
C_SQRT2 = _const(math.sqrt(2.0), 1.41421356237309504880)
C_LOG2E = _const(1.0 / math.log(2.0), 1.4426950408889634)
C_LN2 = _const(math.log(2.0), 0.69314718)
C_3 = _const(1.0 / 3.0, 0.33333334)
C_6 = _const(1.0 / 6.0, 0.16666667)
C_24 = _const(1.0 / 24.0, 0.041666668)


# ----------------------------------------------------------------------------------------------------- function rules on E
def eabs(x):
    return E(x.v.abs(), x.e)


def emax0(x):
    """max(x, 0): exactly 0 where x is negative beyond its error."""
    return E(x.v.clamp_min(0), torch.where(x.v + x.e < 0, torch.zeros_like(x.e), x.e))


def _fun(v, p, ulp):
    return E(v, p + 2.0 * ulp * U * (v.abs() + p))


def eexp(x, ulp):
    v = torch.exp(x.v)
    return _fun(v, v * torch.expm1(x.e), ulp)


def eexp_hw(x):
    """__expf(x) = exp2(x * log2e) on the hardware unit."""
    a = x * C_LOG2E
    v = torch.exp(x.v)
    return _fun(v, v * torch.expm1(a.e * math.log(2.0)), HWEXP2_ULP)


def elog_hw(x):
    """__logf(x) = log2(x) * ln2 on the hardware unit, x >= 1."""
    assert bool((x.v - x.e > 0.5).all())
    l2 = _fun(torch.log2(x.v), x.e / (x.v - x.e) / math.log(2.0), HWLOG2_ULP)
    return l2 * C_LN2


def elog1p(x, ulp):
    assert bool((x.v - x.e > -0.5).all())
    return _fun(torch.log1p(x.v), x.e / (1.0 + x.v - x.e), ulp)


def eexpm1(x, ulp):
    v = torch.expm1(x.v)
    return _fun(v, torch.exp(x.v) * torch.expm1(x.e), ulp)


def etanh(x, ulp):
    v = torch.tanh(x.v)
    return _fun(v, torch.minimum(x.e, 2.0 * torch.ones_like(x.e)), ulp)


def _under(x, p):
    """exp(-beta |z|) leaves the normal range below beta |z| = 87.3 (softplus(100) at z < -0.87): a flushed or subnormal result is
    within 2^-126 of the exact one, and the few operations behind it scale that by beta at the most."""
    return E(x.v, x.e + 16.0 * TINY * max(abs(p), 1.0))


def _pick(first, a, b, exact, arg, switch):
    """a where `first` else b, re-centred on the exact value; where arg lies within its own error of the switch point either
    branch may have been taken: the larger bound."""
    ea, eb = a.e + (a.v - exact).abs(), b.e + (b.v - exact).abs()
    near = (arg.v - switch).abs() <= 2.0 * arg.e + 4.0 * U * abs(switch)
    return E(exact, torch.where(near, torch.maximum(ea, eb), torch.where(first, ea, eb)))


# ----------------------------------------------------------------------------------------------------------- activations
def _inv(p):
    return _const(1.0 / p, np.float32(1.0) / np.float32(p))


def _through(fn, z, lip):
    """The formula fn at an argument known to e_z: |fn^(z^) - f(z)| <= |fn^(z^) - f(z^)| + |f(z^) - f(z)|.  The second term is lip e_z
    with lip a bound on |f'| over [z - e_z, z + e_z]; the first, the formula's own rounding, truncation and step, is evaluated at both
    ends and at the centre of that interval (it follows the magnitudes of the formula's intermediates, which are monotone between
    switch points; an interval that straddles a switch point gets the larger branch through its two ends)."""
    outs = [fn(E(z.v)), fn(E(z.v - z.e)), fn(E(z.v + z.e))]
    many = isinstance(outs[0], tuple)
    if not many:
        outs, lip = [(o,) for o in outs], (lip,)
    res = tuple(E(c.v, l * z.e + torch.maximum(c.e, torch.maximum(a.e, b.e))) for c, a, b, l in zip(outs[0], outs[1], outs[2], lip))
    return res if many else res[0]


def act_forward(z, act, p, family):
    """act(z) for the E pre-activation z, by the family's formula (every activation here is 1-Lipschitz)."""
    if act in (ACT_NONE, ACT_RELU):
        return _act_forward(z, act, p, family)
    return _through(lambda a: _act_forward(a, act, p, family), z, 1.0)


def act_grad_y(y, act, p, form):
    """act'(z) through the E output y = act(z).  form: 'expm1' (recmv_act_grad_2d) or 'hw' (dact_y / softplus_grad).
    d act'/dy = beta exp(-beta y) for softplus, -2 y for tanh."""
    if act in (ACT_NONE, ACT_RELU):
        return _act_grad_y(y, act, p, form)
    lip = p * torch.exp(-p * (y.v - y.e).clamp_min(0)) if act == ACT_SOFTPLUS else 2.0 * (y.v.abs() + y.e)
    return _through(lambda a: _act_grad_y(a, act, p, form), y, lip)


def act_jet(z, act, p):
    """phi, phi', phi'' at the E pre-activation z, by act_jet of mlp_jet.hip.  Lipschitz constants: 1 for phi; for phi' the largest
    phi'' over the interval (softplus: beta s (1 - s) at the point of the interval nearest to 0; tanh: 4 / (3 sqrt 3)); for phi'' the
    largest third derivative (softplus: beta^2 / (6 sqrt 3); tanh: 2)."""
    if act in (ACT_NONE, ACT_RELU):
        return _act_jet(z, act, p)
    if act == ACT_SOFTPLUS:
        s = torch.sigmoid(p * (z.v.abs() - z.e).clamp_min(0))
        lips = (1.0, p * s * (1.0 - s), p * p / (6.0 * math.sqrt(3.0)))
    else:
        lips = (1.0, 4.0 / (3.0 * math.sqrt(3.0)), 2.0)
    return _through(lambda a: _act_jet(a, act, p), z, lips)


def _act_forward(z, act, p, family):
    if act == ACT_NONE:
        return z
    if act == ACT_RELU:
        return emax0(z)
    if act == ACT_TANH:
        return etanh(z, TANHF_ULP)
    exact = LB.act_fn(z.v, ACT_SOFTPLUS, p)
    zb = z * p
    if family == "jet":
        e = eexp(-eabs(zb), EXPF_ULP)
        y = (emax0(zb) + elog1p(e, LOG1PF_ULP)) / p
    else:
        t = eexp_hw(-eabs(zb))
        series = t * (1.0 - t * (0.5 - t * (C_3 - t.scaled(0.25))))
        l = _pick(t.v < 0.015625, series, elog_hw(1.0 + t), torch.log1p(t.v), t, 0.015625)
        y = (emax0(zb) + l) * _inv(p)
    return _under(_pick(zb.v > 20.0, z, y, exact, zb, 20.0), p)


def _act_grad_y(y, act, p, form):
    if act == ACT_NONE:
        return E(torch.ones_like(y.v))
    if act == ACT_RELU:
        return E((y.v > 0).double())
    if act == ACT_TANH:
        return 1.0 - y * y
    exact = -torch.expm1(-p * y.v)
    t = y * p
    if form == "expm1":
        d = -eexpm1(-t, EXPM1F_ULP)
        return _under(E(exact, d.e + (d.v - exact).abs()), p)
    series = t * (1.0 - t * (0.5 - t * (C_6 - t * C_24)))
    return _under(_pick(t.v < 0.015625, series, 1.0 - eexp_hw(-t), exact, t, 0.015625), p)


def _act_jet(z, act, p):
    one, nil = E(torch.ones_like(z.v)), E(torch.zeros_like(z.v))
    if act == ACT_NONE:
        return z, one, nil
    if act == ACT_RELU:
        return emax0(z), E((z.v > 0).double()), nil
    if act == ACT_TANH:
        t = etanh(z, TANHF_ULP)
        d1 = 1.0 - t * t
        return t, d1, t.scaled(-2.0) * d1
    zb = z * p
    e = eexp(-eabs(zb), EXPF_ULP)
    pos = zb.v >= 0
    a, b = 1.0 / (1.0 + e), e / (1.0 + e)
    sig = E(torch.where(pos, a.v, b.v), torch.where(pos, a.e, b.e))
    f = (emax0(zb) + elog1p(e, LOG1PF_ULP)) / p
    d2 = E(torch.tensor(float(p), dtype=torch.float64)) * sig * (1.0 - sig)
    s = torch.sigmoid(p * z.v)
    big = zb.v > 20.0
    return (_under(_pick(big, z, f, LB.act_fn(z.v, ACT_SOFTPLUS, p), zb, 20.0), p), _under(_pick(big, one, sig, s, zb, 20.0), p),
            _under(_pick(big, nil, d2, p * s * (1.0 - s), zb, 20.0), p))


# ------------------------------------------------------------------------------------------------------------ descriptors
def make_net(name, n, L, rows, act, skip=-1, cond_dim=0, residual=False, p=None, pe_w=None, bias=True, key=0, integer=False):
    """A descriptor with weights N(0,1)/sqrt(K) and biases N(0, 0.1) seeded from the case key (integer: entries in {-1,0,1})."""
    d_pe = 3 + 6 * L
    dims = [d_pe + cond_dim]
    for l in range(n):
        dims.append(rows[l] + (d_pe if l + 1 == skip else 0))
    g = _gen(11, key, n, L, *rows)
    W, b = [], []
    for l in range(n):
        if integer:
            W.append(torch.randint(-1, 2, (rows[l], dims[l]), generator=g).float())
            b.append(torch.randint(-1, 2, (rows[l],), generator=g).float() if bias else None)
        else:
            W.append((torch.randn(rows[l], dims[l], generator=g) / math.sqrt(dims[l])).float())
            b.append((0.1 * torch.randn(rows[l], generator=g)).float() if bias else None)
    p = (LB.BETA if act == ACT_SOFTPLUS else 0.0) if p is None else p
    return {"name": name, "n": n, "L": L, "rows": list(rows), "dims": dims, "act": act, "p": float(p), "skip": skip, "cond_dim": cond_dim,
            "residual": bool(residual), "W": W, "b": b, "pe_w": [1.0] * (2 * L) if pe_w is None else [float(np.float32(w)) for w in pe_w],
            "W2": None, "b2": None, "split": 0}


def with_second(net, key=1):
    other = make_net(net["name"], net["n"], net["L"], net["rows"], net["act"], net["skip"], net["cond_dim"], net["residual"], net["p"],
                     net["pe_w"], key=key + 100)
    out = dict(net)
    out.update(name="two", W2=other["W"], b2=other["b"], split=128)
    return out


def second_of(net):
    out = dict(net)
    out.update(W=net["W2"], b=net["b2"], W2=None, b2=None, split=0)
    return out


@functools.lru_cache(maxsize=None)
def net(name):
    if name == "unit_softplus" or name == "unit_tanh":
        m = make_net(name, 2, 0, [1, 1], ACT_SOFTPLUS if name.endswith("softplus") else ACT_TANH, bias=False)
        m["W"] = [torch.tensor([[1.0, 0.0, 0.0]]), torch.tensor([[1.0]])]
        return m
    if name == "one":
        return make_net(name, 1, 2, [3], ACT_SOFTPLUS, residual=True)
    if name == "offset":
        return make_net(name, 3, 2, [17, 33, 3], ACT_RELU, cond_dim=6, residual=True)
    if name == "sdf":
        # six bands, annealed: bands 3 and 4 partly faded, band 5 at 0
        return make_net(name, 4, 6, [40, 25, 48, 7], ACT_SOFTPLUS, skip=2, pe_w=[1, 1, 1, 1, 1, 1, 0.75, 0.75, 0.25, 0.25, 0, 0])
    if name == "skip_last":
        return make_net(name, 3, 1, [20, 11, 2], ACT_TANH, skip=2)
    if name == "skip_first":
        return make_net(name, 3, 0, [13, 16, 1], ACT_RELU, skip=1)
    if name == "deep":
        return make_net(name, 12, 1, [8] * 12, ACT_SOFTPLUS)
    if name == "wide":
        return make_net(name, 3, 8, [512, 461, 16], ACT_SOFTPLUS, skip=2)
    if name == "bands16":
        return make_net(name, 2, 16, [9, 2], ACT_TANH)
    if name == "two":
        return with_second(net("sdf"))
    if name == "last528":
        return make_net(name, 2, 1, [24, 528], ACT_SOFTPLUS)
    if name == "int_offset":
        return make_net(name, 3, 0, [17, 33, 3], ACT_RELU, cond_dim=6, residual=True, integer=True)
    if name == "int_plain":
        return make_net(name, 3, 0, [19, 21, 5], ACT_RELU, integer=True)
    raise KeyError(name)


NETS = ("one", "offset", "sdf", "skip_last", "skip_first", "deep", "wide", "bands16", "two", "last528", "int_offset", "int_plain")
COND_ROWS, COND_LD = 4, 9


def rows_supported(m):
    """The header's rule: 2..12 layers, widths <= 512 (every layer's inputs and outputs, the last layer's included), <= 8 bands,
    one net, the skip (if any) not on layer 0."""
    if not (2 <= m["n"] <= MAX_LAYERS) or not (0 <= m["L"] <= 8) or (m["split"] > 0 and m["W2"] is not None):
        return 0
    if any(d > 512 for d in m["dims"][:m["n"]]) or any(r > 512 for r in m["rows"]):
        return 0
    return 0 if (m["skip"] == 0 or m["skip"] >= m["n"]) else 1


def make_inputs(m, P, key=0, integer=False):
    """x [P,3], the code table [COND_ROWS, cond_dim] with its index [P], cotangents g [P, rows_last] and gt [3P, rows_last]."""
    g = _gen(12, key, P, m["n"], m["L"])
    last = m["rows"][-1]
    if integer:
        x = torch.randint(-2, 3, (P, 3), generator=g).float()
        cond = torch.randint(-2, 3, (COND_ROWS, max(m["cond_dim"], 1)), generator=g).float()
        gy = torch.randint(-3, 4, (P, last), generator=g).float()
        gt = torch.randint(-3, 4, (3 * P, last), generator=g).float()
    else:
        x = (0.5 * torch.randn(P, 3, generator=g)).float()
        cond = torch.randn(COND_ROWS, max(m["cond_dim"], 1), generator=g).float()
        gy = torch.randn(P, last, generator=g).float()
        gt = torch.randn(3 * P, last, generator=g).float()
    idx = torch.randint(0, COND_ROWS, (P,), generator=g)
    if P >= 2:
        idx[0], idx[-1] = COND_ROWS - 1, 0
    return {"x": x, "cond": cond[:, :m["cond_dim"]], "idx": idx, "gy": gy, "gt": gt}


def sweep_x():
    """x [n,3] = (z, 0, 0) for the one-unit nets: |z| log-spaced over [1e-7, 3.2] in both signs, plus the switch points of
    softplus(100) and their neighbours (t = 1/64 at beta |z| = 4.159, beta z = 20, beta y = 1/64)."""
    mag = torch.logspace(-7, 0.5, 4096, dtype=torch.float64)
    extra = torch.tensor([0.0, 0.2, 0.0416, 0.0415, 0.0417, 0.199999, 0.200001, 1.0 / 6400.0])
    z = torch.cat([mag, -mag, extra, -extra]).float()
    return torch.cat([z.unsqueeze(1), torch.zeros(z.numel(), 2)], 1).contiguous()


# -------------------------------------------------------------------------------------------------------------- products
def eprod(a, B):
    """a [M,K] (E) times B [K,N] (E or exact tensor): the project's product bound with both operands' errors carried."""
    B = E.lift(B)
    Bm = B.v.abs() + B.e
    e = 4e-7 * ((a.v.abs() + a.e) @ Bm) + a.e @ Bm + a.v.abs() @ B.e + 1e-6
    return E(a.v @ B.v, e)


def _encode(m, x):
    return R.posenc(x, m["L"], m["pe_w"] if m["L"] else None)


def _input(m, x, cond, idx):
    g = _encode(m, x)
    if not m["cond_dim"]:
        return g
    rows = f64(cond)[idx] if idx is not None else f64(cond)[:1].expand(x.shape[0], -1)
    return ecat([g, E(rows)], -1)


def _bias(z, b):
    return z if b is None else z + E(f64(b))


def _pe_vjp(m, x, g, t=None):
    """skinning_reference.posenc_vjp for an E cotangent g [P, >= 3+6L] (t: the second-derivative form, [1,3] or [P,3])."""
    L, P = m["L"], x.shape[0]
    s, c, f = R._pe_bands(x, L, True)
    w = R._pe_weights(L, m["pe_w"] if L else None).reshape(1, L, 2)
    gb = g[:, 3:3 + 6 * L].map(lambda q: q.reshape(P, L, 2, 3))
    gs, gc = gb[:, :, 0], gb[:, :, 1]
    ws, wc = E(w[:, :, 0:1]), E(w[:, :, 1:2])
    if t is None:
        terms = ecat([(ws * c * gs).scaled(f), (-(wc * s * gc)).scaled(f), g[:, :3].map(lambda q: q.unsqueeze(1))], 1)
        return esum(terms, 1)
    if not L:
        return E(torch.zeros(P, 3, dtype=torch.float64))
    terms = ecat([(-(ws * s * gs)).scaled(f * f), (-(wc * c * gc)).scaled(f * f)], 1)
    return esum(terms, 1) * E(f64(t)[:, :3].expand(P, 3))


# ------------------------------------------------------------------------------------------------- forward and VJP (chain, rows)
def _split_rows(m, P):
    return m["split"] if (m["split"] > 0 and m["W2"] is not None and m["split"] < P) else 0


def _rowcat(parts):
    keys = parts[0].keys()
    out = {}
    for k in keys:
        a, b = parts[0][k], parts[1][k]
        if isinstance(a, E):
            out[k] = ecat([a, b], 0)
        elif isinstance(a, list):
            out[k] = [ecat([u, v], 0) for u, v in zip(a, b)]
        else:
            out[k] = torch.cat([a, b], 0)
    return out


def forward(m, x, cond=None, idx=None, n_out=None, family="chain"):
    """out [P,n_out] (E), the hidden pre-activations z[l] and stored activations y[l] (E, scaled and concatenated as the next layer
    reads them) and ok [P]: no hidden ReLU unit within its own bound of zero."""
    P = x.shape[0]
    s = _split_rows(m, P)
    if s:
        sl = lambda t, a, b: None if t is None else t[a:b]
        return _rowcat([forward(second_of(m) if k else dict(m, W2=None), x[a:b], cond, sl(idx, a, b), n_out, family)
                        for k, (a, b) in enumerate(((0, s), (s, P)))])
    n = m["n"]
    n_out = m["rows"][-1] if n_out is None else n_out
    h = _input(m, x, cond, idx)
    zs, ys = [], []
    ok = torch.ones(P, dtype=torch.bool)
    for l in range(n - 1):
        z = _bias(eprod(h, f64(m["W"][l]).t()), m["b"][l])
        if m["act"] == ACT_RELU:
            ok &= (z.v.abs() > z.e).all(1)
        y = act_forward(z, m["act"], m["p"], family)
        if l + 1 == m["skip"]:
            y = ecat([y * C_INV, _encode(m, x) * C_INV], -1)
        zs.append(z)
        ys.append(y)
        h = y
    Wl = f64(m["W"][n - 1])[:n_out]
    out = eprod(h, Wl.t())
    if family == "rows":
        out = E(out.v, out.e + gamma(7) * ((h.v.abs() + h.e) @ Wl.abs().t()))
    out = _bias(out, None if m["b"][n - 1] is None else m["b"][n - 1][:n_out])
    if m["residual"]:
        out = out + E(f64(x))
    return {"out": out, "z": zs, "y": ys, "ok": ok}


def vjp(m, x, cond=None, idx=None, n_out=None, g_out=None, family="chain"):
    """gx [P,3] (E) = J(x)^T g_out (None: ones on output 0) and ok [P], from the family's own stored activations."""
    P = x.shape[0]
    s = _split_rows(m, P)
    if s:
        sl = lambda t, a, b: None if t is None else t[a:b]
        return _rowcat([vjp(second_of(m) if k else dict(m, W2=None), x[a:b], cond, sl(idx, a, b), n_out, sl(g_out, a, b), family)
                        for k, (a, b) in enumerate(((0, s), (s, P)))])
    n, d_pe = m["n"], 3 + 6 * m["L"]
    n_out = (1 if g_out is None else g_out.shape[1]) if n_out is None else n_out
    fw = forward(m, x, cond, idx, n_out, family)
    Wl = f64(m["W"][n - 1])
    if g_out is None:
        g = E(Wl[0:1].expand(P, -1))
    else:
        g = eprod(E(f64(g_out)[:, :n_out]), Wl[:n_out])
    park = None
    for l in range(n - 2, -1, -1):
        y, rl = fw["y"][l], m["rows"][l]
        skip_next = l + 1 == m["skip"]
        fused = family == "chain" and l <= n - 3 and l + 1 != m["skip"]
        form = "hw" if (family == "rows" or fused) else "expm1"
        if skip_next:
            park = g[:, rl:rl + d_pe] * C_INV
            d = act_grad_y(y[:, :rl] * C_SQRT2, m["act"], m["p"], form)
            dz = (g[:, :rl] * d) * C_INV
        else:
            dz = g * act_grad_y(y, m["act"], m["p"], form)
        g = eprod(dz, f64(m["W"][l]))
    gpe = g[:, :d_pe]
    if park is not None:
        gpe = gpe + park
    gx = _pe_vjp(m, x, gpe)
    if m["residual"]:
        gx = gx + E(f64(g_out)[:, :3])
    return {"gx": gx, "ok": fw["ok"]}


# ------------------------------------------------------------------------------------------------------------------- jet
def _stack4(items):
    return ecat(items, 0)


def jet_forward(m, x, cond=None, idx=None, n_j=None):
    """y [P, rows_last], tang [3P, n_j] (E) and what the reverse sweep reads: H[l] [4P, dims[l]] (the stacked input of layer l),
    Z[l] [4P, rows[l]] (biased z; the tangent rows hold u_k), ok [P]."""
    P, n, L = x.shape[0], m["n"], m["L"]
    n_j = m["rows"][-1] if n_j is None else n_j
    eye = torch.eye(3, dtype=torch.float64)
    pad = E(torch.zeros(P, m["cond_dim"], dtype=torch.float64))
    tans = [ecat([R.posenc_jvp(x, eye[k:k + 1], L, m["pe_w"] if L else None), pad], -1) for k in range(3)]
    h = _stack4([_input(m, x, cond, idx)] + tans)
    Hs, Zs = [], []
    ok = torch.ones(P, dtype=torch.bool)
    for l in range(n - 1):
        Hs.append(h)
        zu = eprod(h, f64(m["W"][l]).t())
        z = _bias(zu[:P], m["b"][l])
        if m["act"] == ACT_RELU:
            ok &= (z.v.abs() > z.e).all(1)
        f, d1, _ = act_jet(z, m["act"], m["p"])
        Zs.append(ecat([z, zu[P:]], 0))
        parts = [f] + [d1 * zu[(k + 1) * P:(k + 2) * P] for k in range(3)]
        y = _stack4(parts)
        if l + 1 == m["skip"]:
            y = ecat([y * C_INV, Hs[0][:, :3 + 6 * L] * C_INV], -1)
        h = y
    Hs.append(h)
    Wl = f64(m["W"][n - 1])
    yv = _bias(eprod(h[:P], Wl.t()), m["b"][n - 1])
    if m["residual"]:
        yv = yv + E(f64(x))
    tang = eprod(h[P:], Wl[:n_j].t())
    return {"y": yv, "tang": tang, "H": Hs, "Z": Zs, "ok": ok}


def jet_backward(m, x, cond=None, idx=None, n_j=None, gy=None, gtang=None):
    """gW[l], gb[l], g_in [4P, dims[0]], gx [P,3] (E) for the cotangents gy [P, rows_last] and gtang [3P, n_j] (None = zeros)."""
    P, n, L = x.shape[0], m["n"], m["L"]
    last, d_pe = m["rows"][-1], 3 + 6 * L
    n_j = last if n_j is None else n_j
    fw = jet_forward(m, x, cond, idx, n_j)
    Wl = f64(m["W"][n - 1])
    K = m["dims"][n - 1]
    H = fw["H"][n - 1]
    gW, gb = [None] * n, [None] * n
    zero = lambda *s: E(torch.zeros(*s, dtype=torch.float64))
    gyE = E(f64(gy)) if gy is not None else None
    gtE = E(f64(gtang)[:, :n_j]) if gtang is not None else None
    gW[n - 1] = eprod(gyE.map(lambda t: t.t()), H[:P]) if gy is not None else zero(last, K)
    if gtang is not None:
        add = gW[n - 1][:n_j] + eprod(gtE.map(lambda t: t.t()), H[P:])
        gW[n - 1] = ecat([add, gW[n - 1][n_j:]], 0)
    gb[n - 1] = esum(gyE, 0) if gy is not None else zero(last)
    hv = eprod(gyE, Wl) if gy is not None else zero(P, K)
    ht = eprod(gtE, Wl[:n_j]) if gtang is not None else zero(3 * P, K)
    hbar = ecat([hv, ht], 0)
    park = None
    for l in range(n - 2, -1, -1):
        rl = m["rows"][l]
        Z = fw["Z"][l]
        if l + 1 == m["skip"]:
            park = hbar[:, rl:rl + d_pe] * C_INV
            yb = hbar[:, :rl] * C_INV
        else:
            yb = hbar
        _, d1, d2 = act_jet(Z[:P], m["act"], m["p"])
        sb = [yb[(k + 1) * P:(k + 2) * P] for k in range(3)]
        acc = esum(R.estack([sb[k] * Z[(k + 1) * P:(k + 2) * P] for k in range(3)], -1), -1)
        zbar = yb[:P] * d1 + d2 * acc
        zb4 = ecat([zbar] + [sb[k] * d1 for k in range(3)], 0)
        gb[l] = esum(zbar, 0)
        gW[l] = eprod(zb4.map(lambda t: t.t()), fw["H"][l])
        hbar = eprod(zb4, f64(m["W"][l]))
    if park is not None:
        hbar = ecat([hbar[:, :d_pe] + park, hbar[:, d_pe:]], -1)
    eye = torch.eye(3, dtype=torch.float64)
    gx = _pe_vjp(m, x, hbar[:P])
    for k in range(3):
        gx = gx + _pe_vjp(m, x, hbar[(k + 1) * P:(k + 2) * P], eye[k:k + 1])
    if m["residual"] and gy is not None:
        gx = gx + E(f64(gy)[:, :3])
    return {"gW": gW, "gb": gb, "g_in": hbar[:, :m["dims"][0]], "gx": gx, "ok": fw["ok"]}


# --------------------------------------------------------------------------------------------------------- integer cases
def int_peak(m, x, cond, idx, gy, gt):
    """The largest sum of magnitudes over every product of the three passes on the integer case (must stay below 2^24)."""
    a = lambda t: f64(t).abs()
    net_abs = dict(m, W=[a(w).float() for w in m["W"]], b=[None if b is None else a(b).float() for b in m["b"]], act=ACT_NONE)
    fw = jet_forward(net_abs, a(x).float(), a(cond).float(), idx)
    bw = jet_backward(net_abs, a(x).float(), a(cond).float(), idx, None, a(gy).float(), a(gt).float())
    peaks = [fw["y"].v.max(), fw["tang"].v.max(), bw["gx"].v.max(), bw["g_in"].v.max()] + [w.v.max() for w in bw["gW"]] + \
            [b.v.max() for b in bw["gb"]]
    return float(max(peaks))
