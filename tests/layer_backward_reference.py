"""Plain float64 references, test inputs and error bounds for the backward of one fused layer y = act(x W^T + b) and the
small kernels around it (csrc/linear_bwd.hip, csrc/elementwise.hip, the glue kernels of csrc/mlp_chain.hip).

Everything here runs on the host in float64 from float32 inputs; nothing depends on how a kernel orders its sums or cuts
its tiles.  tests/test_layer_backward_reference_cpu.py checks the references against float64 autograd and checks every
condition on the inputs that a bound below relies on; tests/test_gpu_layer_backward.py judges the kernels.

Bounds.  u = 2^-24 is the unit round-off of float32 (one correctly rounded operation: relative error <= u; a function with
an error of e ulp: <= 2 e u).  Inputs are exact float32 values.  Terms of second order in u are covered by the slack that
every constant below keeps.

  dZ = gy * act'(z) written through y = act(z)
    relu, none     act' is exactly 0 or 1, the product is exact: torch.equal.  (With an out_scale other than 1 the product
                   out_scale * gy rounds once: u |out_scale gy|.)
    tanh           d = fma(-y, y, 1) rounds once (two roundings without the contraction): |d^ - d| <= u y^2 + u |d| <= 2 u for
                   |y| <= 1 (a tanh output; checked).  gy * d rounds once more: <= 3 u |gy|.   BOUND: 4 u |gy|.
                   With y_scale / out_scale (recmv_act_grad_2d): y * y_scale rounds (the square then carries 2 u y^2 more) and so
                   does out_scale * gy: <= (3 + 1 + 1 + 1) u |out_scale gy|.   BOUND: 8 u |out_scale gy|.
    softplus       d = -expm1(-t), t = beta y >= 0 (a softplus output; checked).  Rounding t moves d by t e^-t u <= (1 - e^-t) u
                   = u d, because t e^-t <= 1 - e^-t for t >= 0.  expm1f: E1 ulp = 2 E1 u.  The product with gy: u.
                   <= (2 + 2 E1) u |gz|.  With E1 = 2 (see below): 6 u.   BOUND: 8 u |gz|.
                   With y_scale / out_scale: two more roundings: 8 u.   BOUND: 10 u |gz|.
                   E1, E2: the ROCm installation this was written against carries no math-library accuracy table (no page
                   under its tree names expm1), so both figures are measured: test_expm1f_and_expf_accuracy
                   (tests/test_gpu_layer_backward.py) runs -expm1f(-t) through recmv_act_grad and expf(-t) through
                   recmv_act_grad2 with gy = a = b = 1 and beta = 1 (every other step is then exact) over log-spaced t
                   in [1e-9, 120] ([1e-9, 87] for expf: normal results) against float64, prints the largest error of each
                   in ulp and in u, and fails if either exceeds the E1 = E2 = 2 ulp that the bounds allow.  Measured on an
                   MI355X (gfx950, ROCm 7.2): expm1f 0.855 ulp (relative 1.447 u), expf 0.804 ulp (relative 1.352 u) — within
                   1 ulp, so the maintainer's 2 ulp and the 8 u bound stand with room.
  act_grad2 = a * b * d(act')/dy
    relu, none     exactly 0: torch.equal.
    tanh           -2 y is exact, a * b and the second product round once each: 2 u.   BOUND: 3 u |ref|.
    softplus       beta * expf(-t): rounding t moves e^-t by t u (relative), expf E2 ulp = 2 E2 u, the products beta *, a * b
                   and the last one u each: (t + 2 E2 + 3) u, E2 = 2.   BOUND: (t + 8) u |ref| + 2^-126 |a b beta|; the second
                   term lets expf flush a result below the normal range (t > 87.3) to zero.
  gb, colsum       The sum of M computed terms z^_r in ANY order (any tree, any chunks) differs from their exact sum by at
                   most gamma sum |z^_r|, gamma = (M-1) u / (1 - (M-1) u) [Higham, Accuracy and Stability, 4.2], and
                   |z^_r| <= |z_r| + bound_dZ_r.   BOUND: sum_r bound_dZ + gamma sum_r (|gz| + bound_dZ)   (the maintainer's
                   sum bound_dZ + (M-1) u sum |gz| with its second-order terms kept).
  gx, gW           The project's product bound (test_gemm_nt_vs_fp64: 4e-7 sum |a b| + 1e-6) holds for the product of the
                   COMPUTED dZ; the error of dZ goes through the product linearly:
                   BOUND: 4e-7 (|gz| + bound_dZ) . |B| + bound_dZ . |B| + 1e-6.  For softplus that is (4e-7 (1 + 8u) + 8u)
                   |gz| . |B| + 1e-6, the maintainer's form; for tanh bound_dZ = 4 u |gy| is not relative to gz (gz vanishes
                   at |y| = 1, its error does not), hence the general form.
  weight norm      n^2 = sum v^2: products u, any summation order (cols - 1) u, all terms positive: relative cols u; the
                   square root halves it and rounds: n^ = n (1 + (cols/2 + 1) u)  -> BOUND norms: (cols/2 + 2) u n.
                   W = v * (g / n^): two more roundings.   BOUND W: (cols/2 + 4) u |W|.
                   The backward kernel is judged as a function of its inputs (v, g, norms, gW) with norms = fl32(n) (u):
                   inv = 1/norms: 2 u.  S = sum v gW in any order: cols u T n with T = sum |vhat gW|.  gg = S * inv:
                   (cols + 3) u T.   BOUND gg: (cols + 4) u T.
                   gv = (g * inv) * fma(-(v * inv), gg^, gW): v * inv 3 u; its product with gg^: |vhat| (3 u |gg| + (cols + 3) u T)
                   <= (cols + 6) u |vhat| T; the fma's rounding u (|gW| + |vhat| T); g * inv 3 u and the last product u on the
                   same magnitude: (g/n) [5 u |gW| + (cols + 11) u |vhat| T].
                   BOUND gv: (cols + 12) u (g/n) (|gW| + |vhat| T) — the maintainer's estimate was cols + 8; the count above
                   gives cols + 11.
  add_scaled_2d    fma(s, b, a) rounds once (twice without the contraction, u |s b| + u |a + s b|).   BOUND: 2 u (|a| + |s b|).
  gather_rows      copies and zeros: torch.equal.

Exact-integer inputs: gy in {-3..3}, y in {-1, 0, 1, 2} with relu / none, x and W in {-2..2}.  Every product and every
partial sum of gb, gx, gW is then an integer of magnitude <= sum |gz| |B| < 2^24 (checked), which float32 holds exactly:
the result is the same in every summation order, and one dropped, doubled or misplaced element changes it.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_TANH = 0, 1, 2, 3
ACTS = (ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_TANH)
BETA = 100.0
EXPM1F_ULP = 2.0       # allowed by the bounds and asserted by test_expm1f_and_expf_accuracy; measured 0.855 (module docstring)
EXPF_ULP = 2.0

# (M, N, K, act) of recmv_linear_backward: one-element, odd, around the 256-row chunk, two chunks, the N = 473 layer with its padded
# dZ stride, a wide tanh layer, many chunks on aligned rows, and two shapes beyond the chunk cap with narrow K
LINEAR_CASES = [(1, 1, 1, ACT_NONE), (3, 5, 3, ACT_TANH), (255, 64, 39, ACT_SOFTPLUS), (256, 63, 40, ACT_RELU),
                (257, 65, 168, ACT_SOFTPLUS), (300, 473, 512, ACT_SOFTPLUS), (1000, 257, 512, ACT_TANH),
                (4099, 512, 512, ACT_SOFTPLUS), (24577, 512, 39, ACT_SOFTPLUS), (24700, 473, 3, ACT_RELU)]
BOUNDED_CASES = [c for c in LINEAR_CASES if c[3] in (ACT_SOFTPLUS, ACT_TANH)]
NEAR_ZERO_CASES = [(255, 64, 39, ACT_SOFTPLUS), (300, 473, 512, ACT_SOFTPLUS)]      # element path and float4 path of the fused kernel
COLSUM_ROWS = (1, 255, 256, 257, 24576, 24577, 30001)
COLSUM_COLS = (1, 9, 63, 64, 65, 473)
ACT_GRAD_N = (1, 3, 4, 1023, 1024, 1025)
WN_ROWS = (1, 473)
WN_COLS = (1, 3, 39, 40, 168, 255, 256, 257, 512, 1000)


def f64(t):
    return t.detach().cpu().double()


def act_param(act):
    return BETA if act == ACT_SOFTPLUS else 0.0


# --------------------------------------------------------------------------------------------------------------- references
def act_fn(z, act, p=BETA):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_SOFTPLUS:
        return torch.nn.functional.softplus(z, beta=p, threshold=1e30)
    if act == ACT_TANH:
        return torch.tanh(z)
    return z


def dact(y, act, p=BETA):
    """act'(z) written through y = act(z), float64."""
    y = f64(y)
    if act == ACT_RELU:
        return (y > 0).double()
    if act == ACT_SOFTPLUS:
        return -torch.expm1(-p * y)
    if act == ACT_TANH:
        return 1.0 - y * y
    return torch.ones_like(y)


def d2act(y, act, p=BETA):
    """d(act')/dy, float64."""
    y = f64(y)
    if act == ACT_SOFTPLUS:
        return p * torch.exp(-p * y)
    if act == ACT_TANH:
        return -2.0 * y
    return torch.zeros_like(y)


def layer_backward(gy, y, x, W, act, p=BETA):
    """gz, gb, gx, gW of y = act(x W^T + b) for the cotangent gy; float64."""
    gz = f64(gy) * dact(y, act, p)
    return {"gz": gz, "gb": gz.sum(0), "gx": gz @ f64(W), "gW": gz.t() @ f64(x)}


def weight_norm(v, g):
    """W = g v / |v| per row and the row norms; g [rows] or [rows,1]."""
    v, g = f64(v), f64(g).reshape(-1, 1)
    n = v.norm(dim=1, keepdim=True)
    return g * v / n, n.reshape(-1)


def weight_norm_backward(v, g, gW):
    """gv [rows,cols], gg [rows] and T = sum_c |vhat gW| [rows] (the magnitude the bounds are stated in)."""
    v, g, gW = f64(v), f64(g).reshape(-1, 1), f64(gW)
    n = v.norm(dim=1, keepdim=True)
    vh = v / n
    gg = (vh * gW).sum(1, keepdim=True)
    gv = (g / n) * (gW - vh * gg)
    return gv, gg.reshape(-1), (vh * gW).abs().sum(1)


def gather_rows(table, index, rows, cols, fill):
    """out [rows, fill]: table[index[r], :cols] (row 0 for every r when index is None), zeros in columns [cols, fill)."""
    out = torch.zeros(rows, fill, dtype=table.dtype)
    if cols:
        src = table[index, :cols] if index is not None else table[:1, :cols].expand(rows, cols)
        out[:, :cols] = src
    return out


def add_scaled(a, s, b):
    return f64(a) + float(np.float32(s)) * f64(b)


# ------------------------------------------------------------------------------------------------------------------- bounds
def bound_dz(gy, y, act, p=BETA, y_scale=1.0, out_scale=1.0):
    """Elementwise bound on |dZ^ - dZ| (zeros: the kernel must be exact)."""
    scaled = y_scale != 1.0 or out_scale != 1.0
    g = (float(np.float32(out_scale)) * f64(gy)).abs()
    if act == ACT_TANH:
        return (8.0 if scaled else 4.0) * U * g * torch.ones_like(f64(y))
    if act == ACT_SOFTPLUS:
        d = dact(f64(y) * float(np.float32(y_scale)), act, p)
        return ((4.0 if scaled else 2.0) + 2.0 * EXPM1F_ULP + 2.0) * U * (g * d).abs()
    return (U if out_scale != 1.0 else 0.0) * g * dact(f64(y) * float(np.float32(y_scale)), act, p)


def bound_act_grad2(a, b, y, act, p=BETA):
    ref = f64(a) * f64(b) * d2act(y, act, p)
    if act == ACT_TANH:
        return 3.0 * U * ref.abs()
    if act == ACT_SOFTPLUS:
        return (p * f64(y).abs() + 2.0 * EXPF_ULP + 4.0) * U * ref.abs() + TINY * (f64(a) * f64(b) * p).abs()
    return torch.zeros_like(ref)


def bound_colsum(gz_abs, bdz=None):
    """Any-order bound on the column sums of the computed dZ (bdz None: the summands are the exact inputs)."""
    M = gz_abs.shape[0]
    gamma = (M - 1) * U / (1.0 - (M - 1) * U)
    if bdz is None:
        return gamma * gz_abs.sum(0)
    return bdz.sum(0) + gamma * (gz_abs + bdz).sum(0)


def bound_product(gz_abs, bdz, B_abs):
    """|gz^ . B - gz . B| for gz^ within bdz of gz; B_abs [inner, out]."""
    return 4e-7 * ((gz_abs + bdz) @ B_abs) + bdz @ B_abs + 1e-6


def bound_wn_forward(v, g):
    W, n = weight_norm(v, g)
    cols = v.shape[1]
    return (cols / 2 + 4) * U * W.abs(), (cols / 2 + 2) * U * n


def bound_wn_backward(v, g, gW):
    v64, g64 = f64(v), f64(g).reshape(-1, 1)
    cols = v.shape[1]
    n = v64.norm(dim=1, keepdim=True)
    T = ((v64 / n) * f64(gW)).abs().sum(1, keepdim=True)
    b_gg = (cols + 4) * U * T.reshape(-1)
    b_gv = (cols + 12) * U * (g64 / n).abs() * (f64(gW).abs() + (v64 / n).abs() * T)
    return b_gv, b_gg


def bound_add_scaled(a, s, b):
    return 2.0 * U * (f64(a).abs() + (float(np.float32(s)) * f64(b)).abs())


# ------------------------------------------------------------------------------------------------------------------- inputs
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randint(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# A case is deterministic in its shape and cheap to rebuild (the largest takes about a second), so the cache only serves consecutive
# uses of one shape: it is kept small so that the float64 references of the largest shapes (some hundred MB) do not outlive their
# tests.  Callers read a case and copy it to the device; they never write to it.
@functools.lru_cache(maxsize=2)
def int_case(M, N, K, act):
    """Exact-integer inputs of one layer backward (softplus / tanh shapes run as relu) and the int64 results as float32."""
    act = ACT_RELU if act in (ACT_SOFTPLUS, ACT_TANH) else act
    g = _gen(1, M, N, K)
    gy = _randint(-3, 3, (M, N), g)
    y = _randint(-1, 2, (M, N), g)
    x = _randint(-2, 2, (M, K), g)
    W = _randint(-2, 2, (N, K), g)
    ref = layer_backward(gy, y, x, W, act)
    peak = max(float(ref["gz"].abs().sum(0).max()) if M else 0.0,
               float((ref["gz"].abs() @ f64(W).abs()).max()) if M else 0.0,
               float((ref["gz"].abs().t() @ f64(x).abs()).max()) if M else 0.0)
    want = {k: v.to(torch.int64).to(torch.float32) for k, v in ref.items()}
    exact = all(torch.equal(want[k].double(), ref[k]) for k in ref)
    return {"act": act, "p": 0.0, "gy": gy, "y": y, "x": x, "W": W, "want": want, "peak": peak, "integral": exact}


def softplus_outputs(shape, g, p=BETA):
    """Outputs of a softplus layer, all >= 0: exact zeros, values log-spaced from 1e-7 to 1 (beta y from 1e-5, where 1 - exp cancels),
    and values with beta y > 104 (act' is exactly 1), shuffled over the matrix."""
    n = int(np.prod(shape))
    y = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 7.0 - 7.0)
    y[0::17] = 0.0
    y[1::17] = (104.5 + 30.0 * torch.rand(y[1::17].shape, generator=g, dtype=torch.float64)) / p
    if n > 2:
        y[2] = 1e-7
    if n > 3:
        y[3] = 1.0
    return y.float().reshape(shape)


@functools.lru_cache(maxsize=2)
def float_case(M, N, K, act, near_zero=False):
    """Rounding inputs of one layer backward: the rows of gy span five decades, y is a plausible output of `act`.  near_zero
    (softplus): every y lies in [1e-7, 1e-6], beta y in [1e-5, 1e-4] — the whole of dZ then sits where 1 - exp(-beta y) has lost
    three digits, so that form shows in gb, gx and gW themselves and not only in dZ."""
    g = _gen(2, M, N, K, 1) if near_zero else _gen(2, M, N, K)
    p = act_param(act)
    gy = torch.randn(M, N, generator=g) * torch.logspace(-3, 2, M).view(-1, 1)
    if act == ACT_SOFTPLUS and near_zero:
        y = (10.0 ** (torch.rand(M, N, generator=g, dtype=torch.float64) - 7.0)).float()
    elif act == ACT_SOFTPLUS:
        y = softplus_outputs((M, N), g)
    elif act == ACT_TANH:
        y = torch.tanh(torch.randn(M, N, generator=g) * 2.0)
        y.view(-1)[0::13] = 1.0
        y.view(-1)[1::13] = -1.0
        y.view(-1)[2::13] = 0.0
    else:
        y = torch.randn(M, N, generator=g)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / np.sqrt(K)
    ref = layer_backward(gy, y, x, W, act, p)
    gza = ref["gz"].abs()
    bdz = bound_dz(gy, y, act, p)
    bound = {"gz": bdz, "gb": bound_colsum(gza, bdz), "gx": bound_product(gza, bdz, f64(W).abs()),
             "gW": bound_product(gza.t(), bdz.t(), f64(x).abs())}
    return {"act": act, "p": p, "gy": gy, "y": y, "x": x, "W": W, "ref": ref, "bound": bound}


def act_inputs(n, act, seed=0):
    """gy, a second cotangent and y [n] for the flat activation-gradient kernels."""
    g = _gen(3, n, act, seed)
    gy = torch.randn(n, generator=g) * torch.logspace(-3, 2, n)
    b = torch.randn(n, generator=g)
    if act == ACT_SOFTPLUS:
        y = softplus_outputs((n,), g)
    elif act == ACT_TANH:
        y = torch.tanh(torch.randn(n, generator=g) * 2.0)
        y[0] = 1.0
    else:
        y = torch.randn(n, generator=g)
        y[0] = 0.0
    return gy, b, y


def wn_inputs(rows, cols):
    """v with row norms over four decades (never 1: a dropped 1/|v| must show), g of both signs, a cotangent gW."""
    g = _gen(4, rows, cols)
    v = torch.randn(rows, cols, generator=g) * torch.logspace(-2, 2, rows).view(-1, 1) * 3.0
    gg = (torch.rand(rows, generator=g) + 0.5) * (1 - 2 * (torch.arange(rows) % 2)).float()
    gW = torch.randn(rows, cols, generator=g)
    return v, gg, gW


def ratio(err, bound):
    """Largest error / bound; an error where the bound is zero counts as infinite."""
    err, bound = err.double().reshape(-1), bound.double().reshape(-1)
    if err.numel() == 0:
        return 0.0
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                           torch.zeros_like(err)))
    return float(r.max())
