"""Plain float64 references, test inputs and error bounds for the per-point geometry front end: the fused linear-blend
skinning passes and the root finder's step (csrc/lbs_fused.hip), the SMPL kinematic chain (csrc/kinematic_chain.hip) and the
positional encoding with its derivatives (csrc/posenc_grad.hip).

Everything here runs on the host in float64 from float32 inputs and shares no code with recmv.
tests/test_skinning_reference_cpu.py checks the references against float64 autograd of plain torch compositions and checks every
condition on the inputs that a bound relies on; tests/test_gpu_skinning.py judges the kernels.

How the bounds are formed.  u = 2^-24 is the unit round-off of float32.  A reference value travels as a pair (v, e) — class E:
v is the exact float64 value of the quantity for the exact float32 inputs, e bounds |computed - v| for ANY float32 evaluation
that uses the same operations on the same operands, in any summation order.  e is computed from the float64 magnitudes alone
(never from a kernel's output) by these rules, which are the standard running error bounds [Higham, Accuracy and Stability of
Numerical Algorithms, ch. 3 and 4.2]:

  input            e = 0 (an exact float32 value).
  a + b, a - b     p = e_a + e_b;                              e = p + u (|v| + p)     one rounding of the perturbed result
  a * b            p = |a| e_b + |b| e_a + e_a e_b;            e = p + u (|v| + p)
  a / b            p = (e_a + |v| e_b) / (|b| - e_b);          e = p + u (|v| + p)     |b| > e_b is asserted
  sqrt(a)          p = sqrt(a) - sqrt(max(a - e_a, 0));        e = p + u (|v| + p)     (concave: the downward move is the larger)
  sum of n terms   p = sum e_i;    e = p + gamma_(n-1) sum (|v_i| + e_i),  gamma_k = k u / (1 - k u): any order, any tree.  A
                   dot product is a sum of products, so this is the sum |a| |b| bound with the operands' own errors carried; an
                   fma has fewer roundings than the product and sum it replaces, so contraction stays inside it.
  f in {sin, cos}  p = e_a (Lipschitz 1);                      e = p + 2 F u (|v| + p)  F = the function's error in ulp
  asin(r)          p = e_r / sqrt(1 - (|r| + e_r)^2);          e = p + 2 F u (|v| + p)  the conditioning 1 / sqrt(1 - r^2)
sqrtf and the division are correctly rounded in this build (build.py passes no fast-math flag): u each, as above.  u is taken as
2^-24 (1 + 2^-10) so that the terms of second order that a rule drops (gamma's denominator aside, which is kept) are covered.
No intermediate of the test inputs falls below the normal range 2^-126 except exact zeros, so no rule needs an underflow term.

What this gives for the quantities the issue names:
  chain            G_j = G_p L_j joint by joint: every element is a sum of 3 (4) products of pairs, so
                   err(G_j) <= err(G_p) |L_j| + |G_p| err(L_j) + err err + gamma_4 |G_p| |L_j| — the rule above; a deep chain
                   accumulates 23 such steps.  err(L_j) is the rodrigues map's own bound (two sqrtf, one sinf, one cosf, three
                   divisions by the angle — the 5.8e7 intermediate of the zero pose is |1/angle| in the tangent of theta/angle and
                   is carried at its magnitude).  The backward differentiates rodrigues with 3-direction dual numbers of E pairs
                   and sums a parent's contributions in any order.
  g_d              u = e x v is a difference of products: e_u = u-order * (|e_y v_z| + |e_z v_y|), an ABSOLUTE error that does not
                   shrink with |u| — the cancellation.  It is then divided by un * dn: the bound is u-order / (un dn), as wanted.
  angle            asin's conditioning 1 / sqrt(1 - r^2) with r = un / dn <= 0.99 (asserted) times 180/pi.
The ray outputs (loss2, angle, g_d) are judged as functions of the kernel's own float32 d (ray_energy), so that they stand in
isolation from the skinning error of d; d itself is judged by lbs_forward.

Sampling geometry (csrc/gs3d_common.inc restated): g = (p - c) * s; ix = ((g + 1) * size - 1) / 2 (the last step in double,
rounded once); border clip with a zero gradient mask where ix <= 0 or ix >= size - 1; x0 = floor(ix); corner weights
f0 = x0 + 1 - ix, f1 = ix - x0; a non-finite coordinate becomes -100 so that every corner is outside and the weights are zero.
e_ix follows from the rules (five roundings: about u size (2|g| + 2)).  The bound on a weight carries it through the corner
products: sum_k |v_k| (e_fx f_y f_z + ...) — the sampler's own derivative magnitudes times the coordinate error.  This holds as
long as the kernel and the reference pick the same cell: the in-voxel points keep every float64 coordinate at least 1/32 voxel
from every integer and from both clip limits and e_ix < 1/64 (both asserted on the host), the clipped points lie at least half
a voxel outside; no point is set aside.  Points ON the lattice may fall in either neighbouring cell: they are judged on the
outputs that are continuous across the cell face (d, v, W) with the cell-free Lipschitz constant sum_k |v_k| f f <= 2 max |v|
in place of the cell's own derivative magnitude.

Library functions.  The ROCm tree carries no accuracy table (tests/layer_backward_reference.py records that search), so sinf,
cosf and sincosf are measured: test_sinf_cosf_sincosf_accuracy (tests/test_gpu_skinning.py) runs recmv_posenc_forward with
weights 1 and out_scale 1 — out = sinf(x 2^b), cosf(x 2^b), every other step exact — and recmv_posenc_vjp with a one-hot g —
out = 2^b cos or -2^b sin from sincosf — over 2^18 log-spaced |x| in [1e-6, 4], both signs, all 16 bands, against float64,
prints the largest error of each in ulp and asserts the allowance.  The allowance is the measured maximum rounded up to the next
whole ulp plus one ulp because the sweep is finite.
Measured on an MI355X (gfx950, ROCm 7.0): sinf 1.548 ulp, cosf 1.577 ulp, sincosf 1.548 ulp (sine) and 1.577 ulp (cosine) — the
largest errors sit in the high bands, where the argument reduction works on arguments up to 5e5.  Rounded up: 2 ulp; allowance
SINF_ULP = COSF_ULP = SINCOSF_ULP = 3 ulp.
asinf cannot be isolated through the ABI: it gets the allowance of sinf and its inputs are kept at ratio <= 0.99 (asserted).

Exact-integer inputs: g_d, gv, gJ in {-3..3}, p in {-2..2}: every entry of Q, Gs and Q4 is an integer of magnitude <= 3 * 2 + 3
< 2^24, exact in float32: torch.equal, and the blocks of the other frames are exactly zero.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24 * (1.0 + 2.0 ** -10)
# measured by test_sinf_cosf_sincosf_accuracy on an MI355X (gfx950, ROCm 7.0): sinf 1.548 ulp, cosf 1.577 ulp, sincosf 1.548 ulp
# (sine) / 1.577 ulp (cosine); allowance = the maximum rounded up to a whole ulp (2) + 1
SINF_ULP = 3.0
COSF_ULP = 3.0
SINCOSF_ULP = 3.0
ASINF_ULP = SINF_ULP
RATIO_MAX = 0.99
KJ = 24
RAD2DEG = float(np.float32(57.29577951308232))
EPS_RODRIGUES = float(np.float32(1e-8))

VOLUMES = ((2, 2, 2), (3, 5, 4), (9, 6, 7))                    # [D,H,W]
LBS_P = (0, 1, 255, 256, 257, 4099)
LBS_B = (1, 3, 56, 57, 128)
WRAP_P = 524288 + 300
WRAP_TILE = 4099
ROOT_P = (0, 1, 63, 64, 65, 256, 257, 5000)
CHAIN_B = (0, 1, 63, 64, 65, 129)
PE_L = (0, 1, 6, 10, 16)
PE_P = (0, 1, 255, 257)
FAM_IN, FAM_CLIP, FAM_LATTICE, FAM_NAN = 0, 1, 2, 3


def f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def gamma(k):
    k = max(int(k), 0)
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------ values with error bounds
class E:
    """(v, e): exact float64 value and a bound on |float32 evaluation - v| (module docstring)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v.double() if torch.is_tensor(v) else torch.tensor(v, dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else (e.double() + torch.zeros_like(self.v))

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(x)

    @staticmethod
    def rounded(v, p):
        return E(v, p + U * (v.abs() + p))

    def __add__(self, o):
        o = E.lift(o)
        return E.rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = E.lift(o)
        return E.rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.lift(o) - self

    def __mul__(self, o):
        o = E.lift(o)
        return E.rounded(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.lift(o)
        assert bool((o.v.abs() > o.e).all()), "division by a quantity whose error reaches its value"
        v = self.v / o.v
        return E.rounded(v, (self.e + v.abs() * o.e) / (o.v.abs() - o.e))

    def __rtruediv__(self, o):
        return E.lift(o) / self

    def __neg__(self):
        return E(-self.v, self.e)

    def map(self, fn):
        """An exact rearrangement (index, reshape, mask by 0 / 1) applied to value and bound alike."""
        return E(fn(self.v), fn(self.e))

    def __getitem__(self, idx):
        return self.map(lambda t: t[idx])

    def scaled(self, c):
        """Product with an exact power of two (or with 0 / +-1): no rounding."""
        c = torch.as_tensor(c, dtype=torch.float64)
        return E(self.v * c, self.e * c.abs())


def ecat(items, dim=-1):
    items = [E.lift(i) for i in items]
    return E(torch.cat([i.v for i in items], dim), torch.cat([i.e for i in items], dim))


def estack(items, dim=-1):
    items = [E.lift(i) for i in items]
    shape = torch.broadcast_shapes(*[i.v.shape for i in items])
    return E(torch.stack([i.v.expand(shape) for i in items], dim), torch.stack([i.e.expand(shape) for i in items], dim))


def esum(x, dim=-1, n=None):
    """Sum along dim in any order; n = the number of terms (default: the size of dim)."""
    n = x.v.shape[dim] if n is None else n
    return E(x.v.sum(dim), x.e.sum(dim) + gamma(n - 1) * (x.v.abs() + x.e).sum(dim))


def esqrt(x):
    if isinstance(x, Dual):
        s = esqrt(x.v)
        h = 0.5 / s
        return Dual(s, [d * h for d in x.d])
    assert bool((x.v >= 0).all())
    v = x.v.sqrt()
    return E.rounded(v, v - (x.v - x.e).clamp_min(0).sqrt())


def _efun(x, fn, ulp):
    v = fn(x.v)
    return E(v, x.e + 2.0 * ulp * U * (v.abs() + x.e))


def esin(x):
    if isinstance(x, Dual):
        s, c = esin(x.v), ecos(x.v)
        return Dual(s, [c * d for d in x.d])
    return _efun(x, torch.sin, SINF_ULP)


def ecos(x):
    if isinstance(x, Dual):
        s, c = esin(x.v), ecos(x.v)
        return Dual(c, [(-s) * d for d in x.d])
    return _efun(x, torch.cos, COSF_ULP)


def easin(x):
    top = x.v.abs() + x.e
    assert bool((top < 1).all())
    v = torch.asin(x.v)
    p = x.e / (1.0 - top * top).sqrt()
    return E(v, p + 2.0 * ASINF_ULP * U * (v.abs() + p))


class Dual:
    """Value and three tangents, each an E: forward-mode derivative with its rounding bound."""
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = v, list(d)

    @staticmethod
    def lift(x, like):
        if isinstance(x, Dual):
            return x
        x = E.lift(x)
        return Dual(x, [E(torch.zeros_like(like.v.v)) for _ in range(3)])

    def __add__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v + o.v, [a + b for a, b in zip(self.d, o.d)])

    __radd__ = __add__

    def __sub__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v - o.v, [a - b for a, b in zip(self.d, o.d)])

    def __mul__(self, o):
        if not isinstance(o, Dual):
            o = E.lift(o)
            return Dual(self.v * o, [d * o for d in self.d])
        return Dual(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.d, o.d)])

    __rmul__ = __mul__

    def __truediv__(self, o):
        q, ib = self.v / o.v, 1.0 / o.v
        return Dual(q, [(a - q * b) * ib for a, b in zip(self.d, o.d)])


def ratio(err, bound):
    """Largest error / bound; an error where the bound is zero counts as infinite; a NaN error counts as infinite."""
    err, bound = err.double().reshape(-1), bound.double().reshape(-1)
    if err.numel() == 0:
        return 0.0
    inf = torch.full_like(err, float("inf"))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), inf, r)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------- skinning
def make_grid(vol, center, scale):
    """vol [D,H,W,24] float32 channels-last; center, scale [3] float32 (x, y, z)."""
    return {"vol": vol, "center": torch.as_tensor(center, dtype=torch.float32), "scale": torch.as_tensor(scale, dtype=torch.float32)}


def coords(p, grid):
    """The unnormalised coordinate before the clip, [P,3] (x <-> W, y <-> H, z <-> D), as an E."""
    D, H, W = grid["vol"].shape[:3]
    size = torch.tensor([W, H, D], dtype=torch.float64)
    g = (E(f64(p)) - E(f64(grid["center"]))) * E(f64(grid["scale"]))
    a = (g + 1.0) * size
    return E.rounded((a.v - 1.0) / 2.0, a.e / 2.0), size


def lbs_weights(p, grid, lattice=None):
    """The sampled blend weights and their derivatives for p [P,3] float32.  Returns a dict of E:
    w [P,24]; D [P,3,24] = dw/dp; H [P,3,24] = the mixed second derivatives d2w/dp_x dp_y, /dp_x dp_z, /dp_y dp_z; and the parts:
    draw / hraw (the raw corner sums), m [P,3] (clip mask * size / 2 * scale), mask [P,3], f [P,3,2], vals [P,8,24], inside [P,8],
    valid [P] (finite point).  lattice [P] bool: points whose weight bound uses the cell-free Lipschitz constant."""
    vol = f64(grid["vol"])
    Dn, Hn, Wn = vol.shape[:3]
    ix, size = coords(p, grid)
    valid = torch.isfinite(f64(p)).all(1)
    bad = ~torch.isfinite(ix.v)
    lo = (ix.v <= 0) & ~bad
    hi = (ix.v >= size - 1) & ~bad
    mask = (~(lo | hi)).double()
    civ = torch.where(lo, torch.zeros_like(ix.v), torch.where(hi, (size - 1).expand_as(ix.v), ix.v))
    civ = torch.where(bad, torch.full_like(civ, -100.0), civ)
    cie = torch.where(lo | hi | bad, torch.zeros_like(ix.e), torch.nan_to_num(ix.e))
    c = E(civ, cie)
    x0 = torch.floor(c.v)
    f = estack([E.rounded(x0 + 1.0 - c.v, c.e), E.rounded(c.v - x0, c.e)], -1)             # [P,3,2]
    # where the coordinate is exact (clipped), so are the corner weights
    f = E(f.v, torch.where((cie == 0).unsqueeze(-1), torch.zeros_like(f.e), f.e))
    x0 = x0.long()
    vals, inside, wk, tx, ty, tz, hxy, hxz, hyz = [], [], [], [], [], [], [], [], []
    for k in range(8):
        bx, by, bz = k & 1, (k >> 1) & 1, k >> 2
        xi, yi, zi = x0[:, 0] + bx, x0[:, 1] + by, x0[:, 2] + bz
        ins = (xi >= 0) & (xi < Wn) & (yi >= 0) & (yi < Hn) & (zi >= 0) & (zi < Dn)
        v = vol[zi.clamp(0, Dn - 1), yi.clamp(0, Hn - 1), xi.clamp(0, Wn - 1)] * ins.double().unsqueeze(-1)
        vals.append(v)
        inside.append(ins)
        fx, fy, fz = f[:, 0, bx], f[:, 1, by], f[:, 2, bz]
        wk.append(fx * fy * fz)
        tx.append((fy * fz).scaled(1.0 if bx else -1.0))
        ty.append((fx * fz).scaled(1.0 if by else -1.0))
        tz.append((fx * fy).scaled(1.0 if bz else -1.0))
        hxy.append(fz.scaled(1.0 if bx == by else -1.0))
        hxz.append(fy.scaled(1.0 if bx == bz else -1.0))
        hyz.append(fx.scaled(1.0 if by == bz else -1.0))
    vals = torch.stack(vals, 1)                                                              # [P,8,24]
    inside = torch.stack(inside, 1)
    V = E(vals)

    def corner_sum(ws):
        return esum(V * estack(ws, 1).map(lambda t: t.unsqueeze(-1)), 1)                    # [P,24]

    w = corner_sum(wk)
    if lattice is not None and bool(lattice.any()):
        # either neighbouring cell: |w^ - w| <= sum_axes e_ix * 2 max|v| + the rounding of the products and the sum
        vmax = vol.reshape(-1, KJ).abs().max(0).values
        free = (torch.nan_to_num(ix.e).sum(1, keepdim=True) + 4.0 * U) * 2.0 * vmax + (3.0 * U + gamma(7)) * vmax
        w = E(w.v, torch.where(lattice.unsqueeze(-1), torch.maximum(w.e, free), w.e))
    draw = estack([corner_sum(tx), corner_sum(ty), corner_sum(tz)], 1)                       # [P,3,24]
    hraw = estack([corner_sum(hxy), corner_sum(hxz), corner_sum(hyz)], 1)
    m = (E(size / 2.0) * E(f64(grid["scale"]))).map(lambda t: t * mask)                      # [P,3]
    Dw = draw * m.map(lambda t: t.unsqueeze(-1))
    mh = estack([m[:, 0] * m[:, 1], m[:, 0] * m[:, 2], m[:, 1] * m[:, 2]], 1)
    Hw = hraw * mh.map(lambda t: t.unsqueeze(-1))
    return {"w": w, "D": Dw, "H": Hw, "draw": draw, "hraw": hraw, "m": m, "mask": mask, "f": f, "vals": vals, "inside": inside,
            "valid": valid, "ix": ix, "size": size}


def _frames(p, frame, A):
    """Ab [P,24,3,4] (rows 0..2 of the point's frame transforms) and ph [P,4] = [p;1], float64."""
    Ab = f64(A)[:, :, :3, :][frame.long()]
    ph = torch.cat([f64(p), torch.ones(p.shape[0], 1, dtype=torch.float64)], 1)
    return Ab, ph


def _transform(T, ph, extra=None):
    """T [P,3,4] (E) applied to ph [P,4], plus an exact extra [P,3]: any-order sum of the four (five) terms."""
    terms = T * E(ph.unsqueeze(1))
    if extra is not None:
        terms = ecat([terms, E(extra.unsqueeze(-1))], -1)
    return esum(terms, -1)


def lbs_forward(p, frame, A, trans, grid, lattice=None, cam=None, rays=None):
    """d [P,3] (E); with cam and rays also loss2, angle, g_d of the reference's own exact d (values for the autograd check)."""
    s = lbs_weights(p, grid, lattice)
    Ab, ph = _frames(p, frame, A)
    T = esum(s["w"].map(lambda t: t[:, :, None, None]) * E(Ab), 1)                           # [P,3,4]
    d = _transform(T, ph, f64(trans)[frame.long()])
    out = {"d": d, "w": s["w"], "valid": s["valid"]}
    if rays is not None:
        out.update(ray_energy(d.v, cam, rays))
    return out


def ray_energy(d, cam, rays):
    """loss2 = |(d-c) x v| / |d-c|, angle = asin(loss2) in degrees, g_d = d loss2 / d d, as E, for d taken as exact."""
    e = E(f64(d)) - E(f64(cam))
    v = E(f64(rays))
    ex, ey, ez = e[:, 0], e[:, 1], e[:, 2]
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    ux, uy, uz = ey * vz - ez * vy, ez * vx - ex * vz, ex * vy - ey * vx
    un = esqrt(esum(estack([ux * ux, uy * uy, uz * uz])))
    dn = esqrt(esum(estack([ex * ex, ey * ey, ez * ez])))
    r = un / dn
    angle = easin(r) * RAD2DEG
    inv = 1.0 / (un * dn)
    gux, guy, guz = ux * inv, uy * inv, uz * inv
    k3 = un / (dn * dn * dn)
    g_d = estack([(vy * guz - vz * guy) - ex * k3, (vz * gux - vx * guz) - ey * k3, (vx * guy - vy * gux) - ez * k3])
    return {"loss2": r, "angle": angle, "g_d": g_d}


def lbs_vjp_input(p, frame, A, grid, g_d):
    s = lbs_weights(p, grid)
    Ab, ph = _frames(p, frame, A)
    g = E(f64(g_d))
    y = esum(E(Ab) * E(ph[:, None, None, :]), -1)                                            # [P,24,3]
    gw = esum(y * g.map(lambda t: t.unsqueeze(1)), -1)                                       # [P,24]
    dot = esum(E(s["vals"]) * gw.map(lambda t: t.unsqueeze(1)), -1)                          # [P,8]
    f = s["f"]
    parts = [[], [], []]
    for k in range(8):
        bx, by, bz = k & 1, (k >> 1) & 1, k >> 2
        fx, fy, fz = f[:, 0, bx], f[:, 1, by], f[:, 2, bz]
        dk = dot[:, k]
        parts[0].append((dk * fy * fz).scaled(1.0 if bx else -1.0))
        parts[1].append((dk * fx * fz).scaled(1.0 if by else -1.0))
        parts[2].append((dk * fx * fy).scaled(1.0 if bz else -1.0))
    gi = estack([esum(estack(q)) for q in parts]) * s["m"]                                   # [P,3]
    atg = esum(E(Ab[:, :, :, :3]) * g.map(lambda t: t[:, None, :, None]), 2)                 # [P,24,3]: A_33^T g
    t = esum(s["w"].map(lambda t_: t_.unsqueeze(-1)) * atg, 1)
    return {"g_p": t + gi, "valid": s["valid"]}


def _blocks(rows, frame, B):
    """rows [P,n] (E) placed in block frame[p] of a [P, B*n] matrix of exact zeros."""
    P, n = rows.v.shape
    idx = frame.long().unsqueeze(1) * n + torch.arange(n).unsqueeze(0)

    def place(t):
        out = torch.zeros(P, B * n, dtype=torch.float64)
        out.scatter_(1, idx, t)
        return out
    return rows.map(place)


def lbs_params_stage(p, frame, B, grid, g_d, lattice=None):
    s = lbs_weights(p, grid, lattice)
    ph = torch.cat([f64(p), torch.ones(p.shape[0], 1, dtype=torch.float64)], 1)
    g = E(f64(g_d))
    q = (g.map(lambda t: t.unsqueeze(-1)) * E(ph.unsqueeze(1))).map(lambda t: t.reshape(-1, 12))
    return {"W": s["w"], "Q": _blocks(q, frame, B), "Gs": _blocks(g, frame, B), "valid": s["valid"]}


def lbs_jet_forward(p, frame, A, trans, grid, lattice=None):
    s = lbs_weights(p, grid, lattice)
    Ab, ph = _frames(p, frame, A)
    T = esum(s["w"].map(lambda t: t[:, :, None, None]) * E(Ab), 1)
    v = _transform(T, ph, f64(trans)[frame.long()])
    y = esum(E(Ab) * E(ph[:, None, None, :]), -1)                                            # [P,24,3]
    S = esum(y.map(lambda t: t.unsqueeze(-1)) * s["draw"].map(lambda t: t.permute(0, 2, 1).unsqueeze(2)), 1)   # [P,3(i),3(k)]
    J = T[:, :, :3] + S * s["m"].map(lambda t: t.unsqueeze(1))
    return {"v": v, "J": J, "valid": s["valid"]}


def lbs_jet_backward(p, frame, A, B, grid, gv=None, gJ=None):
    """g_p [P,3], W4 [4P,24], Q4 [4P,B*12], Gs [P,B*3] for the cotangents gv [P,3] of v and gJ [P,9] of J (None = zeros)."""
    P = p.shape[0]
    s = lbs_weights(p, grid)
    Ab, ph = _frames(p, frame, A)
    gv = E(f64(gv) if gv is not None else torch.zeros(P, 3, dtype=torch.float64))
    gJ = E((f64(gJ) if gJ is not None else torch.zeros(P, 9, dtype=torch.float64)).reshape(P, 3, 3))
    w, Dw, Hw = s["w"], s["D"], s["H"]
    Aj = E(Ab)                                                                                # [P,24,3(i),4]
    y = esum(Aj * E(ph[:, None, None, :]), -1)                                               # [P,24,3(i)]
    Dj = Dw.map(lambda t: t.permute(0, 2, 1))                                                # [P,24,3(m)]
    A33 = Aj[:, :, :, :3]                                                                     # [P,24,i,m]
    wj = w.map(lambda t: t[:, :, None, None])
    Dm = Dj.map(lambda t: t[:, :, None, :])                                                  # [P,24,1,m]
    yi = y.map(lambda t: t[:, :, :, None])                                                   # [P,24,i,1]
    gvi = gv.map(lambda t: t[:, None, :, None])                                              # [P,1,i,1]
    t1 = gvi * (wj * A33 + Dm * yi)                                                          # [P,24,i,m]
    gJr = gJ.map(lambda t: t.unsqueeze(1))                                                   # [P,1,i,k]
    gja = esum(gJr * A33, -1)                                                                # [P,24,i]: sum_k gJ[i][k] A_j[i][k]
    gjd = esum(gJr * Dj.map(lambda t: t[:, :, None, :]), -1)                                 # [P,24,i]: sum_k gJ[i][k] D_jk
    t2 = Dm * gja.map(lambda t: t.unsqueeze(-1))                                             # [P,24,i,m]
    t3 = gjd.map(lambda t: t.unsqueeze(-1)) * A33
    cgy = esum(gJr * yi, 2)                                                                  # [P,24,k]: sum_i gJ[i][k] y_i
    Hxy, Hxz, Hyz = Hw[:, 0], Hw[:, 1], Hw[:, 2]                                             # [P,24]
    c0, c1, c2 = cgy[:, :, 0], cgy[:, :, 1], cgy[:, :, 2]
    t4 = estack([estack([Hxy * c1, Hxz * c2]), estack([Hxy * c0, Hyz * c2]), estack([Hxz * c0, Hyz * c1])], -1)   # [P,24,2,m]
    allt = ecat([t1, t2, t3, t4], 2)                                                         # [P,24,11,m]
    g_p = esum(allt.map(lambda t: t.reshape(P, -1, 3)), 1)
    W4 = ecat([w.map(lambda t: t.unsqueeze(1)), Dw], 1).map(lambda t: t.reshape(4 * P, KJ))
    phE = E(ph[:, None, :])                                                                  # [P,1,k]
    gJ4 = ecat([gJ, E(torch.zeros(P, 3, 1, dtype=torch.float64))], -1)                       # (k < 3) gJ[i][k]
    q0 = (gv.map(lambda t: t.unsqueeze(-1)) * phE + gJ4).map(lambda t: t.reshape(P, 12))
    rows = [_blocks(q0, frame, B)]
    for kp in range(3):
        rows.append(_blocks((gJ[:, :, kp].map(lambda t: t.unsqueeze(-1)) * phE).map(lambda t: t.reshape(P, 12)), frame, B))
    Q4 = estack(rows, 1).map(lambda t: t.reshape(4 * P, B * 12))
    return {"g_p": g_p, "W4": W4, "Q4": Q4, "Gs": _blocks(gv, frame, B), "valid": s["valid"]}


# ---------------------------------------------------------------------------------------------------------- root finder
def rootfind_update(p, f, gf, loss2, angle, gd, unfinished, counter, dthr, athr, w1, w2, do_update):
    """New p [P,3] (E; error 0 where the ray is not moved), the flags (uint8, exact), the counter (exact) and the smallest
    |grad|^2 minus its error over the moved rays (must be positive)."""
    f32 = f.float()
    done = (f32.abs() < np.float32(dthr)) & (angle.float() < np.float32(athr))
    un = (unfinished != 0) & ~done
    count = int(counter) + int(un.sum())
    w1e, w2e = E(float(np.float32(w1))), E(float(np.float32(w2)))
    loss = w1e * E(f64(f).abs()) + w2e * E(f64(loss2))
    sg = torch.sign(f64(f))
    g = (w1e * E(sg)).map(lambda t: t.unsqueeze(-1)) * E(f64(gf)) + w2e * E(f64(gd))          # [P,3]
    den = esum(g * g, -1)
    move = un & bool(do_update)
    safe = E(torch.where(move, den.v, torch.ones_like(den.v)), torch.where(move, den.e, torch.zeros_like(den.e)))
    margin = float((den.v - den.e)[move].min()) if bool(move.any()) else float("inf")
    if margin <= 0:
        return {"margin": margin}
    t = (-loss) / safe
    pn = E(f64(p)) + t.map(lambda x: x.unsqueeze(-1)) * g
    mv = move.unsqueeze(-1)
    pn = E(torch.where(mv, pn.v, f64(p)), torch.where(mv, pn.e, torch.zeros_like(pn.e)))
    return {"p": pn, "unfinished": un.to(torch.uint8), "count": count, "margin": margin, "moved": move}


# ------------------------------------------------------------------------------------------------------ kinematic chain
def rodrigues(tx, ty, tz):
    """angle = ||theta + 1e-8||, q = (cos(a/2), sin(a/2) theta / a), normalise, quaternion -> matrix; the nine entries, generic
    over E and Dual."""
    ax, ay, az = tx + EPS_RODRIGUES, ty + EPS_RODRIGUES, tz + EPS_RODRIGUES
    angle = esqrt(ax * ax + ay * ay + az * az)
    nx, ny, nz = tx / angle, ty / angle, tz / angle
    half = angle * 0.5
    qw, sh = ecos(half), esin(half)
    qx, qy, qz = sh * nx, sh * ny, sh * nz
    qn = esqrt(qw * qw + qx * qx + qy * qy + qz * qz)
    w, x, y, z = qw / qn, qx / qn, qy / qn, qz / qn
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    return [w2 + x2 - y2 - z2, xy * 2.0 - wz * 2.0, wy * 2.0 + xz * 2.0,
            wz * 2.0 + xy * 2.0, w2 - x2 + y2 - z2, yz * 2.0 - wx * 2.0,
            xz * 2.0 - wy * 2.0, wx * 2.0 + yz * 2.0, w2 - x2 - y2 + z2]


def _local(poses, Js, parents):
    """L [B,24,3,4] (E): [R_j | J_j - J_parent]."""
    th = E(f64(poses))
    R = estack(rodrigues(th[..., 0], th[..., 1], th[..., 2]), -1)                            # [B,24,9]
    Bn = R.v.shape[0]
    Jsd = f64(Js)
    par = [int(x) for x in parents]
    rel = [E(Jsd[0])] + [E(Jsd[j]) - E(Jsd[par[j]]) for j in range(1, KJ)]
    t = estack(rel, 0).map(lambda x: x.unsqueeze(0).expand(Bn, KJ, 3))
    return ecat([R.map(lambda x: x.reshape(Bn, KJ, 3, 3)), t.map(lambda x: x.unsqueeze(-1))], -1), par


def _aff_mul(Gp, L):
    """[B,3,4] . [B,3,4] with the implicit last row 0 0 0 1."""
    prod = Gp[:, :, :3].map(lambda t: t.unsqueeze(-1)) * L.map(lambda t: t.unsqueeze(1))     # [B,i,k,c]
    rot = esum(prod[:, :, :, :3], 2)                                                         # three products
    tr = esum(ecat([prod[:, :, :, 3], Gp[:, :, 3:4]], -1), -1)                               # three products and G_p[i][3]
    return ecat([rot, tr.map(lambda t: t.unsqueeze(-1))], -1)


def chain_forward(poses, Js, parents, init_pose=None):
    """G [B,24,4,4] and (with init_pose [24,4,4]) A = G . init_pose, as E."""
    L, par = _local(poses, Js, parents)
    Bn = L.v.shape[0]
    g = [L[:, 0]]
    for j in range(1, KJ):
        g.append(_aff_mul(g[par[j]], L[:, j]))
    G3 = estack(g, 1)                                                                        # [B,24,3,4]
    last = E(torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(Bn, KJ, 1, 4))
    G = ecat([G3, last], 2)
    out = {"G": G, "G3": G3, "L": L}
    if init_pose is not None:
        ip = E(f64(init_pose).unsqueeze(0))                                                  # [1,24,k,c]
        A3 = esum(G3.map(lambda t: t.unsqueeze(-1)) * ip.map(lambda t: t.unsqueeze(2)), 3)    # [B,24,i,c]
        A_last = E(f64(init_pose)[:, 3:4, :].unsqueeze(0).expand(Bn, KJ, 1, 4))
        out["A"] = ecat([A3, A_last], 2)
    return out


def chain_backward(poses, Js, parents, init_pose=None, gG=None, gA=None):
    """gposes [B,24,3] (E) for the cotangents gG, gA [B,24,4,4] (None = zeros)."""
    fw = chain_forward(poses, Js, parents)
    L, G3 = fw["L"], fw["G3"]
    par = [int(x) for x in parents]
    Bn = L.v.shape[0]
    zero = E(torch.zeros(Bn, 3, 4, dtype=torch.float64))
    contrib = [[] for _ in range(KJ)]
    for j in range(KJ):
        if gG is not None:
            contrib[j].append(E(f64(gG)[:, j, :3, :]))
        if gA is not None:
            ga = E(f64(gA)[:, j, :3, :])                                                     # [B,i,c]
            ip = E(f64(init_pose)[j].unsqueeze(0))                                           # [1,k,c]
            contrib[j].append(esum(ga.map(lambda t: t.unsqueeze(2)) * ip.map(lambda t: t.unsqueeze(1)), -1))
    th = E(f64(poses))
    one, nil = E(torch.ones(Bn, KJ, dtype=torch.float64)), E(torch.zeros(Bn, KJ, dtype=torch.float64))
    Rd = rodrigues(Dual(th[..., 0], [one, nil, nil]), Dual(th[..., 1], [nil, one, nil]), Dual(th[..., 2], [nil, nil, one]))
    dR = estack([estack(r.d, -1) for r in Rd], -2)                                           # [B,24,9,3]
    out = [None] * KJ
    for j in range(KJ - 1, -1, -1):
        dg = esum(estack(contrib[j], -1), -1) if contrib[j] else zero                        # [B,3,4]
        if j == 0:
            gR = dg[:, :, :3]
        else:
            p = par[j]
            Lj = L[:, j]                                                                     # [B,k,c]
            up = esum(dg.map(lambda t: t.unsqueeze(2)) * Lj.map(lambda t: t.unsqueeze(1)), -1)   # [B,i,k]
            contrib[p].append(ecat([up, dg[:, :, 3:4]], -1))
            gR = esum(G3[:, p, :, :3].map(lambda t: t.unsqueeze(-1)) * dg[:, :, :3].map(lambda t: t.unsqueeze(2)), 1)   # [B,k,c]
        out[j] = esum(gR.map(lambda t: t.reshape(Bn, 9, 1)) * dR[:, j], 1)                    # [B,3]
    return {"gposes": estack(out, 1)}


# -------------------------------------------------------------------------------------------------- positional encoding
def _pe_weights(L, weights):
    w = torch.ones(2 * L, dtype=torch.float64) if weights is None else f64(torch.as_tensor(weights, dtype=torch.float32))
    return w[:2 * L]


def _pe_bands(x, L, sincos=False):
    """sin and cos of x 2^b, [P,L,3] each (E); the argument is exact.  sincos: the pair comes from one sincosf call."""
    a = f64(x)[:, None, :3] * (2.0 ** torch.arange(L, dtype=torch.float64))[None, :, None]
    s = _efun(E(a), torch.sin, SINCOSF_ULP if sincos else SINF_ULP)
    c = _efun(E(a), torch.cos, SINCOSF_ULP if sincos else COSF_ULP)
    return s, c, (2.0 ** torch.arange(L, dtype=torch.float64))[None, :, None]


def posenc(x, L, weights=None, out_scale=1.0):
    """gamma(x) * out_scale, [P, 3 + 6L] (E)."""
    P = x.shape[0]
    osc = E(float(np.float32(out_scale)))
    s, c, _ = _pe_bands(x, L)
    w = _pe_weights(L, weights).reshape(1, L, 2, 1)
    sc = estack([s, c], 2)                                                                   # [P,L,2,3]
    body = (E(w) * sc) * osc
    return ecat([E(f64(x)[:, :3]) * osc, body.map(lambda t: t.reshape(P, 6 * L))], -1)


def posenc_vjp(x, g, L, weights=None, t=None):
    """t None: J(x)^T g.  t [P,3] (or [1,3] broadcast): t * sum_b f^2 (-w sin g_s - w cos g_c), the second-order form."""
    P = x.shape[0]
    s, c, f = _pe_bands(x, L, True)
    w = _pe_weights(L, weights).reshape(1, L, 2)
    gd = f64(g)
    gb = gd[:, 3:3 + 6 * L].reshape(P, L, 2, 3)
    gs, gc = E(gb[:, :, 0]), E(gb[:, :, 1])
    ws, wc = E(w[:, :, 0:1]), E(w[:, :, 1:2])
    if t is None:
        terms = ecat([(ws * c * gs).scaled(f), (-(wc * s * gc)).scaled(f), E(gd[:, None, :3])], 1)   # [P,2L+1,3]
        return esum(terms, 1)
    terms = ecat([(-(ws * s * gs)).scaled(f * f), (-(wc * c * gc)).scaled(f * f)], 1)
    acc = esum(terms, 1) if L else E(torch.zeros(P, 3, dtype=torch.float64))
    return acc * E(f64(t)[:, :3].expand(P, 3))


def posenc_jvp(x, t, L, weights=None):
    """J(x) t, [P, 3 + 6L] (E)."""
    P = x.shape[0]
    s, c, f = _pe_bands(x, L)
    w = _pe_weights(L, weights).reshape(1, L, 2, 1)
    td = f64(t)[:, :3].expand(P, 3)
    wf = E(w).scaled(f.unsqueeze(2))                                                         # w 2^b: exact
    body = (wf * estack([c, -s], 2)) * E(td[:, None, None, :])
    return ecat([E(td), body.map(lambda u_: u_.reshape(P, 6 * L))], -1)


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_volume(shape, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    D, H, W = shape
    vol = torch.rand(D, H, W, KJ, generator=g)
    return make_grid(vol, [0.05, -0.1, 0.02], [2.0 / 1.6, 2.0 / 2.2, 2.0 / 1.2])


def families(P):
    """The family of every point by its index: mostly in-voxel; clipped, lattice and (every 64th) NaN points in between."""
    i = torch.arange(P)
    fam = torch.full((P,), FAM_IN)
    fam[i % 8 == 5] = FAM_CLIP
    fam[i % 8 == 6] = FAM_LATTICE
    fam[i % 8 == 7] = FAM_CLIP
    fam[i % 64 == 63] = FAM_NAN
    return fam


def make_points(grid, P, seed=0, fam=None):
    """p [P,3] float32 built in voxel coordinates (module docstring) and the family of every point."""
    g = torch.Generator().manual_seed(2000 + seed)
    D, H, W = grid["vol"].shape[:3]
    size = torch.tensor([W, H, D], dtype=torch.float64)
    fam = families(P) if fam is None else fam
    cell = torch.floor(torch.rand(P, 3, generator=g, dtype=torch.float64) * (size - 1)).clamp_max(size - 2)
    frac = 1.0 / 16 + torch.rand(P, 3, generator=g, dtype=torch.float64) * (14.0 / 16)
    ix = cell + frac
    # clipped: every point has one, two or three axes outside, on either side; the 26 combinations in turn
    combos = [(a, b, c) for a in (0, 1, 2) for b in (0, 1, 2) for c in (0, 1, 2) if (a, b, c) != (0, 0, 0)]
    state = torch.tensor(combos)[torch.arange(P) % 26]
    off = 0.5 + 2.5 * torch.rand(P, 3, generator=g, dtype=torch.float64)
    clipped = torch.where(state == 1, -off, torch.where(state == 2, size - 1 + off, ix))
    ix = torch.where((fam == FAM_CLIP).unsqueeze(1), clipped, ix)
    lat = torch.floor(torch.rand(P, 3, generator=g, dtype=torch.float64) * size).clamp_max(size - 1)
    ix = torch.where((fam == FAM_LATTICE).unsqueeze(1), lat, ix)
    gcoord = (2.0 * ix + 1.0) / size - 1.0
    p = (f64(grid["center"]) + gcoord / f64(grid["scale"])).float()
    nanmask = (fam == FAM_NAN).unsqueeze(1) & (torch.arange(3).unsqueeze(0) <= (torch.arange(P) // 64 % 3).unsqueeze(1))
    p = torch.where(nanmask, torch.full_like(p, float("nan")), p)
    return p, fam


def make_frames(P, B, seed=0):
    g = torch.Generator().manual_seed(3000 + seed + B)
    frame = torch.randint(0, B, (P,), generator=g)
    if P >= 2:
        frame[0], frame[-1] = B - 1, 0
    A = torch.rand(B, KJ, 4, 4, generator=g) * 4.0 - 2.0
    trans = torch.randn(B, 3, generator=g)
    return frame, A, trans


def make_rays(d, cam, lo, seed=0):
    """Rays [P,3] float32, unit up to rounding, whose sine against d - cam is log-spaced over [lo, 0.98]."""
    g = torch.Generator().manual_seed(4000 + seed)
    e = f64(d) - f64(cam)
    P = e.shape[0]
    if P == 0:
        return torch.zeros(0, 3)
    eh = e / e.norm(dim=1, keepdim=True)
    r = torch.randn(P, 3, generator=g, dtype=torch.float64)
    n = torch.cross(eh, r, dim=1)
    n = n / n.norm(dim=1, keepdim=True)
    sin = torch.exp(torch.linspace(math.log(lo), math.log(0.98), P, dtype=torch.float64)) if P > 1 else torch.tensor([0.5], dtype=torch.float64)
    sin = sin[torch.randperm(P, generator=g)]
    sign = torch.where(torch.rand(P, generator=g) < 0.5, -1.0, 1.0).double()
    return (((1 - sin * sin).sqrt() * sign).unsqueeze(1) * eh + sin.unsqueeze(1) * n).float()


ROOT_DTHR, ROOT_ATHR, ROOT_W1, ROOT_W2 = float(np.float32(1e-3)), 2.0, 1.0, 0.5
ROOT_FAMILIES = ("finished", "none", "mixed")


def make_rootfind(P, family, seed=0):
    """Inputs of the root finder's step.  finished: every ray meets both thresholds; none: no ray does; mixed, by index mod 8:
    f == 0 exactly with a large angle, angle NaN, |f| == dthreshold exactly, angle == athreshold exactly (`<` is strict: both stay
    unfinished), a finished ray, and random rays; a fifth of the flags is already 0."""
    g = torch.Generator().manual_seed(10000 + seed + P)
    p = torch.randn(P, 3, generator=g)
    gf = torch.randn(P, 3, generator=g)
    gd = torch.randn(P, 3, generator=g)
    loss2 = torch.rand(P, generator=g) * 0.1
    sign = torch.where(torch.rand(P, generator=g) < 0.5, -1.0, 1.0)
    small_f = sign * torch.rand(P, generator=g) * ROOT_DTHR * 0.9
    large_f = sign * (ROOT_DTHR * 1.1 + torch.rand(P, generator=g) * 0.1)
    small_a = torch.rand(P, generator=g) * ROOT_ATHR * 0.9
    large_a = ROOT_ATHR * 1.1 + torch.rand(P, generator=g) * 5
    unfinished = (torch.rand(P, generator=g) > 0.2).to(torch.uint8)
    if family == "finished":
        f, angle = small_f, small_a
    elif family == "none":
        f, angle = large_f, small_a
    else:
        i = torch.arange(P) % 8
        f = torch.where(i < 5, small_f, torch.where(i == 5, large_f, small_f))
        angle = torch.where(i == 6, large_a, small_a)
        f = torch.where(i == 0, torch.zeros(P), f)
        angle = torch.where(i == 0, large_a, angle)
        angle = torch.where(i == 1, torch.full((P,), float("nan")), angle)
        f = torch.where(i == 2, sign * ROOT_DTHR, f)
        angle = torch.where(i == 3, torch.full((P,), ROOT_ATHR), angle)
    return {"p": p, "f": f.float(), "gf": gf, "loss2": loss2, "angle": angle.float(), "gd": gd, "unfinished": unfinished}


def smpl_parents():
    return [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]


def parent_tables():
    return {"smpl": smpl_parents(), "chain": [-1] + list(range(23)), "star": [-1] + [0] * 23}


def make_poses(B, seed=0):
    """N(0, 0.4) with exact zero rows, rows of magnitude 1e-6 and 1e-3, one row of norm near pi and one near 2 pi."""
    g = torch.Generator().manual_seed(5000 + seed + B)
    poses = 0.4 * torch.randn(B, KJ, 3, generator=g)
    if B:
        poses[0, 3] = 0.0
        poses[0, 0] = 0.0
        poses[B - 1, 5] = torch.tensor([1e-6, -2e-6, 0.5e-6])
        poses[B - 1, 7] = torch.tensor([1e-3, 2e-3, -1e-3])
        a = torch.tensor([0.6, -0.64, 0.48])
        poses[B // 2, 2] = a / a.norm() * 3.14
        poses[B // 2, 9] = a / a.norm() * 6.28
        poses[B // 2, 23] = 0.0
    return poses


def make_joints(seed=0):
    g = torch.Generator().manual_seed(6000 + seed)
    return torch.randn(KJ, 3, generator=g) * 0.3


def make_init_pose(seed=0, general_last_row=False):
    g = torch.Generator().manual_seed(7000 + seed)
    ip = torch.randn(KJ, 4, 4, generator=g)
    if not general_last_row:
        ip[:, 3, :] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    return ip


def pe_weight_sets(L):
    """NULL, annealing weights with exact zeros, negative weights."""
    g = torch.Generator().manual_seed(8000 + L)
    ann = torch.linspace(1.5, -0.5, 2 * L).clamp(0, 1) if L else torch.zeros(0)
    return {"null": None, "anneal": ann.float(), "negative": (torch.rand(2 * L, generator=g) * 2 - 1.5).float()}


def make_pe_x(P, seed=0):
    g = torch.Generator().manual_seed(9000 + seed + P)
    return (torch.rand(P, 3, generator=g) * 2 - 1) * torch.logspace(-4, 0.5, max(P, 1))[:P].unsqueeze(1)
