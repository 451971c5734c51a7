"""recmv_linear_backward and the kernels around it (recmv_colsum, recmv_act_grad, recmv_act_grad2, recmv_act_grad_2d, the weight
norm, recmv_gather_rows, recmv_add_scaled_2d) against the float64 references of tests/layer_backward_reference.py.

Two kinds of test for every kernel: exact-integer inputs (every partial sum is an integer below 2^24, so the result must be
torch.equal to the int64 reference in any summation order: one dropped, doubled or misplaced element fails) and inputs over several
decades judged by bounds that hold for any summation order.  The bounds are derived in the docstring of layer_backward_reference;
every bounded test prints its largest error / bound.  Buffers are surrounded by NaN: a kernel that reads a padding column poisons its
sums, one that writes past its output destroys a sentinel.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
import layer_backward_reference as R  # noqa: E402

DEV = "cuda:0"
ERR_WORKSPACE = -4
NAN = float("nan")


def _lib():
    from recmv import _lib as L
    return L, L.lib()


def _stream():
    L, _ = _lib()
    return L.stream_ptr(torch.device(DEV))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _placed(t, pad=0, shift=0):
    """A device copy of the 2-D (or 1-D) float32 tensor `t` whose rows are `pad` floats apart beyond their width and whose base
    pointer is moved by `shift` floats off the allocation's 16-byte alignment; everything around the values is NaN."""
    t2 = t.reshape(1, -1) if t.dim() == 1 else t
    rows, cols = t2.shape
    ld = cols + pad
    flat = torch.full((rows * ld + shift + 8,), NAN, device=DEV)
    view = flat[shift:shift + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t2)
    return view.reshape(-1) if t.dim() == 1 else view


def _around(view):
    """Every element of the buffer behind a _placed view that is not one of the view's own (rows x cols) values."""
    base = view._base
    rows, cols = view.shape
    own = view.storage_offset() + torch.arange(rows, device=DEV).view(-1, 1) * view.stride(0) + torch.arange(cols, device=DEV)
    mask = torch.ones(base.numel(), dtype=torch.bool, device=DEV)
    mask[own.reshape(-1)] = False
    return base[mask]


def _ld(v, width):
    return v.stride(0) if v.shape[0] > 1 else max(width, 1)


def _report(name, **ratios):
    print("ratio %s: %s" % (name, "  ".join("%s %.3g" % kv for kv in ratios.items())))
    for k, v in ratios.items():
        assert v <= 1.0, "%s: %s error / bound = %.4g" % (name, k, v)


def _ratio(got, ref, bound):
    return R.ratio((got.cpu().double() - ref).abs(), bound)


@pytest.fixture
def f32_matrix_mode():
    L, _ = _lib()
    prev = L.set_gemm_mode(0)
    try:
        yield
    finally:
        L.set_gemm_mode(prev)


def _linear_backward(gy, y, x, W, act, p, want=("gx", "gW", "gb")):
    """recmv_linear_backward through the C ABI on device views (any row stride / base alignment) with a workspace of exactly the
    advertised size; the outputs not in `want` are passed as NULL."""
    L, lib = _lib()
    M, N = gy.shape
    K = x.shape[1]
    Wt = W.t().contiguous()
    ws = torch.empty(int(lib.recmv_linear_backward_workspace_bytes(M, N, K)), dtype=torch.uint8, device=DEV)
    out = {"gx": torch.full((M, K), NAN, device=DEV) if "gx" in want else None,
           "gW": torch.full((N, K), NAN, device=DEV) if "gW" in want else None,
           "gb": torch.full((N,), NAN, device=DEV) if "gb" in want else None}
    L.check(lib.recmv_linear_backward(_p(gy), _ld(gy, N), _p(y), _ld(y, N), _p(x), _ld(x, K), _p(Wt), N, M, N, K, act, float(p),
                                      _p(out["gx"]), K, _p(out["gW"]), _p(out["gb"]), _p(ws), ws.numel(), _stream()),
            "linear_backward")
    return out


def _on_device(c):
    return {k: c[k].to(DEV) for k in ("gy", "y", "x", "W")}


# ------------------------------------------------------------------------------------------------ recmv_linear_backward
@pytest.mark.parametrize("M,N,K,act", R.LINEAR_CASES)
def test_linear_backward_exact_on_integers(f32_matrix_mode, M, N, K, act):
    from recmv import ops
    c = R.int_case(M, N, K, act)
    d = _on_device(c)
    got = _linear_backward(d["gy"], d["y"], d["x"], d["W"], c["act"], 0.0)
    for k in ("gb", "gx", "gW"):
        assert torch.equal(got[k].cpu(), c["want"][k]), k
    # the wrapper the autograd Function calls
    gx, gW, gb = ops.linear_backward(d["gy"], d["y"], d["x"], d["W"], c["act"], 0.0)
    assert torch.equal(gx.cpu(), c["want"]["gx"]) and torch.equal(gW.cpu(), c["want"]["gW"]) and torch.equal(gb.cpu(), c["want"]["gb"])
    # the same values inside wider NaN-padded buffers, rows and base off the 16-byte alignment
    got = _linear_backward(_placed(c["gy"], 1, 1), _placed(c["y"], 3, 0), _placed(c["x"], 1, 0), d["W"], c["act"], 0.0)
    for k in ("gb", "gx", "gW"):
        assert torch.equal(got[k].cpu(), c["want"][k]), k + " (strided)"


@pytest.mark.parametrize("M,N,K,act", R.BOUNDED_CASES)
def test_linear_backward_within_float64_bounds(M, N, K, act):
    c = R.float_case(M, N, K, act)
    d = _on_device(c)
    got = _linear_backward(d["gy"], d["y"], d["x"], d["W"], act, c["p"])
    _report("linear_backward M=%d N=%d K=%d act=%d" % (M, N, K, act),
            **{k: _ratio(got[k], c["ref"][k], c["bound"][k]) for k in ("gb", "gx", "gW")})


@pytest.mark.parametrize("M,N,K,act", R.NEAR_ZERO_CASES)
def test_linear_backward_softplus_near_zero_within_float64_bounds(M, N, K, act):
    """Every beta y in [1e-5, 1e-4]: a derivative computed as 1 - exp(-beta y) is wrong by up to 1e-2 of every element of dZ, far
    beyond the bounds of gb, gx and gW; -expm1(-beta y) meets them."""
    c = R.float_case(M, N, K, act, True)
    d = _on_device(c)
    got = _linear_backward(d["gy"], d["y"], d["x"], d["W"], act, c["p"])
    _report("linear_backward near zero M=%d N=%d K=%d" % (M, N, K),
            **{k: _ratio(got[k], c["ref"][k], c["bound"][k]) for k in ("gb", "gx", "gW")})


def test_linear_backward_of_an_empty_batch():
    """M = 0: OK, zero parameter gradients — with the NULL data pointers that empty tensors carry, and through LinearAct."""
    from recmv import ops
    L, lib = _lib()
    N, K = 5, 3
    Wt = torch.randn(K, N, device=DEV)
    ws = torch.empty(int(lib.recmv_linear_backward_workspace_bytes(0, N, K)), dtype=torch.uint8, device=DEV)
    one = torch.zeros(8, device=DEV)
    for inputs in (one, None):
        gW, gb = torch.full((N, K), NAN, device=DEV), torch.full((N,), NAN, device=DEV)
        rc = lib.recmv_linear_backward(_p(inputs), N, _p(inputs), N, _p(inputs), K, _p(Wt), N, 0, N, K, R.ACT_SOFTPLUS, 100.0,
                                       _p(inputs), K, _p(gW), _p(gb), _p(ws), ws.numel(), _stream())
        assert rc == 0, lib.recmv_last_error()
        assert torch.equal(gW, torch.zeros_like(gW)) and torch.equal(gb, torch.zeros_like(gb))
    for create_graph in (False, True):
        x = torch.zeros(0, K, device=DEV, requires_grad=True)
        W = torch.randn(N, K, device=DEV, requires_grad=True)
        b = torch.randn(N, device=DEV, requires_grad=True)
        y = ops.linear_act(x, W, b, ops.ACT_SOFTPLUS, 100.0)
        gx, gW, gb = torch.autograd.grad(y, [x, W, b], torch.zeros(0, N, device=DEV), create_graph=create_graph)
        assert gx.shape == (0, K) and not gW.any() and not gb.any() and gW.shape == (N, K) and gb.shape == (N,)


@pytest.mark.parametrize("M,N,K,act", [(255, 64, 39, R.ACT_SOFTPLUS), (300, 473, 512, R.ACT_SOFTPLUS),
                                       (4099, 512, 512, R.ACT_SOFTPLUS)])
def test_linear_backward_routes_agree(M, N, K, act):
    """gy and y as column slices of wider buffers (row stride N + 4: 16-byte rows when N % 4 == 0; N + 1: element accesses) and from
    a base pointer moved by one float.  dZ is element-wise, so gx and gW are the same bits on every route; gb meets its bound."""
    c = R.float_case(M, N, K, act)
    d = _on_device(c)
    base = _linear_backward(d["gy"], d["y"], d["x"], d["W"], act, c["p"])
    worst = {}
    for name, pad, shift in (("ld+4", 4, 0), ("ld+1", 1, 0), ("base+1", 0, 1), ("ld+4,base+1", 4, 1)):
        got = _linear_backward(_placed(c["gy"], pad, shift), _placed(c["y"], pad, shift), d["x"], d["W"], act, c["p"])
        assert torch.equal(got["gx"], base["gx"]) and torch.equal(got["gW"], base["gW"]), name
        worst[name] = _ratio(got["gb"], c["ref"]["gb"], c["bound"]["gb"])
    _report("linear_backward routes gb M=%d N=%d" % (M, N), **worst)


@pytest.mark.parametrize("M,N,K,act", [(257, 65, 168, R.ACT_SOFTPLUS), (300, 473, 512, R.ACT_SOFTPLUS), (1000, 257, 512, R.ACT_TANH),
                                       (4099, 512, 512, R.ACT_SOFTPLUS)])
def test_linear_backward_output_subsets_equal_the_full_call(M, N, K, act):
    c = R.float_case(M, N, K, act)
    d = _on_device(c)
    full = _linear_backward(d["gy"], d["y"], d["x"], d["W"], act, c["p"])
    for want in (("gx", "gW"), ("gx",), ("gW",), ("gb",)):              # without gb: the recmv_act_grad_2d route
        got = _linear_backward(d["gy"], d["y"], d["x"], d["W"], act, c["p"], want)
        for k in want:
            assert torch.equal(got[k], full[k]), (want, k)


@pytest.mark.parametrize("M,N,K,act", [(300, 473, 512, R.ACT_SOFTPLUS), (1000, 257, 512, R.ACT_TANH), (257, 65, 168, R.ACT_RELU),
                                       (3, 5, 3, R.ACT_NONE)])
def test_linear_act_backward_both_routes_within_float64_bounds(M, N, K, act):
    """LinearAct.backward replayed without a graph (one recmv_linear_backward call) and with create_graph=True (ActGrad, MatmulNT,
    MatmulTN, a torch column sum), both judged by the float64 reference of the layer's own float32 output y."""
    from recmv import ops
    g = torch.Generator().manual_seed(M + N)
    p = R.act_param(act)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / np.sqrt(K) * (0.2 if act == R.ACT_SOFTPLUS else 1.0)
    b = torch.randn(N, generator=g) * 0.02
    gy = torch.randn(M, N, generator=g) * torch.logspace(-3, 2, M).view(-1, 1)
    xd, Wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, W, b))
    y = ops.linear_act(xd, Wd, bd, act, p)
    assert act != R.ACT_SOFTPLUS or (y >= 0).all()
    assert act != R.ACT_TANH or (y.abs() <= 1).all()
    ref = R.layer_backward(gy, y, x, W, act, p)
    gza, bdz = ref["gz"].abs(), R.bound_dz(gy, y, act, p)
    bound = {"gb": R.bound_colsum(gza, bdz), "gx": R.bound_product(gza, bdz, R.f64(W).abs()),
             "gW": R.bound_product(gza.t(), bdz.t(), R.f64(x).abs())}
    for create_graph in (False, True):
        gx, gW, gb = torch.autograd.grad(y, [xd, Wd, bd], gy.to(DEV), create_graph=create_graph, retain_graph=True)
        assert gx.requires_grad == create_graph
        _report("LinearAct M=%d N=%d K=%d act=%d create_graph=%s" % (M, N, K, act, create_graph),
                gb=_ratio(gb.detach(), ref["gb"], bound["gb"]), gx=_ratio(gx.detach(), ref["gx"], bound["gx"]),
                gW=_ratio(gW.detach(), ref["gW"], bound["gW"]))


# ----------------------------------------------------------------------------------------------------------- recmv_colsum
@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_exact_and_bounded(rows):
    L, lib = _lib()
    worst = 0.0
    for cols in R.COLSUM_COLS:
        g = torch.Generator().manual_seed(rows * 7 + cols)
        ints = torch.randint(-3, 4, (rows, cols), generator=g).float()
        vals = torch.randn(rows, cols, generator=g) * torch.logspace(-3, 2, rows).view(-1, 1)
        need = int(lib.recmv_colsum_workspace_bytes(rows, cols))
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        for k, src in enumerate((ints, vals)):
            buf = _placed(src, 3, k)                                     # ld = cols + 3 > cols, NaN between the rows
            out = torch.full((cols + 2,), -7.0, device=DEV)
            L.check(lib.recmv_colsum(_p(buf), _ld(buf, cols), rows, cols, _p(out), _p(ws), need, _stream()), "colsum")
            assert torch.equal(out[cols:].cpu(), torch.full((2,), -7.0)), "wrote beyond cols"
            ref = src.double().sum(0)
            if k == 0:
                assert ints.abs().sum(0).max() < 2 ** 24
                assert torch.equal(out[:cols].cpu(), ref.to(torch.int64).float()), (rows, cols)
            else:
                worst = max(worst, _ratio(out[:cols], ref, R.bound_colsum(src.double().abs())))
    _report("colsum rows=%d" % rows, colsum=worst)


@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_refuses_a_workspace_one_byte_short(rows):
    L, lib = _lib()
    for cols in R.COLSUM_COLS:
        src = _placed(torch.ones(rows, cols), 3, 0)
        need = int(lib.recmv_colsum_workspace_bytes(rows, cols))
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        out = torch.full((cols,), -7.0, device=DEV)
        assert lib.recmv_colsum(_p(src), _ld(src, cols), rows, cols, _p(out), _p(ws), need - 1, _stream()) == ERR_WORKSPACE
        assert torch.equal(out.cpu(), torch.full((cols,), -7.0)), "wrote its output although it refused the call"


# ------------------------------------------------------------------------------------- activation-gradient kernels
def _ulps(got, ref):
    """|got - ref| in units in the last place of the float32 nearest to ref (float64 tensors, ref != 0)."""
    _, e = torch.frexp(ref.abs())                                        # |ref| = m 2^e, 0.5 <= m < 1: ulp = 2^(e - 24)
    return (got - ref).abs() / torch.ldexp(torch.ones_like(ref), e - 24)


def test_expm1f_and_expf_accuracy():
    """The figures E1 and E2 that the softplus bounds allow for the device's expm1f and expf, measured against float64: with
    gy = a = b = 1 and beta = 1 every other step of recmv_act_grad / recmv_act_grad2 is exact."""
    L, lib = _lib()
    t = torch.cat([torch.logspace(-9, float(np.log10(120.0)), 1 << 18, dtype=torch.float64).float(),
                   torch.tensor([1e-7, 1e-5, 1.0, 87.0, 104.0, 120.0])])
    n = t.numel()
    td, one = t.to(DEV), torch.ones(n, device=DEV)
    out = torch.empty(n, device=DEV)
    L.check(lib.recmv_act_grad(_p(one), _p(td), _p(out), n, R.ACT_SOFTPLUS, 1.0, _stream()), "act_grad")
    ref = -torch.expm1(-t.double())
    e1 = _ulps(out.cpu().double(), ref)
    r1 = (out.cpu().double() - ref).abs() / (R.U * ref)
    L.check(lib.recmv_act_grad2(_p(one), _p(one), _p(td), _p(out), n, R.ACT_SOFTPLUS, 1.0, _stream()), "act_grad2")
    keep = t <= 87.0                                                     # exp(-t) is a normal float32
    ref = torch.exp(-t.double())[keep]
    e2 = _ulps(out.cpu().double()[keep], ref)
    r2 = (out.cpu().double()[keep] - ref).abs() / (R.U * ref)
    print("measured expm1f: %.3f ulp, relative %.3f u;  expf: %.3f ulp, relative %.3f u" % (e1.max(), r1.max(), e2.max(), r2.max()))
    assert float(e1.max()) <= R.EXPM1F_ULP and float(r1.max()) <= 2.0 * R.EXPM1F_ULP
    assert float(e2.max()) <= R.EXPF_ULP and float(r2.max()) <= 2.0 * R.EXPF_ULP


@pytest.mark.parametrize("act", R.ACTS)
def test_act_grad_and_act_grad2_flat(act):
    L, lib = _lib()
    p = R.act_param(act)
    worst1 = worst2 = 0.0
    for n in R.ACT_GRAD_N:
        gy, b, y = R.act_inputs(n, act)
        ref1 = R.f64(gy) * R.dact(y, act, p)
        ref2 = R.f64(gy) * R.f64(b) * R.d2act(y, act, p)
        b1, b2 = R.bound_dz(gy, y, act, p), R.bound_act_grad2(gy, b, y, act, p)
        for shifts in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 1), (1, 0, 0, 0)):          # gy, b, y, out
            gd, bd, yd = _placed(gy, 0, shifts[0]), _placed(b, 0, shifts[1]), _placed(y, 0, shifts[2])
            for which in (1, 2):
                buf = torch.full((n + shifts[3] + 4,), -7.0, device=DEV)
                out = buf[shifts[3]:shifts[3] + n]
                if which == 1:
                    L.check(lib.recmv_act_grad(_p(gd), _p(yd), _p(out), n, act, p, _stream()), "act_grad")
                else:
                    L.check(lib.recmv_act_grad2(_p(gd), _p(bd), _p(yd), _p(out), n, act, p, _stream()), "act_grad2")
                assert (buf[:shifts[3]] == -7.0).all() and (buf[shifts[3] + n:] == -7.0).all(), "wrote outside out"
                ref, bound = (ref1, b1) if which == 1 else (ref2, b2)
                if act in (R.ACT_NONE, R.ACT_RELU):
                    assert torch.equal(out.cpu().double(), ref), (which, n, shifts)
                elif which == 1:
                    worst1 = max(worst1, _ratio(out, ref, bound))
                else:
                    worst2 = max(worst2, _ratio(out, ref, bound))
    _report("act_grad / act_grad2 act=%d" % act, act_grad=worst1, act_grad2=worst2)


@pytest.mark.parametrize("act", R.ACTS)
def test_act_grad_2d(act):
    """Widths around the float4 path on aligned and one-float-offset pointers, padded rows, y_scale and out_scale other than 1, and one
    cotangent row for every point (row stride 0)."""
    L, lib = _lib()
    p = R.act_param(act)
    rows = 5
    worst = 0.0
    for cols in R.ACT_GRAD_N:
        gy, _, y = R.act_inputs(rows * cols, act, seed=1)
        gy, y = gy.view(rows, cols), y.view(rows, cols)
        for pad, shift, ys, os_, bcast in ((0, 0, 1.0, 1.0, False), (4, 0, 1.0, 1.0, False), (1, 0, 1.0, 1.0, False),
                                           (0, 1, 1.0, 1.0, False), (0, 0, 0.7, 1.3, False), (3, 1, 0.7, 1.3, False),
                                           (0, 0, 1.0, 1.0, True), (1, 1, 0.7, 1.3, True)):
            g_used = gy[:1].expand(rows, cols) if bcast else gy
            gd = _placed(gy[:1].contiguous() if bcast else gy, pad, shift)
            yd = _placed(y, pad, shift)
            ldo = cols + pad
            buf = torch.full((rows * ldo + shift + 4,), -7.0, device=DEV)
            L.check(lib.recmv_act_grad_2d(_p(gd), 0 if bcast else ldo, _p(yd), ldo, C.c_void_p(buf.data_ptr() + 4 * shift), ldo, rows,
                                          cols, act, p, ys, os_, _stream()), "act_grad_2d")
            body = buf[shift:shift + rows * ldo].view(rows, ldo)
            assert (body[:, cols:] == -7.0).all() and (buf[:shift] == -7.0).all() and (buf[shift + rows * ldo:] == -7.0).all()
            ref = float(np.float32(os_)) * R.f64(g_used) * R.dact(R.f64(y) * float(np.float32(ys)), act, p)
            bound = R.bound_dz(g_used, y, act, p, ys, os_)
            if act in (R.ACT_NONE, R.ACT_RELU) and os_ == 1.0:
                assert torch.equal(body[:, :cols].cpu().double(), ref), (cols, pad, shift)
            else:
                worst = max(worst, _ratio(body[:, :cols], ref, bound))
    _report("act_grad_2d act=%d" % act, dz=worst)


# -------------------------------------------------------------------------------------------------------------- weight norm
@pytest.mark.parametrize("rows", R.WN_ROWS)
def test_weight_norm_forward_and_backward(rows):
    L, lib = _lib()
    worst = {"W": 0.0, "norms": 0.0, "gv": 0.0, "gg": 0.0}
    for cols in R.WN_COLS:
        v, g, gW = R.wn_inputs(rows, cols)
        vd, gd, gWd = v.to(DEV), g.to(DEV), gW.to(DEV)
        W = torch.full((rows, cols), NAN, device=DEV)
        norms = torch.full((rows + 1,), -7.0, device=DEV)
        L.check(lib.recmv_weight_norm_forward(_p(vd), _p(gd), _p(W), _p(norms), rows, cols, _stream()), "weight_norm_forward")
        assert float(norms[rows]) == -7.0
        W64, n64 = R.weight_norm(v, g)
        bW, bn = R.bound_wn_forward(v, g)
        worst["W"] = max(worst["W"], _ratio(W, W64, bW))
        worst["norms"] = max(worst["norms"], _ratio(norms[:rows], n64, bn))
        # the backward kernel as a function of its own inputs: norms = the float64 norm rounded to float32
        nd = n64.float().to(DEV)
        gv = torch.full((rows, cols), NAN, device=DEV)
        gg = torch.full((rows + 1,), -7.0, device=DEV)
        L.check(lib.recmv_weight_norm_backward(_p(vd), _p(gd), _p(nd), _p(gWd), _p(gv), _p(gg), rows, cols, _stream()),
                "weight_norm_backward")
        assert float(gg[rows]) == -7.0
        gv64, gg64, _ = R.weight_norm_backward(v, g, gW)
        bgv, bgg = R.bound_wn_backward(v, g, gW)
        worst["gv"] = max(worst["gv"], _ratio(gv, gv64, bgv))
        worst["gg"] = max(worst["gg"], _ratio(gg[:rows], gg64, bgg))
    _report("weight_norm rows=%d" % rows, **worst)


# -------------------------------------------------------------------------------------------------------------- glue kernels
def test_gather_rows():
    L, lib = _lib()
    g = torch.Generator().manual_seed(3)
    T, cols, rows = 7, 9, 300
    table = torch.randn(T, cols, generator=g)
    td = _placed(table, 2, 1)                                            # ldt = cols + 2
    index = torch.randint(0, T, (rows,), generator=g)
    index[:6] = torch.tensor([6, 6, 0, 6, 3, 0])                         # repeated, unordered
    idx_d = index.to(DEV)
    for idx, fill, pad in ((idx_d, cols, 0), (idx_d, cols + 5, 0), (idx_d, cols + 5, 3), (None, cols + 1, 2), (None, cols, 0)):
        ldo = fill + pad
        out = torch.full((rows, ldo), -7.0, device=DEV)
        L.check(lib.recmv_gather_rows(_p(td), td.stride(0), _p(idx), _p(out), ldo, rows, cols, fill, _stream()), "gather_rows")
        want = R.gather_rows(table, index if idx is not None else None, rows, cols, fill)
        assert torch.equal(out[:, :fill].cpu(), want), (fill, pad)
        assert (out[:, fill:] == -7.0).all()
    out = torch.full((rows, 6), -7.0, device=DEV)                        # cols = 0: no table is read, `fill` columns are zeroed
    L.check(lib.recmv_gather_rows(C.c_void_p(0), 0, _p(idx_d), _p(out), 6, rows, 0, 4, _stream()), "gather_rows")
    assert torch.equal(out[:, :4].cpu(), torch.zeros(rows, 4)) and (out[:, 4:] == -7.0).all()


def test_add_scaled_2d():
    L, lib = _lib()
    g = torch.Generator().manual_seed(4)
    rows, cols = 301, 39
    ai = torch.randint(-9, 10, (rows, cols), generator=g).float()
    bi = torch.randint(-9, 10, (rows, cols), generator=g).float()
    af = torch.randn(rows, cols, generator=g) * torch.logspace(-3, 2, rows).view(-1, 1)
    bf = torch.randn(rows, cols, generator=g) * torch.logspace(2, -3, rows).view(-1, 1)
    s_skip = float(np.float32(1.0 / np.sqrt(2.0)) - np.float32(1.0))
    worst = 0.0
    for a, b, s in ((ai, bi, 2.0), (af, bf, 0.0), (af, bf, s_skip)):
        for alias in (False, True):
            # strides cols + 1, cols + 5 and, for a separate output, cols + 2; with alias the output IS a (stride cols + 1), in place
            ad, bd = _placed(a, 1, 0), _placed(b, 5, 1)
            full = torch.full((rows, cols + 2), -7.0, device=DEV)
            out = ad if alias else full[:, :cols]
            L.check(lib.recmv_add_scaled_2d(_p(ad), ad.stride(0), _p(bd), bd.stride(0), s, _p(out), out.stride(0), rows, cols,
                                            _stream()), "add_scaled_2d")
            assert (full[:, cols:] == -7.0).all() and (alias or (full[:, :cols] != -7.0).any())
            assert torch.isnan(_around(ad)).all() and torch.isnan(_around(bd)).all(), "wrote into the padding of an operand"
            if not alias:
                assert torch.equal(ad.cpu(), a), "changed its input a"
            if s == 2.0:
                assert torch.equal(out.cpu(), (ai.double() + 2.0 * bi.double()).float())
            elif s == 0.0:
                assert torch.equal(out.cpu(), a)
            else:
                worst = max(worst, _ratio(out, R.add_scaled(a, s, b), R.bound_add_scaled(a, s, b)))
    _report("add_scaled_2d", skip_scale=worst)
