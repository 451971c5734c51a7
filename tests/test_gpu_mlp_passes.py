"""The whole-MLP passes — the per-layer chain (csrc/mlp_chain.hip), the row-tile kernels (csrc/mlp_rows.hip) and the jet pass
(csrc/mlp_jet.hip) — through the C ABI against the float64 references of tests/mlp_reference.py.

Every bounded test prints `ratio name: ...` (largest error / bound) and asserts <= 1; the bounds are derived in the docstring of
mlp_reference and never fitted.  Exact outputs (integer inputs, keep 0 against keep 1, the two fill modes, a ray in another tile) are
compared bit for bit.  Outputs are pre-filled with NaN and guarded by sentinels on both sides; strided operands sit in NaN-padded
buffers; workspaces start as NaN.  The rows of a pass are independent, so one reference of 257 rows per descriptor serves every
smaller row count (the jet's parameter gradients, which sum over the rows, have their own).
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
import mlp_reference as M  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
SENT = -7.0
GUARD = 8
ERR_ARG, ERR_WORKSPACE = -1, -4
PMAX = 257


def _lib():
    from recmv import _lib as L
    return L, L.lib()


def _stream():
    L, _ = _lib()
    return L.stream_ptr(torch.device(DEV))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _out(*shape):
    """An output buffer full of NaN between two rows of sentinels."""
    n = int(np.prod(shape)) if shape else 1
    base = torch.full((n + 2 * GUARD,), SENT, device=DEV)
    base[GUARD:GUARD + n] = NAN
    return base[GUARD:GUARD + n].view(*shape)


def _guards_ok(*views):
    for v in views:
        base = v._base
        assert bool((base[:GUARD] == SENT).all()) and bool((base[-GUARD:] == SENT).all()), "wrote outside its output"


def _placed(t, ld):
    """A device copy of the [rows, cols] float32 tensor with row stride ld >= cols; NaN everywhere else."""
    rows, cols = t.shape
    flat = torch.full((max(rows, 1) * ld + 8,), NAN, device=DEV)
    view = flat[:rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    return view


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _report(name, **ratios):
    print("ratio %s: %s" % (name, "  ".join("%s %.3g" % kv for kv in ratios.items())))
    for k, v in ratios.items():
        assert v <= 1.0, "%s: %s error / bound = %.4g" % (name, k, v)


def _ratio(got, ref, rows=None, ok=None):
    """Largest |got - ref.v| / ref.e over the first `rows` rows, the rows with ok False left out (they must still be finite)."""
    got = got.detach().cpu().double()
    v, e = ref.v, ref.e
    if rows is not None:
        v, e = v[:rows], e[:rows]
        ok = ok[:rows] if ok is not None else None
    assert bool(torch.isfinite(got).all()), "a non-finite output"
    err = (got.reshape(v.shape) - v).abs()
    if ok is not None:
        err, e = err[ok], e[ok]
    return M.ratio(err, e)


def _ws(nbytes):
    return torch.full((max(int(nbytes), 256),), 0xff, dtype=torch.uint8, device=DEV)


class _Net:
    """The recmv_mlp descriptor of a reference net over device tensors that it keeps alive."""

    def __init__(self, m):
        L, _ = _lib()
        self.m, self.d, self.keep = m, L.Mlp(), []
        d = self.d
        d.n_layers, d.multires, d.cond_dim, d.skip_layer = m["n"], m["L"], m["cond_dim"], m["skip"]
        d.hidden_act, d.residual, d.act_param = m["act"], int(m["residual"]), m["p"]
        for i, v in enumerate(m["dims"]):
            d.dims[i] = v
        for i in range(32):
            d.pe_weights[i] = m["pe_w"][i] if i < 2 * m["L"] else 1.0
        for l in range(m["n"]):
            d.rows[l] = m["rows"][l]
            d.W[l], d.Wt[l], d.bias[l] = self._put(m["W"][l]), self._put(m["W"][l].t()), self._put(m["b"][l])
            if m["W2"] is not None:
                d.W2[l], d.Wt2[l], d.bias2[l] = self._put(m["W2"][l]), self._put(m["W2"][l].t()), self._put(m["b2"][l])
        d.split_row = m["split"]

    def _put(self, t):
        if t is None:
            return None
        t = t.contiguous().to(DEV)
        self.keep.append(t)
        return t.data_ptr()

    def ref(self):
        return C.byref(self.d)


@functools.lru_cache(maxsize=None)
def _net(name):
    return _Net(M.net(name))


@functools.lru_cache(maxsize=None)
def _inputs(name, P=PMAX, integer=False):
    m = M.net(name)
    inp = M.make_inputs(m, P, integer=integer)
    dev = {"x": inp["x"].to(DEV), "idx": inp["idx"].to(DEV),
           "cond": _placed(inp["cond"], M.COND_LD) if m["cond_dim"] else None}
    return inp, dev


@functools.lru_cache(maxsize=None)
def _ref_fwd(name, family, n_out, use_idx=True, P=PMAX):
    m = M.net(name)
    inp, _ = _inputs(name, P)
    return M.forward(m, inp["x"], inp["cond"], inp["idx"] if use_idx else None, n_out, family)


@functools.lru_cache(maxsize=None)
def _ref_vjp(name, family, n_out, null, use_idx=True, P=PMAX):
    m = M.net(name)
    inp, _ = _inputs(name, P)
    return M.vjp(m, inp["x"], inp["cond"], inp["idx"] if use_idx else None, n_out, None if null else inp["gy"][:, :n_out], family)


def _ld_cond(m):
    return M.COND_LD if m["cond_dim"] else 0


# ------------------------------------------------------------------------------------------------------------ runners
def _chain_forward(N, dev, P, n_out, keep, use_idx=True, ldo=None, rows=slice(None), ws=None):
    _, lib = _lib()
    ldo = n_out if ldo is None else ldo
    need = lib.recmv_mlp_workspace_bytes(N.ref(), P, keep)
    ws = _ws(need) if ws is None else ws
    out = _out(max(P, 1), ldo)
    x = dev["x"][rows][:P].contiguous()
    idx = dev["idx"][rows][:P].contiguous() if (use_idx and N.m["cond_dim"]) else None
    rc = lib.recmv_mlp_forward(N.ref(), _p(x), _p(dev["cond"]), _ld_cond(N.m), _p(idx), P, n_out, _p(out), ldo, _p(ws), need, keep,
                               _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib()[1].recmv_last_error()
    _guards_ok(out)
    return out, ws, x


def _chain_vjp(N, x, P, n_out, g, ws):
    _, lib = _lib()
    gx = _out(max(P, 1), 3)
    gd = _placed(g[:P, :n_out], n_out + 3) if g is not None else None
    rc = lib.recmv_mlp_vjp_input(N.ref(), _p(x), P, n_out, _p(gd), n_out + 3 if g is not None else 0, _p(gx), _p(ws),
                                 lib.recmv_mlp_workspace_bytes(N.ref(), P, 1), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.recmv_last_error()
    _guards_ok(gx)
    return gx


@functools.lru_cache(maxsize=None)
def _packed(name):
    _, lib = _lib()
    N = _net(name)
    n = lib.recmv_mlp_pack_bytes(N.ref())
    assert n > 0
    buf = _ws(n)
    assert lib.recmv_mlp_pack(N.ref(), _p(buf), n - 1, _stream()) == ERR_ARG          # a buffer one byte short
    assert lib.recmv_mlp_pack(N.ref(), _p(buf), n, _stream()) == 0, lib.recmv_last_error()
    torch.cuda.synchronize()
    return buf


def _rows_forward(name, dev, P, n_out, keep, use_idx=True, ldo=None, rows=slice(None)):
    _, lib = _lib()
    N = _net(name)
    ldo = n_out if ldo is None else ldo
    need = lib.recmv_mlp_rows_workspace_bytes(N.ref(), P)
    ws = _ws(need)
    out = _out(max(P, 1), ldo)
    x = dev["x"][rows][:P].contiguous()
    idx = dev["idx"][rows][:P].contiguous() if (use_idx and N.m["cond_dim"]) else None
    rc = lib.recmv_mlp_rows_forward(N.ref(), _p(_packed(name)), _p(x), _p(dev["cond"]), _ld_cond(N.m), _p(idx), P, n_out, _p(out),
                                    ldo, _p(ws) if keep else None, need if keep else 0, keep, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.recmv_last_error()
    _guards_ok(out)
    return out, ws, x


def _rows_vjp(name, x, P, n_out, g, ws):
    _, lib = _lib()
    N = _net(name)
    gx = _out(max(P, 1), 3)
    gd = _placed(g[:P, :n_out], n_out + 3) if g is not None else None
    rc = lib.recmv_mlp_rows_vjp_input(N.ref(), _p(_packed(name)), _p(x), P, n_out, _p(gd), n_out + 3 if g is not None else 0, _p(gx),
                                      _p(ws), lib.recmv_mlp_rows_workspace_bytes(N.ref(), P), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.recmv_last_error()
    _guards_ok(gx)
    return gx


@functools.lru_cache(maxsize=None)
def _eye3():
    return torch.eye(3, device=DEV).contiguous()


def _jet(N, inp, dev, P, n_j, use_gy=True, use_gt=True, want=("gW", "gb", "g_in", "gx"), null_layer=None):
    """One forward and one reverse sweep of the jet on the first P rows; outputs as device tensors (None where not asked for)."""
    _, lib = _lib()
    m = N.m
    n, last = m["n"], m["rows"][-1]
    need = lib.recmv_mlp_jet_workspace_bytes(N.ref(), P)
    ws = _ws(need)
    ldy = last + 2
    y, tang = _out(max(P, 1), ldy), _out(max(3 * P, 1), n_j)
    x = dev["x"][:P].contiguous()
    idx = dev["idx"][:P].contiguous() if m["cond_dim"] else None
    rc = lib.recmv_mlp_jet_forward(N.ref(), _p(x), _p(dev["cond"]), _ld_cond(m), _p(idx), _p(_eye3()), P, n_j, _p(y), ldy, _p(tang),
                                   _p(ws), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.recmv_last_error()
    gy = _placed(inp["gy"][:P], last + 3) if use_gy else None
    gt = torch.cat([inp["gt"][k * PMAX:k * PMAX + P, :n_j] for k in range(3)]).contiguous().to(DEV) if use_gt else None
    ld_in = (m["dims"][0] + 3) // 4 * 4
    gW = [_out(m["rows"][l], m["dims"][l]) if ("gW" in want and l != null_layer) else None for l in range(n)]
    gb = [_out(m["rows"][l]) if ("gb" in want and l != null_layer) else None for l in range(n)]
    g_in = _out(max(4 * P, 1), ld_in) if "g_in" in want else None
    gx = _out(max(P, 1), 3) if "gx" in want else None
    pW = (C.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in gW])
    pb = (C.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in gb])
    rc = lib.recmv_mlp_jet_backward(N.ref(), _p(x), _p(_eye3()), P, n_j, _p(gy), last + 3 if use_gy else 0, _p(gt),
                                    C.cast(pW, C.c_void_p), C.cast(pb, C.c_void_p), _p(g_in), _p(gx), _p(ws), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.recmv_last_error()
    _guards_ok(y, tang, *[t for t in gW + gb + [g_in, gx] if t is not None])
    return {"y": y, "tang": tang, "gW": gW, "gb": gb, "g_in": g_in, "gx": gx, "ldy": ldy, "ld_in": ld_in}


def _jet_gt(inp, P, n_j):
    return torch.cat([inp["gt"][k * PMAX:k * PMAX + P, :n_j] for k in range(3)]).contiguous()


@functools.lru_cache(maxsize=None)
def _ref_jet(name, P, n_j, use_gy, use_gt):
    m = M.net(name)
    inp, _ = _inputs(name)
    x, idx = inp["x"][:P], inp["idx"][:P]
    return M.jet_backward(m, x, inp["cond"], idx, n_j, inp["gy"][:P] if use_gy else None, _jet_gt(inp, P, n_j) if use_gt else None), \
        M.jet_forward(m, x, inp["cond"], idx, n_j)


class _mode:
    """A process-global switch of the library set for a block and put back behind it."""

    def __init__(self, setter, value, restore):
        self.setter, self.value, self.restore = setter, value, restore

    def __enter__(self):
        self.prev = self.setter(self.value)

    def __exit__(self, *exc):
        self.setter(self.prev if self.restore is None else self.restore)
        return False


def _gemm_mode(v):
    _, lib = _lib()
    return _mode(lib.recmv_set_gemm_mode, v, None)


def _rows_tile(v):
    _, lib = _lib()
    return _mode(lib.recmv_set_mlp_rows_tile, v, 0)


def _jet_fill(v):
    _, lib = _lib()
    return _mode(lib.recmv_set_jet_fill, v, None)


# ------------------------------------------------------------------------------------------------------- activation sweeps
@pytest.mark.parametrize("act", ["softplus", "tanh"])
@pytest.mark.parametrize("family", M.FAMILIES)
def test_activation_sweep(family, act):
    """out = act(x_0), gx_0 = act'(.) (jet: tang = phi', gx under a one-hot gtang = phi'') on the one-unit net, every other step exact;
    judged with the bound built from the per-function allowances and the formula's roundings."""
    name = "unit_" + act
    m, N = M.net(name), _net(name)
    x = M.sweep_x()
    P = x.shape[0]
    dev = {"x": x.to(DEV), "idx": None, "cond": None}
    z = M.E(x[:, :1].double())
    # beyond beta z = 20 softplus returns z itself and the bound IS that step (a ratio of 1 by construction): the samples below it are
    # reported on their own as well
    le20 = (x[:, 0].double() * m["p"] <= 20.0) if act == "softplus" else torch.ones(x.shape[0], dtype=torch.bool)

    def u(got, ref):       # the largest relative error in units of u, over the samples whose exact value is a normal float32
        rel = (got.cpu().double() - ref.v).abs() / (M.U * ref.v.abs().clamp_min(1e-300))
        return float(rel[ref.v.abs() > 2.0 ** -100].max())

    if family == "jet":
        inp = {"gy": torch.zeros(PMAX, 1), "gt": None}
        _, lib = _lib()
        need = lib.recmv_mlp_jet_workspace_bytes(N.ref(), P)
        ws = _ws(need)
        y, tang, gx = _out(P, 1), _out(3 * P, 1), _out(P, 3)
        gt = torch.zeros(3 * P, 1, device=DEV)
        gt[:P] = 1.0
        assert lib.recmv_mlp_jet_forward(N.ref(), _p(dev["x"]), None, 0, None, _p(_eye3()), P, 1, _p(y), 1, _p(tang), _p(ws), need,
                                         _stream()) == 0
        pn = (C.c_void_p * 2)(None, None)
        assert lib.recmv_mlp_jet_backward(N.ref(), _p(dev["x"]), _p(_eye3()), P, 1, None, 0, _p(gt), C.cast(pn, C.c_void_p),
                                          C.cast(pn, C.c_void_p), None, _p(gx), _p(ws), need, _stream()) == 0
        torch.cuda.synchronize()
        _guards_ok(y, tang, gx)
        f, d1, d2 = M.act_jet(z, m["act"], m["p"])
        print("largest error in u (%s, jet): phi %.3g  phi' %.3g  phi'' (absolute, in u beta) %.3g" % (
            act, u(y, f), u(tang[:P], d1), float((gx[:, :1].cpu().double() - d2.v).abs().max() / (M.U * max(m["p"], 1.0)))))
        _report("sweep %s jet" % act, phi=_ratio(y, f), d1=_ratio(tang[:P], d1), d2=_ratio(gx[:, :1], d2),
                phi_le20=_ratio(y, f, ok=le20), d1_le20=_ratio(tang[:P], d1, ok=le20), d2_le20=_ratio(gx[:, :1], d2, ok=le20))
        assert bool((tang[P:] == 0).all()) and bool((gx[:, 1:] == 0).all())
        return
    if family == "chain":
        out, ws, xd = _chain_forward(N, dev, P, 1, 1)
        gx = _chain_vjp(N, xd, P, 1, None, ws)
    else:
        out, ws, xd = _rows_forward(name, dev, P, 1, 1)
        gx = _rows_vjp(name, xd, P, 1, None, ws)
    f = M.act_forward(z, m["act"], m["p"], family)
    # act' is judged as a function of the kernel's own y.  (n = 2: no product is fused, the chain takes recmv_act_grad_2d)
    d = M.act_grad_y(M.E(out.cpu().double()), m["act"], m["p"], "hw" if family == "rows" else "expm1")
    print("largest error in u (%s, %s): act %.3g  act' through y %.3g" % (act, family, u(out, f), u(gx[:, :1], d)))
    _report("sweep %s %s" % (act, family), act=_ratio(out, f), dact=_ratio(gx[:, :1], d), act_le20=_ratio(out, f, ok=le20))
    assert bool((gx[:, 1:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ chain
CHAIN_CASES = [("one", 3, False), ("offset", 3, False), ("sdf", 1, True), ("sdf", 7, False), ("sdf", 1, False), ("skip_last", 2, False),
               ("skip_last", 1, True), ("skip_first", 1, True), ("deep", 8, False), ("deep", 1, True), ("wide", 16, False),
               ("bands16", 2, False), ("last528", 528, False), ("last528", 1, True)]
CHAIN_P = (0, 1, 255, 256, 257)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,n_out,null", CHAIN_CASES)
def test_chain_vs_float64(name, n_out, null, mode):
    N, m = _net(name), M.net(name)
    inp, dev = _inputs(name)
    worst = {"out": 0.0, "gx": 0.0}
    with _gemm_mode(mode):
        for P in ((0, 33) if name == "wide" else CHAIN_P):
            for use_idx in ((True, False) if m["cond_dim"] and P == 257 else (True,)):
                ref, rv = _ref_fwd(name, "chain", n_out, use_idx), _ref_vjp(name, "chain", n_out, null, use_idx)
                out1, ws, x = _chain_forward(N, dev, P, n_out, 1, use_idx, ldo=n_out + 2)
                out0, _, _ = _chain_forward(N, dev, P, n_out, 0, use_idx)
                if P == 0:
                    assert bool(torch.isnan(out1).all()) and bool(torch.isnan(out0).all()), "P = 0 must touch nothing"
                    gx = _chain_vjp(N, x, 0, n_out, None if null else inp["gy"], ws)
                    assert bool(torch.isnan(gx).all())
                    continue
                assert bool(torch.isnan(out1[:, n_out:]).all()), "wrote between the rows of its output"
                assert _same_bits(out1[:, :n_out], out0), "keep 0 and keep 1 differ"
                worst["out"] = max(worst["out"], _ratio(out0, ref["out"], P, ref["ok"]))
                if m["n"] == 1 and null:
                    continue
                gx = _chain_vjp(N, x, P, n_out, None if null else inp["gy"], ws)
                worst["gx"] = max(worst["gx"], _ratio(gx, rv["gx"], P, rv["ok"]))
    _report("chain %s n_out %d %s mode %d" % (name, n_out, "NULL" if null else "g", mode), **worst)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("null", [True, False])
@pytest.mark.parametrize("P", [128, 133, 256])
def test_chain_two_nets(P, null, mode):
    """Rows >= split_row = 128 through the second weight set; split_row >= P behaves as one net."""
    name, n_out = "two", 1 if null else 7
    N = _net(name)
    ref, rv = _ref_fwd(name, "chain", n_out, True, P), _ref_vjp(name, "chain", n_out, null, True, P)
    inpP, devP = _inputs(name, P)
    with _gemm_mode(mode):
        out, ws, x = _chain_forward(N, devP, P, n_out, 1)
        out0, _, _ = _chain_forward(N, devP, P, n_out, 0)
        gx = _chain_vjp(N, x, P, n_out, None if null else inpP["gy"], ws)
    assert _same_bits(out, out0)
    _report("chain two P %d %s mode %d" % (P, "NULL" if null else "g", mode), out=_ratio(out, ref["out"]), gx=_ratio(gx, rv["gx"]))
    if P == 128:      # one net: the same bits as the first net alone
        one = _net("sdf")
        with _gemm_mode(mode):
            o1, _, _ = _chain_forward(one, devP, P, n_out, 0)
        assert _same_bits(out, o1)


# --------------------------------------------------------------------------------------------------------------- row tile
ROWS_CASES = [("offset", 3, False), ("sdf", 1, True), ("sdf", 7, False), ("skip_last", 2, False), ("skip_last", 1, True),
              ("skip_first", 1, True), ("skip_first", 1, False), ("deep", 8, False), ("wide", 16, False), ("wide", 1, True)]
ROWS_P = (0, 1, 15, 16, 17, 31, 32, 33, 257)


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("name,n_out,null", ROWS_CASES)
def test_rows_vs_float64(name, n_out, null, tile):
    m = M.net(name)
    inp, dev = _inputs(name)
    worst = {"out": 0.0, "gx": 0.0}
    with _rows_tile(tile):
        for P in ((0, 33) if name == "wide" else ROWS_P):
            for use_idx in ((True, False) if m["cond_dim"] and P == 257 else (True,)):
                ref, rv = _ref_fwd(name, "rows", n_out, use_idx), _ref_vjp(name, "rows", n_out, null, use_idx)
                out1, ws, x = _rows_forward(name, dev, P, n_out, 1, use_idx, ldo=n_out + 2)
                out0, _, _ = _rows_forward(name, dev, P, n_out, 0, use_idx)
                if P == 0:
                    assert bool(torch.isnan(out1).all()) and bool(torch.isnan(out0).all()), "P = 0 must touch nothing"
                    continue
                assert bool(torch.isnan(out1[:, n_out:]).all()), "wrote between the rows of its output"
                assert _same_bits(out1[:, :n_out], out0), "keep 0 and keep 1 differ"
                gx = _rows_vjp(name, x, P, n_out, None if null else inp["gy"], ws)
                worst["out"] = max(worst["out"], _ratio(out0, ref["out"], P, ref["ok"]))
                worst["gx"] = max(worst["gx"], _ratio(gx, rv["gx"], P, rv["ok"]))
                if P == 33:      # a ray's bits do not depend on its tile: the same rows shifted by 5
                    o5, w5, x5 = _rows_forward(name, dev, P - 5, n_out, 1, use_idx, rows=slice(5, None))
                    g5 = _rows_vjp(name, x5, P - 5, n_out, None if null else inp["gy"][5:], w5)
                    assert _same_bits(o5, out0[5:]) and _same_bits(g5, gx[5:]), "a ray's result depends on the tile it sits in"
    _report("rows %s n_out %d %s tile %d" % (name, n_out, "NULL" if null else "g", tile), **worst)


@pytest.mark.parametrize("P", [4096, 4097])
def test_rows_tile_by_row_count(P):
    """The default picks 16-row tiles up to 4 096 rows and 32-row tiles above."""
    name = "offset"
    inp, dev = _inputs(name, P)
    ref, rv = _ref_fwd(name, "rows", 3, True, P), _ref_vjp(name, "rows", 3, False, True, P)
    out, ws, x = _rows_forward(name, dev, P, 3, 1)
    gx = _rows_vjp(name, x, P, 3, inp["gy"], ws)
    _report("rows offset P %d" % P, out=_ratio(out, ref["out"], P, ref["ok"]), gx=_ratio(gx, rv["gx"], P, rv["ok"]))
    assert int((~ref["ok"]).sum()) <= 0.01 * P


def test_rows_supported_follows_the_header():
    _, lib = _lib()
    for name in M.NETS:
        assert lib.recmv_mlp_rows_supported(_net(name).ref()) == M.rows_supported(M.net(name)), name


def test_rows_refuses_a_last_layer_wider_than_512():
    """528 rows in the last layer: the reverse pass would stage 33 chunks into an LDS row of 520 floats.  Unsupported; the chain
    serves such a net (test_chain_vs_float64[last528-...])."""
    _, lib = _lib()
    N = _net("last528")
    _, dev = _inputs("last528")
    assert lib.recmv_mlp_rows_supported(N.ref()) == 0
    assert lib.recmv_mlp_pack_bytes(N.ref()) == 0
    assert lib.recmv_mlp_rows_workspace_bytes(N.ref(), 33) == 0
    buf, out, gx = _ws(1 << 20), _out(33, 1), _out(33, 3)
    assert lib.recmv_mlp_pack(N.ref(), _p(buf), buf.numel(), _stream()) == ERR_ARG
    assert lib.recmv_mlp_rows_forward(N.ref(), _p(buf), _p(dev["x"]), None, 0, None, 33, 1, _p(out), 1, _p(buf), buf.numel(), 1,
                                      _stream()) == ERR_ARG
    assert lib.recmv_mlp_rows_vjp_input(N.ref(), _p(buf), _p(dev["x"]), 33, 1, None, 0, _p(gx), _p(buf), buf.numel(), _stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(gx).all())


# -------------------------------------------------------------------------------------------------------------------- jet
JET_NETS = ("one", "offset", "sdf", "skip_last", "skip_first", "deep", "bands16")
JET_P = (0, 1, 63, 64, 65, 257)


def _judge_jet(name, got, P, n_j, use_gy, use_gt, want=("gW", "gb", "g_in", "gx"), null_layer=None):
    m = M.net(name)
    bw, fw = _ref_jet(name, P, n_j, use_gy, use_gt)
    ok, last = bw["ok"], m["rows"][-1]
    assert bool(torch.isnan(got["y"][:, last:]).all())
    r = {"y": _ratio(got["y"][:, :last], fw["y"], ok=ok), "tang": _ratio(got["tang"], fw["tang"], ok=ok.repeat(3))}
    if "gx" in want:
        r["gx"] = _ratio(got["gx"], bw["gx"], ok=ok)
    if "g_in" in want:
        d0 = m["dims"][0]
        assert bool(torch.isnan(got["g_in"][:, d0:]).all())
        r["g_in"] = _ratio(got["g_in"][:, :d0], bw["g_in"], ok=ok.repeat(4))        # the code columns are judged per point
    if bool(ok.all()):        # the parameter gradients sum over every row
        for l in range(m["n"]):
            if "gW" in want and l != null_layer:
                r["gW%d" % l] = _ratio(got["gW"][l], bw["gW"][l])
            if "gb" in want and l != null_layer:
                r["gb%d" % l] = _ratio(got["gb"][l], bw["gb"][l])
    return r


@pytest.mark.parametrize("name", JET_NETS + ("wide",))
def test_jet_vs_float64(name):
    N, m = _net(name), M.net(name)
    inp, dev = _inputs(name)
    last = m["rows"][-1]
    worst = {}
    # (wide at P = 1: the last layer's [16, 512] product gtang^T T is larger than a cotangent block of 4 rows)
    for P in ((0, 1, 33) if name == "wide" else JET_P):
        for n_j in sorted({1, last}):
            if P != 65 and n_j != last:
                continue
            if P == 0:
                got = _jet(N, inp, dev, 0, n_j)
                assert all(bool(torch.isnan(t).all()) for t in [got["y"], got["tang"], got["g_in"], got["gx"]] + got["gW"] + got["gb"])
                continue
            for use_gy, use_gt in (((True, True), (True, False), (False, True)) if P in (33, 65) else ((True, True),)):
                got = _jet(N, inp, dev, P, n_j, use_gy, use_gt)
                with _jet_fill(0):
                    alt = _jet(N, inp, dev, P, n_j, use_gy, use_gt)
                for k in ("y", "tang", "g_in", "gx"):
                    assert _same_bits(got[k], alt[k]), "the two fill modes differ in " + k
                for k, v in _judge_jet(name, got, P, n_j, use_gy, use_gt).items():
                    worst[k] = max(worst.get(k, 0.0), v)
    _report("jet %s" % name, **worst)


@pytest.mark.parametrize("name", ["sdf", "offset"])
def test_jet_null_outputs(name):
    """Each of gW[l], gb[l], g_in and gx NULL in turn: the others are still right."""
    N, m = _net(name), M.net(name)
    inp, dev = _inputs(name)
    P, n_j = 65, m["rows"][-1]
    worst = {}
    variants = [(("gb", "g_in", "gx"), None), (("gW", "g_in", "gx"), None), (("gW", "gb", "gx"), None), (("gW", "gb", "g_in"), None),
                (("gW", "gb"), None)] + [(("gW", "gb", "g_in", "gx"), l) for l in range(m["n"])]
    for want, null_layer in variants:
        got = _jet(N, inp, dev, P, n_j, want=want, null_layer=null_layer)
        for k, v in _judge_jet(name, got, P, n_j, True, True, want, null_layer).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _report("jet %s with NULL outputs" % name, **worst)


# ------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("P", [1, 33, 257])
@pytest.mark.parametrize("name", ["int_offset", "int_plain"])
def test_integer_inputs_are_exact_in_every_family(name, P):
    """Integer inputs, weights and cotangents: every partial sum is an integer below 2^24, so the result does not depend on the
    summation order and one dropped, doubled or misplaced column, row or code index changes it."""
    N, m = _net(name), M.net(name)
    inp, dev = _inputs(name, P, True)
    last = m["rows"][-1]
    x, cond, idx = inp["x"], inp["cond"], inp["idx"]
    assert M.int_peak(m, x, cond, idx, inp["gy"], inp["gt"]) < 2 ** 24
    want_out = M.forward(m, x, cond, idx, last)["out"].v.float()
    want_gx = M.vjp(m, x, cond, idx, last, inp["gy"])["gx"].v.float()
    for mode in (0, 1):
        with _gemm_mode(mode):
            out, ws, xd = _chain_forward(N, dev, P, last, 1)
            gx = _chain_vjp(N, xd, P, last, inp["gy"], ws)
        assert torch.equal(out.cpu(), want_out) and torch.equal(gx.cpu(), want_gx), "chain, mode %d" % mode
    for tile in (1, 2):
        with _rows_tile(tile):
            out, ws, xd = _rows_forward(name, dev, P, last, 1)
            gx = _rows_vjp(name, xd, P, last, inp["gy"], ws)
        assert torch.equal(out.cpu(), want_out) and torch.equal(gx.cpu(), want_gx), "rows, tile %d" % tile
    gt = inp["gt"]
    bw = M.jet_backward(m, x, cond, idx, last, inp["gy"], gt)
    fw = M.jet_forward(m, x, cond, idx, last)
    # (_jet cuts the tangent cotangent out of PMAX-row blocks: lay this case's rows out that way)
    blocks = torch.zeros(3 * PMAX, last)
    for k in range(3):
        blocks[k * PMAX:k * PMAX + P] = gt[k * P:(k + 1) * P]
    got = _jet(N, {"gy": inp["gy"], "gt": blocks}, dev, P, last)
    assert torch.equal(got["y"][:, :last].cpu(), fw["y"].v.float()) and torch.equal(got["tang"].cpu(), fw["tang"].v.float())
    assert torch.equal(got["gx"].cpu(), bw["gx"].v.float())
    assert torch.equal(got["g_in"][:, :m["dims"][0]].cpu(), bw["g_in"].v.float())
    for l in range(m["n"]):
        assert torch.equal(got["gW"][l].cpu(), bw["gW"][l].v.float()), "gW[%d]" % l
        assert torch.equal(got["gb"][l].cpu(), bw["gb"][l].v.float()), "gb[%d]" % l


# -------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_return_without_a_launch():
    _, lib = _lib()
    s = _stream()
    P = 33
    sdf, off, two = _net("sdf"), _net("offset"), _net("two")
    _, dsdf = _inputs("sdf")
    inpo, doff = _inputs("offset")
    out, gx = _out(P, 8), _out(P, 3)
    g3 = _placed(inpo["gy"][:P], 3)
    x, xo = dsdf["x"][:P].contiguous(), doff["x"][:P].contiguous()
    need = lib.recmv_mlp_workspace_bytes(sdf.ref(), P, 1)
    ws = _ws(max(need, lib.recmv_mlp_jet_workspace_bytes(sdf.ref(), P), lib.recmv_mlp_workspace_bytes(off.ref(), P, 1)))

    def fwd(N, xx, cond, n_out, nbytes=None, ld_cond=0):
        return lib.recmv_mlp_forward(N.ref(), _p(xx), _p(cond), ld_cond, None, P, n_out, _p(out), 8, _p(ws),
                                     ws.numel() if nbytes is None else nbytes, 1, s)

    def vjp(N, xx, n_out, g):
        return lib.recmv_mlp_vjp_input(N.ref(), _p(xx), P, n_out, _p(g), 3 if g is not None else 0, _p(gx), _p(ws), ws.numel(), s)

    assert fwd(sdf, x, None, 1, need - 1) == ERR_WORKSPACE
    assert fwd(sdf, x, None, 0) == ERR_ARG and fwd(sdf, x, None, 8) == ERR_ARG
    assert fwd(off, xo, doff["cond"], 1, ld_cond=M.COND_LD) == ERR_ARG                    # residual nets are 3-d
    assert fwd(off, xo, None, 3) == ERR_ARG                                                # a code net without its table
    assert vjp(sdf, x, 2, None) == ERR_ARG                                                 # NULL cotangent with n_out > 1
    assert vjp(sdf, x, 0, g3) == ERR_ARG and vjp(sdf, x, 8, g3) == ERR_ARG
    assert vjp(off, xo, 1, g3) == ERR_ARG and vjp(off, xo, 1, None) == ERR_ARG             # residual without its 3-d cotangent
    two.d.split_row = 100
    try:
        assert fwd(two, x, None, 1) == ERR_ARG                                             # split_row not a multiple of 128
    finally:
        two.d.split_row = 128
    # row tile
    pk, pko = _packed("sdf"), _packed("offset")
    rneed = lib.recmv_mlp_rows_workspace_bytes(sdf.ref(), P)

    def rfwd(N, pkd, xx, cond, n_out, nbytes=None, ld_cond=0):
        return lib.recmv_mlp_rows_forward(N.ref(), _p(pkd), _p(xx), _p(cond), ld_cond, None, P, n_out, _p(out), 8, _p(ws),
                                          ws.numel() if nbytes is None else nbytes, 1, s)

    def rvjp(N, pkd, xx, n_out, g):
        return lib.recmv_mlp_rows_vjp_input(N.ref(), _p(pkd), _p(xx), P, n_out, _p(g), 3 if g is not None else 0, _p(gx), _p(ws),
                                            ws.numel(), s)

    assert rfwd(sdf, pk, x, None, 1, rneed - 1) == ERR_WORKSPACE
    assert rfwd(sdf, pk, x, None, 0) == ERR_ARG and rfwd(sdf, pk, x, None, 8) == ERR_ARG
    assert rfwd(off, pko, xo, doff["cond"], 1, ld_cond=M.COND_LD) == ERR_ARG
    assert rfwd(off, pko, xo, None, 3) == ERR_ARG
    assert rvjp(sdf, pk, x, 2, None) == ERR_ARG and rvjp(off, pko, xo, 1, g3) == ERR_ARG and rvjp(off, pko, xo, 3, None) == ERR_ARG
    assert lib.recmv_mlp_pack_bytes(two.ref()) == 0 and lib.recmv_mlp_rows_supported(two.ref()) == 0
    # jet
    jneed = lib.recmv_mlp_jet_workspace_bytes(sdf.ref(), P)
    tang = _out(3 * P, 8)

    def jfwd(N, xx, cond, n_j, nbytes, ld_cond=0):
        return lib.recmv_mlp_jet_forward(N.ref(), _p(xx), _p(cond), ld_cond, None, _p(_eye3()), P, n_j, _p(out), 8, _p(tang), _p(ws),
                                         nbytes, s)

    assert jfwd(sdf, x, None, 1, jneed - 1) == ERR_WORKSPACE
    assert jfwd(sdf, x, None, 0, jneed) == ERR_ARG and jfwd(sdf, x, None, 8, jneed) == ERR_ARG
    assert jfwd(off, xo, None, 3, ws.numel()) == ERR_ARG
    pn = (C.c_void_p * 4)(None, None, None, None)
    assert lib.recmv_mlp_jet_backward(sdf.ref(), _p(x), _p(_eye3()), P, 1, None, 0, None, C.cast(pn, C.c_void_p), C.cast(pn, C.c_void_p),
                                      None, _p(gx), _p(ws), jneed - 1, s) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(gx).all()) and bool(torch.isnan(tang).all()), "an error path launched"
    _guards_ok(out, gx, tang)
