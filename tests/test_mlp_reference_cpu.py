"""CPU checks of tests/mlp_reference.py: the float64 references of the whole-MLP passes against float64 autograd of a plain torch
composition, the conditions the bounds rely on, and the bounds themselves against a separate float32 emulation of every family
(which must sit well inside them) and against that emulation with one mistake planted (which must leave them by a wide margin).
"""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mlp_reference as M  # noqa: E402

FLOAT_NETS = ("one", "offset", "sdf", "skip_last", "skip_first", "deep", "bands16", "wide")
P_CPU = 9


# ------------------------------------------------------------------------------------------- a plain torch composition, float64
def _t_act(z, m):
    if m["act"] == M.ACT_RELU:
        return F.relu(z)
    if m["act"] == M.ACT_SOFTPLUS:
        return F.softplus(z, beta=m["p"], threshold=1e30)
    if m["act"] == M.ACT_TANH:
        return torch.tanh(z)
    return z


def _t_gamma(m, x):
    cols = [x]
    for b in range(m["L"]):
        cols += [m["pe_w"][2 * b] * torch.sin(x * 2.0 ** b), m["pe_w"][2 * b + 1] * torch.cos(x * 2.0 ** b)]
    return torch.cat(cols, -1)


def _t_tail(m, h0, gam, W, b, n_out):
    """The layers behind the input h0 = [gamma | code]."""
    h = h0
    n = m["n"]
    for l in range(n - 1):
        h = _t_act(F.linear(h, W[l], b[l]), m)
        if l + 1 == m["skip"]:
            h = torch.cat([h, gam], -1) / math.sqrt(2.0)
    return F.linear(h, W[n - 1][:n_out], None if b[n - 1] is None else b[n - 1][:n_out])


def _t_params(m):
    W = [w.double().clone().requires_grad_(True) for w in m["W"]]
    b = [None if v is None else v.double().clone().requires_grad_(True) for v in m["b"]]
    return W, b


def _t_net(m, x, c, W, b, n_out):
    gam = _t_gamma(m, x)
    h0 = torch.cat([gam, c], -1) if m["cond_dim"] else gam
    out = _t_tail(m, h0, gam, W, b, n_out)
    return out + x if m["residual"] else out


def _code(m, inp, use_idx=True):
    if not m["cond_dim"]:
        return None
    P = inp["x"].shape[0]
    return inp["cond"].double()[inp["idx"]] if use_idx else inp["cond"].double()[:1].expand(P, -1)


def _close(ref, want, what):
    scale = max(float(want.abs().max()), 1e-30)
    err = float((ref - want).abs().max())
    assert err <= 1e-12 * scale, "%s: %.3g of %.3g" % (what, err, scale)


def _cases():
    out = []
    for name in FLOAT_NETS:
        m = M.net(name)
        outs = sorted({1, m["rows"][-1]}) if not m["residual"] else [3]
        for n_out in outs:
            out.append((name, n_out))
    return out


@pytest.mark.parametrize("name,n_out", _cases())
def test_forward_and_vjp_equal_autograd(name, n_out):
    m = M.net(name)
    P = 33 if name == "wide" else P_CPU
    n_out = min(n_out, 16)
    inp = M.make_inputs(m, P)
    for use_idx in ((True, False) if m["cond_dim"] else (True,)):
        idx = inp["idx"] if use_idx else None
        W, b = _t_params(m)
        x = inp["x"].double().clone().requires_grad_(True)
        out = _t_net(m, x, _code(m, inp, use_idx), W, b, n_out)
        g = inp["gy"][:, :n_out].double()
        for fam in ("chain", "rows"):
            fw = M.forward(m, inp["x"], inp["cond"], idx, n_out, fam)
            _close(fw["out"].v, out.detach(), "out")
            gx, = torch.autograd.grad(out, x, g, retain_graph=True)
            _close(M.vjp(m, inp["x"], inp["cond"], idx, n_out, inp["gy"][:, :n_out], fam)["gx"].v, gx, "gx")
            if n_out == 1:
                gx1, = torch.autograd.grad(out[:, 0].sum(), x, retain_graph=True)
                _close(M.vjp(m, inp["x"], inp["cond"], idx, 1, None, fam)["gx"].v, gx1, "gx (NULL cotangent)")


@pytest.mark.parametrize("P", [128, 133])
def test_two_nets_equal_autograd(P):
    m = M.net("two")
    inp = M.make_inputs(m, P)
    s = 128 if P > 128 else 0
    parts = []
    gparts = []
    for k, (a, e) in enumerate(((0, s), (s, P)) if s else ((0, P),)):
        mm = M.second_of(m) if (k and s) else m
        W, b = _t_params(mm)
        x = inp["x"][a:e].double().clone().requires_grad_(True)
        out = _t_net(mm, x, None, W, b, 7)
        parts.append(out.detach())
        gparts.append(torch.autograd.grad(out, x, inp["gy"][a:e].double())[0])
    _close(M.forward(m, inp["x"], n_out=7)["out"].v, torch.cat(parts), "out")
    _close(M.vjp(m, inp["x"], n_out=7, g_out=inp["gy"])["gx"].v, torch.cat(gparts), "gx")


@pytest.mark.parametrize("name", [n for n in FLOAT_NETS if n != "wide"])
@pytest.mark.parametrize("full", [True, False])
def test_jet_equals_autograd(name, full):
    m = M.net(name)
    P, last = P_CPU, m["rows"][-1]
    n_j = last if full else 1
    inp = M.make_inputs(m, P)
    gy, gt = inp["gy"], inp["gt"][:, :n_j].contiguous()
    W, b = _t_params(m)
    x = inp["x"].double().clone().requires_grad_(True)
    c = _code(m, inp)
    y = _t_net(m, x, c, W, b, last)
    mlp = y - x if m["residual"] else y
    cols = [torch.autograd.grad(mlp[:, j].sum(), x, create_graph=True)[0] for j in range(n_j)]       # [P,3] each
    tang = torch.stack(cols, -1).permute(1, 0, 2).reshape(3 * P, n_j)                                # [k*P + p, j]
    fw = M.jet_forward(m, inp["x"], inp["cond"], inp["idx"], n_j)
    _close(fw["y"].v, y.detach(), "y")
    _close(fw["tang"].v, tang.detach(), "tang")
    for use_gy, use_gt in ((True, False), (False, True), (True, True)):
        loss = (y * gy.double()).sum() * float(use_gy) + (tang * gt.double()).sum() * float(use_gt)
        leaves = [x] + W + [v for v in b if v is not None]
        grads = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
        grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
        bw = M.jet_backward(m, inp["x"], inp["cond"], inp["idx"], n_j, gy if use_gy else None, gt if use_gt else None)
        _close(bw["gx"].v, grads[0], "gx")
        for l in range(m["n"]):
            _close(bw["gW"][l].v, grads[1 + l], "gW[%d]" % l)
        gbs = iter(grads[1 + m["n"]:])
        for l in range(m["n"]):
            if m["b"][l] is not None:
                _close(bw["gb"][l].v, next(gbs), "gb[%d]" % l)
        # g_in: the cotangent of the stacked layer-0 input, by torch's forward mode over the layers behind the input
        gam = _t_gamma(m, x).detach()
        h0 = (torch.cat([gam, c], -1) if m["cond_dim"] else gam).clone().requires_grad_(True)
        eye = torch.eye(3, dtype=torch.float64)
        tans = [torch.cat([M.R.posenc_jvp(inp["x"], eye[k:k + 1], m["L"], m["pe_w"] if m["L"] else None).v,
                           torch.zeros(P, m["cond_dim"], dtype=torch.float64)], -1).requires_grad_(True) for k in range(3)]
        d_pe = 3 + 6 * m["L"]
        Wd, bd = [w.detach() for w in W], [None if v is None else v.detach() for v in b]
        f = lambda h: _t_tail(m, h, h[:, :d_pe], Wd, bd, last)
        loss = 0.0
        for k in range(3):
            yk, sk = torch.func.jvp(f, (h0,), (tans[k],))
            loss = loss + (sk[:, :n_j] * gt[k * P:(k + 1) * P].double()).sum() * float(use_gt)
        loss = loss + (yk * gy.double()).sum() * float(use_gy)
        gin = torch.autograd.grad(loss, [h0] + tans, allow_unused=True)
        gin = torch.cat([torch.zeros(P, m["dims"][0], dtype=torch.float64) if g is None else g for g in gin], 0)
        _close(bw["g_in"].v, gin, "g_in")


# ------------------------------------------------------------------------------------------------ conditions of the bounds
@pytest.mark.parametrize("name", ["offset", "skip_first"])
@pytest.mark.parametrize("P", [1, 17, 33, 257])
def test_relu_rows_left_out_stay_below_one_percent(name, P):
    m = M.net(name)
    inp = M.make_inputs(m, P)
    for fam in ("chain", "rows"):
        ok = M.forward(m, inp["x"], inp["cond"], inp["idx"], None, fam)["ok"]
        assert int((~ok).sum()) <= 0.01 * P
    assert int((~M.jet_forward(m, inp["x"], inp["cond"], inp["idx"])["ok"]).sum()) <= 0.01 * P


@pytest.mark.parametrize("name", ["int_offset", "int_plain"])
@pytest.mark.parametrize("P", [1, 33, 257])
def test_integer_cases_are_exact(name, P):
    m = M.net(name)
    inp = M.make_inputs(m, P, integer=True)
    peak = M.int_peak(m, inp["x"], inp["cond"], inp["idx"], inp["gy"], inp["gt"])
    assert peak < 2 ** 24, peak
    bw = M.jet_backward(m, inp["x"], inp["cond"], inp["idx"], None, inp["gy"], inp["gt"])
    for t in [bw["gx"].v, bw["g_in"].v] + [w.v for w in bw["gW"]]:
        assert torch.equal(t, t.round())
    assert float(bw["gW"][0].v.abs().max()) > 0 and float(bw["gx"].v.abs().max()) > 0


def test_no_subnormal_intermediates():
    for name in FLOAT_NETS:
        if name == "wide":
            continue
        m = M.net(name)
        inp = M.make_inputs(m, P_CPU)
        fw = M.forward(m, inp["x"], inp["cond"], inp["idx"])
        for t in fw["z"] + [fw["out"]]:
            nz = t.v[t.v != 0].abs()
            assert float(nz.min()) > 2.0 ** -126 * 2 ** 24, name
        if m["act"] == M.ACT_SOFTPLUS:           # the one place that underflows carries its term
            assert all(float(y.e[:, :r].min()) >= 8 * 2.0 ** -126 * m["p"] for y, r in zip(fw["y"], m["rows"]))     # (16, times 1/sqrt2 behind a skip)


def test_rows_supported_rule():
    want = {"one": 0, "offset": 1, "sdf": 1, "skip_last": 1, "skip_first": 1, "deep": 1, "wide": 1, "bands16": 0, "two": 0, "last528": 0}
    assert {k: M.rows_supported(M.net(k)) for k in want} == want


# ---------------------------------------------------------------------------------------------------- float32 emulation
F32 = torch.float32
LOG2E, LN2, INV, SQ2 = (torch.tensor(v, dtype=F32) for v in (1.4426950408889634, 0.69314718, 0.70710678118654752440, 1.41421356237309504880))


def _e_gamma(m, x, mut):
    w = list(m["pe_w"])
    if mut == "band_weight" and m["L"] >= 2:
        w = w[:2] + w[:-2]
    cols = [x]
    for b in range(m["L"]):
        s, c = torch.sin(x * float(2 ** b)), torch.cos(x * float(2 ** b))
        if mut == "sincos_swap" and b == m["L"] - 1:
            s, c = c, s
        cols += [np.float32(w[2 * b]) * s, np.float32(w[2 * b + 1]) * c]
    return torch.cat(cols, -1)


def _e_softplus_hw(z, p, c3=0.33333334):
    zb = z * p
    t = torch.exp2(-zb.abs() * LOG2E)
    series = t * (1 - t * (0.5 - t * (np.float32(c3) - 0.25 * t)))
    l = torch.where(t < 0.015625, series, torch.log2(1 + t) * LN2)
    y = (zb.clamp_min(0) + l) * (np.float32(1) / np.float32(p))
    return torch.where(zb > 20, z, y)


def _e_act(z, m, fam):
    if m["act"] == M.ACT_RELU:
        return z.clamp_min(0)
    if m["act"] == M.ACT_TANH:
        return torch.tanh(z)
    if m["act"] == M.ACT_SOFTPLUS:
        if fam == "jet":
            zb = z * m["p"]
            return torch.where(zb > 20, z, (zb.clamp_min(0) + torch.log1p(torch.exp(-zb.abs()))) / m["p"])
        return _e_softplus_hw(z, m["p"])
    return z


def _e_dact(y, m, form, c6=0.16666667):
    if m["act"] == M.ACT_RELU:
        return (y > 0).to(F32)
    if m["act"] == M.ACT_TANH:
        return 1 - y * y
    if m["act"] == M.ACT_SOFTPLUS:
        t = y * m["p"]
        if form == "expm1":
            return -torch.expm1(-t)
        series = t * (1 - t * (0.5 - t * (np.float32(c6) - np.float32(0.041666668) * t)))
        return torch.where(t < 0.015625, series, 1 - torch.exp2(-t * LOG2E))
    return torch.ones_like(y)


def _e_input(m, x, cond, idx, mut):
    g = _e_gamma(m, x, mut)
    if not m["cond_dim"]:
        return g
    P = x.shape[0]
    i = idx if idx is not None else torch.zeros(P, dtype=torch.long)
    if mut == "cond_off":
        i = (i + 1) % cond.shape[0]
    return torch.cat([g, cond[i]], -1)


def _e_join(m, y, gam, mut):
    a = y if mut == "skip_act_unscaled" else y * INV
    g = gam if mut == "skip_enc_unscaled" else gam * INV
    return torch.cat([g, a] if mut == "skip_order" else [a, g], -1)


def emu_forward(m, x, cond, idx, n_out, fam, mut=None):
    P = x.shape[0]
    s = M._split_rows(m, P)
    if s:
        s2 = s + 1 if mut == "second_from" else s
        a = emu_forward(dict(m, W2=None), x[:s2], cond, idx, n_out, fam, mut)
        b = emu_forward(M.second_of(m), x[s2:], cond, idx, n_out, fam, mut)
        return {"out": torch.cat([a["out"], b["out"]]), "y": [torch.cat(q) for q in zip(a["y"], b["y"])]}
    n = m["n"]
    h = _e_input(m, x, cond, idx, mut)
    ys = []
    for l in range(n - 1):
        z = torch.matmul(h, m["W"][l].t())
        if m["b"][l] is not None:
            z = z + m["b"][l]
        y = _e_act(z, m, fam)
        if mut == "col25" and m["rows"][l] == 25:
            y = torch.cat([y[:, :24], torch.zeros(P, 1)], -1)
        if l + 1 == m["skip"]:
            y = _e_join(m, y, _e_gamma(m, x, mut), mut)
        ys.append(y)
        h = y
    out = torch.matmul(h, m["W"][n - 1][:n_out].t())
    if m["b"][n - 1] is not None:
        out = out + m["b"][n - 1][:n_out]
    if m["residual"]:
        out = out + x
    return {"out": out, "y": ys}


def _e_pe_vjp(m, x, g, t=None):
    acc = torch.zeros_like(x) if t is not None else g[:, :3].clone()
    for b in range(m["L"]):
        f = float(2 ** b)
        s, c = torch.sin(x * f), torch.cos(x * f)
        gs, gc = g[:, 3 + 6 * b:6 + 6 * b], g[:, 6 + 6 * b:9 + 6 * b]
        ws, wc = np.float32(m["pe_w"][2 * b]), np.float32(m["pe_w"][2 * b + 1])
        if t is None:
            acc = acc + f * (ws * c * gs - wc * s * gc)
        else:
            acc = acc - f * f * (ws * s * gs + wc * c * gc)
    return acc if t is None else acc * t


def emu_vjp(m, x, cond, idx, n_out, g_out, fam, mut=None):
    P = x.shape[0]
    s = M._split_rows(m, P)
    if s:
        s2 = s + 1 if mut == "second_from" else s
        go = lambda a, b: None if g_out is None else g_out[a:b]
        return torch.cat([emu_vjp(dict(m, W2=None), x[:s2], cond, idx, n_out, go(0, s2), fam, mut),
                          emu_vjp(M.second_of(m), x[s2:], cond, idx, n_out, go(s2, P), fam, mut)])
    n, d_pe = m["n"], 3 + 6 * m["L"]
    ys = emu_forward(m, x, cond, idx, n_out, fam, mut)["y"]
    Wl = m["W"][n - 1]
    if g_out is None:
        g = Wl[1 if (mut == "null_row1" and Wl.shape[0] > 1) else 0].unsqueeze(0).expand(P, -1)
    else:
        g = torch.matmul(g_out[:, :n_out], Wl[:n_out])
    park = None
    for l in range(n - 2, -1, -1):
        y, rl = ys[l], m["rows"][l]
        fused = fam == "chain" and l <= n - 3 and l + 1 != m["skip"]
        form = "hw" if (fam == "rows" or fused) else "expm1"
        if l + 1 == m["skip"]:
            park = g[:, rl:rl + d_pe] * INV
            ya = y[:, :rl] if mut == "dact_unscaled" else y[:, :rl] * SQ2
            dz = g[:, :rl] * _e_dact(ya, m, form) * INV
        else:
            dz = g * _e_dact(y, m, form)
        g = torch.matmul(dz, m["W"][l])
    gpe = g[:, :d_pe] if park is None else g[:, :d_pe] + park
    gx = _e_pe_vjp(m, x, gpe)
    if m["residual"] and mut != "no_residual":
        gx = gx + g_out[:, :3]
    return gx


def _e_act_jet(z, m):
    if m["act"] == M.ACT_SOFTPLUS:
        p = m["p"]
        zb = z * p
        e = torch.exp(-zb.abs())
        sig = torch.where(zb >= 0, 1 / (1 + e), e / (1 + e))
        f = (zb.clamp_min(0) + torch.log1p(e)) / p
        big = zb > 20
        return torch.where(big, z, f), torch.where(big, torch.ones_like(z), sig), torch.where(big, torch.zeros_like(z), p * sig * (1 - sig))
    if m["act"] == M.ACT_TANH:
        t = torch.tanh(z)
        d1 = 1 - t * t
        return t, d1, -2 * t * d1
    if m["act"] == M.ACT_RELU:
        return z.clamp_min(0), (z > 0).to(F32), torch.zeros_like(z)
    return z, torch.ones_like(z), torch.zeros_like(z)


def emu_jet(m, x, cond, idx, n_j, gy, gt, mut=None):
    """The jet's forward and reverse sweep in float32: y, tang, gW, gb, g_in, gx."""
    P, n, L = x.shape[0], m["n"], m["L"]
    d_pe, last = 3 + 6 * L, m["rows"][-1]
    tans = []
    for k in range(3):
        cols = [torch.zeros(P, 3)]
        cols[0][:, k] = 1
        for b in range(L):
            f = float(2 ** b)
            s, c = torch.zeros(P, 3), torch.zeros(P, 3)
            s[:, k] = np.float32(m["pe_w"][2 * b]) * f * torch.cos(x[:, k] * f)
            c[:, k] = -np.float32(m["pe_w"][2 * b + 1]) * f * torch.sin(x[:, k] * f)
            cols += [s, c]
        tans.append(torch.cat(cols + [torch.zeros(P, m["cond_dim"])], -1))
    h = torch.cat([_e_input(m, x, cond, idx, mut)] + tans, 0)
    Hs, Zs = [], []
    for l in range(n - 1):
        Hs.append(h)
        z = torch.matmul(h, m["W"][l].t())
        if m["b"][l] is not None:
            z = torch.cat([z[:P] + m["b"][l], z[P:] + (m["b"][l] if mut == "tang_bias" else 0)], 0)
        f, d1, _ = _e_act_jet(z[:P], m)
        Zs.append(z)
        y = torch.cat([f] + [d1 * z[(k + 1) * P:(k + 2) * P] for k in range(3)], 0)
        if l + 1 == m["skip"]:
            y = torch.cat([y * INV, Hs[0][:, :d_pe] * INV], -1)
        h = y
    Hs.append(h)
    Wl = m["W"][n - 1]
    y = torch.matmul(h[:P], Wl.t())
    if m["b"][n - 1] is not None:
        y = y + m["b"][n - 1]
    if m["residual"]:
        y = y + x
    tang = torch.matmul(h[P:], Wl[:n_j].t())
    gW, gb = [None] * n, [None] * n
    K = m["dims"][n - 1]
    gW[n - 1] = torch.matmul(gy.t(), h[:P]) if gy is not None else torch.zeros(last, K)
    if gt is not None:
        tmp = torch.matmul(gt.t(), h[P:])
        if mut == "gtang_all_rows":
            tmp = tmp[torch.arange(last) % n_j]
        gW[n - 1] = torch.cat([gW[n - 1][:tmp.shape[0]] + tmp, gW[n - 1][tmp.shape[0]:]], 0)
    gb[n - 1] = gy.sum(0) if gy is not None else torch.zeros(last)
    hbar = torch.cat([torch.matmul(gy, Wl) if gy is not None else torch.zeros(P, K),
                      torch.matmul(gt, Wl[:n_j]) if gt is not None else torch.zeros(3 * P, K)], 0)
    park = None
    for l in range(n - 2, -1, -1):
        rl, Z = m["rows"][l], Zs[l]
        if l + 1 == m["skip"]:
            park = hbar[:, rl:rl + d_pe] * INV
            yb = hbar[:, :rl] * INV
        else:
            yb = hbar
        _, d1, d2 = _e_act_jet(Z[:P], m)
        sb = [yb[(k + 1) * P:(k + 2) * P] for k in range(3)]
        acc = sb[0] * Z[P:2 * P] + sb[1] * Z[2 * P:3 * P] + sb[2] * Z[3 * P:]
        zbar = yb[:P] * d1 + (0 if mut == "no_d2" else d2 * acc)
        zb4 = torch.cat([zbar] + [s * d1 for s in sb], 0)
        gb[l] = zbar.sum(0)
        gW[l] = torch.matmul(zb4.t(), Hs[l])
        hbar = torch.matmul(zb4, m["W"][l])
    if park is not None:
        hbar = torch.cat([hbar[:, :d_pe] + park, hbar[:, d_pe:]], -1)
    gx = _e_pe_vjp(m, x, hbar[:P])
    eye = torch.eye(3)
    for k in range(3):
        gx = gx + _e_pe_vjp(m, x, hbar[(k + 1) * P:(k + 2) * P], eye[k:k + 1])
    if m["residual"] and gy is not None:
        gx = gx + gy[:, :3]
    return {"y": y, "tang": tang, "gW": gW, "gb": gb, "g_in": hbar[:, :m["dims"][0]], "gx": gx}


EMU_CASES = [("one", 9, 3), ("offset", 33, 3), ("sdf", 33, 1), ("sdf", 17, 7), ("skip_last", 17, 2), ("skip_first", 17, 1),
             ("deep", 17, 8), ("bands16", 9, 2), ("two", 133, 7), ("two", 133, 1)]
MUTATIONS = ("skip_enc_unscaled", "skip_act_unscaled", "skip_order", "dact_unscaled", "band_weight", "sincos_swap", "cond_off",
             "no_residual", "null_row1", "tang_bias", "no_d2", "gtang_all_rows", "col25", "second_from")


def _r(got, ref, ok=None):
    err, bound = (got.double() - ref.v).abs(), ref.e
    if ok is not None:
        err, bound = err[ok], bound[ok]
    return M.ratio(err, bound)


def _emu_ratios(mut=None):
    """Largest error / bound of the emulation per family over EMU_CASES."""
    worst = {"chain": 0.0, "rows": 0.0, "jet": 0.0}
    for name, P, n_out in EMU_CASES:
        m = M.net(name)
        inp = M.make_inputs(m, P)
        x, cond, idx = inp["x"], inp["cond"], inp["idx"]
        for fam in ("chain", "rows"):
            if fam == "rows" and not M.rows_supported(m):
                continue
            if name == "one":
                cots = [inp["gy"]]
            else:
                cots = [None] if n_out == 1 else [inp["gy"][:, :n_out].contiguous()]
            for g_out in cots:
                if m["n"] == 1 and g_out is None:
                    continue
                ref = M.forward(m, x, cond, idx, n_out, fam)
                emu = emu_forward(m, x, cond, idx, n_out, fam, mut)
                worst[fam] = max(worst[fam], _r(emu["out"], ref["out"], ref["ok"]))
                rv = M.vjp(m, x, cond, idx, n_out, g_out, fam)
                worst[fam] = max(worst[fam], _r(emu_vjp(m, x, cond, idx, n_out, g_out, fam, mut), rv["gx"], rv["ok"]))
        if name == "two":
            continue
        last = m["rows"][-1]
        n_j = min(n_out, last)
        gt = inp["gt"][:, :n_j].contiguous()
        ref = M.jet_backward(m, x, cond, idx, n_j, inp["gy"], gt)
        fw = M.jet_forward(m, x, cond, idx, n_j)
        emu = emu_jet(m, x, cond, idx, n_j, inp["gy"], gt, mut)
        ok = ref["ok"]
        ok4 = ok.repeat(4)
        rs = [_r(emu["y"], fw["y"], ok), _r(emu["tang"], fw["tang"], ok.repeat(3)), _r(emu["gx"], ref["gx"], ok),
              _r(emu["g_in"], ref["g_in"], ok4)]
        if bool(ok.all()):                     # the parameter gradients sum over every row
            rs += [_r(emu["gW"][l], ref["gW"][l]) for l in range(m["n"])] + [_r(emu["gb"][l], ref["gb"][l]) for l in range(m["n"])]
        worst["jet"] = max(worst["jet"], *rs)
    return worst


def test_emulation_sits_inside_the_bounds():
    worst = _emu_ratios()
    print("ratio emulation: " + "  ".join("%s %.3g" % kv for kv in worst.items()))
    for fam, r in worst.items():
        assert r <= 0.5, "%s: the float32 emulation reaches %.3g of its bound" % (fam, r)


@pytest.mark.parametrize("mut", MUTATIONS)
def test_planted_mistake_leaves_the_bounds(mut):
    worst = _emu_ratios(mut)
    print("ratio mutation %s: %s" % (mut, "  ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) >= 10.0, "%s goes unnoticed: %s" % (mut, worst)


# ------------------------------------------------------------------------------------------------- the activation sweeps
def _sweep_ratios(act, c3=0.33333334, c6=0.16666667):
    """The one-unit sweep of test_gpu_mlp_passes.py::test_activation_sweep on the float32 emulation of every family; the samples
    beyond the beta z = 20 step, where the bound is the step itself, are judged apart ("step")."""
    m = M.net("unit_" + act)
    z32 = M.sweep_x()[:, :1]
    z = M.E(z32.double())
    le20 = (z.v[:, 0] * m["p"] <= 20.0) if act == "softplus" else torch.ones(z32.shape[0], dtype=torch.bool)
    out = {"step": 0.0}

    def put(key, got, ref):
        out[key] = _r(got, ref, le20)
        out["step"] = max(out["step"], _r(got, ref, ~le20))
    for fam in ("chain", "rows"):
        y = _e_softplus_hw(z32, m["p"], c3) if act == "softplus" else torch.tanh(z32)
        form = "hw" if fam == "rows" else "expm1"
        put(fam + " act", y, M.act_forward(z, m["act"], m["p"], fam))
        put(fam + " act'", _e_dact(y, m, form, c6), M.act_grad_y(M.E(y.double()), m["act"], m["p"], form))
    f, d1, d2 = _e_act_jet(z32, m)
    rf, r1, r2 = M.act_jet(z, m["act"], m["p"])
    put("jet phi", f, rf)
    put("jet phi'", d1, r1)
    put("jet phi''", d2, r2)
    return out


@pytest.mark.parametrize("act", ["softplus", "tanh"])
def test_activation_sweep_of_the_emulation(act):
    worst = _sweep_ratios(act)
    print("ratio sweep emulation %s: %s" % (act, "  ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


def test_changed_series_coefficient_fails_the_sweep():
    """The sweeps are judged with bounds built from the per-function allowances and the formula's roundings, so a formula that is
    slightly off does not hide in an allowance for the activation as a whole."""
    fwd = _sweep_ratios("softplus", c3=0.25)           # the next coefficient of the series in the place of 1/3
    grad = _sweep_ratios("softplus", c6=0.125)
    print("ratio sweep with 1/3 -> 1/4: %.3g   with 1/6 -> 1/8: %.3g" % (fwd["chain act"], grad["rows act'"]))
    assert fwd["chain act"] >= 10.0 and fwd["rows act"] >= 10.0 and grad["rows act'"] >= 10.0
