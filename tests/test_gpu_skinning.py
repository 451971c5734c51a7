"""The per-point geometry front end — the five skinning entry points and the root finder's step (csrc/lbs_fused.hip), the kinematic
chain (csrc/kinematic_chain.hip), the positional encoding and its derivatives (csrc/posenc_grad.hip) — through the C ABI against the
float64 references of tests/skinning_reference.py.

Every bounded test prints `ratio name: ...` (largest error / bound) and asserts <= 1; the bounds are derived in the docstring of
skinning_reference and never fitted.  Exact outputs (integer inputs, flags, counters, copies, zero blocks, tiled repeats across the
grid-stride wrap) are compared bit for bit.  Outputs are pre-filled with NaN and guarded by sentinels on both sides; strided inputs
sit in NaN-padded buffers.
"""
import ctypes as C
import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
import skinning_reference as R  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
SENT = -7.0
GUARD = 8
ERR_ARG = -1


def _lib():
    from recmv import _lib as L
    return L, L.lib()


def _stream():
    L, _ = _lib()
    return L.stream_ptr(torch.device(DEV))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _sentinel(dtype):
    return SENT if dtype.is_floating_point else 121


def _out(*shape, dtype=torch.float32, fill=NAN):
    """An output buffer full of `fill` between two rows of sentinels."""
    n = int(np.prod(shape)) if shape else 1
    base = torch.full((n + 2 * GUARD,), _sentinel(dtype), dtype=dtype, device=DEV)
    base[GUARD:GUARD + n] = fill
    return base[GUARD:GUARD + n].view(*shape)


def _guards_ok(*views):
    for v in views:
        base = v._base
        s = _sentinel(base.dtype)
        assert bool((base[:GUARD] == s).all()) and bool((base[-GUARD:] == s).all()), "wrote outside its output"


def _placed(t, ld):
    """A device copy of the [rows, cols] float32 tensor with row stride ld >= cols; NaN everywhere else."""
    rows, cols = t.shape
    flat = torch.full((max(rows, 1) * ld + 8,), NAN, device=DEV)
    view = flat[:rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    return view


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _report(name, **ratios):
    print("ratio %s: %s" % (name, "  ".join("%s %.3g" % kv for kv in ratios.items())))
    for k, v in ratios.items():
        assert v <= 1.0, "%s: %s error / bound = %.4g" % (name, k, v)


def _ratio(got, ref, rows=None):
    """Largest |got - ref.v| / ref.e over the selected rows (dim 0)."""
    got = got.detach().cpu().double().reshape(ref.v.shape)
    err, bound = (got - ref.v).abs(), ref.e
    if rows is not None:
        err, bound = err[rows], bound[rows]
    return R.ratio(err, bound)


def _dev(t):
    return t.to(DEV).contiguous() if t is not None else None


# ------------------------------------------------------------------------------------------------------------- skinning
class _Grid:
    def __init__(self, grid):
        L, _ = _lib()
        self.vol = _dev(grid["vol"])
        self.desc = L.LbsGrid()
        self.desc.volume = self.vol.data_ptr()
        self.desc.D, self.desc.H, self.desc.W = grid["vol"].shape[:3]
        for i in range(3):
            self.desc.center[i] = float(grid["center"][i])
            self.desc.scale[i] = float(grid["scale"][i])

    def ref(self):
        return C.byref(self.desc)


@functools.lru_cache(maxsize=None)
def _case(shape, P, B):
    grid = R.make_volume(shape)
    p, fam = R.make_points(grid, P)
    frame, A, trans = R.make_frames(P, B)
    g = torch.Generator().manual_seed(P * 131 + B)
    c = {"grid": grid, "p": p, "fam": fam, "frame": frame, "A": A, "trans": trans, "B": B, "P": P,
         "g_d": torch.randn(P, 3, generator=g), "gv": torch.randn(P, 3, generator=g), "gJ": torch.randn(P, 9, generator=g)}
    c["valid"] = fam != R.FAM_NAN
    c["lattice"] = fam == R.FAM_LATTICE
    c["smooth"] = c["valid"] & ~c["lattice"]                  # the points judged on every output, the discontinuous ones included
    return c


def _tiled(c, P):
    """The case repeated with period len(c) up to P rows (device tensors of the point inputs)."""
    idx = torch.arange(P) % c["P"]
    return {k: c[k][idx] for k in ("p", "frame", "g_d", "gv", "gJ")}, idx.to(DEV)


def _run_forward(c, G, pts=None, rays=None, cam=None):
    L, lib = _lib()
    pts = pts or c
    P = pts["p"].shape[0]
    o = {"d": _out(P, 3), "loss2": _out(P), "angle": _out(P), "g_d": _out(P, 3)}
    hold = [_dev(pts["p"]), _dev(pts["frame"]), _dev(c["A"]), _dev(c["trans"]), _dev(cam), _dev(rays)]
    L.check(lib.recmv_lbs_forward(_p(hold[0]), _p(hold[1]), P, _p(hold[2]), _p(hold[3]), c["B"], G.ref(), _p(hold[4]), _p(hold[5]),
                                  _p(o["d"]), _p(o["loss2"]), _p(o["angle"]), _p(o["g_d"]), _stream()), "lbs_forward")
    torch.cuda.synchronize()
    _guards_ok(*o.values())
    return o


def _run_vjp(c, G, pts=None):
    L, lib = _lib()
    pts = pts or c
    P = pts["p"].shape[0]
    o = {"g_p": _out(P, 3)}
    hold = [_dev(pts["p"]), _dev(pts["frame"]), _dev(c["A"]), _dev(pts["g_d"])]
    L.check(lib.recmv_lbs_vjp_input(_p(hold[0]), _p(hold[1]), P, _p(hold[2]), c["B"], G.ref(), _p(hold[3]), _p(o["g_p"]),
                                    _stream()), "lbs_vjp_input")
    torch.cuda.synchronize()
    _guards_ok(*o.values())
    return o


def _run_stage(c, G, pts=None, g_d=None):
    L, lib = _lib()
    pts = pts or c
    P, B = pts["p"].shape[0], c["B"]
    o = {"W": _out(P, R.KJ), "Q": _out(P, B * 12), "Gs": _out(P, B * 3)}
    hold = [_dev(pts["p"]), _dev(pts["frame"]), _dev(pts["g_d"] if g_d is None else g_d)]
    L.check(lib.recmv_lbs_vjp_params_stage(_p(hold[0]), _p(hold[1]), P, B, G.ref(), _p(hold[2]), _p(o["W"]), _p(o["Q"]),
                                           _p(o["Gs"]), _stream()), "lbs_vjp_params_stage")
    torch.cuda.synchronize()
    _guards_ok(*o.values())
    return o


def _run_jet(c, G, pts=None):
    L, lib = _lib()
    pts = pts or c
    P = pts["p"].shape[0]
    o = {"v": _out(P, 3), "J": _out(P, 9)}
    hold = [_dev(pts["p"]), _dev(pts["frame"]), _dev(c["A"]), _dev(c["trans"])]
    L.check(lib.recmv_lbs_jet_forward(_p(hold[0]), _p(hold[1]), P, _p(hold[2]), _p(hold[3]), c["B"], G.ref(), _p(o["v"]),
                                      _p(o["J"]), _stream()), "lbs_jet_forward")
    torch.cuda.synchronize()
    _guards_ok(*o.values())
    return o


def _run_jet_bwd(c, G, pts=None, gv=True, gJ=True):
    L, lib = _lib()
    pts = pts or c
    P, B = pts["p"].shape[0], c["B"]
    o = {"g_p": _out(P, 3), "W4": _out(4 * P, R.KJ), "Q4": _out(4 * P, B * 12), "Gs": _out(P, B * 3)}
    gv = pts["gv"] if gv is True else gv
    gJ = pts["gJ"] if gJ is True else gJ
    hold = [_dev(pts["p"]), _dev(pts["frame"]), _dev(c["A"]), _dev(gv), _dev(gJ)]
    L.check(lib.recmv_lbs_jet_backward_stage(_p(hold[0]), _p(hold[1]), P, _p(hold[2]), B, G.ref(), _p(hold[3]), _p(hold[4]),
                                             _p(o["g_p"]), _p(o["W4"]), _p(o["Q4"]), _p(o["Gs"]), _stream()),
            "lbs_jet_backward_stage")
    torch.cuda.synchronize()
    _guards_ok(*o.values())
    return o


def _rows4(mask):
    return mask.repeat_interleave(4)


def _nan_rows_are_zero(c, W, per_point=1):
    nan = ~c["valid"]
    if bool(nan.any()):
        rows = nan.repeat_interleave(per_point) if per_point > 1 else nan
        if per_point > 1:                                                 # only the weight row of the four
            rows = rows & (torch.arange(rows.numel()) % per_point == 0)
        assert bool((W.cpu()[rows] == 0).all()), "a NaN point must sample zero weights"


def _judge_forward(c, o, name):
    ref = R.lbs_forward(c["p"], c["frame"], c["A"], c["trans"], c["grid"], c["lattice"])
    _report(name, d=_ratio(o["d"], ref["d"], c["valid"]))


def _judge_vjp(c, o, name):
    ref = R.lbs_vjp_input(c["p"], c["frame"], c["A"], c["grid"], c["g_d"])
    _report(name, g_p=_ratio(o["g_p"], ref["g_p"], c["smooth"]))


def _judge_stage(c, o, name):
    ref = R.lbs_params_stage(c["p"], c["frame"], c["B"], c["grid"], c["g_d"], c["lattice"])
    _report(name, W=_ratio(o["W"], ref["W"], c["valid"]), Q=_ratio(o["Q"], ref["Q"], c["valid"]))
    assert torch.equal(o["Gs"].cpu().double(), ref["Gs"].v), "Gs is a copy into the frame block, zeros elsewhere"
    _nan_rows_are_zero(c, o["W"])


def _judge_jet(c, o, name):
    ref = R.lbs_jet_forward(c["p"], c["frame"], c["A"], c["trans"], c["grid"], c["lattice"])
    _report(name, v=_ratio(o["v"], ref["v"], c["valid"]), J=_ratio(o["J"].view(-1, 3, 3), ref["J"], c["smooth"]))


def _judge_jet_bwd(c, o, name, gv=True, gJ=True):
    ref = R.lbs_jet_backward(c["p"], c["frame"], c["A"], c["B"], c["grid"], c["gv"] if gv else None, c["gJ"] if gJ else None)
    _report(name, g_p=_ratio(o["g_p"], ref["g_p"], c["smooth"]), W4=_ratio(o["W4"], ref["W4"], _rows4(c["smooth"])),
            Q4=_ratio(o["Q4"], ref["Q4"], _rows4(c["valid"])))
    assert torch.equal(o["Gs"].cpu().double(), ref["Gs"].v)
    _nan_rows_are_zero(c, o["W4"], 4)


PV = [(s, P) for s in R.VOLUMES for P in R.LBS_P]


@pytest.mark.parametrize("shape,P", PV)
def test_lbs_forward_within_float64_bounds(shape, P):
    c = _case(shape, P, 3)
    o = _run_forward(c, _Grid(c["grid"]))
    if P:
        _judge_forward(c, o, "lbs_forward %s P=%d" % (shape, P))


@pytest.mark.parametrize("shape,P", PV)
def test_lbs_vjp_input_within_float64_bounds(shape, P):
    c = _case(shape, P, 3)
    o = _run_vjp(c, _Grid(c["grid"]))
    if P:
        _judge_vjp(c, o, "lbs_vjp_input %s P=%d" % (shape, P))


@pytest.mark.parametrize("shape,P", PV)
def test_lbs_vjp_params_stage_within_float64_bounds(shape, P):
    c = _case(shape, P, 3)
    o = _run_stage(c, _Grid(c["grid"]))
    if P:
        _judge_stage(c, o, "lbs_vjp_params_stage %s P=%d" % (shape, P))


@pytest.mark.parametrize("shape,P", PV)
def test_lbs_jet_forward_within_float64_bounds(shape, P):
    c = _case(shape, P, 3)
    o = _run_jet(c, _Grid(c["grid"]))
    if P:
        _judge_jet(c, o, "lbs_jet_forward %s P=%d" % (shape, P))


@pytest.mark.parametrize("shape,P", PV)
def test_lbs_jet_backward_stage_within_float64_bounds(shape, P):
    c = _case(shape, P, 3)
    o = _run_jet_bwd(c, _Grid(c["grid"]))
    if P:
        _judge_jet_bwd(c, o, "lbs_jet_backward_stage %s P=%d" % (shape, P))


@pytest.mark.parametrize("B", R.LBS_B)
def test_lbs_entry_points_over_the_frame_counts(B):
    """B = 1, the usual 3, 56 / 57 and the header's limit 128 (147 456 bytes of dynamic LDS for the staged transforms)."""
    c = _case((3, 5, 4), 257, B)
    G = _Grid(c["grid"])
    assert set(c["frame"].tolist()) >= {0, B - 1}
    _judge_forward(c, _run_forward(c, G), "lbs_forward B=%d" % B)
    _judge_vjp(c, _run_vjp(c, G), "lbs_vjp_input B=%d" % B)
    _judge_stage(c, _run_stage(c, G), "lbs_vjp_params_stage B=%d" % B)
    _judge_jet(c, _run_jet(c, G), "lbs_jet_forward B=%d" % B)
    _judge_jet_bwd(c, _run_jet_bwd(c, G), "lbs_jet_backward_stage B=%d" % B)


def test_lbs_refuses_frame_counts_outside_the_header_range():
    """A host return code, no launch: B = 0 and B = 129."""
    L, lib = _lib()
    c = _case((3, 5, 4), 257, 3)
    G = _Grid(c["grid"])
    p, fr, A, tr, g = _dev(c["p"]), _dev(c["frame"]), _dev(c["A"]), _dev(c["trans"]), _dev(c["g_d"])
    gJ = _dev(c["gJ"])
    for B in (0, 129, -1):
        d, W, Q, Gs, J, W4, Q4 = _out(257, 3), _out(257, 24), _out(257, 12), _out(257, 3), _out(257, 9), _out(1028, 24), _out(1028, 12)
        assert lib.recmv_lbs_forward(_p(p), _p(fr), 257, _p(A), _p(tr), B, G.ref(), None, None, _p(d), None, None, None, _stream()) == ERR_ARG
        assert lib.recmv_lbs_vjp_input(_p(p), _p(fr), 257, _p(A), B, G.ref(), _p(g), _p(d), _stream()) == ERR_ARG
        assert lib.recmv_lbs_vjp_params_stage(_p(p), _p(fr), 257, B, G.ref(), _p(g), _p(W), _p(Q), _p(Gs), _stream()) == ERR_ARG
        assert lib.recmv_lbs_jet_forward(_p(p), _p(fr), 257, _p(A), _p(tr), B, G.ref(), _p(d), _p(J), _stream()) == ERR_ARG
        assert lib.recmv_lbs_jet_backward_stage(_p(p), _p(fr), 257, _p(A), B, G.ref(), _p(g), _p(gJ), _p(d), _p(W4), _p(Q4), _p(Gs),
                                                _stream()) == ERR_ARG
        torch.cuda.synchronize()
        for t in (d, W, Q, Gs, J, W4, Q4):
            assert bool(torch.isnan(t).all()), "wrote an output although it refused the call"


@pytest.mark.parametrize("entry", ["forward", "vjp_input", "jet_forward", "params_stage", "jet_backward_stage"])
def test_lbs_grid_stride_wrap_repeats_the_first_block_bit_for_bit(entry):
    """P = 524 288 + 300 > 256 * 8 * 256: the lanes are independent, so rows i and i mod 4099 carry the same bits; the first 4099
    rows are judged against float64."""
    c = _case((3, 5, 4), R.WRAP_TILE, 1)
    G = _Grid(c["grid"])
    pts, idx = _tiled(c, R.WRAP_P)
    run, judge = {"forward": (_run_forward, _judge_forward), "vjp_input": (_run_vjp, _judge_vjp), "jet_forward": (_run_jet, _judge_jet),
                  "params_stage": (_run_stage, _judge_stage), "jet_backward_stage": (_run_jet_bwd, _judge_jet_bwd)}[entry]
    o = run(c, G, pts)
    first = {}
    for k, t in o.items():
        if entry == "forward" and k != "d":
            continue
        per = t.shape[0] // R.WRAP_P
        rows = (idx.repeat_interleave(per) * per + torch.arange(per, device=DEV).repeat(R.WRAP_P)) if per > 1 else idx
        head = t[:R.WRAP_TILE * per]
        assert _same_bits(t, head[rows]), k
        first[k] = head
    judge(c, first, "%s across the wrap" % entry)


def test_lbs_ray_outputs_in_isolation():
    """loss2, angle and g_d as functions of the kernel's own d: the sine of the ray against d - cam covers [1e-6, 0.98] for loss2
    and angle and [1e-3, 0.98] for g_d (its bound carries the cancellation of the cross product, u / (un dn))."""
    c = _case((9, 6, 7), 4099, 3)
    G = _Grid(c["grid"])
    plain = _run_forward(c, G)
    for k in ("loss2", "angle", "g_d"):
        assert bool(torch.isnan(plain[k]).all()), "rays == NULL must leave %s untouched" % k
    cam = torch.tensor([0.3, -2.5, 0.4])
    d = plain["d"].cpu()
    ok = c["valid"]
    dfix = torch.where(ok.unsqueeze(1), d, torch.ones_like(d))
    for lo, keys in ((1e-6, ("loss2", "angle")), (1e-3, ("g_d",))):
        rays = R.make_rays(dfix, cam, lo)
        o = _run_forward(c, G, rays=rays, cam=cam)
        assert _same_bits(o["d"], plain["d"])
        ref = R.ray_energy(dfix, cam, rays)
        assert float((ref["loss2"].v + ref["loss2"].e).max()) <= R.RATIO_MAX and float(ref["loss2"].v.min()) < 1.5 * lo
        _report("lbs_forward rays sin >= %g" % lo, **{k: _ratio(o[k], ref[k], ok) for k in keys})


def test_lbs_jet_reverse_with_one_cotangent_missing():
    c = _case((9, 6, 7), 257, 3)
    G = _Grid(c["grid"])
    _judge_jet_bwd(c, _run_jet_bwd(c, G, gv=None), "lbs_jet_backward_stage gv=NULL", gv=False)
    _judge_jet_bwd(c, _run_jet_bwd(c, G, gJ=None), "lbs_jet_backward_stage gJ=NULL", gJ=False)


@pytest.mark.parametrize("shape", R.VOLUMES)
def test_lbs_entry_points_agree_bit_for_bit(shape):
    c = _case(shape, 4099, 3)
    G = _Grid(c["grid"])
    assert _same_bits(_run_stage(c, G)["W"], _run_jet_bwd(c, G)["W4"][0::4])
    assert _same_bits(_run_jet(c, G)["v"], _run_forward(c, G)["d"])


@pytest.mark.parametrize("B", (1, 3, 57))
def test_lbs_staged_matrices_exact_on_integers(B):
    """g_d, gv, gJ in {-3..3}, p in {-2..2}: Q, Gs and Q4 are integers: one misplaced frame block or row fails."""
    P = 257
    g = torch.Generator().manual_seed(B)
    c = dict(_case((3, 5, 4), P, B))
    c["p"] = torch.randint(-2, 3, (P, 3), generator=g).float()
    c["g_d"] = c["gv"] = torch.randint(-3, 4, (P, 3), generator=g).float()
    c["gJ"] = torch.randint(-3, 4, (P, 9), generator=g).float()
    G = _Grid(c["grid"])
    st, bw = _run_stage(c, G), _run_jet_bwd(c, G)
    rs = R.lbs_params_stage(c["p"], c["frame"], B, c["grid"], c["g_d"])
    rb = R.lbs_jet_backward(c["p"], c["frame"], c["A"], B, c["grid"], c["gv"], c["gJ"])
    for got, ref, k in ((st["Q"], rs["Q"], "Q"), (st["Gs"], rs["Gs"], "Gs"), (bw["Q4"], rb["Q4"], "Q4"), (bw["Gs"], rb["Gs"], "Gs4")):
        assert float(ref.v.abs().max()) < 2 ** 24
        assert torch.equal(got.cpu(), ref.v.float()), k
    own = torch.zeros(P, B * 12, dtype=torch.bool)
    own.scatter_(1, c["frame"].unsqueeze(1) * 12 + torch.arange(12).unsqueeze(0), True)
    assert bool((st["Q"].cpu()[~own] == 0).all()) and bool((bw["Q4"].cpu().view(P, 4, B * 12)[~own.unsqueeze(1).expand(P, 4, B * 12)] == 0).all())


# ---------------------------------------------------------------------------------------------------------- root finder
def _rootfind_update(c, counter0, do_update):
    L, lib = _lib()
    P = c["p"].shape[0]
    p = _out(P, 3)
    p.copy_(c["p"])
    un = _out(P, dtype=torch.uint8, fill=0)
    un.copy_(c["unfinished"])
    cnt = _out(1, dtype=torch.int32, fill=0)
    cnt.fill_(counter0)
    hold = [_dev(c[k]) for k in ("f", "gf", "loss2", "angle", "gd")]
    L.check(lib.recmv_rootfind_update(_p(p), _p(hold[0]), _p(hold[1]), _p(hold[2]), _p(hold[3]), _p(hold[4]), _p(un), _p(cnt), P,
                                      R.ROOT_DTHR, R.ROOT_ATHR, R.ROOT_W1, R.ROOT_W2, do_update, _stream()), "rootfind_update")
    torch.cuda.synchronize()
    _guards_ok(p, un, cnt)
    return p, un, cnt


def _judge_rootfind(c, p, un, count, counter0, do_update, name):
    ref = R.rootfind_update(c["p"], c["f"], c["gf"], c["loss2"], c["angle"], c["gd"], c["unfinished"], counter0, R.ROOT_DTHR,
                            R.ROOT_ATHR, R.ROOT_W1, R.ROOT_W2, do_update)
    assert ref["margin"] > 0
    assert torch.equal(un.cpu(), ref["unfinished"]), "flags"
    assert int(count) == ref["count"], "counter"
    still = ~ref["moved"]
    assert _same_bits(p.cpu()[still], c["p"][still]), "p of a finished ray (or with do_update == 0) must keep its bits"
    _report(name, p=_ratio(p, ref["p"]))
    return ref


@pytest.mark.parametrize("family", R.ROOT_FAMILIES)
@pytest.mark.parametrize("P", R.ROOT_P + (R.WRAP_P,))
def test_rootfind_update_against_float64(P, family):
    c = R.make_rootfind(P, family)
    for do_update in (1, 0):
        p, un, cnt = _rootfind_update(c, 5, do_update)
        if P == 0:
            assert int(cnt) == 5
            continue
        ref = _judge_rootfind(c, p, un, int(cnt), 5, do_update, "rootfind_update %s P=%d update=%d" % (family, P, do_update))
        if family == "finished":
            assert int(cnt) == 5 and not bool(un.any())
        if family == "none":
            assert ref["count"] == 5 + int(c["unfinished"].sum())


@pytest.mark.parametrize("times", (0, 1, 3))
def test_rootfind_step_protocol(times):
    """times + 2 calls: state[0] counts the calls, counters[step] receives the unfinished rays of that step, marks[step] is
    counters[step] + 1, and p moves only while step < times; every step is judged against float64 from the p it started with."""
    L, lib = _lib()
    P = 257
    c = dict(R.make_rootfind(P, "mixed", 1))
    calls = times + 2
    p = _out(P, 3)
    p.copy_(c["p"])
    un = _out(P, dtype=torch.uint8, fill=0)
    un.copy_(c["unfinished"])
    counters, marks, state = (_out(calls, dtype=torch.int32, fill=0), _out(calls, dtype=torch.int32, fill=0),
                              _out(1, dtype=torch.int32, fill=0))
    hold = [_dev(c[k]) for k in ("f", "gf", "loss2", "angle", "gd")]
    for step in range(calls):
        L.check(lib.recmv_rootfind_step(_p(p), _p(hold[0]), _p(hold[1]), _p(hold[2]), _p(hold[3]), _p(hold[4]), _p(un), _p(counters),
                                        _p(marks), _p(state), P, R.ROOT_DTHR, R.ROOT_ATHR, R.ROOT_W1, R.ROOT_W2, times, _stream()),
                "rootfind_step")
        torch.cuda.synchronize()
        _guards_ok(p, un, counters, marks, state)
        ref = _judge_rootfind(c, p, un, int(counters[step]), 0, int(step < times), "rootfind_step times=%d step=%d" % (times, step))
        assert int(state[0]) == step + 1 and int(marks[step]) == ref["count"] + 1
        assert bool((counters[step + 1:] == 0).all()) and bool((marks[step + 1:] == 0).all())
        c["p"], c["unfinished"] = p.cpu().clone(), un.cpu().clone()
    z = torch.zeros(4, device=DEV)
    assert lib.recmv_rootfind_step(_p(z), _p(z), _p(z), _p(z), _p(z), _p(z), _p(un), _p(counters), _p(marks), _p(state), 0, 1.0, 1.0,
                                   1.0, 1.0, 1, _stream()) == ERR_ARG


# ------------------------------------------------------------------------------------------------------ kinematic chain
def _host(a, dtype):
    arr = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    return arr, arr.ctypes.data_as(C.c_void_p)


def _chain_forward(poses, Js, parents, ip, want_A=True):
    L, lib = _lib()
    B = poses.shape[0]
    G = _out(B, 24, 4, 4)
    A = _out(B, 24, 4, 4) if want_A else None
    js, jsp = _host(Js.numpy(), np.float32)
    pa, pap = _host(parents, np.int32)
    hold = [_dev(poses), _dev(ip)]
    L.check(lib.recmv_kinematic_chain_forward(_p(hold[0]), jsp, pap, _p(hold[1]) if ip is not None else None, _p(G),
                                              _p(A) if want_A else None, B, _stream()), "chain_forward")
    torch.cuda.synchronize()
    _guards_ok(*([G, A] if want_A else [G]))
    return G, A


def _chain_backward(poses, Js, parents, ip, gG, gA):
    L, lib = _lib()
    B = poses.shape[0]
    out = _out(B, 24, 3)
    js, jsp = _host(Js.numpy(), np.float32)
    pa, pap = _host(parents, np.int32)
    hold = [_dev(poses), _dev(ip), _dev(gG), _dev(gA)]
    L.check(lib.recmv_kinematic_chain_backward(_p(hold[0]), jsp, pap, _p(hold[1]) if ip is not None else None,
                                               _p(hold[2]) if gG is not None else None, _p(hold[3]) if gA is not None else None,
                                               _p(out), B, _stream()), "chain_backward")
    torch.cuda.synchronize()
    _guards_ok(out)
    return out


@pytest.mark.parametrize("table", sorted(R.parent_tables()))
@pytest.mark.parametrize("B", R.CHAIN_B)
def test_kinematic_chain_against_float64(B, table):
    parents = R.parent_tables()[table]
    poses, Js = R.make_poses(B), R.make_joints()
    g = torch.Generator().manual_seed(B + 1)
    gG, gA = torch.randn(B, 24, 4, 4, generator=g), torch.randn(B, 24, 4, 4, generator=g)
    worst = {}
    for general in (False, True):
        ip = R.make_init_pose(0, general)
        G, A = _chain_forward(poses, Js, parents, ip)
        G0, _ = _chain_forward(poses, Js, parents, None, want_A=False)
        assert _same_bits(G, G0), "G must not depend on whether A is asked for"
        if B == 0:
            continue
        ref = R.chain_forward(poses, Js, parents, ip)
        tag = "general" if general else "rigid"
        worst["G_" + tag], worst["A_" + tag] = _ratio(G, ref["G"]), _ratio(A, ref["A"])
        for name, a, b in (("gG", gG, None), ("gA", None, gA), ("both", gG, gA)):
            got = _chain_backward(poses, Js, parents, ip if b is not None else (ip if general else None), a, b)
            worst["%s_%s" % (name, tag)] = _ratio(got, R.chain_backward(poses, Js, parents, ip, a, b)["gposes"])
    if B:
        _report("kinematic_chain %s B=%d" % (table, B), **worst)


# -------------------------------------------------------------------------------------------------- positional encoding
def _wptr(w):
    if w is None:
        return None, None
    arr = np.ascontiguousarray(w.numpy().astype(np.float32))
    return arr, arr.ctypes.data_as(C.c_void_p)


def _posenc_forward(x, L_, w, out_scale, ldx, ldo, ldo_fill):
    L, lib = _lib()
    P = x.shape[0]
    xv = _placed(x, ldx)
    out = _out(P, ldo)
    keep, wp = _wptr(w)
    L.check(lib.recmv_posenc_forward(_p(xv), ldx, _p(out), ldo, ldo_fill, P, L_, wp, out_scale, _stream()), "posenc_forward")
    torch.cuda.synchronize()
    _guards_ok(out)
    return out


def _posenc_vjp(x, g, t, L_, w, ldx, ldg, ldt):
    L, lib = _lib()
    P = x.shape[0]
    xv, gv = _placed(x, ldx), _placed(g, ldg)
    tv = None if t is None else _placed(t if ldt else t[:1], max(ldt, 3))
    out = _out(P, 3)
    keep, wp = _wptr(w)
    L.check(lib.recmv_posenc_vjp(_p(xv), ldx, _p(gv), ldg, _p(tv) if tv is not None else None, ldt, _p(out), P, L_, wp, _stream()),
            "posenc_vjp")
    torch.cuda.synchronize()
    _guards_ok(out)
    return out


def _posenc_jvp(x, t, L_, w, ldx, ldt, ldo):
    L, lib = _lib()
    P = x.shape[0]
    xv = _placed(x, ldx)
    tv = _placed(t if ldt else t[:1], max(ldt, 3))
    out = _out(P, ldo)
    keep, wp = _wptr(w)
    L.check(lib.recmv_posenc_jvp(_p(xv), ldx, _p(tv), ldt, _p(out), ldo, P, L_, wp, _stream()), "posenc_jvp")
    torch.cuda.synchronize()
    _guards_ok(out)
    return out


PE_CASES = [(L_, P) for L_ in R.PE_L for P in R.PE_P]


@pytest.mark.parametrize("L_,P", PE_CASES + [(6, 40400)])
def test_posenc_forward_against_float64(L_, P):
    x = R.make_pe_x(P)
    nf = 3 + 6 * L_
    ldo = nf + 5
    scale = float(np.float32(2 ** -0.5))
    worst = {}
    for name, w in R.pe_weight_sets(L_).items():
        for fill in (nf, ldo):
            out = _posenc_forward(x, L_, w, scale, 5, ldo, fill)
            if P == 0:
                continue
            worst["%s_fill%d" % (name, fill)] = _ratio(out[:, :nf], R.posenc(x, L_, w, scale))
            assert bool((out[:, nf:fill] == 0).all()), "zero fill"
            assert bool(torch.isnan(out[:, fill:]).all()), "columns beyond ldo_fill are not the kernel's"
    if P:
        _report("posenc_forward L=%d P=%d" % (L_, P), **worst)


@pytest.mark.parametrize("L_,P", PE_CASES + [(6, 174800)])
def test_posenc_vjp_first_and_second_order_against_float64(L_, P):
    x = R.make_pe_x(P)
    g = torch.Generator().manual_seed(L_ * 7 + P % 1000)
    gm = torch.randn(P, 3 + 6 * L_, generator=g)
    t = torch.randn(max(P, 1), 3, generator=g)
    worst = {}
    for name, w in R.pe_weight_sets(L_).items():
        out = _posenc_vjp(x, gm, None, L_, w, 4, 3 + 6 * L_ + 2, 0)
        if P:
            worst[name] = _ratio(out, R.posenc_vjp(x, gm, L_, w))
        for ldt in (0, 3, 5):
            out = _posenc_vjp(x, gm, t, L_, w, 3, 3 + 6 * L_, ldt)
            if P:
                worst["%s_t_ld%d" % (name, ldt)] = _ratio(out, R.posenc_vjp(x, gm, L_, w, t[:P] if ldt else t[:1]))
    if P:
        _report("posenc_vjp L=%d P=%d" % (L_, P), **worst)


@pytest.mark.parametrize("L_,P", PE_CASES + [(6, 40400)])
def test_posenc_jvp_against_float64(L_, P):
    x = R.make_pe_x(P)
    g = torch.Generator().manual_seed(L_ * 11 + P % 1000)
    t = torch.randn(max(P, 1), 3, generator=g)
    nf = 3 + 6 * L_
    worst = {}
    for name, w in R.pe_weight_sets(L_).items():
        for ldt in (0, 3, 5):
            out = _posenc_jvp(x, t, L_, w, 5, ldt, nf + 3)
            if P:
                worst["%s_ld%d" % (name, ldt)] = _ratio(out[:, :nf], R.posenc_jvp(x, t[:P] if ldt else t[:1], L_, w))
                assert bool(torch.isnan(out[:, nf:]).all())
    if P:
        _report("posenc_jvp L=%d P=%d" % (L_, P), **worst)


def _ulps(got, ref):
    """|got - ref| in units of the float32 ulp of ref (float64 tensors on the device)."""
    _, e = torch.frexp(ref)
    return ((got - ref).abs() / torch.ldexp(torch.ones_like(ref), e - 24)).max().item()


def test_sinf_cosf_sincosf_accuracy():
    """The measurement behind SINF_ULP, COSF_ULP and SINCOSF_ULP: 2^18 log-spaced |x| in [1e-6, 4], both signs, all 16 bands (arguments
    up to 2^15 * 4).  With weights 1 and out_scale 1 the forward returns sinf / cosf of the exact argument; the vjp of a one-hot g
    returns 2^b cos / -2^b sin from sincosf, every other step exact."""
    n = 2 ** 18
    mag = torch.exp(torch.linspace(math.log(1e-6), math.log(4.0), n, dtype=torch.float64)).float()
    vals = torch.cat([mag, -mag, mag[:1]])                                 # 2^19 + 1 = 3 * 174763
    P = vals.numel() // 3
    x = vals.view(P, 3)
    Lmax, nf = 16, 3 + 6 * 16
    xd = _dev(x).double()
    f = (2.0 ** torch.arange(Lmax, dtype=torch.float64, device=DEV)).view(1, Lmax, 1)
    arg = xd.unsqueeze(1) * f
    rs, rc = torch.sin(arg), torch.cos(arg)
    out = _posenc_forward(x, Lmax, None, 1.0, 3, nf, nf)[:, 3:].double().view(P, Lmax, 2, 3)
    sin_ulp, cos_ulp = _ulps(out[:, :, 0], rs), _ulps(out[:, :, 1], rc)
    L, lib = _lib()
    xv, g, got = _dev(x), torch.zeros(P, nf, device=DEV), _out(P, 3)
    sc_sin = sc_cos = 0.0
    for b in range(Lmax):
        for part in (0, 1):
            g.zero_()
            g[:, 3 + 6 * b + 3 * part:3 + 6 * b + 3 * part + 3] = 1.0
            L.check(lib.recmv_posenc_vjp(_p(xv), 3, _p(g), nf, None, 0, _p(got), P, Lmax, None, _stream()), "posenc_vjp")
            val = got.double() / f[0, b, 0]
            if part == 0:
                sc_cos = max(sc_cos, _ulps(val, rc[:, b]))
            else:
                sc_sin = max(sc_sin, _ulps(-val, rs[:, b]))
    _guards_ok(got)
    print("measured ulp: sinf %.3f  cosf %.3f  sincosf sin %.3f cos %.3f" % (sin_ulp, cos_ulp, sc_sin, sc_cos))
    assert sin_ulp <= R.SINF_ULP and cos_ulp <= R.COSF_ULP and max(sc_sin, sc_cos) <= R.SINCOSF_ULP
