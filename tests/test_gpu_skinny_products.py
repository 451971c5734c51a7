"""The skinny and the unaligned routes of recmv_gemm_nt / recmv_gemm_tn (csrc/gemm_f32.hip, csrc/gemm_tn.hip; which launch takes which
kernel: the planner of csrc/gemm_route.h), through the ctypes entry points.

  NT, N <= 4 (last layers' forward)       gemm_nt_thin_n_kernel
  NT, K <= 4 (their input gradients)      gemm_nt_thin_k_kernel
  NT, unaligned, >= 512 large tiles       gemm_nt_occ_kernel<..., SCAL>
  TN, <= 4 output rows or columns         gemm_tn_thin_kernel
  TN, leading dimension % 4 != 0          gemm_tn_occ_kernel<16, SCAL>

Every case is judged twice.  Against float64 by the project's contract |err| <= 4e-7 * sum|a b| + 1e-6 on the pre-activation (ReLU and
softplus are 1-Lipschitz, so the bound passes through them; it is multiplied by |out_scale| and by the factor of the output transform).
And bit for bit (==, so +0 and -0 compare equal): the NT routes against the aligned MFMA route on a zero-padded, 16-byte aligned copy
of the same operands, and against themselves at another row count; the TN routes against a second run (skinny) or the aligned route on
a padded copy (unaligned).

The aligned MFMA reference of the N <= 4 cases: the same rows, N padded to 128 and K to a multiple of 4.  Which MFMA kernel that is
depends on the row count (the tile choice of plan_nt), and the kernels do not all round alike: the 64 x 32 kernel of the small
launches (up to 40 896 rows here) sums the two halves of every 32-wide K-tile on separate chains, the 64 x 64 and the high-occupancy
kernels of the larger launches on one.  The skinny kernel takes the order of the kernel its launch had before, so every launch keeps
its bits: rows compare equal between launches of one regime (63 / 130 / 16 421 rows; 41 000 / 66 001 rows), which the cases below
check on both sides of the boundary.
The aligned MFMA reference of the K <= 4 cases pads K to 8 (K = 4 itself is a skinny shape); their order does not depend on the rows.
The skinny TN route keeps the order and the split lengths of the MFMA route, so it is also compared with that route on a copy padded
to 8 output rows / columns, on top of a second run of itself (run-to-run reproducibility).  The unaligned TN route keeps the split length of the kernel
it replaces (rounded to 32 rows; the aligned route rounds to 16): equal for the shape tested here (20 005 rows in 128 splits: 160).

The last test replays the route census (tests/gemm_route_cases.py, tests/golden/gemm_routes.json): every case under the default routes
and under RECMV_GEMM_SKINNY=0 must land in the profile slot and give the bits that the library gave before its routes were planned in
gemm_route.h.
"""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest
import torch

sys.path[:0] = [str(Path(__file__).resolve().parent)]
import gemm_route_cases as GC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
ACT_NONE, ACT_RELU, ACT_SOFTPLUS = 0, 1, 2
MS = (1, 63, 130, 16421)
MS_LARGE = (41000, 66001)          # N <= 4 only: the launches whose MFMA route was a single-chain kernel


def _lib():
    from recmv import _lib as L
    return L, L.lib()


def _stream():
    L, _ = _lib()
    return L.stream_ptr(torch.device(DEV))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.fixture(autouse=True)
def f32_matrix_mode():
    L, _ = _lib()
    prev = L.set_gemm_mode(0)
    try:
        yield
    finally:
        L.set_gemm_mode(prev)


def _rand(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).to(DEV)


def _placed(t, ld=None, shift=0):
    """A device copy of the 2-D tensor inside a NaN-filled buffer: row stride `ld`, base `shift` floats off a 16-byte boundary."""
    rows, cols = t.shape
    ld = cols if ld is None else ld
    flat = torch.full((max(rows, 1) * ld + shift + 8,), NAN, device=DEV)
    view = flat[shift:shift + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    return view


def _padded(t, rows, cols):
    out = torch.zeros(rows, cols, device=DEV)
    out[:t.shape[0], :t.shape[1]] = t
    return out


def _act64(z, act, beta):
    if act == ACT_RELU:
        return z.clamp_min(0)
    if act == ACT_SOFTPLUS:
        return torch.nn.functional.softplus(z, beta=beta, threshold=1e9)
    return z


def _gemm_nt(A, B, bias, M, N, K, act=ACT_NONE, p=0.0, out_scale=1.0, ldc=None, lda=None, ldb=None):
    L, lib = _lib()
    ldc = N if ldc is None else ldc
    out = torch.full((max(M, 1), ldc), NAN, device=DEV)
    L.check(lib.recmv_gemm_nt(_p(A), A.stride(0) if lda is None else lda, _p(B), B.stride(0) if ldb is None else ldb, _p(bias), _p(out),
                              ldc, M, N, K, act, float(p), float(out_scale), _stream()), "gemm_nt")
    return out


def _check64(got, ref, mag, factor, name):
    bound = (4e-7 * mag + 1e-6) * factor
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print("ratio %s: %.3g" % (name, ratio))
    assert ratio <= 1.0, "%s: error / bound = %.4g" % (name, ratio)


# ------------------------------------------------------------------------------------------------ NT, N <= 4
_fwd_cache = {}


def _fwd_operands(K):
    """A [66001, K] and its zero-padded aligned copy, shared by every case of this K (never modified)."""
    if K not in _fwd_cache:
        A = _rand(MS_LARGE[-1], K, seed=100 + K)
        Kp = (K + 3) // 4 * 4
        _fwd_cache[K] = (A, _padded(A, MS_LARGE[-1], Kp), Kp)
    return _fwd_cache[K]


@pytest.mark.parametrize("K", [5, 40, 512])
@pytest.mark.parametrize("N", [1, 3, 4])
@pytest.mark.parametrize("act,use_bias", [(ACT_NONE, False), (ACT_RELU, True), (ACT_SOFTPLUS, True), (ACT_SOFTPLUS, False)])
def test_nt_forward_skinny(N, K, act, use_bias):
    L, lib = _lib()
    A, Apad, Kp = _fwd_operands(K)
    B = _rand(N, K, seed=7 * N + K) * (3.0 / K ** 0.5)
    bias = _rand(1, N, seed=N + 1).reshape(-1).contiguous() if use_bias else None
    beta, out_scale, ldc = 100.0, 0.7071067811865476, N + 3
    Bpad = _padded(B, 128, Kp)
    bpad = _padded(bias.view(1, -1), 1, 128).reshape(-1) if use_bias else None
    z64 = A.double() @ B.double().t() + (bias.double() if use_bias else 0.0)
    ref64 = _act64(z64, act, beta) * out_scale
    mag = A.double().abs() @ B.double().abs().t()
    outs = {}
    for M in MS + MS_LARGE:
        ref_mfma = _gemm_nt(Apad, Bpad, bpad, M, 128, Kp, act, beta, out_scale)
        # rows one float apart from a multiple of 4 and an unaligned base for the odd K; the aligned layout for the others
        Av = _placed(A[:M], K + 1 if K % 4 else K, 1 if K % 4 else 0)
        got = _gemm_nt(Av, B, bias, M, N, K, act, beta, out_scale, ldc=ldc)
        assert torch.isnan(got[:, N:]).all(), "wrote past N"
        outs[M] = got[:M, :N]
        _check64(outs[M], ref64[:M], mag[:M], out_scale, "nt_fwd M=%d N=%d K=%d act=%d" % (M, N, K, act))
        assert (outs[M] == ref_mfma[:M, :N]).all(), "M=%d: differs from the aligned MFMA route" % M
    assert (outs[16421][:63] == outs[63]).all() and (outs[16421][:130] == outs[130]).all()
    assert (outs[66001][:41000] == outs[41000]).all()


def test_nt_forward_skinny_mulgrad_and_seg():
    """The output transform (recmv_gemm_nt_mulgrad) and the two-net row split (recmv_gemm_nt_seg) on N = 3."""
    L, lib = _lib()
    K, N, M = 512, 3, 16421
    A, Apad, Kp = _fwd_operands(K)
    B, B2 = _rand(N, K, seed=1) * 0.13, _rand(N, K, seed=2) * 0.13
    bias, bias2 = _rand(1, N, seed=3).reshape(-1).contiguous(), _rand(1, N, seed=4).reshape(-1).contiguous()
    Y = _rand(M, N, seed=5)
    # mulgrad: C = (A B^T) (.) relu'(Y) * 0.5
    out = torch.full((M, N), NAN, device=DEV)
    L.check(lib.recmv_gemm_nt_mulgrad(_p(A), K, _p(B), K, _p(out), N, M, N, K, _p(Y), N, ACT_RELU, 0.0, 1.0, 0.5, _stream()), "mulgrad")
    ref = torch.full((M, 128), NAN, device=DEV)
    L.check(lib.recmv_gemm_nt_mulgrad(_p(Apad), K, _p(_padded(B, 128, K)), K, _p(ref), 128, M, 128, K,
                                      _p(_padded(Y, M, 128)), 128, ACT_RELU, 0.0, 1.0, 0.5, _stream()), "mulgrad ref")
    assert (out == ref[:M, :N]).all()
    f = (Y > 0).double() * 0.5
    _check64(out, (A[:M].double() @ B.double().t()) * f, A[:M].double().abs() @ B.double().abs().t(), 0.5, "nt_fwd mulgrad")
    # seg: rows >= 128 through the second net
    out = torch.full((M, N), NAN, device=DEV)
    L.check(lib.recmv_gemm_nt_seg(_p(A), K, _p(B), K, _p(bias), _p(B2), _p(bias2), 128, _p(out), N, M, N, K, ACT_RELU, 0.0, 1.0,
                                  _stream()), "seg")
    lo = _gemm_nt(A[:128], B, bias, 128, N, K, ACT_RELU)
    hi = _gemm_nt(A[128:M], B2, bias2, M - 128, N, K, ACT_RELU)
    assert (out[:128] == lo).all() and (out[128:] == hi[:M - 128]).all()


# ------------------------------------------------------------------------------------------------ NT, K <= 4
def _thin_k_call(kind, A, lda, B, B2, Y, ldy, M, N, K, ldb):
    """kind: plain | amul (operand transform) | emul (output transform) | seg (emul with a second net from row 128)."""
    L, lib = _lib()
    out = torch.full((M, N), NAN, device=DEV)
    if kind == "plain":
        L.check(lib.recmv_gemm_nt(_p(A), lda, _p(B), ldb, None, _p(out), N, M, N, K, ACT_NONE, 0.0, 1.0, _stream()), kind)
    elif kind == "amul":
        L.check(lib.recmv_gemm_nt_actgrad(_p(A), lda, _p(Y), ldy, _p(B), ldb, _p(out), N, M, N, K, ACT_RELU, 0.0, 1.0, 0.75,
                                          _stream()), kind)
    elif kind == "emul":
        L.check(lib.recmv_gemm_nt_mulgrad(_p(A), lda, _p(B), ldb, _p(out), N, M, N, K, _p(Y), ldy, ACT_RELU, 0.0, 1.0, 0.75,
                                          _stream()), kind)
    else:
        L.check(lib.recmv_gemm_nt_mulgrad_seg(_p(A), lda, _p(B), _p(B2), 128, ldb, _p(out), N, M, N, K, _p(Y), ldy, ACT_RELU, 0.0,
                                              1.0, 0.75, _stream()), kind)
    return out


@pytest.mark.parametrize("N", [39, 168, 512])
@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("kind", ["plain", "amul", "emul", "seg"])
def test_nt_input_gradient_skinny(K, N, kind):
    Mx = MS[-1]
    A = _rand(Mx, K, seed=K)
    B, B2 = _rand(N, K, seed=10 + N + K), _rand(N, K, seed=20 + N + K)
    Y = _rand(Mx, K if kind == "amul" else N, seed=30 + N)
    wy = Y.shape[1]
    A64 = A.double() * ((Y > 0).double() * 0.75 if kind == "amul" else 1.0)
    ref64 = A64 @ B.double().t()
    mag = A64.abs() @ B.double().abs().t()
    if kind == "seg":
        ref64[128:] = A64[128:] @ B2.double().t()
        mag[128:] = A64[128:].abs() @ B2.double().abs().t()
    if kind in ("emul", "seg"):
        ref64 = ref64 * ((Y > 0).double() * 0.75)
    # the aligned MFMA route: K padded to 8 with zeros (the operand transform's Y too)
    Ap, Bp, B2p = _padded(A, Mx, 8), _padded(B, N, 8), _padded(B2, N, 8)
    Yp = _padded(Y, Mx, 8) if kind == "amul" else Y.contiguous()
    outs = {}
    for M in MS:
        if kind == "seg" and M <= 128:
            continue
        ref_mfma = _thin_k_call(kind, Ap, 8, Bp, B2p, Yp, Yp.stride(0), M, N, 8, 8)
        for lda in (K, K + 1):
            Av = _placed(A[:M], lda)
            Yv = _placed(Y[:M], wy + (lda - K)) if kind == "amul" else Y
            got = _thin_k_call(kind, Av, lda, B, B2, Yv, Yv.stride(0), M, N, K, K)
            assert (got == ref_mfma).all(), "M=%d lda=%d: differs from the aligned MFMA route" % (M, lda)
        outs[M] = got
        _check64(got, ref64[:M], mag[:M], 0.75 if kind != "plain" else 1.0, "nt_dx %s M=%d N=%d K=%d" % (kind, M, N, K))
    assert (outs[16421][:130] == outs[130]).all()
    if 63 in outs:
        assert (outs[16421][:63] == outs[63]).all()


# ------------------------------------------------------------------------------------------------ NT, unaligned, large-tile route
@pytest.mark.parametrize("K", [39, 167, 257])
@pytest.mark.parametrize("N", [473, 512])
def test_nt_unaligned_large_tiles(N, K):
    Mx = 115301
    A = _rand(Mx, K, seed=K + N)
    B = _rand(N, K, seed=K + N + 1) * (3.0 / K ** 0.5)
    bias = _rand(1, N, seed=2).reshape(-1).contiguous()
    Kp = (K + 3) // 4 * 4
    Ap, Bp = _padded(A, Mx, Kp), _padded(B, N, Kp)
    Av, Bv = _placed(A, K, 1), _placed(B, K, 1)       # lda = ldb = K, bases one float off the 16-byte boundary
    ref64 = (A.double() @ B.double().t() + bias.double()).clamp_min(0)
    mag = A.double().abs() @ B.double().abs().t()
    outs = {}
    for M in (16421, Mx):
        ref_mfma = _gemm_nt(Ap, Bp, bias, M, N, Kp, ACT_RELU)
        got = _gemm_nt(Av, Bv, bias, M, N, K, ACT_RELU)
        assert (got == ref_mfma).all(), "M=%d: differs from the aligned route" % M
        _check64(got, ref64[:M], mag[:M], 1.0, "nt_unaligned M=%d N=%d K=%d" % (M, N, K))
        outs[M] = got
    assert (outs[Mx][:16421] == outs[16421]).all()


# ------------------------------------------------------------------------------------------------ TN
def _gemm_tn(A, B, M, N, K):
    L, lib = _lib()
    ws = torch.empty(int(lib.recmv_gemm_tn_workspace_bytes(M, N, K)), dtype=torch.uint8, device=DEV)
    out = torch.full((M, N), NAN, device=DEV)
    L.check(lib.recmv_gemm_tn(_p(A), A.stride(0), _p(B), B.stride(0), _p(out), N, M, N, K, _p(ws), ws.numel(), _stream()), "gemm_tn")
    return out


@pytest.mark.parametrize("M,N,lda,ldb", [(1, 512, 1, 512), (3, 512, 4, 512), (3, 512, 3, 513), (512, 3, 512, 3), (512, 1, 512, 4)])
def test_tn_skinny(M, N, lda, ldb):
    K = 20005
    A, B = _placed(_rand(K, M, seed=M), lda), _placed(_rand(K, N, seed=N + 1), ldb)
    got = _gemm_tn(A, B, M, N, K)
    again = _gemm_tn(A, B, M, N, K)
    assert (got == again).all(), "not reproducible"
    # the MFMA route: the thin operand padded with zero columns to 8 (same splits: the tile count does not change)
    Ap = _placed(_padded(A, K, 8), 8) if M <= 4 else A
    Bp = _placed(_padded(B, K, 8), 8) if N <= 4 else B
    mfma = _gemm_tn(Ap, Bp, max(M, 8) if M <= 4 else M, max(N, 8) if N <= 4 else N, K)
    assert (got == mfma[:M, :N]).all(), "differs from the MFMA route"
    _check64(got, A.double().t() @ B.double(), A.double().abs().t() @ B.double().abs(), 1.0, "tn_skinny %dx%d" % (M, N))


def test_tn_unaligned():
    K, M, N = 20005, 512, 167
    A, B = _rand(K, M, seed=1), _rand(K, N, seed=2)
    Bv = _placed(B, 167)
    got = _gemm_tn(A, Bv, M, N, K)
    ref = _gemm_tn(A, _placed(B, 168), M, N, K)        # the aligned route reads whole float4s of the 168-wide rows
    assert (got == ref).all(), "differs from the aligned route"
    _check64(got, A.double().t() @ B.double(), A.double().abs().t() @ B.double().abs(), 1.0, "tn_unaligned")
    # both operands off: A's base one float off the boundary
    got2 = _gemm_tn(_placed(A, 513, 1), Bv, M, N, K)
    assert (got2 == ref).all()


# ------------------------------------------------------------------------------------------------ empty launches
def test_empty_launches():
    L, lib = _lib()
    B, bias = _rand(3, 8, seed=1), _rand(1, 3, seed=2).reshape(-1).contiguous()
    out = torch.full((4, 3), 5.0, device=DEV)
    # M = 0: OK, nothing read or written (NULL operands)
    L.check(lib.recmv_gemm_nt(None, 8, _p(B), 8, _p(bias), _p(out), 3, 0, 3, 8, ACT_NONE, 0.0, 1.0, _stream()), "M=0")
    assert (out == 5.0).all()
    # K = 0: the empty sum, through the epilogue
    A = _rand(4, 1, seed=3)
    L.check(lib.recmv_gemm_nt(_p(A), 1, _p(B), 8, _p(bias), _p(out), 3, 4, 3, 0, ACT_RELU, 0.0, 2.0, _stream()), "K=0")
    assert torch.equal(out, (bias.clamp_min(0) * 2.0).expand(4, 3))
    wide = torch.full((4, 512), 5.0, device=DEV)
    Bw = _rand(512, 1, seed=4)
    L.check(lib.recmv_gemm_nt(_p(A), 1, _p(Bw), 1, None, _p(wide), 512, 4, 512, 0, ACT_NONE, 0.0, 1.0, _stream()), "K=0 wide")
    assert (wide == 0).all()
    # TN: M = 0 leaves C alone, K = 0 zeroes it
    c = torch.full((3, 512), 5.0, device=DEV)
    L.check(lib.recmv_gemm_tn(None, 3, None, 512, _p(c), 512, 0, 512, 7, None, 0, _stream()), "tn M=0")
    assert (c == 5.0).all()
    L.check(lib.recmv_gemm_tn(None, 3, None, 512, _p(c), 512, 3, 512, 0, None, 0, _stream()), "tn K=0")
    assert (c == 0).all()


# ------------------------------------------------------------------------------------------------ recmv_linear_backward
@pytest.mark.parametrize("N,act", [(3, ACT_RELU), (1, ACT_NONE)])
def test_linear_backward_skinny_layer(N, act):
    L, lib = _lib()
    M, K = 16421, 512
    x, W = _rand(M, K, seed=1), _rand(N, K, seed=2) * 0.13
    gy = _rand(M, N, seed=3)
    y = _rand(M, N, seed=4)                      # the layer's output: only its sign matters to ReLU'
    Wt = W.t().contiguous()
    ws = torch.empty(int(lib.recmv_linear_backward_workspace_bytes(M, N, K)), dtype=torch.uint8, device=DEV)
    gx, gW, gb = torch.full((M, K), NAN, device=DEV), torch.full((N, K), NAN, device=DEV), torch.full((N,), NAN, device=DEV)
    L.check(lib.recmv_linear_backward(_p(gy), N, _p(y), N, _p(x), K, _p(Wt), N, M, N, K, act, 0.0, _p(gx), K, _p(gW), _p(gb), _p(ws),
                                      ws.numel(), _stream()), "linear_backward")
    gz = gy.double() * ((y > 0).double() if act == ACT_RELU else 1.0)
    _check64(gx, gz @ W.double(), gz.abs() @ W.double().abs(), 1.0, "linear_backward gx N=%d" % N)
    _check64(gW, gz.t() @ x.double(), gz.abs().t() @ x.double().abs(), 1.0, "linear_backward gW N=%d" % N)
    _check64(gb, gz.sum(0), gz.abs().sum(0), 1.0, "linear_backward gb N=%d" % N)


# ------------------------------------------------------------------------------------------------ the route census
def test_routes_keep_the_slot_and_the_bits_of_the_census(monkeypatch):
    """Every case of gemm_route_cases under the default routes and under RECMV_GEMM_SKINNY=0 (the library reads it at every launch):
    the slot of a bracketing profile and the digest of the output's bits equal those recorded on an MI355X at the commit before the
    route planner (tests/golden/gemm_routes.json).  RECMV_GEMM_OCC=0 is read once per process: test_gpu_kernels.py runs it in a child."""
    census = json.loads((Path(__file__).resolve().parent / "golden" / "gemm_routes.json").read_text())["settings"]
    wrong = []
    for setting in ("default", "skinny0"):
        monkeypatch.delenv("RECMV_GEMM_SKINNY", raising=False)
        for k, v in GC.SETTINGS[setting].items():
            monkeypatch.setenv(k, v)
        assert sorted(census[setting]) == sorted(c["name"] for c in GC.CASES)
        for c in GC.CASES:
            want = census[setting][c["name"]]
            slot, out = GC.profiled_slot(c, DEV)
            got = GC.digest(out)
            print("%s %s: slot %d digest %s" % (setting, c["name"], slot, got))
            if slot != want["slot"] or got != want["digest"]:
                wrong.append((setting, c["name"], slot, want["slot"], got, want["digest"]))
    assert not wrong, wrong
