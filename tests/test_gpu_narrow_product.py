"""The 64 x 32 product of the small launches (csrc/gemm_f32.hip): gemm_nt_narrow_kernel against the kernel it replaced.

RECMV_GEMM_NARROW=0 (read by the library at every launch) selects gemm_nt_narrow_v1_kernel, the kernel of the library before the
half-tile schedule.  Both keep, for every output element, two accumulation chains over K (k mod 32 < 16 and the rest) in ascending tile
order, within 8 consecutive k the order 0, 4, 1, 5, 2, 6, 3, 7, exact zeros past K, chain0 + chain1, then the bias, activation,
out_scale and the output transform — so every comparison below is torch.equal (the unwritten padding of C, poisoned with NaN, must
stay poisoned), on shapes that reach each edge of the staging:

  M in {1, 63, 64, 65, 200}      one row, a partial / whole / whole + 1 tile, several workgroups
  N in {5, 31, 32, 33, 512}      a partial float4 strip, a partial / whole / whole + 1 tile, the ray path's width
  K in {8, 32, 39, 40, 64, 72, 96, 104, 167, 512}
                                 1 to 16 K-tiles, a partial last tile, K % 4 != 0 (the unaligned instantiation), both LDS buffers as the
                                 last one and every position of the half-tile fragment ring
  act none / relu / softplus(100) / tanh, bias on and off, out_scale != 1, lda and ldc wider than the matrices, a base pointer moved by
  4 bytes, the operand transform (actgrad), the output transform (mulgrad), two weight sets split inside the row range (seg).

Every launch stays on the narrow route: N > 4 and K > 4 (the thin kernels take those) and at most 4 x 8 tiles of 64 x 64 (below 640).
One launch of each instantiation is also judged against float64 by the project's bound |err| <= 4e-7 * sum|a b| + 1e-6 on the
pre-activation (softplus(100) is 1-Lipschitz; the operand transform uses ReLU, whose derivative is exactly 0 or 1, so the bound is
that of the product of the transformed operand).
"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_TANH = 0, 1, 2, 3
ACTS = {"none": (ACT_NONE, 0.0), "relu": (ACT_RELU, 0.0), "softplus": (ACT_SOFTPLUS, 100.0), "tanh": (ACT_TANH, 0.0)}
MS = (1, 63, 64, 65, 200)
NS = (5, 31, 32, 33, 512)
KS = (8, 32, 39, 40, 64, 72, 96, 104, 167, 512)
MMAX, NMAX = max(MS), max(NS)


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
        os.environ.pop("RECMV_GEMM_NARROW", None)


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)


def _ld(K):
    """A row stride wider than K that keeps the alignment class of K: a multiple of 4 for K % 4 == 0, odd rows otherwise."""
    return K + 4 if K % 4 == 0 else K + 1


def _view(buf, rows, cols, ld, shift=0):
    """[rows, cols] with row stride ld inside the flat buffer `buf`, its first element `shift` floats into it."""
    return buf.as_strided((rows, cols), (ld, 1), shift)


def _both(launch, out):
    """`launch()` under the replaced kernel and under the kernel in use; `out` is poisoned before each.  -> (old, new)"""
    res = []
    for v in ("0", "1"):
        os.environ["RECMV_GEMM_NARROW"] = v
        out.fill_(float("nan"))
        launch()
        res.append(out.clone())
    os.environ.pop("RECMV_GEMM_NARROW", None)
    return res


def _same(old, new):
    """== on every element the launches wrote, and the poison still in place everywhere else, in both buffers."""
    return torch.equal(torch.nan_to_num(old, nan=12345.0), torch.nan_to_num(new, nan=12345.0))


@pytest.fixture(scope="module")
def operands():
    """One flat pool per operand, shared by every test and never written: views of every shape are cut from them."""
    kmax = max(KS) + 8
    return {
        "A": _rand(MMAX * kmax + 8, seed=1),
        "B": _rand(NMAX * kmax + 8, seed=2, scale=0.2),
        "B2": _rand(NMAX * kmax + 8, seed=3, scale=0.2),
        "Y": _rand(MMAX * (NMAX + 8) + 8, seed=4, scale=0.05).abs_(),       # y = act(z) >= 0, p y up to 5
        "bias": _rand(NMAX + 1, seed=5),
        "bias2": _rand(NMAX + 1, seed=6),
    }


def _plain(ops, M, N, K, act, param, bias, out_scale, shift=0):
    L, lib = _lib()
    lda = ldb = _ld(K)
    ldc = N + 3
    A, B = _view(ops["A"], M, K, lda, shift), _view(ops["B"], N, K, ldb, shift)
    out = torch.empty(M * ldc + 1, device=DEV)
    Cv = _view(out, M, N, ldc, shift)
    b = ops["bias"][shift:shift + N] if bias else None

    def launch():
        L.check(lib.recmv_gemm_nt(_p(A), lda, _p(B), ldb, _p(b), _p(Cv), ldc, M, N, K, act, param, out_scale, _stream()), "gemm_nt")
    return launch, out


@pytest.mark.parametrize("act", list(ACTS))
def test_same_bits_as_the_replaced_kernel(operands, act):
    """recmv_gemm_nt over the whole M x N x K grid, bias on and off, out_scale 0.75, lda / ldc wider than the matrices; K = 39 and 167
    take the unaligned instantiation (row strides 40 and 168 with K % 4 != 0)."""
    a, param = ACTS[act]
    bad = []
    for K in KS:
        for M in MS:
            for N in NS:
                for bias in (False, True):
                    launch, out = _plain(operands, M, N, K, a, param, bias, 0.75)
                    old, new = _both(launch, out)
                    if not _same(old, new):
                        bad.append((M, N, K, bias))
    assert not bad, f"(M, N, K, bias): {bad[:10]} ... {len(bad)} shapes"


def test_same_bits_with_the_base_pointers_moved_by_4_bytes(operands):
    """A, B, bias and C start 4 bytes into their buffers: no operand is 16-byte aligned, whatever K (the unaligned instantiation, dword
    staging loads and 4-byte stores)."""
    a, param = ACTS["softplus"]
    bad = []
    for K in KS:
        for M in (1, 65, 200):
            for N in (5, 33, 512):
                launch, out = _plain(operands, M, N, K, a, param, True, 0.75, shift=1)
                old, new = _both(launch, out)
                assert torch.isnan(out[0]) and torch.isnan(out[1 + (M - 1) * (N + 3) + N:]).all()   # nothing outside C is written
                if not _same(old, new):
                    bad.append((M, N, K))
    assert not bad, bad


@pytest.mark.parametrize("act", ["relu", "softplus", "tanh"])
def test_operand_and_output_transform_same_bits(operands, act):
    """recmv_gemm_nt_actgrad (A (.) act'(y_scale Y) g_scale while A is staged: Y [M, K]) and recmv_gemm_nt_mulgrad (the same factor
    on the output: Y [M, N])."""
    L, lib = _lib()
    a, param = ACTS[act]
    bad = []
    for K in KS:
        lda = ldb = _ld(K)
        for M in MS:
            for N in (5, 33, 512):
                ldc = N + 3
                A, B = _view(operands["A"], M, K, lda), _view(operands["B"], N, K, ldb)
                Yk, Yn = _view(operands["Y"], M, K, lda), _view(operands["Y"], M, N, N + 4)
                out = torch.empty(M * ldc, device=DEV)
                Cv = _view(out, M, N, ldc)

                def actgrad():
                    L.check(lib.recmv_gemm_nt_actgrad(_p(A), lda, _p(Yk), lda, _p(B), ldb, _p(Cv), ldc, M, N, K, a, param, 1.25, 0.5,
                                                      _stream()), "gemm_nt_actgrad")

                def mulgrad():
                    L.check(lib.recmv_gemm_nt_mulgrad(_p(A), lda, _p(B), ldb, _p(Cv), ldc, M, N, K, _p(Yn), N + 4, a, param, 1.25, 0.5,
                                                      _stream()), "gemm_nt_mulgrad")
                for name, fn in (("actgrad", actgrad), ("mulgrad", mulgrad)):
                    old, new = _both(fn, out)
                    if not _same(old, new):
                        bad.append((name, M, N, K))
    assert not bad, bad[:10]


def test_two_weight_sets_split_inside_the_rows_same_bits(operands):
    """recmv_gemm_nt_seg, 200 rows split at 128: the tiles of rows 0..127 multiply by B + bias, the others by B2 + bias2."""
    L, lib = _lib()
    a, param = ACTS["softplus"]
    M, split = 200, 128
    bad = []
    for K in KS:
        lda = ldb = _ld(K)
        for N in NS:
            ldc = N + 3
            A = _view(operands["A"], M, K, lda)
            B, B2 = _view(operands["B"], N, K, ldb), _view(operands["B2"], N, K, ldb)
            out = torch.empty(M * ldc, device=DEV)
            Cv = _view(out, M, N, ldc)

            def seg():
                L.check(lib.recmv_gemm_nt_seg(_p(A), lda, _p(B), ldb, _p(operands["bias"]), _p(B2), _p(operands["bias2"]), split, _p(Cv),
                                              ldc, M, N, K, a, param, 0.75, _stream()), "gemm_nt_seg")
            old, new = _both(seg, out)
            if not _same(old, new):
                bad.append((N, K))
            # and the second weight set is really used below the split
            launch, out1 = _plain(operands, M, N, K, a, param, True, 0.75)
            launch()
            one = _view(out1, M, N, ldc)
            assert torch.equal(_view(new, M, N, ldc)[:split], one[:split]) and not torch.equal(_view(new, M, N, ldc)[split:], one[split:])
    assert not bad, bad


@pytest.mark.parametrize("inst", ["aligned", "unaligned", "aligned_actgrad", "unaligned_actgrad"])
def test_each_instantiation_against_float64(operands, inst):
    """|C - float64| <= 4e-7 * sum|a b| + 1e-6 on the pre-activation, one launch of each instantiation of gemm_nt_narrow_kernel."""
    L, lib = _lib()
    M, N = 200, 33
    K = 104 if inst.startswith("aligned") else 167
    lda = ldb = _ld(K)
    A, B = _view(operands["A"], M, K, lda), _view(operands["B"], N, K, ldb)
    out = torch.empty(M, N, device=DEV)
    if inst.endswith("actgrad"):
        Y = _view(operands["A"], M, K, lda, 8)             # signed: ReLU's derivative takes both values
        L.check(lib.recmv_gemm_nt_actgrad(_p(A), lda, _p(Y), lda, _p(B), ldb, _p(out), N, M, N, K, ACT_RELU, 0.0, 1.25, 0.5, _stream()),
                "gemm_nt_actgrad")
        a64 = A.double() * (Y.double() > 0).double() * 0.5
        ref = a64 @ B.double().T
        bound = 4e-7 * (a64.abs() @ B.double().abs().T) + 1e-6
    else:
        bias = operands["bias"][:N]
        L.check(lib.recmv_gemm_nt(_p(A), lda, _p(B), ldb, _p(bias), _p(out), N, M, N, K, ACT_SOFTPLUS, 100.0, 1.0, _stream()), "gemm_nt")
        z = A.double() @ B.double().T + bias.double()
        ref = torch.where(z * 100 > 20, z, torch.log1p(torch.exp(torch.clamp(z * 100, max=20.0))) / 100)
        bound = 4e-7 * (A.double().abs() @ B.double().abs().T + bias.double().abs()) + 1e-6
    err = (out.double() - ref).abs()
    worst = (err / bound).max().item()
    print(f"{inst}: M={M} N={N} K={K} max err {err.max().item():.3e}, max err / bound {worst:.3f}")
    assert worst <= 1.0
