"""The shapes of the GEMM route census (tests/golden/gemm_routes.json): one list, read by the generator
tests/golden/make_golden_gemm_routes.py, by tests/test_gemm_route_cpu.py and by tests/test_gpu_skinny_products.py.

A case is a dict: name, entry (nt | actgrad | mulgrad | seg | mulgrad_seg | tn), M, N, K, lda, ldb, a_shift (floats the base of A
lies off a 16-byte boundary) and split_row (seg entries).  NT: C[M,N] = A[M,K] . B[N,K]^T; TN: C[M,N] = A[K,M]^T . B[K,N].
K is small so that a case runs in milliseconds; the row counts are what the routes' thresholds are written in.

`run_case` launches one case on the GPU and returns its output; `digest` hashes the output's bit patterns on the device.
Operands are seeded CPU torch.rand in [-1, 1); no activation, a bias where the entry point takes one: a pure fma chain.
"""
import ctypes as C

SETTINGS = {"default": {}, "skinny0": {"RECMV_GEMM_SKINNY": "0"}, "occ0": {"RECMV_GEMM_OCC": "0"}}
N_SLOTS = 14


def _case(name, entry, M, N, K, lda=None, ldb=None, a_shift=0, split_row=0):
    tn = entry == "tn"
    return dict(name=name, entry=entry, M=M, N=N, K=K, lda=(M if tn else K) if lda is None else lda,
                ldb=(N if tn else K) if ldb is None else ldb, a_shift=a_shift, split_row=split_row)


def _cases():
    out = []
    # NT, aligned: the two sides of the 2.5-per-CU rule, of the 512-tile rule and of the 3600-tile rule
    for entry in ("nt", "actgrad"):
        for M, N, K in ((20416, 128, 16), (20417, 128, 16), (65408, 128, 16), (65409, 128, 16), (115072, 512, 8), (115073, 512, 8)):
            out.append(_case("%s_aligned_M%d_N%d" % (entry, M, N), entry, M, N, K))
    # NT, unaligned
    for M, N in ((66000, 512), (115200, 512), (20000, 128), (30000, 128)):
        out.append(_case("nt_k39_M%d_N%d" % (M, N), "nt", M, N, 39))
    out.append(_case("nt_k40_base_off_4_bytes", "nt", 66000, 512, 40, a_shift=1))
    # NT, thin K (rows 8 floats apart; K = 5 is the first K past the thin route)
    for K in (1, 3, 4, 5):
        out.append(_case("nt_thin_k%d" % K, "nt", 66000, 512, K, lda=8, ldb=8))
    out.append(_case("nt_thin_k3_lda3", "nt", 66000, 512, 3))
    out.append(_case("actgrad_thin_k4", "actgrad", 66000, 512, 4))
    # NT, thin N: the two sides of the order rule, then N past the thin route, the output transform (thin) and the operand transform (not)
    for M in (40896, 40897):
        out.append(_case("nt_thin_n4_M%d" % M, "nt", M, 4, 1024))
    for N in (1, 3, 4, 5):
        out.append(_case("nt_thin_n%d" % N, "nt", 66000, N, 512))
    out.append(_case("mulgrad_thin_n3", "mulgrad", 66000, 3, 512))
    out.append(_case("actgrad_n3", "actgrad", 66000, 3, 512))
    # NT, two nets over one row block
    for entry in ("seg", "mulgrad_seg"):
        out.append(_case("%s_occ" % entry, entry, 66000, 512, 16, split_row=128 * 100))
        out.append(_case("%s_thin_n3" % entry, entry, 66000, 3, 512, split_row=128 * 100))
    # TN
    for M, N in ((3, 512), (512, 3), (4, 512), (5, 512), (512, 512)):
        out.append(_case("tn_%dx%d" % (M, N), "tn", M, N, 66000))
    out.append(_case("tn_257x289_ldb289", "tn", 257, 289, 66000))
    out.append(_case("tn_512x512_base_off_4_bytes", "tn", 512, 512, 66000, a_shift=1))
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _cases()


def host_line(c, setting, mode=0, families=7):
    """The case as one input line of tools/gemm_route_host_check: the alignment flags the entry points derive from the pointers and
    leading dimensions (run_case below allocates every operand and the result 16-byte aligned, A `a_shift` floats further; ldc = N;
    the Y of actgrad lies like A), then the switches of `setting`."""
    occ, skinny = int(SETTINGS[setting].get("RECMV_GEMM_OCC", "1") != "0"), int(SETTINGS[setting].get("RECMV_GEMM_SKINNY", "1") != "0")
    a_vec, b_vec = int(c["a_shift"] % 4 == 0 and c["lda"] % 4 == 0), int(c["ldb"] % 4 == 0)
    e = c["entry"]
    if e == "tn":
        return "tn %s %d %d %d %d %d %d %d %d %d %d %d" % (c["name"], c["M"], c["N"], c["K"], c["lda"], c["ldb"], a_vec, b_vec, mode, families,
                                                          occ, skinny)
    flags = (a_vec, b_vec, int(c["N"] % 4 == 0), int(e == "actgrad"), int(e in ("mulgrad", "mulgrad_seg")), int(e in ("seg", "mulgrad_seg")),
             int(c["lda"] >= c["K"]))
    return "nt %s %d %d %d %s %d %d %d %d" % (c["name"], c["M"], c["N"], c["K"], " ".join(map(str, flags)), mode, families, occ, skinny)


# ------------------------------------------------------------------------------------------------ running a case (GPU)
_pool = {}


def _rand(rows, cols, seed, dev):
    """rows x cols of seeded CPU torch.rand in [-1, 1) on the device; built once per (shape, seed) and never modified."""
    import torch
    key = (rows, cols, seed, dev)
    if key not in _pool:
        g = torch.Generator(device="cpu").manual_seed(seed)
        _pool[key] = (torch.rand(rows, cols, generator=g) * 2 - 1).to(dev)
    return _pool[key]


def _placed(t, ld, shift, dev):
    """The 2-D tensor in a fresh buffer with row stride `ld`, its base `shift` floats off the allocation's (16-byte aligned) start."""
    import torch
    rows, cols = t.shape
    if ld == cols and shift == 0:
        return t
    flat = torch.zeros(rows * ld + shift + 8, device=dev)
    view = flat[shift:shift + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    return view


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def run_case(c, dev="cuda:0"):
    """Launch the case's product on the current stream of `dev`; returns the [M, N] output."""
    import torch
    from recmv import _lib as L
    lib, s = L.lib(), L.stream_ptr(torch.device(dev))
    M, N, K, e = c["M"], c["N"], c["K"], c["entry"]
    out = torch.full((M, N), float("nan"), device=dev)
    if e == "tn":
        A = _placed(_rand(K, M, 1000 + M, dev), c["lda"], c["a_shift"], dev)
        B = _placed(_rand(K, N, 2000 + N, dev), c["ldb"], 0, dev)
        ws = torch.empty(int(lib.recmv_gemm_tn_workspace_bytes(M, N, K)), dtype=torch.uint8, device=dev)
        L.check(lib.recmv_gemm_tn(_p(A), c["lda"], _p(B), c["ldb"], _p(out), N, M, N, K, _p(ws), ws.numel(), s), c["name"])
        return out
    # one pool of rows per K: a case takes the first M
    rows = max(x["M"] for x in CASES if x["entry"] != "tn" and x["K"] == K)
    A = _placed(_rand(rows, K, 3000 + K, dev)[:M], c["lda"], c["a_shift"], dev)
    B, B2 = (_placed(_rand(N, K, sd + 7 * N + K, dev), c["ldb"], 0, dev) for sd in (4000, 5000))
    bias, bias2 = (_rand(1, N, sd + N, dev).reshape(-1) for sd in (6000, 7000))
    lda, ldb, sr = c["lda"], c["ldb"], c["split_row"]
    if e == "nt":
        rc = lib.recmv_gemm_nt(_p(A), lda, _p(B), ldb, _p(bias), _p(out), N, M, N, K, 0, 0.0, 1.0, s)
    elif e == "seg":
        rc = lib.recmv_gemm_nt_seg(_p(A), lda, _p(B), ldb, _p(bias), _p(B2), _p(bias2), sr, _p(out), N, M, N, K, 0, 0.0, 1.0, s)
    elif e == "actgrad":                                   # act = none: the operand transform multiplies by g_scale alone
        Y = _placed(_rand(rows, K, 8000 + K, dev)[:M], lda, c["a_shift"], dev)
        rc = lib.recmv_gemm_nt_actgrad(_p(A), lda, _p(Y), lda, _p(B), ldb, _p(out), N, M, N, K, 0, 0.0, 1.0, 0.75, s)
    else:
        Y = _rand(M, N, 9000 + N, dev)
        if e == "mulgrad":
            rc = lib.recmv_gemm_nt_mulgrad(_p(A), lda, _p(B), ldb, _p(out), N, M, N, K, _p(Y), N, 0, 0.0, 1.0, 0.75, s)
        else:
            rc = lib.recmv_gemm_nt_mulgrad_seg(_p(A), lda, _p(B), _p(B2), sr, ldb, _p(out), N, M, N, K, _p(Y), N, 0, 0.0, 1.0, 0.75, s)
    L.check(rc, c["name"])
    return out


def profiled_slot(c, dev="cuda:0"):
    """(the profile slot that received the case's one product launch, the output): a bracketing profile of every launch."""
    import torch
    from recmv import _lib as L
    lib = L.lib()
    buf = (C.c_double * (5 * N_SLOTS))()
    L.check(lib.recmv_profile_begin(0.0), "profile_begin")
    try:
        out = run_case(c, dev)
    finally:
        L.check(lib.recmv_profile_end(C.cast(buf, C.c_void_p), N_SLOTS), "profile_end")
    hits = [v for v in range(N_SLOTS) if buf[5 * v] or buf[5 * v + 3]]
    assert len(hits) == 1 and buf[5 * hits[0]] == 1.0, "%s: launches per slot %s" % (c["name"], [buf[5 * v] for v in range(N_SLOTS)])
    return hits[0], out


def _i64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= 1 << 63 else x


def digest(out):
    """A position-dependent 64-bit digest of the tensor's bit patterns, on the tensor's device (int64 arithmetic wraps mod 2^64):
    sum_i mix((bits_i + 1) * (2 i + 1) * c1) * c2 with mix(h) = h ^ (h >> 31).  Returned as 16 hex digits."""
    import torch
    bits = out.contiguous().view(torch.int32).reshape(-1).to(torch.int64) & 0xffffffff
    idx = torch.arange(bits.numel(), device=out.device, dtype=torch.int64)
    h = (bits + 1) * ((2 * idx + 1) * _i64(0x9E3779B97F4A7C15))
    h = h ^ (h >> 31)
    return "%016x" % (int((h * _i64(0xD6E8FEB86659FD93)).sum().item()) & ((1 << 64) - 1))
