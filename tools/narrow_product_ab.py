"""The 64 x 32 product: the replaced kernel (RECMV_GEMM_NARROW=0, gemm_nt_narrow_v1_kernel) against the kernel in use, per shape.

    python tools/narrow_product_ab.py > profiles/narrow_product_ab.txt

One process, hipGraph replay.  RECMV_GEMM_NARROW is read by the library at every launch, so the kernel is fixed when the graph is
captured.  Each timing: 20 launches per graph, 5 replays; old / new take turns three times and the table shows the smallest time of
each, with the spread (max - min) of the three old timings: a new time above old + spread is a loss.
Shapes: the surface root finder's (RECMV_GEMM_SHAPES=1 run of the bench: 1.5 k - 3.1 k rows against 512 outputs, K = 512 hidden, 40 /
39 first layer, 167 / 473 skip layers; plain with softplus, output transform, operand transform) and the N = 128 shapes of the
route census (tests/gemm_route_cases.py).
"""
import ctypes as C
import os
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(REPO))
from bench import _graph_time  # noqa: E402
from recmv import _lib as L  # noqa: E402

DEV = "cuda:0"
ACT_SOFTPLUS = 2
# (entry, M, N, K, lda)
SHAPES = [(e, M, 512, 512, 512) for M in (1536, 2560, 3072) for e in ("nt", "mulgrad", "actgrad")]
SHAPES += [("nt", M, 512, K, lda) for M in (1536, 3072) for K, lda in ((40, 40), (39, 40), (39, 39), (167, 168), (473, 476))]
SHAPES += [("mulgrad", 3072, 512, 40, 40), ("actgrad", 3072, 512, 167, 168), ("actgrad", 3072, 512, 473, 476)]
SHAPES += [("nt", 20416, 128, 16, 16), ("actgrad", 20416, 128, 16, 16), ("nt", 20000, 128, 39, 39)]


def p(t):
    return C.c_void_p(t.data_ptr())


def main():
    lib = L.lib()
    L.set_gemm_mode(0)
    stream = lambda: L.stream_ptr(torch.device(DEV))  # noqa: E731
    print("# replaced kernel (RECMV_GEMM_NARROW=0) against the kernel in use, us per launch, hipGraph replay; speed-up = old / new")
    print("# %-8s %6s %4s %4s %4s %9s %9s %10s %8s %s" % ("entry", "M", "N", "K", "lda", "old_us", "new_us", "old_spread", "speed-up", ""))
    worst = 0.0
    for entry, M, N, K, lda in SHAPES:
        A = torch.randn(M, lda, device=DEV)[:, :K]
        B = torch.randn(N, lda, device=DEV)[:, :K] * 0.1
        bias = torch.randn(N, device=DEV)
        Yk = torch.rand(M, lda, device=DEV)[:, :K] * 0.05
        Yn = torch.rand(M, N, device=DEV) * 0.05
        out = torch.empty(M, N, device=DEV)
        if entry == "nt":
            def fn():
                L.check(lib.recmv_gemm_nt(p(A), lda, p(B), lda, p(bias), p(out), N, M, N, K, ACT_SOFTPLUS, 100.0, 1.0, stream()), entry)
        elif entry == "mulgrad":
            def fn():
                L.check(lib.recmv_gemm_nt_mulgrad(p(A), lda, p(B), lda, p(out), N, M, N, K, p(Yn), N, ACT_SOFTPLUS, 100.0, 1.0, 1.0,
                                                  stream()), entry)
        else:
            def fn():
                L.check(lib.recmv_gemm_nt_actgrad(p(A), lda, p(Yk), lda, p(B), lda, p(out), N, M, N, K, ACT_SOFTPLUS, 100.0, 1.0, 1.0,
                                                  stream()), entry)
        t = {"0": [], "1": []}
        for _ in range(3):
            for mode in ("0", "1"):
                os.environ["RECMV_GEMM_NARROW"] = mode
                t[mode].append(_graph_time(fn)[0] * 1e6)
        old, new, spread = min(t["0"]), min(t["1"]), max(t["0"]) - min(t["0"])
        lost = new > old + spread
        worst = max(worst, new - old - spread)
        print("  %-8s %6d %4d %4d %4d %9.2f %9.2f %10.2f %8.3f %s" % (entry, M, N, K, lda, old, new, spread, old / new, "SLOWER" if lost else ""),
              flush=True)
    os.environ.pop("RECMV_GEMM_NARROW", None)
    print("# shapes slower than old + spread: %s" % ("none" if worst <= 0 else "see SLOWER rows"))


if __name__ == "__main__":
    main()
