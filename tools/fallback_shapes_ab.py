"""Old route against new route for the shapes of profiles/r07_fallback_shapes.txt, one process, hipGraph replay.

    python tools/fallback_shapes_ab.py > profiles/r07_fallback_shapes_ab.txt

RECMV_GEMM_SKINNY is read by the library at every launch: "0" gives a launch the route it had before the skinny and the SCAL
kernels (gemm_nt_kernel<2, false, ...> / gemm_tn_kernel<false>, or the aligned high-occupancy kernel for the N <= 4 forward), anything
else the new one.  The route is fixed when the graph is captured.  Each shape: 20 launches per graph, 5 replays, old / new / old / new;
the table shows the smaller of the two times of each route.  The TN rows include the split-K reduction pass.
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
# (kind, M, N, K, lda, ldb) — NT: C[M,N] = A[M,K] B[N,K]^T; TN: C[M,N] = A[K,M]^T B[K,N]
SHAPES = [
    ("nt", 226309, 512, 39, 40, 39), ("nt", 68921, 512, 39, 40, 39), ("nt", 35836, 512, 39, 40, 39), ("nt", 17072, 512, 39, 40, 39),
    ("nt", 134364, 512, 167, 168, 167), ("nt", 27716, 512, 167, 168, 167),
    ("nt", 87998, 512, 473, 476, 473), ("nt", 35836, 512, 473, 512, 473), ("nt", 17072, 512, 473, 512, 473),
    ("nt", 263994, 3, 512, 512, 512), ("nt", 100773, 3, 512, 512, 512), ("nt", 72754, 3, 512, 512, 512),
    ("nt", 263994, 512, 3, 3, 3), ("nt", 100773, 512, 3, 3, 3), ("nt", 72754, 512, 3, 3, 3),
    ("tn", 3, 512, 263994, 3, 512), ("tn", 3, 512, 100773, 3, 512), ("tn", 3, 512, 72754, 3, 512),
    ("tn", 512, 289, 3069, 512, 289), ("tn", 257, 512, 8959, 257, 512), ("tn", 257, 512, 3051, 257, 512),
]


def p(t):
    return C.c_void_p(t.data_ptr())


def main():
    lib = L.lib()
    L.set_gemm_mode(0)
    stream = lambda: L.stream_ptr(torch.device(DEV))  # noqa: E731
    new_mode = "1"
    print("# old route (RECMV_GEMM_SKINNY=0) against new route, us per launch, hipGraph replay; speed-up = old / new")
    print("# %-4s %8s %5s %7s %5s %5s %10s %10s %8s" % ("kind", "M", "N", "K", "lda", "ldb", "old_us", "new_us", "speed-up"))
    for kind, M, N, K, lda, ldb in SHAPES:
        if kind == "nt":
            A = torch.randn(M, lda, device=DEV)[:, :K]
            B = torch.randn(N, ldb, device=DEV)[:, :K] * 0.1
            out = torch.empty(M, N, device=DEV)

            def fn():
                L.check(lib.recmv_gemm_nt(p(A), lda, p(B), ldb, None, p(out), N, M, N, K, 0, 0.0, 1.0, stream()), "gemm_nt")
        else:
            A = torch.randn(K, lda, device=DEV)[:, :M]
            B = torch.randn(K, ldb, device=DEV)[:, :N]
            out = torch.empty(M, N, device=DEV)
            ws = torch.empty(int(lib.recmv_gemm_tn_workspace_bytes(M, N, K)), dtype=torch.uint8, device=DEV)

            def fn():
                L.check(lib.recmv_gemm_tn(p(A), lda, p(B), ldb, p(out), N, M, N, K, p(ws), ws.numel(), stream()), "gemm_tn")
        t = {"0": [], new_mode: []}
        for _ in range(2):
            for mode in ("0", new_mode):
                os.environ["RECMV_GEMM_SKINNY"] = mode
                t[mode].append(_graph_time(fn)[0] * 1e6)
        old, new = min(t["0"]), min(t[new_mode])
        print("  %-4s %8d %5d %7d %5d %5d %10.1f %10.1f %8.2f" % (kind, M, N, K, lda, ldb, old, new, old / new), flush=True)
    os.environ.pop("RECMV_GEMM_SKINNY", None)


if __name__ == "__main__":
    main()
