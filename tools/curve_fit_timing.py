"""Time of one step of the curve fit (`recmv.curves.fit_curves_to_loops`): the fused kernel step against its torch statement.

At the shape in use — S = 200 samples per curve, M = 2000 polyline points, 4 pairs — it times 200 steps after a warm-up, each
step the objective with its gradients plus the AdamW update, once with recmv_curve_fit_step (csrc/curve_tubes.hip) and once with
`fit_step_torch` differentiated by autograd, on the same GPU, alternating, and reports the median over the repeats of the
stream-synchronised wall time.  Also reports how far the two paths' curves are apart after those steps.

    python tools/curve_fit_timing.py [--out profiles/curve_fit_timing.json]
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))


def case(S, M, pairs, device):
    import torch
    from recmv import curves as fl
    g = torch.Generator().manual_seed(1)
    t = torch.linspace(0, 2 * math.pi, S + 1)[:-1]
    tm = torch.linspace(0, 2 * math.pi, M + 1)[:-1]
    rings, targets = [], []
    for k in range(pairs):
        r, y0 = 0.25 + 0.05 * k, 0.4 - 0.25 * k
        rings.append(torch.stack([r * torch.cos(t), 0.02 * torch.sin(3 * t) + y0, r * torch.sin(t)], -1).float())
        y = torch.stack([1.9 * r * torch.cos(tm), 0.02 * torch.sin(3 * tm) + y0, 1.9 * r * torch.sin(tm)], -1)
        targets.append((y + 0.002 * torch.randn(M, 3, generator=g)).float())
    names = ['curve%d' % k for k in range(pairs)]
    return (lambda: fl.Intersect_Free_Curve(rings, [0.9 * c for c in rings], names).to(device)), targets


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "curve_fit_timing.json"))
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    from recmv import curves as fl
    assert torch.cuda.is_available(), "curve_fit_timing.py measures on the GPU"
    dev = torch.device("cuda:0")
    make, targets = case(args.samples, args.points, args.pairs, dev)
    idx = list(range(args.pairs))

    def torch_step(c, tg, ti):
        loss = fl.fit_step_torch(c, tg, idx)
        g = torch.autograd.grad(loss.sum(), [c.scale, c.nx_scale])
        return loss.detach(), g[0], g[1]

    def run(step, iters):
        curve = make()
        fl.fit_curves_to_loops(curve, targets, idx, iters=args.warmup, step=step)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = fl.fit_curves_to_loops(curve, targets, idx, iters=iters, step=step)     # ends in a device-to-host read
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters, curve.inference(), info

    times = {"kernel": [], "torch": []}
    for _ in range(args.repeats):
        for name, step in (("kernel", None), ("torch", torch_step)):
            dt, pts, info = run(step, args.steps)
            times[name].append(dt)
            times[name + "_pts"], times[name + "_info"] = pts, info
    med = {k: statistics.median(times[k]) for k in ("kernel", "torch")}
    apart = float((times["kernel_pts"] - times["torch_pts"]).norm(dim=-1).max())
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "points": args.points, "pairs": args.pairs,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "kernel_step_seconds": med["kernel"], "torch_step_seconds": med["torch"],
           "kernel_step_seconds_all": times["kernel"], "torch_step_seconds_all": times["torch"],
           "torch_over_kernel": med["torch"] / med["kernel"],
           "projected_20000_steps_seconds": {"kernel": 20000 * med["kernel"], "torch": 20000 * med["torch"]},
           "curves_apart_after_steps": apart,
           "first_loss": times["kernel_info"]["first_loss"], "last_loss": times["kernel_info"]["last_loss"]}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
