"""Time of one ICP iteration (recmv.align.icp) at the evaluation's size: 1e5 surface samples of a mesh of about 160 000 faces
against that mesh moved by a small similarity, split into its three parts
  search       x = s p R^T + t and the exact closest point through a grid built before (MeshGrid.closest_point)
  accumulate   recmv_icp_accumulate (align.icp_sums, plane part and border flags included) and the read-back of the 56 sums
  solve        align.solve_plane on the host
and the accumulate step against the same sums written in plain torch float64 on the same card (`torch_sums` below: the same
acceptance rules, the region of the point-triangle test from iso_remesh._closest_st, gathers and reductions of torch).  The two
alternate inside one process, repeat by repeat, after a warm-up of each; every sample is a host clock around work that ends in
the read-back of the sums.  The file also holds the largest difference between the two results relative to the sum of
magnitudes.  No threshold hangs on these numbers.

    python tools/icp_timing.py [--samples 100000] [--lat 200] [--reps 20] [--out profiles/icp_timing.json]
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


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _stats(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def bumpy_ellipsoid(lat, device):
    """A closed latitude-longitude mesh of 4 lat (lat - 1) faces with unequal axes and a smooth bump: (verts f32, faces)."""
    import torch
    lon = 2 * lat
    th = torch.linspace(0, math.pi, lat + 1, dtype=torch.float64)[1:-1]
    ph = torch.linspace(0, 2 * math.pi, lon + 1, dtype=torch.float64)[:-1]
    T, Pp = torch.meshgrid(th, ph, indexing="ij")
    ring = torch.stack([T.sin() * Pp.cos(), T.sin() * Pp.sin(), T.cos()], -1).reshape(-1, 3)
    v = torch.cat([ring, torch.tensor([[0., 0., 1.], [0., 0., -1.]], dtype=torch.float64)])
    v = v * (1 + 0.06 * torch.sin(3 * v[:, 0:1] + 1) * torch.cos(2 * v[:, 1:2])) * torch.tensor([0.5, 0.35, 0.225], dtype=torch.float64)
    i = torch.arange(lat - 2)[:, None] * lon + torch.arange(lon)[None, :]
    j = torch.arange(lat - 2)[:, None] * lon + (torch.arange(lon)[None, :] + 1) % lon
    quads = torch.cat([torch.stack([i, i + lon, j], -1), torch.stack([j, i + lon, j + lon], -1)]).reshape(-1, 3)
    top, bot = ring.shape[0], ring.shape[0] + 1
    k, k1 = torch.arange(lon), (torch.arange(lon) + 1) % lon
    last = (lat - 2) * lon
    caps = torch.cat([torch.stack([torch.full_like(k, top), k, k1], -1), torch.stack([torch.full_like(k, bot), last + k1, last + k], -1)])
    return v.float().to(device).contiguous(), torch.cat([quads, caps]).long().to(device).contiguous()


def torch_sums(x, q, face, dist2, verts, faces, border, max_dist2, centre):
    """recmv_icp_accumulate with with_plane = 1 in plain torch, float64 [56] on the device."""
    import torch
    from recmv import iso_remesh
    F, V = faces.shape[0], verts.shape[0]
    ok = (face >= 0) & (face < F)
    idx = faces[face.clamp(0, F - 1)]
    ok &= ((idx >= 0) & (idx < V)).all(1) & torch.isfinite(x).all(1) & torch.isfinite(q).all(1) & torch.isfinite(dist2)
    if max_dist2 is not None:
        ok &= dist2 <= max_dist2
    idx = idx.clamp(0, V - 1)
    a, b, c = verts[idx[:, 0]], verts[idx[:, 1]], verts[idx[:, 2]]
    if border is not None:
        s, t, _ = iso_remesh._closest_st(x, a, b - a, c - a)
        on_ab, on_ac, on_bc = t == 0, s == 0, (s > 0) & (t > 0) & (s + t >= 1)
        bits = border[face.clamp(0, F - 1)].long()
        # vertex a / b / c: two of the three; otherwise the one edge
        region = torch.where(on_ab & on_ac, 3, torch.where(on_ab & (s == 1), 4, torch.where(on_ac & (t == 1), 5, torch.where(
            on_ab, 0, torch.where(on_ac, 1, torch.where(on_bc, 2, 6))))))
        ok &= ((bits >> region.clamp(max=5)) & 1 == 0) | (region == 6)
    a, b, c = a.double(), b.double(), c.double()
    m = torch.linalg.cross(b - a, c - a, dim=-1)
    ln = m.norm(dim=1, keepdim=True)
    ok &= (ln[:, 0] > 0) & torch.isfinite(ln[:, 0])
    k = ok.double()[:, None]
    cen = torch.tensor(centre, dtype=torch.float64, device=x.device)
    u = torch.nan_to_num(x.double() - cen) * k
    w = torch.nan_to_num(q.double() - cen) * k
    m = torch.nan_to_num(m / ln) * k
    e = u - w
    J = torch.cat([torch.linalg.cross(u, m, dim=-1), m, (u * m).sum(1, keepdim=True)], 1)
    r = (e * m).sum(1)
    iu = torch.triu_indices(7, 7, device=x.device)
    return torch.cat([k.sum().reshape(1), u.sum(0), w.sum(0), (u.T @ w).reshape(-1), (u * u).sum().reshape(1),
                      (w * w).sum().reshape(1), (e * e).sum().reshape(1), (J.T @ J)[iu[0], iu[1]], J.T @ r,
                      (r * r).sum().reshape(1), torch.zeros(1, dtype=torch.float64, device=x.device)])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--lat", type=int, default=200, help="latitude bands of the mesh: 4 lat (lat - 1) faces")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from recmv import align, metrics
    dev = torch.device("cuda:0")
    v, f = bumpy_ellipsoid(args.lat, dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    p = metrics.sample_surface(v, f, args.samples, gen)[0].contiguous()
    a = math.radians(2.)
    M = torch.tensor([[math.cos(a), -math.sin(a), 0.], [math.sin(a), math.cos(a), 0.], [0., 0., 1.]], device=dev) * 1.01
    t = torch.tensor([0.004, -0.003, 0.002], device=dev)
    grid = metrics.MeshGrid(v, f)
    border = align.border_flags(f, v.shape[0])
    centre = (0.5 * (v.amin(0) + v.amax(0))).double().cpu().tolist()
    limit = torch.tensor([0.05 ** 2], dtype=torch.float32, device=dev)

    def search():
        return grid.closest_point(p @ M.T + t)

    x = p @ M.T + t
    face, q, d2 = search()

    def hip():
        return align.icp_sums(x, q, face, d2, v, f, border=border, max_dist2=limit, centre=centre, plane=True).cpu()

    def plain():
        return torch_sums(x, q, face, d2, v, f, border, limit, centre).cpu()
    s_hip, s_torch = hip(), plain()                        # warm-up of both, and the comparison
    search()
    scale = torch.maximum(s_hip.abs(), s_torch.abs()).clamp(min=1e-300)
    t_search, t_hip, t_torch, t_solve = [], [], [], []
    for _ in range(args.reps):                             # alternated, repeat by repeat
        t_search.append(_clock(search)[0])
        t_hip.append(_clock(hip)[0])
        t_torch.append(_clock(plain)[0])
        t0 = time.perf_counter()
        align.solve_plane(s_hip, True)
        t_solve.append(time.perf_counter() - t0)
    res = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "faces": int(f.shape[0]), "reps": args.reps,
           "accepted": int(s_hip[0]), "search": _stats(t_search), "accumulate_hip": _stats(t_hip),
           "accumulate_torch_float64": _stats(t_torch), "solve_host": _stats(t_solve),
           "same_count": bool(s_hip[0] == s_torch[0]),
           "largest_relative_difference": float(((s_hip - s_torch).abs() / scale).max()),
           "hip_over_torch_median": statistics.median(t_hip) / statistics.median(t_torch)}
    res["faster"] = "hip" if res["hip_over_torch_median"] < 1 else "torch"
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
