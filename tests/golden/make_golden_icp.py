"""Golden vectors for the rigid fit, from the REAL reference class imported from /root/reference:

  icp_solver.npz
    engineer/optimizer/icp_optimzier.py `ICP_Optimizer.solver(source, target)` (:40-85) on 50 seeded float32 points: the
    target is the source under a rotation of 25 degrees about (2, -1, 3), a translation and noise of 1 %, so the fit is not
    exact.  The reference's solver is float32 only (its `torch.eye(3)` is; float64 input fails in the product) and
    subtracts the means from its arguments in place: it gets clones.  Stored: the inputs, R [3,3] and t [1,3].

    python tests/golden/make_golden_icp.py
"""
import math
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path[:0] = [str(REPO / "rec-mv_amd"), str(REPO)]
import ref_loader  # noqa: E402

ref_loader.install()
from make_golden import save  # noqa: E402


def main():
    torch.set_num_threads(1)
    ref_loader.ref_module("model.network")       # the reference's own entry order (its packages import each other)
    I = ref_loader.ref_module("engineer.optimizer.icp_optimzier")
    g = torch.Generator().manual_seed(41)
    source = (torch.rand(50, 3, generator=g) - 0.5) * torch.tensor([1.0, 0.6, 0.3]) + torch.tensor([0.2, -0.1, 0.4])
    axis = torch.tensor([2., -1., 3.]) / math.sqrt(14.)
    K = torch.tensor([[0., -axis[2], axis[1]], [axis[2], 0., -axis[0]], [-axis[1], axis[0], 0.]])
    a = math.radians(25.)
    R = torch.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    target = source @ R.T + torch.tensor([0.3, 0.1, -0.2]) + 0.01 * torch.randn(50, 3, generator=g)
    source, target = source.float().contiguous(), target.float().contiguous()
    opt = I.ICP_Optimizer(0)
    solve_R, solve_t = opt.solver(source.clone(), target.clone())
    assert solve_R.dtype == torch.float32 and abs(float(torch.det(solve_R)) - 1) < 1e-5
    save("icp_solver", source=source, target=target, R=solve_R, t=solve_t)


if __name__ == "__main__":
    main()
