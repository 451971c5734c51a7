"""engineer/optimizer/icp_optimzier.py (reference; the file name is the reference's): `ICP_Optimizer`, one closed-form rigid
fit of a source point set to its nearest neighbours in a target point set.

`solver(source, target)` is the reference's: the rotation R and translation t that minimise sum |R source_i + t - target_i|^2,
R = V diag(1, 1, det(V U^T)) U^T from the SVD of the centred covariance, `new_source = (R @ source.T).T + t`.  Here it is
recmv.align.solve_point on float64 sums of the pairs, and — unlike the reference, whose solver subtracts the means from its
arguments IN PLACE — it leaves `source` and `target` unchanged.  `fitting(inputs)` is the reference's single step: the
boundary points of `inputs['smpl_slice']` and `inputs['target_polygon']` (any objects with the reference's `get_fields()`,
`get_boundary(*fields)` and `transform_R_t(R, t)`), every source point's nearest target point by recmv_knn1 (the reference:
pytorch3d `knn_points`), the solver, the sum of squared distances after the step, and `transform_R_t` on the source.
"""
import numpy as np
import torch

from ... import align, nricp


def pair_sums(source, target):
    """recmv.align's sums 0 .. 18 about the origin for the pairs (source_i, target_i), in float64 on the tensors' device
    (entries 19 .. 55 zero): what recmv_icp_accumulate gives without a plane part when every pair is accepted."""
    u, w = source.double(), target.double()
    sums = torch.zeros(align.N_SUMS, dtype=torch.float64, device=source.device)
    sums[0] = u.shape[0]
    sums[1:4], sums[4:7] = u.sum(0), w.sum(0)
    sums[7:16] = (u.T @ w).reshape(-1)
    sums[16], sums[17], sums[18] = (u * u).sum(), (w * w).sum(), ((u - w) ** 2).sum()
    return sums


class ICP_Optimizer:
    """`ICP_Optimizer(epoch, optimizer_setting=None)`; `__call__(**inputs)` -> the loss of `fitting(inputs)`."""

    def __init__(self, epoch, optimizer_setting=None):
        self.name = "ICP_Optimizer"
        self.epoch = epoch
        self.optimizier_setting = optimizer_setting      # (the reference's spelling of its base class's attribute)
        self.energy_func = lambda x, y: torch.sum((x - y) ** 2)

    def __call__(self, **inputs):
        return self.fitting(inputs)

    def solver(self, source, target):
        """(R [3,3], t [1,3]) in the dtype and on the device of `source` [N,3], for target [N,3]."""
        if source.dim() != 2 or source.shape[1] != 3 or source.shape != target.shape:
            raise ValueError("ICP_Optimizer.solver: source and target must both be [N,3]")
        _, R, t = align.solve_point(pair_sums(source.detach(), target.detach()), False)
        return (torch.as_tensor(np.ascontiguousarray(R), dtype=source.dtype, device=source.device),
                torch.as_tensor(t[None], dtype=source.dtype, device=source.device))

    def _collect_data(self, inputs):
        smpl_slice, target_polygon = inputs['smpl_slice'], inputs['target_polygon']
        fields = target_polygon.get_fields()
        target = target_polygon.get_boundary(*fields)
        source = smpl_slice.get_boundary(*fields)
        return torch.cat(list(source), dim=0), torch.cat(list(target), dim=0)

    @torch.no_grad()
    def fitting(self, inputs):
        source, target = self._collect_data(inputs)
        idx, _ = nricp.knn1(source.float().contiguous(), target.float().contiguous())
        target = target[idx]
        R, t = self.solver(source, target)
        new_source = (R @ source.T).T + t
        loss = self.energy_func(new_source, target)
        inputs['smpl_slice'].transform_R_t(R, t)
        return loss
