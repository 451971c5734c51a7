"""NR-ICP registration of a garment template (engineer/optimizer/nricp_optimizer.py:35-112, 242-452 of the reference):
`Local_Affine` and `NRICP_Optimizer_AdamW` with the reference's constructor arguments, defaults, schedule and log line.

Two paths compute the same fit:
  * kernels (default on the GPU): recmv.nricp.knn1 once per epoch and recmv.nricp.NricpEnergy once per inner iteration,
    which writes the loss and the gradients of A and b into `.grad`; torch's AdamW steps.  No host synchronisation
    inside an epoch.
  * torch (`use_kernels=False`, and always on the CPU): the reference restated line by line with autograd — the test
    oracle and the CPU fallback.
Static points (`static_pts_type`) are not supported: the registration always passes none.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import nricp as K
from ...nricp import TriMesh


def _inv3x3_torch(A):
    """Fast3x3Minv in plain torch (cofactors, |det| < 1e-4 -> zero matrix and check False)."""
    m = A.reshape(-1, 9)
    c00 = m[:, 4] * m[:, 8] - m[:, 5] * m[:, 7]
    c01 = -m[:, 3] * m[:, 8] + m[:, 5] * m[:, 6]
    c02 = m[:, 3] * m[:, 7] - m[:, 4] * m[:, 6]
    c10 = -m[:, 1] * m[:, 8] + m[:, 2] * m[:, 7]
    c11 = m[:, 0] * m[:, 8] - m[:, 2] * m[:, 6]
    c12 = -m[:, 0] * m[:, 7] + m[:, 1] * m[:, 6]
    c20 = m[:, 1] * m[:, 5] - m[:, 2] * m[:, 4]
    c21 = -m[:, 0] * m[:, 5] + m[:, 2] * m[:, 3]
    c22 = m[:, 0] * m[:, 4] - m[:, 1] * m[:, 3]
    det = m[:, 0] * c00 + m[:, 1] * c01 + m[:, 2] * c02
    ok = det.double().abs() >= 1e-4
    inv = torch.stack([c00, c10, c20, c01, c11, c21, c02, c12, c22], 1) / det[:, None]
    inv = torch.where(ok[:, None], inv, torch.zeros_like(inv))
    return inv.view(-1, 3, 3), ok


def inv3x3(A):
    if A.is_cuda:
        from ...FastMinv import Fast3x3Minv
        return Fast3x3Minv(A.contiguous())
    return _inv3x3_torch(A)


class Local_Affine(nn.Module):
    """A per-vertex affine map (A [B,N,3,3], b [B,N,3,1]) with its edge stiffness (nricp_optimizer.py:35-112)."""

    def __init__(self, num_points, batch_size=1, edges=None, gamma=1):
        super().__init__()
        self.A = nn.Parameter(torch.eye(3).unsqueeze(0).unsqueeze(0).repeat(batch_size, num_points, 1, 1))
        self.b = nn.Parameter(torch.zeros(3).unsqueeze(0).unsqueeze(0).unsqueeze(3).repeat(batch_size, num_points, 1, 1))
        G = torch.eye(4).unsqueeze(0).unsqueeze(0).repeat(batch_size, 1, 1, 1)
        G[..., 3, 3] = gamma
        self.register_buffer('G', G)
        self.edges = edges
        self.num_points = num_points

    def stiffness(self):
        if self.edges is None:
            raise Exception("edges cannot be none when calculate stiff")
        w = torch.cat((self.A, self.b), dim=3)
        w_diff = torch.index_select(w, 1, self.edges[:, 0]) - torch.index_select(w, 1, self.edges[:, 1])
        w_diff = torch.einsum('bnhw,bnwj->bnhj', w_diff, self.G.repeat(1, w_diff.shape[1], 1, 1))
        return w_diff ** 2

    def forward(self, x, pool_num=0, return_stiff=False):
        out_x = (torch.matmul(self.A, x.unsqueeze(3)) + self.b).squeeze(3)
        if return_stiff:
            return out_x, self.stiffness()
        return out_x

    def forward_normal(self, x):
        b, n = self.A.shape[:2]
        A_inv, A_inv_mask = inv3x3(self.A.detach().reshape(-1, 3, 3))
        normal = A_inv.transpose(-1, -2).view(b, n, 3, 3) @ x.unsqueeze(3)
        return normal.squeeze(-1), A_inv_mask[None]


class NRICP_Optimizer_AdamW:
    """Registers a template mesh to a target mesh by non-rigid ICP with AdamW (Optimal Step Nonrigid ICP, CVPR 2007, with
    the reference's normal check and target mask).  `__call__(**inputs)` / `fitting(inputs)` -> (loss, TriMesh)."""

    def __init__(self, epoch, dense_pcl, use_normal, stiffness_weight=[], mile_stone=[], inner_iter=10,
                 laplacian_weight=0., gamma=1, threshold=0.5, optimizer_setting=None, device='cuda:0', use_kernels=True,
                 log=print):
        self.name = 'NRICP_Optimizer_GPU'
        self.optimizier_setting = optimizer_setting
        self.dense_pcl = int(dense_pcl)
        self.use_normal = use_normal
        self.mile_times = 0
        self.mile_idx = 0
        self.stiffness_weight = stiffness_weight
        self.laplacian_weight = laplacian_weight
        self.inner_iter = inner_iter
        self.mile_stone = mile_stone
        self.epoch = epoch
        self.device = torch.device(device)
        self.gamma = gamma
        self.local_affine = None
        self.threshold = threshold
        self.use_kernels = bool(use_kernels) and self.device.type == 'cuda'
        self.log = log
        self.history = []                 # per epoch: (mean update, valid, vert_sum, stiffness_sum, laplacian, loss)
        assert len(self.mile_stone) == len(self.stiffness_weight) - 1

    def __call__(self, **inputs):
        return self.fitting(inputs)

    def _collect_data(self, inputs):
        smpl_slice = inputs['smpl_slice']
        verts, faces = densify(smpl_slice.verts, smpl_slice.faces, self.dense_pcl)
        smpl_slice = TriMesh(verts, faces)
        inputs['smpl_slice'] = smpl_slice
        if inputs.get('static_pts_type'):
            raise NotImplementedError("static points (static_pts_type) are not supported; registration passes none")
        return (smpl_slice, inputs['cano_meshes'], inputs.get('save_path'), inputs.get('garment_name'),
                inputs.get('nricp_masks'))

    def fitting(self, inputs):
        self.mile_times = 0
        self.mile_idx = 0
        self.history = []
        smpl_slice, cano_meshes, save_path, garment_name, nricp_masks = self._collect_data(inputs)
        if save_path is not None:
            save_path = os.path.join(save_path, 'nricp_deform', str(garment_name))
            os.makedirs(save_path, exist_ok=True)
        dev = self.device
        smpl_slice = smpl_slice.to(dev)
        source_v = smpl_slice.verts.float()[None].contiguous()
        source_f = smpl_slice.faces
        V = source_v.shape[1]
        source_normals = K.verts_normals(smpl_slice.verts.float(), source_f)[None].contiguous()
        target_v = cano_meshes.verts.to(dev).float()
        target_normals = K.verts_normals(target_v, cano_meshes.faces.to(dev))
        if nricp_masks is not None:
            keep = nricp_masks.to(dev) > 0
            target_v, target_normals = target_v[keep], target_normals[keep]
        target_v, target_normals = target_v.contiguous(), target_normals.contiguous()
        topo = K.EnergyTopology(source_f, V, dev)
        inner_mask = topo.interior[None]
        self.local_affine = Local_Affine(V, 1, topo.edges, gamma=self.gamma).to(dev)
        if self.use_kernels:
            loss = self._fit_kernels(source_v, source_normals, target_v, target_normals, topo)
        else:
            loss = self._fit_torch(source_v, source_f, source_normals, target_v, target_normals, topo, inner_mask)
        with torch.no_grad():
            new_source_v = self.local_affine(source_v, pool_num=0, return_stiff=False)
            if save_path is not None:
                from ... import utils
                utils.write_obj(os.path.join(save_path, '{}.obj'.format(self.mile_times)), new_source_v[0].cpu(),
                                source_f.cpu())
        return loss, TriMesh(new_source_v[0].detach(), source_f)

    def _epoch_log(self, distance, valid, n, vert, stiff, lap, loss, lw, sw):
        self.history.append((distance, valid, vert, stiff, lap, loss))
        if self.log is not None:
            self.log("current {:03d} NRICP avg_update:{:.5f} valid{:d}/{:d}: dis:{:.4f}, stiffness:{:.4f}, laplacian:{:.4f}, "
                     "total:{:.4f} laplacian_weight:{:.4f}, stiffness_weight:{:.4f}, static_sum:{:.4f}".format(
                         self.mile_times, distance, valid, n, vert, stiff, lap, loss, lw, sw, 0.))

    def _next_epoch(self):
        self.mile_times += 1
        if self.mile_times in self.mile_stone:
            self.mile_idx += 1

    def _fit_torch(self, source_v, source_f, source_normals, target_v, target_normals, topo, inner_mask):
        """The reference's loop (:365-437) with autograd."""
        la = self.local_affine
        loss = None
        for i in range(self.epoch):
            new_source_v, stiffness = la(source_v, pool_num=0, return_stiff=True)
            old_source_v = new_source_v.detach().clone()
            with torch.no_grad():
                new_source_normals, inv_mask = la.forward_normal(source_normals)
                inner_inv_mask = torch.logical_and(inv_mask, inner_mask)
            inner_optimizer = torch.optim.AdamW([{'params': la.parameters()}], lr=1e-4, amsgrad=True)
            idx, _ = K.knn1_torch(new_source_v[0].detach(), target_v)
            close_points = target_v[idx][None]
            close_normals = target_normals[idx][None]
            stiffness_weight = self.stiffness_weight[self.mile_idx]
            laplacian_weight = self.laplacian_weight[self.mile_idx]
            for inner_i in range(100 if i == 0 else self.inner_iter):
                inner_optimizer.zero_grad()
                with torch.no_grad():
                    normal_cos_sim = F.cosine_similarity(close_normals, new_source_normals, dim=2)
                    weight_mask = torch.logical_and(inner_inv_mask, normal_cos_sim > self.threshold)
                vert_distance = (new_source_v - close_points) ** 2
                bsize = vert_distance.shape[0]
                vert_sum = torch.sum((weight_mask[..., None] * vert_distance).view(bsize, -1)) / bsize
                stiffness_sum = torch.sum(stiffness.view(bsize, -1)) * stiffness_weight / bsize
                laplacian_loss = K.laplacian_smoothing_torch(new_source_v[0], topo.edges) * laplacian_weight
                loss = torch.sqrt(vert_sum + stiffness_sum) + laplacian_loss
                loss.backward()
                inner_optimizer.step()
                new_source_v, stiffness = la(source_v, pool_num=0, return_stiff=True)
                with torch.no_grad():
                    new_source_normals, inv_mask = la.forward_normal(source_normals)
                    inner_inv_mask = torch.logical_and(inv_mask, inner_mask)
            distance = torch.mean(torch.sqrt(torch.sum((old_source_v - new_source_v) ** 2, dim=2)))
            self._epoch_log(distance.item(), int(weight_mask.sum()), weight_mask.numel(), vert_sum.item(),
                            stiffness_sum.item(), laplacian_loss.item(), loss.item(), laplacian_weight, stiffness_weight)
            self._next_epoch()
        return loss.detach() if loss is not None else None

    def _fit_kernels(self, source_v, source_normals, target_v, target_normals, topo):
        """The same loop on csrc/nricp.hip: knn1 per epoch, one energy launch chain per inner iteration (it fills
        `.grad`), torch's AdamW step."""
        la = self.local_affine
        energy = K.NricpEnergy(topo, source_v.device)
        la.A.grad = energy.dA.view_as(la.A)
        la.b.grad = energy.db.view_as(la.b)
        x = source_v[0].contiguous()
        nx = source_normals[0].contiguous()
        loss = None
        for i in range(self.epoch):
            with torch.no_grad():
                old_source_v = la(source_v)
                idx, _ = K.knn1(old_source_v[0].contiguous(), target_v)
                close_points = target_v[idx].contiguous()
                close_normals = target_normals[idx].contiguous()
            inner_optimizer = torch.optim.AdamW([{'params': la.parameters()}], lr=1e-4, amsgrad=True)
            stiffness_weight = self.stiffness_weight[self.mile_idx]
            laplacian_weight = self.laplacian_weight[self.mile_idx]
            for inner_i in range(100 if i == 0 else self.inner_iter):
                scalars, mask = energy(la.A.data, la.b.data, x, close_points, close_normals, nx, self.gamma,
                                       stiffness_weight, laplacian_weight, self.threshold)
                inner_optimizer.step()
            loss = scalars[0].clone()
            with torch.no_grad():
                distance = torch.mean(torch.sqrt(torch.sum((old_source_v - la(source_v)) ** 2, dim=2)))
            s = scalars.tolist()
            self._epoch_log(distance.item(), int(mask.sum()), mask.numel(), s[1], s[2], s[3], s[0], laplacian_weight,
                            stiffness_weight)
            self._next_epoch()
        return loss


def densify(verts, faces, dense_pcl):
    return K.densify(verts, faces, dense_pcl)
