"""Feature-curve branch of the iteration (SURVEY.md §8f "next" row 3): explicit curves, their 2-D projection loss and
z-buffer visibility.

Restates, on torch ops + the HIP mesh rasteriser (the curves hold a few hundred points; the tube sweep and the fit to boundary
loops of `curve_to_mesh` run on csrc/curve_tubes.hip):
  * `Intersect_Free_Curve`            engineer/utils/garment_structure.py:36-147 (forward / inference / regularization /
                                      query_canosmpl_verts; the constructor takes the uniformly resampled curves directly —
                                      the reference extracts them from template meshes with `extract_edge`, data path)
  * `curve_to_mesh` / `fit_curves_to_loops`   :176-274, the tubes infer_fl_curve.py writes and the AdamW fit to boundary loops
  * `fl_proj_loss`                    engineer/core/fl_optimizer.py:72-110, with pytorch3d's `chamfer_distance(
                                      point_reduction='sum')` restated (third party, parity unpinned)
  * `zbuff_check` / `surface_depth_check`   the body of fl_visible_by_body_zbuff, OptimGarmentNetwork.py:1374-1448
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from .connectivity import boundary_loops
from .utils.constant import FL_EXTRACT, ZBUF_THRESHOLD  # noqa: E402,F401  (utils/constant.py:65-74, :219-227)

FIT_ITERS = 20000            # AdamW steps of curve_to_mesh's fit to boundary loops (garment_structure.py:188)


def _legacy_cross(a, b):
    """`torch.cross(a, b)` as the reference calls it (garment_structure.py:89, no `dim`): the legacy default is the
    FIRST axis of size 3 — the line axis when there are exactly three feature lines, else the coordinate axis."""
    dim = next(i for i, n in enumerate(a.shape) if n == 3)
    return torch.linalg.cross(a, b, dim=dim)


class Intersect_Free_Curve(nn.Module):
    """Closed curves parametrised around their centre: every sample keeps its direction from the centre and learns a
    radial scale (through a ReLU, so the curve cannot fold through its centre) plus an offset along the curve normal."""

    def __init__(self, uni_curve_verts_list, cano_smpl_verts_list, fl_names):
        super().__init__()
        self.fl_names = list(fl_names)
        self.register_buffer('cano_smpl_verts', torch.stack([v for v in cano_smpl_verts_list], dim=0))
        cano_verts_tensor = torch.stack([v for v in uni_curve_verts_list], dim=0)                 # [L,S,3]
        cano_verts_center = cano_verts_tensor.mean(1, keepdim=True)                                # :81
        self.register_buffer('cano_verts_center', cano_verts_center)
        rel = cano_verts_tensor - cano_verts_center
        cano_v_dirs = rel / (rel.norm(dim=-1, keepdim=True) + 1e-6)                                 # :84
        nx = _legacy_cross(cano_v_dirs[:, :-1, :], cano_v_dirs[:, 1:, :])                             # :85-87
        nx = nx / nx.norm(dim=-1, keepdim=True)
        nx = nx.mean(dim=1, keepdim=True)
        self.register_buffer('cano_nx', nx)
        self.register_buffer('cano_v_dirs', cano_v_dirs)
        init_scale = torch.clamp_min((rel * cano_v_dirs).sum(dim=-1, keepdim=True), 0.)              # :93-94
        self.register_buffer('init_scale', init_scale)
        self.scale = nn.Parameter(torch.full(init_scale.shape, 1.0, device=init_scale.device))      # :98-99
        self.nx_scale = nn.Parameter(torch.full(init_scale.shape, 0., device=init_scale.device))

    def query_canosmpl_verts(self, query_names):                                                    # :50-63
        table = {name: v for name, v in zip(self.fl_names, self.cano_smpl_verts)}
        return [table[name] for name in query_names]

    def forward(self):                                                                              # :104-109
        v_dir_offset = self.cano_v_dirs * self.init_scale * F.relu(self.scale)
        nx_offset = self.nx_scale * self.cano_nx
        return self.cano_verts_center + v_dir_offset + nx_offset

    def inference(self):
        with torch.no_grad():
            return self.forward()

    def regularization(self, fl_masks, cano_verts=None):                                            # :120-141
        """`cano_verts`: the curves of this iteration when the caller has them already (`self.forward()` otherwise, as the
        reference does on every call)."""
        if cano_verts is None:
            cano_verts = self.forward()
        used_flag = (fl_masks.sum() > 0).float()
        center_loss = used_flag * abs(cano_verts.mean(1, keepdim=True) - self.cano_verts_center).sum()
        diff_a = cano_verts[:, :-1, :] - cano_verts[:, 1:, :]
        diff_b = cano_verts[:, -1:, :] - cano_verts[:, 0:1, :]
        diff_c = cano_verts[:, 0:1, :] - cano_verts[:, 1:2, :]
        diff_a = torch.cat([diff_a, diff_b, diff_c], dim=1)
        diff_a = diff_a / (diff_a.norm(dim=-1, keepdim=True) + 1e-6)
        diff_a_loss = 1 - F.cosine_similarity(diff_a[:, :-1, :], diff_a[:, 1:, :], dim=-1)
        return {'center_offset': 0 * center_loss, 'diff_a_loss': diff_a_loss.sum()}

    def curve_to_mesh(self, curve_radius=0.002, num_joints=6, curve_verts=None, curve_idx=None, target_idx=None,
                      iters=FIT_ITERS, log=None):                                                   # :176-274
        """One thin tube per curve: a list of `shading.Meshes` (one mesh each: `verts_packed()` [S*J,3], `faces_packed()`
        [2*S*J,3] int64, indices local to the curve), swept by csrc/curve_tubes.hip.  With `curve_verts` (a list of
        polylines [M,3]) curve `target_idx[k]` is first fitted to polyline `curve_idx[k]` (`fit_curves_to_loops`; `iters`
        and `log`, a dict that receives the fit log, are additions).  The reference's `torch.cross(d, n)` carries no
        `dim`; with exactly three curves its legacy default crosses ALONG the curve axis, which is not reproduced."""
        from . import shading
        if curve_verts is not None:
            if curve_idx is None or target_idx is None or len(curve_idx) != len(target_idx):
                raise ValueError("curve_to_mesh: curve_verts needs curve_idx and target_idx of one length")
            info = fit_curves_to_loops(self, [curve_verts[c] for c in curve_idx], list(target_idx), iters=iters)
            if log is not None:
                log.update(info)
        verts, faces = curve_tubes(self.inference(), self.cano_nx[:, 0, :], curve_radius, num_joints)
        return [shading.Meshes(v[None], f) for v, f in zip(verts, faces)]


FIT_W_CHAMFER, FIT_W_SMOOTH = 1000., 0.1                    # garment_structure.py:198, :208


def curve_tubes(curves, nx, radius=0.002, num_joints=6):
    """recmv_curve_tubes: closed curves [L,S,3] and their normals [L,3] -> (verts [L,S*J,3] f32, faces [L,2*S*J,3] int64)."""
    L.require_cuda(curves, "curves")
    L.require_cuda(nx, "nx")
    if curves.dim() != 3 or curves.shape[-1] != 3 or tuple(nx.shape) != (curves.shape[0], 3):
        raise ValueError("curve_tubes: curves [L,S,3] and nx [L,3], got %s and %s" % (tuple(curves.shape), tuple(nx.shape)))
    curves, nx = curves.detach().float().contiguous(), nx.detach().float().contiguous()
    n, S = curves.shape[0], curves.shape[1]
    J = int(num_joints)
    verts = L.scratch((n, S * max(J, 0), 3), torch.float32, curves.device)
    faces = L.scratch((n, 2 * S * max(J, 0), 3), torch.int64, curves.device)
    with L.device_guard(curves.device):
        L.check(L.lib().recmv_curve_tubes(L.ptr(curves), L.ptr(nx), float(radius), n, S, J, L.ptr(verts), L.ptr(faces),
                                          L.stream_ptr(curves.device)), "curve_tubes")
    return verts, faces


def fit_step(curve, targets, target_idx):
    """recmv_curve_fit_step on the parameters of `curve`: (loss [P] per pair, d sum(loss) / d scale, d sum(loss) / d nx_scale).
    `targets` [P,M,3] f32 and `target_idx` [P] int32 live on the curve's device."""
    L.require_cuda(curve.scale, "curve.scale")
    L.require_cuda(targets, "targets")
    L.require_cuda(target_idx, "target_idx")
    if targets.dtype != torch.float32 or target_idx.dtype != torch.int32 or not targets.is_contiguous():
        raise ValueError("fit_step: targets contiguous float32 [P,M,3] and target_idx int32 [P]")
    if targets.dim() != 3 or targets.shape[2] != 3 or tuple(target_idx.shape) != (targets.shape[0],):
        raise ValueError("fit_step: targets [P,M,3] and target_idx [P], got %s and %s"
                         % (tuple(targets.shape), tuple(target_idx.shape)))
    n, S = curve.scale.shape[0], curve.scale.shape[1]
    P, M = targets.shape[0], targets.shape[1]
    dev = curve.scale.device
    bufs = [curve.cano_verts_center, curve.cano_v_dirs, curve.init_scale, curve.cano_nx, curve.scale.detach(),
            curve.nx_scale.detach()]
    bufs = [b.float().contiguous() for b in bufs]
    loss = L.scratch((P,), torch.float32, dev)
    g_scale, g_nx = L.scratch_like(bufs[4]), L.scratch_like(bufs[5])
    with L.device_guard(dev):
        L.check(L.lib().recmv_curve_fit_step(*[L.ptr(b) for b in bufs], L.ptr(targets), L.ptr(target_idx), n, S, P, M,
                                             FIT_W_CHAMFER, FIT_W_SMOOTH, L.ptr(loss), L.ptr(g_scale), L.ptr(g_nx),
                                             L.stream_ptr(dev)), "curve_fit_step")
    return loss, g_scale, g_nx


def fit_step_torch(curve, targets, target_idx):
    """The objective of `fit_step` in torch, as the reference writes it (:190-208, pytorch3d's default chamfer_distance
    restated: mean over the points of each side, both sides added): loss [P] per pair, differentiable with respect to
    `curve.scale` and `curve.nx_scale`.  Works on any device and dtype; `target_idx` is a sequence of ints."""
    curves = curve()
    out = []
    for gt, t_i in zip(targets, target_idx):
        x = curves[int(t_i)]
        d = ((x[:, None, :] - gt[None, :, :].to(x.dtype)) ** 2).sum(-1)
        cham = d.min(dim=1).values.mean() + d.min(dim=0).values.mean()
        diff_a = torch.cat([x[:-1, :] - x[1:, :], x[-1:, :] - x[0:1, :]], dim=0)
        diff_a = diff_a / (diff_a.norm(dim=-1, keepdim=True) + 1e-6)
        diff_a_loss = (1 - F.cosine_similarity(diff_a[:-1, :], diff_a[1:, :], dim=-1)).sum()
        out.append(FIT_W_CHAMFER * cham + FIT_W_SMOOTH * diff_a_loss)
    return torch.stack(out)


def fit_curves_to_loops(curve, targets, target_idx, iters=FIT_ITERS, lr=1e-4, step=None):
    """The fit branch of `curve_to_mesh` (:179-212): curve `target_idx[k]` is pulled onto the polyline `targets[k]` ([M,3],
    one M for all pairs) by `iters` AdamW steps (torch defaults) over `scale` and `nx_scale`, every step one launch of
    recmv_curve_fit_step (`step`: another implementation of `fit_step`, e.g. the torch one of tools/curve_fit_timing.py).
    As the reference does first, `scale[target_idx]` is set to its mean and `init_scale[target_idx]` doubled — in place: the
    fit changes the module.  Returns {'iters', 'target_idx', 'first_loss', 'last_loss'} (per-pair lists)."""
    L.require_cuda(curve.scale, "curve.scale")
    dev = curve.scale.device
    target_idx = [int(t) for t in target_idx]
    n = curve.scale.shape[0]
    if not target_idx or len(targets) != len(target_idx):
        raise ValueError("fit_curves_to_loops: one polyline per target index, at least one pair")
    if any(t < 0 or t >= n for t in target_idx):
        raise ValueError("fit_curves_to_loops: target_idx %s outside the %d curves" % (target_idx, n))
    tg = torch.stack([torch.as_tensor(t).float().reshape(-1, 3) for t in targets]).to(dev).contiguous()
    idx = torch.tensor(target_idx, dtype=torch.int32, device=dev)
    with torch.no_grad():
        sel = torch.tensor(target_idx, dtype=torch.int64, device=dev)
        curve.scale[sel] = curve.scale[sel].mean()                                     # :180-181
        curve.init_scale[sel] *= 2                                                     # :186
    params = [curve.scale, curve.nx_scale]
    opt = torch.optim.AdamW(params, lr=lr)
    step = step or fit_step
    first = last = None
    for _ in range(int(iters)):
        loss, g_scale, g_nx = step(curve, tg, idx)
        curve.scale.grad, curve.nx_scale.grad = g_scale, g_nx
        opt.step()
        if first is None:
            first = loss
        last = loss
    as_list = lambda t: [] if t is None else [float(v) for v in t.detach().cpu()]   # noqa: E731
    return {'iters': int(iters), 'target_idx': target_idx, 'first_loss': as_list(first), 'last_loss': as_list(last)}


def longest_boundary_loop(faces):
    """Vertex indices along the longer of the two boundary loops of a ribbon mesh — the curve a template feature line stands
    for (`Intersect_Free_Curve.extract_edge`, engineer/utils/garment_structure.py:149-173, which asks trimesh's `outline()`
    for the boundary paths and keeps the one with more points).  trimesh is third party and absent: the loops are
    connectivity.boundary_loops' walks over the edges that belong to exactly one face, each from its lowest vertex index
    towards its lower neighbour — the same point set; start and direction of trimesh's path are not reproduced (parity
    unpinned)."""
    loops = boundary_loops(faces)
    walked = [v for loop in loops for v in loop]           # a vertex with four boundary edges is walked through twice
    assert len(walked) == len(set(walked)), "a feature-line template is a band: every boundary vertex has two boundary edges"
    assert len(loops) == 2, "a feature-line template has two boundary loops, found %d" % len(loops)
    return loops[0] if len(loops[0]) > len(loops[1]) else loops[1]


def chamfer_distance_sum(x, y):
    """pytorch3d `chamfer_distance(x, y, point_reduction='sum')[0]` for one cloud pair x [1,n,D], y [1,m,D]: squared
    distance of every point to its nearest neighbour in the other set, summed over both directions.  An empty side
    contributes nothing (upstream: zero-length clouds give zero terms)."""
    if x.shape[1] == 0 or y.shape[1] == 0:
        return x.sum() * 0.
    d = ((x[0, :, None, :] - y[0, None, :, :]) ** 2).sum(-1)                # [n,m]
    return d.min(dim=1).values.sum() + d.min(dim=0).values.sum()


def chamfer_visible_sum(x, vis, y):
    """`chamfer_distance_sum(x[vis][None], y[None])` without forming x[vis] (boolean indexing is a `nonzero`: a host
    round trip that stalls the stream's feeder).  x [n,D], vis [n] bool, y [m,D].  Hidden samples contribute no row
    term and are kept out of the column minima; no visible sample or an empty side = zero, as upstream."""
    if x.shape[0] == 0 or y.shape[0] == 0:
        return x.sum() * 0.
    d = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)                      # [n,m]
    rows = torch.where(vis, d.min(dim=1).values, d.new_zeros(()))
    cols = torch.where(vis[:, None], d, d.new_full((), float('inf'))).min(dim=0).values
    cols = torch.where(vis.any(), cols, cols.new_zeros(()))
    return rows.sum() + cols.sum()


def fl_proj_loss(fl_pts_list, gt_fl_pts_list, fl_masks, proj_fl_weights=None):
    """engineer/core/fl_optimizer.py:72-110.  Per feature line: chamfer between the VISIBLE projected samples of each
    frame and that frame's 2-D ground-truth curve, averaged over the frames that see the line and over the visible
    samples, then over the lines."""
    if proj_fl_weights is None:
        proj_fl_weights = [1. for _ in range(len(fl_pts_list))]
    if (len(fl_pts_list) > 0 and fl_pts_list[0].dim() == 3 and isinstance(gt_fl_pts_list[0], torch.Tensor)
            and all(p.shape == fl_pts_list[0].shape for p in fl_pts_list)
            and all(m.shape == fl_masks[0].shape for m in fl_masks)
            and all(g.dim() == 3 and g.shape == gt_fl_pts_list[0].shape for g in gt_fl_pts_list)):
        return _fl_proj_loss_batched(fl_pts_list, gt_fl_pts_list, fl_masks, proj_fl_weights)
    loss = fl_pts_list[0].new_zeros(())          # (no host tensor: a pageable H2D copy would block the host on this stream)
    for fl_pts, gt_fl_pts, fl_mask, w in zip(fl_pts_list, gt_fl_pts_list, fl_masks, proj_fl_weights):
        screen_fl_pts = fl_pts[..., :2]
        screen_fl_masks = fl_mask[..., :2]
        valid_batch = (fl_mask[..., 0].sum(dim=-1) > 0).float().sum()
        batch_loss = 0.
        for screen_fl_pt, screen_fl_mask, gt_fl_pt in zip(screen_fl_pts, screen_fl_masks, gt_fl_pts):
            # the reference compacts `screen_fl_pt[screen_fl_mask == 1]` (:92); same sums, no compaction
            batch_loss = batch_loss + w * chamfer_visible_sum(screen_fl_pt, screen_fl_mask[..., 0] == 1,
                                                              gt_fl_pt.view(-1, 2))
        # the reference branches on `valid_batch != 0` / `masks.sum() != 0` through host reads; the same selection is
        # made on the device here
        batch_loss = torch.where(valid_batch != 0, batch_loss / valid_batch.clamp(min=1.), batch_loss)
        n_vis = torch.div(screen_fl_masks.sum(), 2, rounding_mode='floor')
        loss = loss + torch.where(n_vis != 0, batch_loss / n_vis.clamp(min=1.), batch_loss)
    return loss / len(fl_pts_list)


_WEIGHT_ROWS = {}


def _fl_proj_loss_batched(fl_pts_list, gt_fl_pts_list, fl_masks, weights):
    """fl_proj_loss when every line has the same number of samples and of ground-truth points (what the loop produces):
    all (line, frame) chamfers as ONE distance tensor [L,N,S,M] — a dozen launches instead of a dozen per pair.  The sums
    over frames and over lines are taken in the loop version's order (a sequence of adds)."""
    X = torch.stack([p[..., :2] for p in fl_pts_list], dim=0)                       # [L,N,S,2]
    Y = torch.stack([g.reshape(g.shape[0], -1, 2) for g in gt_fl_pts_list], dim=0)  # [L,N,M,2]
    Mk = torch.stack([m[..., :2] for m in fl_masks], dim=0)                         # [L,N,S,2]
    V = Mk[..., 0] == 1                                                             # [L,N,S]
    L_, N = X.shape[0], X.shape[1]
    w = None
    if any(float(v) != 1. for v in weights):
        key = (tuple(float(v) for v in weights), X.device, X.dtype)
        w = _WEIGHT_ROWS.get(key)                 # uploaded once: a per-call host tensor would stall the stream's feeder
        if w is None:
            w = _WEIGHT_ROWS[key] = torch.tensor(key[0], dtype=X.dtype, device=X.device)
    d = ((X[..., :, None, :] - Y[..., None, :, :]) ** 2).sum(-1)                    # [L,N,S,M]
    rows = torch.where(V, d.min(dim=-1).values, d.new_zeros(())).sum(-1)            # [L,N]
    cols = torch.where(V[..., None], d, d.new_full((), float('inf'))).min(dim=-2).values
    cols = torch.where(V.any(-1)[..., None], cols, cols.new_zeros(())).sum(-1)      # [L,N]
    per = rows + cols
    if w is not None:
        per = w.view(-1, 1) * per
    batch_loss = per[:, 0]
    for j in range(1, N):
        batch_loss = batch_loss + per[:, j]                                         # [L]
    valid_batch = (Mk[..., 0].sum(dim=-1) > 0).to(X.dtype).sum(-1)                  # [L]
    batch_loss = torch.where(valid_batch != 0, batch_loss / valid_batch.clamp(min=1.), batch_loss)
    n_vis = torch.div(Mk.reshape(L_, -1).sum(-1), 2, rounding_mode='floor')         # [L]
    terms = torch.where(n_vis != 0, batch_loss / n_vis.clamp(min=1.).to(X.dtype), batch_loss)
    loss = terms[0]
    for i in range(1, L_):
        loss = loss + terms[i]
    return loss / L_


def zbuff_check(z_buff, uv):
    """`z_buff_check` of OptimGarmentNetwork.py:1378-1387: bilinear read of a [B,H,W,1] depth image at uv in [-1,1]
    (align_corners=True) -> [B,P]."""
    zb = z_buff.permute(0, 3, 1, 2)
    return F.grid_sample(zb, uv.unsqueeze(2), align_corners=True)[:, 0, :, 0]


def surface_depth_check(cameras, image_size, frags_zbuf, verts_world, query_world):
    """The depth test of fl_visible_by_body_zbuff (:1394-1420 for the garment, :1424-1446 for the body): how far
    behind the rasterised surface (world z) each query point lies.  `frags_zbuf` [N,H,W,1] is the mesh rasteriser's
    view-space depth with -1 = background, replaced by the farthest vertex depth of the frame; `verts_world` [N,V,3]
    are the rasterised vertices, `query_world` [N,P,3] the curve samples."""
    W, H = image_size
    N = query_world.shape[0]
    cam_z = cameras.cam_pos().detach()[-1]
    zbuf = frags_zbuf.clone()
    z_max = (verts_world[..., -1].detach() - cam_z).max(-1).values                    # [N]
    z_max = z_max[:, None, None, None].expand_as(zbuf)
    zbuf = torch.where(zbuf == -1., z_max, zbuf)
    screen = cameras.project(query_world.reshape(-1, 3)).view(N, -1, 2)               # transform_points_screen xy
    u = 2 * screen[..., 0] / W - 1
    v = 2 * screen[..., 1] / H - 1
    uv = torch.stack([u, v], dim=-1)
    surf_depth = zbuff_check(zbuf, uv) + cam_z
    return query_world[..., -1] - surf_depth
