"""Inference of a trained run: per-frame posed garment meshes, their Phong renders and their colour renders.

`OptimGarmentNetwork.infer` (engineer/networks/OptimGarmentNetwork.py:3216-3306), the function infer_fl.py's loop is built
on, restated on the recmv kernels for every garment of a HotLoop:
  deformer (offset MLP + skinning)   -> posed meshes of the N frames                               :3242-3246
  MeshRasterizer + HardPhongShader   -> `imgs` (white TexturesVertex, PointLights at (0,1,0)),    :3247-3258
                                        mask error 1 - |M n G| / |M u G| when a ground truth is given
  canonical-pose mesh (offset only)  -> `def1imgs` through a camera behind the subject             :3262-3269
  FindSurfacePs + camera rays + OptimizeGarmentSurfaceSinlge + SDF normal + compute_cardinal_rays
  + netRender                        -> `colors` on a white canvas                                 :3271-3300
`infer_garment_animation` (:2729-2859) is the same chain driven by poses the capture never saw, with the capture's
conditions averaged over its frames, the posed body rendered beside every garment and, as an addition, the body-collision
repair of recmv.collide.
`infer_garment_fl` (:2861-2935) poses the feature curves, swept into thin tubes (csrc/curve_tubes.hip), with the deformer.
The shading runs on csrc/shade_meshes.hip (recmv.shading), the rest on the kernels the loop uses.  Everything runs
without autograd except the SDF normal and the cardinal rays, which differentiate the nets as the reference does.
"""
import time

import numpy as np
import torch

from . import raster, shading, utils
from .utils.constant import FL_EXTRACT
from .model import RectifiedPerspectiveCameras

COLOR_CHUNK = 10000            # rays per root-finder / colour call (:3275)
_DEF1_R = ((-1., 0., 0.), (0., 1., 0.), (0., 0., -1.))       # second camera of :3264


def _to_uint8(x):
    """torch.clamp(x * 255, 0, 255) -> numpy uint8 by truncation, as the reference converts (:3258, :3268)."""
    return torch.clamp(x * 255., min=0., max=255.).cpu().numpy().astype(np.uint8)


class _Clock:
    """Wall-time split of the inference (shading / colour-branch root finding / ...), synchronised at each boundary; a
    no-op without a dict to fill."""

    def __init__(self, acc, device):
        self.acc, self.cuda = acc, acc is not None and torch.device(device).type == 'cuda'
        self.t = time.perf_counter() if acc is not None else None

    def lap(self, name):
        if self.acc is None:
            return
        if self.cuda:
            torch.cuda.synchronize()
        now = time.perf_counter()
        self.acc[name] = self.acc.get(name, 0.0) + (now - self.t)
        self.t = now


def _render(meshes, cameras, H, W, lights, gt_mask=None):
    """maskRender(defMeshes, cameras=..., lights=...) with the HardPhongShader: (images [N,H,W,4], fragments, counts)."""
    frags = raster.MeshRasterizer(cameras, (H, W), blur_radius=0., perspective_correct=True, cull_backfaces=False)(
        meshes.verts_padded(), meshes.faces)
    N = meshes.verts_padded().shape[0]
    out = shading.hard_phong_shade(frags, meshes.verts_padded(), meshes.faces, meshes.verts_normals_padded(),
                                   meshes.textures.verts_features_padded(), shading._camera_centers(cameras, N, frags.pix_to_face.device),
                                   lights, shading.Materials(), shading.BlendParams(), gt_mask)
    images, counts = out if gt_mask is not None else (out, None)
    return images, frags, counts


def infer_garments(loop, TmpVs_list, Tmpfs_list, H, W, ratio, frame_ids, notcolor=False, gts=None, garments=None,
                   chunk=COLOR_CHUNK, timings=None):
    """The per-garment body of `infer` for every garment (or the indices in `garments`): a dict of lists over garments,
    'colors' (uint8 [N,H,W,3], None with `notcolor`), 'imgs' (uint8 [N,H,W,3] with `gts`, [N,H,W,4] without), 'def1imgs'
    (uint8 [N,H,W,4]), 'defMeshVs' (float32 [N,V,3]) and 'maskE' (float32 [N] with `gts`, else None).
    `gts`: {'mask': [N,H,W] float, optional 'image': [N,H,W,3] in [0,1], B,G,R}.  `timings`: a dict that receives the
    wall time in seconds of 'deform', 'shading', 'surface_points', 'root_finding' and 'color' (synchronised)."""
    device = TmpVs_list[0].device
    clock = _Clock(timings, device)
    N = frame_ids.numel()
    focals, pps, Rs, Ts, _, _ = loop.dataset.get_camera_parameters(1, device)
    with torch.no_grad():
        cameras = RectifiedPerspectiveCameras(focals.detach(), pps.detach(), Rs.detach(), Ts.detach(), image_size=[(W, H)])
        newTs = loop.dataset.trans.detach().mean(0).to(device).view(1, 3)
        newcameras = RectifiedPerspectiveCameras(focals.detach(), pps.detach(), torch.tensor([_DEF1_R], device=device), newTs,
                                                 image_size=[(W, H)])
        def1_lights = shading.PointLights(location=((0., 1., float(newTs[0, 2])),))
        d_cond_list, poses, trans, rendcond = loop.get_grad_parameters(frame_ids, device)
        d_cond_list = [c.detach() for c in d_cond_list[1:]]           # idx 0: the body's code
        poses, trans = poses.detach(), trans.detach()
        rendcond = rendcond.detach() if rendcond is not None else None
    out = {k: [] for k in ('colors', 'imgs', 'def1imgs', 'defMeshVs', 'maskE')}
    for g_i, (TmpVs, Tmpfs, name) in enumerate(zip(TmpVs_list, Tmpfs_list, loop.garment_names)):
        if garments is not None and g_i not in garments:
            continue
        TmpVs = TmpVs.detach()
        d_cond = d_cond_list[g_i]
        if TmpVs.shape[0] == 0 or Tmpfs.shape[0] == 0:
            _empty_garment(out, N, H, W, notcolor, gts, device)
            continue
        white = shading.TexturesVertex(torch.ones_like(TmpVs)[None])
        with torch.no_grad():
            defTmpVs = loop.deformer(TmpVs[None, :, :].expand(N, -1, 3), [d_cond, [poses, trans]], ratio=ratio,
                                     offset_type=name).contiguous()
            defMeshVs = defTmpVs.cpu().numpy()
            cano = loop.deformer.defs[0](TmpVs[None, :, :].expand(N, -1, 3), d_cond, ratio=ratio, offset_type=name)
            clock.lap('deform')
            meshes = shading.Meshes(defTmpVs, Tmpfs, white)
            gt_mask = gts['mask'].to(device) if gts else None
            imgs, frags, counts = _render(meshes, cameras, H, W, shading.PointLights(), gt_mask)
            maskE = None
            if gts:
                masks = frags.pix_to_face[..., 0] >= 0
                maskE = shading.mask_error(counts).cpu().numpy()
                gts['maskE'] = maskE
                imgs = imgs[..., :3]
                if 'image' in gts:
                    imgs[~masks] = gts['image'].to(device)[~masks][:, [2, 1, 0]]
            imgs = _to_uint8(imgs)
            cmeshes = shading.Meshes(cano.contiguous(), Tmpfs, white)
            cmeshes._adjacency = meshes._adjacency                    # same face table
            def1imgs, _, _ = _render(cmeshes, newcameras, H, W, def1_lights)
            def1imgs = _to_uint8(def1imgs)
            clock.lap('shading')
            batch_inds, row_inds, col_inds, initTmpPs, _ = utils.FindSurfacePs(TmpVs, Tmpfs, frags)
            rays = cameras.view_rays_pix(col_inds, row_inds)
            defconds = [d_cond, [poses, trans]]
            clock.lap('surface_points')
        colors = None
        if not notcolor:
            colors = _color_branch(loop, g_i, name, cameras, rays, initTmpPs, batch_inds, defconds, rendcond, ratio, chunk,
                                   clock)
            canvas = torch.ones(N, H, W, 3, device=device) * 255.
            canvas[batch_inds, row_inds, col_inds, :] = colors
            if gts and 'image' in gts:
                canvas[~masks] = gts['image'].to(device)[~masks][:, :3] * 255.
            colors = canvas.cpu().numpy().astype(np.uint8)
            clock.lap('color')
        out['colors'].append(colors)
        out['imgs'].append(imgs)
        out['def1imgs'].append(def1imgs)
        out['defMeshVs'].append(defMeshVs)
        out['maskE'].append(maskE)
    return out


def _empty_garment(out, N, H, W, notcolor, gts, device):
    """A garment whose extraction found no surface: nothing covers a pixel (images of the background, maskE = 1 - 0 / |G|)."""
    maskE = None
    if gts:
        g = (gts['mask'].to(device) != 0).view(N, -1).sum(1)
        maskE = shading.mask_error(torch.stack([torch.zeros_like(g), g], 1)).cpu().numpy()
        gts['maskE'] = maskE
        imgs = (gts['image'].to(device)[..., [2, 1, 0]] if 'image' in gts else torch.ones(N, H, W, 3, device=device))
    else:
        imgs = torch.ones(N, H, W, 4, device=device)
    colors = None
    if not notcolor:
        colors = (gts['image'].to(device)[..., :3] * 255. if gts and 'image' in gts
                  else torch.ones(N, H, W, 3, device=device) * 255.).cpu().numpy().astype(np.uint8)
    out['colors'].append(colors)
    out['imgs'].append(_to_uint8(imgs))
    out['def1imgs'].append(np.full((N, H, W, 4), 255, np.uint8))
    out['defMeshVs'].append(np.zeros((N, 0, 3), np.float32))
    out['maskE'].append(maskE)


def _color_branch(loop, g_i, name, cameras, rays, initTmpPs, batch_inds, defconds, rendcond, ratio, chunk, clock):
    """:3271-3296 — per chunk of rays: root finder, SDF normal, cardinal rays, colour net; clamp((c/2 + .5) * 255).  Every
    step is per ray (the kernels' rows are independent), so the colours do not depend on `chunk`."""
    net = loop.garment_nets[g_i]
    cam_pos = cameras.cam_pos().detach()
    tcolors = []
    for rays_, ps_, b_ in zip(torch.split(rays, chunk), torch.split(initTmpPs, chunk), torch.split(batch_inds, chunk)):
        with torch.no_grad():
            ps_, _check = utils.OptimizeGarmentSurfaceSinlge(cam_pos, rays_.detach(), ps_.clone(), b_, net, ratio,
                                                             loop.deformer, defconds, dthreshold=1.e-4,
                                                             athreshold=loop.angThred, w1=3.05, w2=1., times=30,
                                                             offset_type=name)
        clock.lap('root_finding')
        with torch.enable_grad():
            ps_ = ps_.detach().clone().requires_grad_(True)
            sdfs = net(ps_, ratio)
            feats = net.rendcond
            nx = torch.autograd.grad(sdfs, ps_, torch.ones_like(sdfs), retain_graph=False, create_graph=False)[0]
            nx = nx / nx.norm(dim=1, keepdim=True)
            crays, defVs = utils.compute_cardinal_rays(loop.deformer, ps_, rays_, defconds, b_, ratio, 'test',
                                                       offset_type=name)
        with torch.no_grad():
            c = utils.compute_netRender_color(loop.netRender, ps_.detach(), defVs.detach(), nx.detach(), crays.detach(),
                                              feats.detach(), rendcond[b_] if rendcond is not None else None, ratio)
            tcolors.append(c)
        clock.lap('color')
    if not tcolors:
        return torch.zeros(0, 3, device=rays.device)
    return torch.clamp((torch.cat(tcolors, dim=0) / 2. + 0.5) * 255., min=0., max=255.)


def infer(loop, TmpVs_list, Tmpfs_list, H, W, ratio, frame_ids, notcolor=False, gts=None):
    """OptimGarmentNetwork.infer (:3216-3306): (colors_list, imgs_list, def1imgs_list, defMeshVs_list) of numpy arrays;
    with `notcolor` the reference returns after its first garment: (None, imgs, def1imgs, defMeshVs).  With `gts`,
    gts['maskE'] is set to the mask error of the last garment rendered."""
    if notcolor:
        r = infer_garments(loop, TmpVs_list, Tmpfs_list, H, W, ratio, frame_ids, True, gts, garments=(0,))
        return None, r['imgs'][0], r['def1imgs'][0], r['defMeshVs'][0]
    r = infer_garments(loop, TmpVs_list, Tmpfs_list, H, W, ratio, frame_ids, False, gts)
    return r['colors'], r['imgs'], r['def1imgs'], r['defMeshVs']


@torch.no_grad()
def posed_body(loop, frame_ids, ratio=None):
    """The canonical body template posed by the skinner with each frame's pose and translation (deformer.defs[1]):
    (vertices [N,V,3], faces [F,3]) — what infer_fl.py writes to smpl_meshs/."""
    loop._ensure_body_template()
    _, poses, trans, _ = loop.get_grad_parameters(frame_ids, loop.device)
    N = frame_ids.numel()
    vs = loop.deformer.defs[1](loop.tmpBodyVs.view(1, -1, 3).expand(N, -1, 3), [poses.detach(), trans.detach()])
    return vs, loop.tmpBodyFs


@torch.no_grad()
def merged_render(loop, defMeshVs_list, Tmpfs_list, colors, H, W):
    """The merged render of infer_garment (OptimGarmentNetwork.py:3077-3117): every garment's posed mesh of each frame as
    one mesh, garment g in the flat RGB colour colors[g] (0-255), through the dataset camera and the Phong shader:
    uint8 [N,H,W,3] RGB and the coverage masks [N,H,W] bool."""
    device = Tmpfs_list[0].device
    focals, pps, Rs, Ts, _, _ = loop.dataset.get_camera_parameters(1, device)
    cameras = RectifiedPerspectiveCameras(focals.detach(), pps.detach(), Rs.detach(), Ts.detach(), image_size=[(W, H)])
    vs, fs, cs = [], [], []
    offset = 0
    for defVs, fc, col in zip(defMeshVs_list, Tmpfs_list, colors):
        v = torch.as_tensor(defVs).to(device)
        vs.append(v)
        fs.append(fc.to(device) + offset)
        cs.append(torch.tensor(col, dtype=torch.float32, device=device).div(255.).expand(v.shape[1], 3))
        offset += v.shape[1]
    verts = torch.cat(vs, 1).contiguous()
    meshes = shading.Meshes(verts, torch.cat(fs, 0).contiguous(), shading.TexturesVertex(torch.cat(cs, 0)[None].contiguous()))
    imgs, frags, _ = _render(meshes, cameras, H, W, shading.PointLights())
    return _to_uint8(imgs[..., :3]), (frags.pix_to_face[..., 0] >= 0).cpu().numpy()


def animation_conditions(loop, N, device):
    """The conditions an animation is driven with (:2767-2771): every garment's deformer code, the translation and the colour
    code averaged over the capture's `origin_size()` frames, one (identical) row per animated frame: (d_cond_list over the
    garments, trans [N,3], rendcond [N,C] or None)."""
    ds = loop.dataset
    n_capture = ds.origin_size() if hasattr(ds, 'origin_size') else len(ds)
    d_cond_list, _, trans, rendcond = loop.get_grad_parameters(torch.arange(n_capture, device=device), device)
    mean = lambda t: t.detach().mean(0, keepdim=True).expand(N, -1).contiguous()  # noqa: E731
    return [mean(c) for c in d_cond_list[1:]], mean(trans), (mean(rendcond) if rendcond is not None else None)


def animation_meshes(loop, TmpVs_list, Tmpfs_list, root=None):
    """The meshes an animation poses: the registered templates `root/registry_<garment>.obj` (register_fl.py) when every one
    of them exists, else the meshes passed in.  (The reference registers on the first call, :2734-2738; here registration
    stays the separate command it is.)"""
    import os.path as osp
    from . import registration
    if root is not None and all(osp.isfile(registration.registry_path(root, n)) for n in loop.garment_names):
        meshes = registration.register_garments(loop, None, TmpVs_list, Tmpfs_list, root)
        return [v for v, _ in meshes], [f for _, f in meshes]
    return list(TmpVs_list), list(Tmpfs_list)


def infer_garment_animation(loop, TmpVs_list, Tmpfs_list, poses_y, H, W, ratio, frame_ids, root=None, notcolor=False,
                            fix_collisions=False, collision_eps=None, collision_max_depth=None, collision_iters=None,
                            collision_stats=None, chunk=COLOR_CHUNK, intersection_stats=None,
                            intersection_penetration=False):
    """OptimGarmentNetwork.infer_garment_animation (:2729-2859): the garments driven by the poses `poses_y` [N,72] (or
    [N,24,3]) with the capture's averaged conditions (`animation_conditions`).  Returns (colors_list, imgs_list,
    defMeshVs_list) of numpy arrays, one entry per garment: `colors` uint8 [N,H,W,3] (None with `notcolor`), `imgs` uint8
    [N,H,2W,3] — the Phong render of the posed body template on the left, of the posed garment on the right — and
    `defMeshVs` float32 [N,V,3].  `root`: the run folder whose registry_<garment>.obj files are posed when present
    (`animation_meshes`).  The reference runs one frame per call (its averaged conditions have one row); here every row of
    `poses_y` is a frame.
    Addition, off by default: `fix_collisions` repairs each garment against the posed body (recmv.collide.resolve with
    `collision_eps`, `collision_max_depth`, `collision_iters`) before it is rendered and returned; `collision_stats` (a
    dict) then receives {garment: resolve's stats}.  The colour branch, which renders the implicit surface through the
    deformer, is not affected by the repair.  `intersection_stats` (a list) receives recmv.collide.intersection_report of
    the meshes returned (after the repair when both are asked for), one entry per frame; `intersection_penetration` is
    its `penetration` option (the garment vertices inside the body and their largest depth)."""
    from . import collide
    device = TmpVs_list[0].device
    N = frame_ids.numel()
    poses = poses_y.to(device).float().reshape(-1, 24, 3)
    if poses.shape[0] != N:
        raise ValueError("infer_garment_animation: %d poses for %d frame ids" % (poses.shape[0], N))
    TmpVs_list, Tmpfs_list = animation_meshes(loop, TmpVs_list, Tmpfs_list, root)
    focals, pps, Rs, Ts, _, _ = loop.dataset.get_camera_parameters(1, device)
    with torch.no_grad():
        cameras = RectifiedPerspectiveCameras(focals.detach(), pps.detach(), Rs.detach(), Ts.detach(), image_size=[(W, H)])
        d_cond_list, trans, rendcond = animation_conditions(loop, N, device)
        loop._ensure_body_template()
        body_vs = loop.deformer.defs[1](loop.tmpBodyVs.view(1, -1, 3).expand(N, -1, 3), [poses, trans]).contiguous()
        body = shading.Meshes(body_vs, loop.tmpBodyFs, shading.TexturesVertex(torch.ones_like(loop.tmpBodyVs)[None]))
        smpl_imgs = _to_uint8(_render(body, cameras, H, W, shading.PointLights())[0][..., :3])
    colors_list, imgs_list, defMeshVs_list = [], [], []
    posed = {}
    for g_i, (TmpVs, Tmpfs, name) in enumerate(zip(TmpVs_list, Tmpfs_list, loop.garment_names)):
        TmpVs = TmpVs.detach()
        d_cond = d_cond_list[g_i]
        if TmpVs.shape[0] == 0 or Tmpfs.shape[0] == 0:                 # no surface: nothing covers a pixel
            blank = np.full((N, H, W, 3), 255, np.uint8)
            colors_list.append(None if notcolor else blank)
            imgs_list.append(np.concatenate([smpl_imgs, blank], axis=2))
            defMeshVs_list.append(np.zeros((N, 0, 3), np.float32))
            continue
        with torch.no_grad():
            defTmpVs = loop.deformer(TmpVs[None, :, :].expand(N, -1, 3), [d_cond, [poses, trans]], ratio=ratio,
                                     offset_type=name).contiguous()
            if fix_collisions:
                kw = {k: v for k, v in (('eps', collision_eps), ('max_depth', collision_max_depth),
                                        ('iters', collision_iters)) if v is not None}
                defTmpVs, stats = collide.resolve(defTmpVs, body_vs, loop.tmpBodyFs, **kw)
                if collision_stats is not None:
                    collision_stats[name] = stats
            meshes = shading.Meshes(defTmpVs, Tmpfs, shading.TexturesVertex(torch.ones_like(TmpVs)[None]))
            imgs, frags, _ = _render(meshes, cameras, H, W, shading.PointLights())
            imgs = np.concatenate([smpl_imgs, _to_uint8(imgs[..., :3])], axis=2)
            colors = None
            if not notcolor:
                batch_inds, row_inds, col_inds, initTmpPs, _ = utils.FindSurfacePs(TmpVs, Tmpfs, frags)
                rays = cameras.view_rays_pix(col_inds, row_inds)
        if not notcolor:
            tcolors = _color_branch(loop, g_i, name, cameras, rays, initTmpPs, batch_inds, [d_cond, [poses, trans]], rendcond,
                                    ratio, chunk, _Clock(None, device))
            canvas = torch.ones(N, H, W, 3, device=device) * 255.
            canvas[batch_inds, row_inds, col_inds, :] = tcolors
            colors = canvas.cpu().numpy().astype(np.uint8)
        colors_list.append(colors)
        imgs_list.append(imgs)
        defMeshVs_list.append(defTmpVs.cpu().numpy())
        posed[name] = (defTmpVs, Tmpfs)
    if intersection_stats is not None:
        intersection_stats.extend(collide.intersection_report(posed, body_vs, loop.tmpBodyFs,
                                                              penetration=intersection_penetration))
    return colors_list, imgs_list, defMeshVs_list


class CurveMesh:
    """What `infer_garment_fl` returns in place of the reference's `trimesh.Trimesh(vertices, faces, process=False)`."""

    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces

    def export(self, path):
        utils.write_obj(path, self.vertices, self.faces)


def infer_garment_fl(loop, TmpVs_list, Tmpfs_list, H, W, ratio, frame_ids, notcolor=False, gts=None, root=None,
                     curve_radius=0.002, num_joints=6):
    """OptimGarmentNetwork.infer_garment_fl (:2861-2935): the feature curves as thin tubes (`Intersect_Free_Curve.
    curve_to_mesh`, built on the first call and kept in `loop.fl_curve_meshes`), per garment the tubes of FL_EXTRACT[garment]
    posed together by the deformer with that garment's code, all merged into one mesh: a `CurveMesh` with `.vertices`
    [sum S*J,3] float32 and `.faces` int64 on the host and `.export(path)`.  As in the reference only the first frame of
    `frame_ids` is returned (its `[0]` after the deformer) and the meshes, sizes and `notcolor` / `gts` / `root` play no
    part.  `curve_radius` / `num_joints` (additions) only count on the call that builds the tubes."""
    if getattr(loop, 'fl_curve_meshes', None) is None:
        loop.fl_curve_meshes = loop.inter_free_curve.curve_to_mesh(curve_radius=curve_radius, num_joints=num_joints)
    fl_map = {name: i for i, name in enumerate(loop.fl_names)}
    device = loop.fl_curve_meshes[0].verts.device
    N = frame_ids.numel()
    verts_list, faces_list = [], []
    with torch.no_grad():
        d_cond_list, poses, trans, _ = loop.get_grad_parameters(frame_ids, device)
        d_cond_list = d_cond_list[1:]                                  # idx 0: the body's code
        extract = getattr(loop, 'fl_extract', None) or {}
        for g_i, name in enumerate(loop.garment_names):
            lines = extract[name] if name in extract else FL_EXTRACT[name]
            meshes = [loop.fl_curve_meshes[fl_map[fl]] for fl in lines]
            if not meshes:
                continue
            sizes = [m.verts_packed().shape[0] for m in meshes]
            TmpVs = torch.cat([m.verts_packed() for m in meshes], dim=0)
            defTmpVs = loop.deformer(TmpVs[None, :, :].expand(N, -1, 3), [d_cond_list[g_i], [poses, trans]], ratio=ratio,
                                     offset_type=name)[0]
            verts_list.extend(torch.split(defTmpVs, sizes))
            faces_list.extend(m.faces_packed() for m in meshes)
    offset, faces = 0, []
    for v, f in zip(verts_list, faces_list):
        faces.append(f + offset)
        offset += v.shape[0]
    if not verts_list:
        return CurveMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64))
    return CurveMesh(torch.cat(verts_list).detach().cpu(), torch.cat(faces).detach().cpu())
