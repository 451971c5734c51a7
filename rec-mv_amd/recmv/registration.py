"""Garment-template registration: `OptimGarmentNetwork.registration` (engineer/networks/OptimGarmentNetwork.py:2316-2514).

register_garments fits a template mesh to each reconstructed canonical garment by non-rigid ICP and writes
`root/registry_<garment>.obj`; when every such file exists it loads them instead (:2432-2440).  Per garment:
  surface_finder (:2321-2387)   12 views (0-330 deg about y, re-centred) through the dataset camera with R = diag(-1,1,-1) and
                                T = the mean dataset translation, on raster.MeshRasterizer: a target vertex counts when a
                                face that holds it is hit in some view (the NR-ICP target mask)
  fl_init_registry              with `curves`: Laplacian alignment of the template's boundary loops to the feature curves,
                                3 epochs (Laplacian_Optimizer, :2407, :2451-2454)
  fl_fit_registry               coarse NR-ICP, 200 epochs (:2411-2418)
  remesh_garment_mesh           with `iso_remesh`: isotropic remeshing, then Loop subdivision of the coarse result (:2477,
                                engineer/utils/garment_structure.py:440-458; recmv.iso_remesh)
  fl_refine_registry            refine NR-ICP, 100 epochs (:2420-2426)
Deviations: the templates are inputs (the SMPL-asset cut and `dense_boundary` are not done), their
boundary loops are assigned to the feature lines by centroid (recmv.lap_align.assign_loops), and the iso-remesh step is opt-in
(without it the coarse result keeps its topology into the refine pass), refines uniformly (MeshLab's Loop filter refines only
long edges), is not checked against pymeshlab, keeps boundary and crease vertices fixed and relaxes by the uniform one-ring
mean.  The reference's remesh_garment_mesh also writes nricp_coarse.obj / remesh.obj scratch files and copies the boundary
colour labels to the new mesh by nearest neighbour; plain templates carry no labels, so neither is done.
"""
import math
import os.path as osp

import torch

from . import iso_remesh as IR, nricp, raster, utils
from .engineer.optimizer import Laplacian_Optimizer, NRICP_Optimizer_AdamW
from .model import RectifiedPerspectiveCameras

# engineer/networks/OptimGarmentNetwork.py:2411-2426
FIT_REGISTRY = dict(epoch=200, dense_pcl=4e4, stiffness_weight=[50, 20, 5, 2, 0.8, 0.5, 0.35, 0.2, 0.1], use_normal=True,
                    inner_iter=50, mile_stone=[50, 80, 100, 110, 120, 130, 140, 150],
                    laplacian_weight=[250, 250, 250, 250, 250, 250, 250, 250, 250], threshold=0.3)
INIT_REGISTRY = dict(epoch=3, constrain_weight=1.)            # Laplacian_Optimizer() (:2407)
ISO_REMESH = dict(iterations=3, target_len_frac=0.01, feature_deg=30., subdiv_levels=1)   # pymeshlab's filter defaults
REFINE_REGISTRY = dict(epoch=100, dense_pcl=4e4, stiffness_weight=[2, 0.8, 0.5, 0.35, 0.2, 0.1], use_normal=True,
                       inner_iter=50, mile_stone=[10, 20, 30, 40, 80], laplacian_weight=[250, 250, 250, 250, 250, 250],
                       threshold=0.5)
_VIEW_R = ((-1., 0., 0.), (0., 1., 0.), (0., 0., -1.))
CULL_BACKFACES = False            # the loop's mask renderer does not cull (loop.py, :2336-2347)


def registry_path(root, name):
    return osp.join(root, 'registry_{}.obj'.format(name))


def _rotate_y(degree):
    """trimesh.transformations.rotation_matrix(radians(degree), [0, 1, 0])[:3, :3]."""
    a = math.radians(degree)
    c, s = math.cos(a), math.sin(a)
    return torch.tensor([[c, 0., s], [0., 1., 0.], [-s, 0., c]], dtype=torch.float32)


@torch.no_grad()
def surface_finder(loop, verts, faces):
    """bool [V]: the target vertices that some face hit in one of the 12 views holds (:2321-2387)."""
    device = verts.device
    focals, pps, _, _, H, W = loop.dataset.get_camera_parameters(1, device)
    newTs = loop.dataset.trans.detach().mean(0).to(device).view(1, 3)
    cams = RectifiedPerspectiveCameras(focals.detach(), pps.detach(), torch.tensor([_VIEW_R], device=device), newTs,
                                       image_size=[(W, H)])
    rast = raster.MeshRasterizer(cams, (H, W), blur_radius=0., perspective_correct=True, cull_backfaces=CULL_BACKFACES)
    seen = torch.zeros(verts.shape[0], dtype=torch.bool, device=device)
    for degree in range(0, 360, 30):
        v = verts @ _rotate_y(degree).to(device).t()
        v = v - v.mean(0, keepdim=True)
        p2f = rast(v[None].contiguous(), faces).pix_to_face[0, ..., 0]
        hit = p2f[p2f != -1]
        seen[faces[hit].reshape(-1)] = True
    return seen


def _iso_remesh(mesh, conf, use_kernels, log):
    """`registry_mesh.remesh_garment_mesh(root)` (:2477): isotropic remeshing, then Loop subdivision."""
    v, f = mesh.verts.detach(), mesh.faces
    diag = float((v.max(0)[0] - v.min(0)[0]).norm())
    v, f, _ = IR.isotropic_remesh(v, f, target_len=conf['target_len_frac'] * diag, iterations=conf['iterations'],
                                  feature_deg=conf['feature_deg'], use_kernels=use_kernels, log=log)
    v, f = IR.loop_subdivide(v, f, levels=conf['subdiv_levels'], use_kernels=use_kernels)
    if log is not None:
        log('iso-remesh: %d -> %d vertices, %d faces after %d Loop level(s)' % (
            mesh.verts.shape[0], v.shape[0], f.shape[0], conf['subdiv_levels']))
    return nricp.TriMesh(v.float().contiguous(), f.contiguous())


def register_garments(loop, templates, target_vs, target_fs, root, fit=None, refine=None, use_kernels=True, log=print,
                      curves=None, align=None, iso_remesh=None):
    """Registered meshes [(verts [V,3], faces [F,3])] on the targets' device, one per `loop.garment_names` entry.
    `templates`: one (verts, faces) per garment; `target_vs` / `target_fs`: the canonical garment meshes.  `fit` / `refine`
    update the NR-ICP settings of the two passes (FIT_REGISTRY, REFINE_REGISTRY).  `curves` ({fl_name: [S,3]}, the run's
    feature curves): align each template to them by Laplacian deformation before NR-ICP; `align` updates that step's
    settings (INIT_REGISTRY: epoch, constrain_weight).  Without `curves` the templates go to NR-ICP as they are.
    `iso_remesh` (a dict, possibly empty, updating ISO_REMESH: iterations, target_len_frac, feature_deg, subdiv_levels):
    iso-remesh the coarse pass's mesh before the refine pass; None leaves it as it is."""
    names = list(loop.garment_names)
    device = target_vs[0].device if target_vs else torch.device(loop.device)
    paths = [registry_path(root, n) for n in names]
    if all(osp.isfile(p) for p in paths):
        out = []
        for p in paths:
            v, f = utils.read_obj(p)
            out.append((v.float().to(device), f.long().to(device)))
        return out
    if not (len(templates) == len(target_vs) == len(target_fs) == len(names)):
        raise ValueError("one template and one target mesh per garment (%s)" % ", ".join(names))
    fit_conf = dict(FIT_REGISTRY, **(fit or {}))
    refine_conf = dict(REFINE_REGISTRY, **(refine or {}))
    init_conf = dict(INIT_REGISTRY, **(align or {}))
    iso_conf = None if iso_remesh is None else dict(ISO_REMESH, **iso_remesh)
    if iso_conf is not None and set(iso_conf) != set(ISO_REMESH):
        raise ValueError("iso_remesh: unknown setting(s) %s" % ", ".join(sorted(set(iso_conf) - set(ISO_REMESH))))
    out = []
    for name, (tv, tf), gv, gf, path in zip(names, templates, target_vs, target_fs, paths):
        gv, gf = gv.detach().float().contiguous(), gf.long().contiguous()
        masks = surface_finder(loop, gv, gf)
        target = nricp.TriMesh(gv, gf)
        mesh = nricp.TriMesh(torch.as_tensor(tv).float().to(device), torch.as_tensor(tf).long().to(device))
        if curves is not None:
            names_fl = list(curves)
            Laplacian_Optimizer(use_kernels=use_kernels, log=log, **init_conf)(
                source_fl_meshes=[mesh], target_meshes=[curves[n].to(device) for n in names_fl], source_type=[name],
                target_fl_type=names_fl, outlayer=True)
        for conf in (fit_conf, refine_conf):
            if conf is refine_conf and iso_conf is not None:
                mesh = _iso_remesh(mesh, iso_conf, use_kernels, log)
            opt = NRICP_Optimizer_AdamW(device=device, use_kernels=use_kernels, log=log, **conf)
            _, mesh = opt(smpl_slice=mesh, cano_meshes=target, save_path=None, garment_name=name, static_pts_type=[],
                          nricp_masks=masks)
        utils.write_obj(path, mesh.verts.cpu(), mesh.faces.cpu())
        out.append((mesh.verts.detach(), mesh.faces))
    return out
