"""Hard Phong shading of rasterised meshes on the HIP kernels of csrc/shade_meshes.hip (inference only).

Stands where the reference's inference uses pytorch3d 0.4.0's `MeshRendererWithFragments(MeshRasterizer, HardPhongShader)`
with `PointLights`, `Materials`, `TexturesVertex` and the meshes' vertex normals (engineer/networks/OptimGarmentNetwork.py:
3216-3306 `infer`; infer_fl.py sets `maskRender.shader = HardPhongShader(device, cameras)`).  Parameter names and defaults
are pytorch3d's.  Batches are N meshes that share ONE face table (one garment posed in N frames), the only case the
reference renders.  No autograd through the shader, no CPU path: host tensors are refused.
"""
from collections import namedtuple

import torch

from . import _lib as L
from . import raster

BlendParams = namedtuple("BlendParams", ["sigma", "gamma", "background_color"])
BlendParams.__new__.__defaults__ = (1e-4, 1e-4, (1.0, 1.0, 1.0))


def _rgb(x, name):
    t = torch.as_tensor(x, dtype=torch.float32).detach().cpu().reshape(-1)
    if t.numel() != 3:
        raise ValueError("%s: one RGB triple / 3-vector is supported (got %d values)" % (name, t.numel()))
    return [float(v) for v in t]


class PointLights:
    """pytorch3d.renderer.PointLights: one point light (the reference renders with one per call)."""

    def __init__(self, ambient_color=((0.5, 0.5, 0.5),), diffuse_color=((0.3, 0.3, 0.3),),
                 specular_color=((0.2, 0.2, 0.2),), location=((0, 1, 0),), device="cpu"):
        self.ambient_color = _rgb(ambient_color, "ambient_color")
        self.diffuse_color = _rgb(diffuse_color, "diffuse_color")
        self.specular_color = _rgb(specular_color, "specular_color")
        self.location = _rgb(location, "location")
        self.device = device


class Materials:
    """pytorch3d.renderer.Materials."""

    def __init__(self, ambient_color=((1, 1, 1),), diffuse_color=((1, 1, 1),), specular_color=((1, 1, 1),),
                 shininess=64, device="cpu"):
        self.ambient_color = _rgb(ambient_color, "ambient_color")
        self.diffuse_color = _rgb(diffuse_color, "diffuse_color")
        self.specular_color = _rgb(specular_color, "specular_color")
        self.shininess = float(torch.as_tensor(shininess, dtype=torch.float32).reshape(-1)[0])
        self.device = device


class TexturesVertex:
    """pytorch3d.renderer.TexturesVertex: per-vertex colours, a list of [V,3] or a tensor [N,V,3]; a batch of 1 serves
    every mesh."""

    def __init__(self, verts_features):
        if isinstance(verts_features, (list, tuple)):
            verts_features = torch.stack(list(verts_features))
        self.verts_features = verts_features

    def verts_features_padded(self):
        return self.verts_features


class Meshes:
    """The part of pytorch3d's `Meshes` the renderer reads, for N meshes with one face table: verts [N,V,3] (or a list
    of N [V,3]), faces [F,3] int64 (or a list of N references to one face table)."""

    def __init__(self, verts, faces, textures=None):
        if isinstance(verts, (list, tuple)):
            verts = torch.stack([v.reshape(-1, 3) for v in verts])
        if isinstance(faces, (list, tuple)):
            if any(f.shape != faces[0].shape for f in faces):
                raise ValueError("Meshes: the meshes of a batch share one face table")
            faces = faces[0]
        self.verts = verts
        self.faces = faces
        self.textures = textures
        self._normals = None
        self._adjacency = None

    def __len__(self):
        return self.verts.shape[0]

    def verts_padded(self):
        return self.verts

    def verts_packed(self):
        return self.verts.reshape(-1, 3)

    def faces_packed(self):
        """The face table of a single mesh (a batch shares one table: packing it would need per-mesh offsets)."""
        if len(self) != 1:
            raise ValueError("faces_packed: a batch of %d meshes shares one face table" % len(self))
        return self.faces

    def verts_normals_padded(self):
        if self._normals is None:
            if self._adjacency is None:
                self._adjacency = vertex_face_adjacency(self.faces, self.verts.shape[1])
            self._normals = verts_normals(self.verts, self.faces, self._adjacency)
        return self._normals


def vertex_face_adjacency(faces, V):
    """Vertex -> (face, corner) lists of a face table [F,3] int64 on the device, in pytorch3d's summation order of
    `Meshes._compute_vertex_normals` (three `index_add`s: corner 1, corner 2, corner 0, each over the faces in order):
    (offsets int32 [V+1], codes int32 [3F], code = face * 3 + corner).  A stable sort, so the order is unique."""
    L.require_cuda(faces, "faces")
    if faces.dtype != torch.int64 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be int64 of shape [F,3]")
    F, V = faces.shape[0], int(V)
    if 3 * F >= 2 ** 31 or V >= 2 ** 31:
        raise ValueError("vertex_face_adjacency: at most 2^31 / 3 faces and 2^31 vertices")
    dev = faces.device
    if F > 0:
        lo, hi = torch.aminmax(faces)
        if int(lo) < 0 or int(hi) >= V:
            raise ValueError("faces index vertices outside [0, %d)" % V)
    order = [1, 2, 0]
    vid = faces[:, order].t().reshape(-1)                                          # [corner1 faces | corner2 | corner0]
    codes = (torch.arange(F, device=dev, dtype=torch.int64).view(1, F) * 3
             + torch.tensor(order, device=dev, dtype=torch.int64).view(3, 1)).reshape(-1)
    _, perm = torch.sort(vid, stable=True)
    counts = torch.bincount(vid, minlength=V)
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets.to(torch.int32).contiguous(), codes[perm].to(torch.int32).contiguous()


@torch.no_grad()
def verts_normals(verts, faces, adjacency=None):
    """pytorch3d `Meshes.verts_normals_padded` for N meshes with one face table: verts [N,V,3] (or [V,3]) f32 CUDA,
    faces [F,3] int64 -> unit normals of the same shape.  `adjacency`: vertex_face_adjacency(faces, V), built here when
    not given (keep it when the same face table is used again)."""
    L.require_cuda(verts, "verts")
    squeeze = verts.dim() == 2
    v3 = verts.unsqueeze(0) if squeeze else verts
    if v3.dtype != torch.float32 or v3.dim() != 3 or v3.shape[2] != 3:
        raise ValueError("verts must be float32 of shape [N,V,3] or [V,3]")
    v3 = v3.contiguous()
    N, V = v3.shape[0], v3.shape[1]
    if adjacency is None:
        adjacency = vertex_face_adjacency(faces, V)
    offsets, codes = adjacency
    L.require_cuda(faces, "faces")
    L.require_contiguous(faces, "faces")
    if offsets.numel() != V + 1 or codes.numel() != 3 * faces.shape[0]:
        raise ValueError("adjacency does not belong to this face table / vertex count")
    out = torch.empty_like(v3)
    with L.device_guard(v3.device):
        L.check(L.lib().recmv_verts_normals(L.ptr(v3), L.ptr(faces), L.ptr(offsets), L.ptr(codes), N, V, faces.shape[0],
                                            L.ptr(out), L.stream_ptr(v3.device)), "verts_normals")
    return out[0] if squeeze else out


def _camera_centers(cameras, N, device):
    """Camera centre -R T of each image (pytorch3d's `get_camera_center`; RectifiedPerspectiveCameras.cam_pos)."""
    if hasattr(cameras, "cam_pos"):
        nc = cameras.R.shape[0]
        c = torch.stack([cameras.cam_pos(i) for i in range(nc)]) if nc > 1 else cameras.cam_pos().view(1, 3)
    else:
        c = cameras.get_camera_center()
    c = c.detach().to(device=device, dtype=torch.float32).reshape(-1, 3)
    if c.shape[0] not in (1, N):
        raise ValueError("one camera, or one per mesh")
    return c.expand(N, 3).contiguous()


@torch.no_grad()
def hard_phong_shade(fragments, verts, faces, normals, colors, cam_centers, lights=None, materials=None,
                     blend_params=None, gt_mask=None):
    """HardPhongShader + hard_rgb_blend on the fragments of raster.MeshRasterizer: images [N,H,W,4] f32 (RGB, alpha 1).
    With `gt_mask` [N,H,W] (nonzero = inside) also the per-frame integer counts [N,2] int64 (|M n G|, |M u G|),
    M = pix_to_face >= 0, the terms of the reference's mask error (OptimGarmentNetwork.py:3241-3243)."""
    lights = lights or PointLights()
    materials = materials or Materials()
    blend_params = blend_params or BlendParams()
    p2f, bary = fragments.pix_to_face, fragments.bary_coords
    for t, name in ((p2f, "pix_to_face"), (bary, "bary_coords"), (verts, "verts"), (faces, "faces"), (normals, "normals"),
                    (colors, "colors"), (cam_centers, "cam_centers")):
        L.require_cuda(t, name)
    if p2f.dim() != 4 or p2f.shape[-1] != 1 or p2f.dtype != torch.int64:
        raise ValueError("pix_to_face must be int64 [N,H,W,1] (faces_per_pixel = 1)")
    N, H, W = p2f.shape[:3]
    if tuple(bary.shape) != (N, H, W, 1, 3) or bary.dtype != torch.float32:
        raise ValueError("bary_coords must be float32 [N,H,W,1,3]")
    if verts.dim() != 3 or verts.shape[0] != N or verts.shape[2] != 3 or verts.dtype != torch.float32:
        raise ValueError("verts must be float32 [N,V,3] with one mesh per image")
    V = verts.shape[1]
    if normals.shape != verts.shape or normals.dtype != torch.float32:
        raise ValueError("normals must be float32 of verts' shape")
    if colors.dim() != 3 or colors.shape[0] not in (1, N) or colors.shape[1:] != verts.shape[1:]:
        raise ValueError("colors must be [1,V,3] or [N,V,3]")
    if faces.dtype != torch.int64 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be int64 [F,3]")
    if tuple(cam_centers.shape) != (N, 3):
        raise ValueError("cam_centers must be [N,3]")
    p2f, bary = p2f.contiguous(), bary.contiguous()
    verts, normals, faces = verts.contiguous(), normals.contiguous(), faces.contiguous()
    colors = colors.to(torch.float32).contiguous()
    cam_centers = cam_centers.to(torch.float32).contiguous()
    lib = L.lib()
    params = (lights.location + lights.ambient_color + lights.diffuse_color + lights.specular_color
              + materials.ambient_color + materials.diffuse_color + materials.specular_color + [materials.shininess]
              + _rgb(blend_params.background_color, "background_color"))
    assert len(params) == int(lib.recmv_hard_phong_params_floats())
    host = (L.C.c_float * len(params))(*params)
    dev = p2f.device
    images = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
    counts = None
    if gt_mask is not None:
        L.require_cuda(gt_mask, "gt_mask")
        if tuple(gt_mask.shape) != (N, H, W):
            raise ValueError("gt_mask must be [N,H,W]")
        gt_mask = gt_mask.to(torch.float32).contiguous()
        counts = torch.empty((N, 2), dtype=torch.int64, device=dev)
    with L.device_guard(dev):
        L.check(lib.recmv_hard_phong_shade(L.ptr(p2f), L.ptr(bary), L.ptr(verts), L.ptr(normals), L.ptr(colors),
                                           colors.shape[0], L.ptr(faces), L.ptr(cam_centers), N, V, faces.shape[0], H, W,
                                           host, L.ptr(images), L.ptr(gt_mask), L.ptr(counts), L.stream_ptr(dev)),
                "hard_phong_shade")
    return (images, counts) if gt_mask is not None else images


def mask_error(counts):
    """maskE = 1 - |M n G| / |M u G| per frame in float32: the reference's formula bit for bit while |M u G| < 2^24
    (its float sums of 0/1 pixels are exact there)."""
    c = counts.to(torch.float32)
    return 1. - c[:, 0] / c[:, 1]


class HardPhongShader:
    """pytorch3d.renderer.HardPhongShader(device, cameras, lights, materials, blend_params); `__call__(fragments, meshes,
    **kwargs)` with the same per-call overrides (cameras=, lights=, materials=, blend_params=)."""

    def __init__(self, device="cpu", cameras=None, lights=None, materials=None, blend_params=None):
        self.device = device
        self.cameras = cameras
        self.lights = lights if lights is not None else PointLights(device=device)
        self.materials = materials if materials is not None else Materials(device=device)
        self.blend_params = blend_params if blend_params is not None else BlendParams()

    def __call__(self, fragments, meshes, **kwargs):
        cameras = kwargs.get("cameras", self.cameras)
        if cameras is None:
            raise ValueError("Cameras must be specified either at initialization or in the forward pass of HardPhongShader")
        verts = meshes.verts_padded()
        N = verts.shape[0]
        colors = meshes.textures.verts_features_padded() if meshes.textures is not None else torch.ones_like(verts[:1])
        return hard_phong_shade(fragments, verts, meshes.faces, meshes.verts_normals_padded(), colors,
                                _camera_centers(cameras, N, verts.device), kwargs.get("lights", self.lights),
                                kwargs.get("materials", self.materials), kwargs.get("blend_params", self.blend_params))


class MeshRendererWithFragments:
    """pytorch3d.renderer.MeshRendererWithFragments(rasterizer, shader): `(images, fragments)`; a `cameras=` keyword
    re-targets the rasteriser for this call only, as pytorch3d's does."""

    def __init__(self, rasterizer, shader):
        self.rasterizer = rasterizer
        self.shader = shader

    def __call__(self, meshes, **kwargs):
        rast = self.rasterizer
        if kwargs.get("cameras") is not None:
            rast = raster.MeshRasterizer(kwargs["cameras"], rast.image_size, rast.blur_radius, rast.perspective_correct,
                                         rast.cull_backfaces)
        with torch.no_grad():
            fragments = rast(meshes.verts_padded().detach(), meshes.faces)
        kwargs.setdefault("cameras", rast.cameras)
        images = self.shader(fragments, meshes, **kwargs)
        return images, fragments
