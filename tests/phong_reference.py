"""Plain torch restatement of pytorch3d 0.4.0's vertex normals and hard Phong shading, the yardstick of
recmv.shading (csrc/shade_meshes.hip).  pytorch3d is not installed; the functions restated are:
  pytorch3d/structures/meshes.py        Meshes._compute_vertex_normals
  pytorch3d/ops/interp_face_attrs.py    interpolate_face_attributes
  pytorch3d/renderer/mesh/shading.py    phong_shading, _apply_lighting
  pytorch3d/renderer/lighting.py        diffuse, specular, PointLights
  pytorch3d/renderer/blending.py        hard_rgb_blend (alpha channel 1)
Computed on the host in float32."""
import torch
import torch.nn.functional as F


def verts_normals_ref(verts, faces):
    """verts [V,3], faces [F,3] -> [V,3]: three index_adds in corner order 1, 2, 0, then F.normalize(eps=1e-6)."""
    verts, faces = verts.float().cpu(), faces.long().cpu()
    vf = verts[faces]
    n = torch.zeros_like(verts)
    n = n.index_add(0, faces[:, 1], torch.cross(vf[:, 2] - vf[:, 1], vf[:, 0] - vf[:, 1], dim=1))
    n = n.index_add(0, faces[:, 2], torch.cross(vf[:, 0] - vf[:, 2], vf[:, 1] - vf[:, 2], dim=1))
    n = n.index_add(0, faces[:, 0], torch.cross(vf[:, 1] - vf[:, 0], vf[:, 2] - vf[:, 0], dim=1))
    return F.normalize(n, eps=1e-6, dim=1)


def _interp(p2f, bary, face_vals):
    """interpolate_face_attributes: p2f [N,H,W,1] packed, bary [N,H,W,1,3], face_vals [NF,3,D] -> [N,H,W,1,D]."""
    mask = p2f < 0
    idx = p2f.clamp(min=0)
    vals = face_vals[idx]                                                    # [N,H,W,1,3,D]
    out = (bary[..., None] * vals).sum(dim=-2)
    out[mask] = 0.
    return out


def hard_phong_ref(p2f, bary, verts, faces, normals, colors, cam_centers, light_location=(0., 1., 0.),
                   light_ambient=(0.5,) * 3, light_diffuse=(0.3,) * 3, light_specular=(0.2,) * 3,
                   mat_ambient=(1.,) * 3, mat_diffuse=(1.,) * 3, mat_specular=(1.,) * 3, shininess=64.,
                   background=(1., 1., 1.)):
    """images [N,H,W,4] of pytorch3d's HardPhongShader for N meshes with one face table (verts / normals [N,V,3],
    colors [1 or N,V,3], cam_centers [N,3])."""
    p2f, bary = p2f.cpu(), bary.float().cpu()
    verts, normals, colors, faces = verts.float().cpu(), normals.float().cpu(), colors.float().cpu(), faces.long().cpu()
    N, V = verts.shape[:2]
    colors = colors.expand(N, -1, -1)
    packed = (faces[None] + (torch.arange(N) * V).view(N, 1, 1)).reshape(-1, 3)
    pts = _interp(p2f, bary, verts.reshape(-1, 3)[packed])
    nrm = _interp(p2f, bary, normals.reshape(-1, 3)[packed])
    tex = _interp(p2f, bary, colors.reshape(-1, 3)[packed])
    t = lambda x: torch.tensor(x, dtype=torch.float32)                      # noqa: E731
    # PointLights.diffuse / specular (lighting.py)
    direction = t(light_location).view(1, 1, 1, 1, 3) - pts
    n_ = F.normalize(nrm, p=2, dim=-1, eps=1e-6)
    d_ = F.normalize(direction, p=2, dim=-1, eps=1e-6)
    angle = F.relu(torch.sum(n_ * d_, dim=-1))
    light_diff = t(light_diffuse) * angle[..., None]
    cos_angle = torch.sum(n_ * d_, dim=-1)
    mask = (cos_angle > 0).to(torch.float32)
    view = F.normalize(cam_centers.float().cpu().view(N, 1, 1, 1, 3) - pts, p=2, dim=-1, eps=1e-6)
    reflect = -d_ + 2 * (cos_angle[..., None] * n_)
    alpha = F.relu(torch.sum(view * reflect, dim=-1)) * mask
    light_spec = t(light_specular) * torch.pow(alpha, shininess)[..., None]
    # _apply_lighting + phong_shading
    ambient = t(mat_ambient) * t(light_ambient)
    diffuse = t(mat_diffuse) * light_diff
    specular = t(mat_specular) * light_spec
    rgb = ((ambient + diffuse) * tex + specular)[..., 0, :]
    # hard_rgb_blend
    bg = p2f[..., 0] < 0
    rgb[bg] = t(background)
    return torch.cat([rgb, torch.ones(rgb.shape[:-1] + (1,))], dim=-1)
