"""Texture baking (csrc/texture_bake.hip) — an ADDITION to the reference: what the uv coordinates of recmv.param are for.

  fit_uv            a chart scaled uniformly (in texels) and centred in the image, `margin` texels from every side
  rasterize_uv      the chart rasterised in the UV plane: per texel the owning face, its barycentrics, the number of covering faces
  gutter, pad       edge padding as an index map, and the one gather that pads any baked map with it
  interpolate       a vertex attribute at every texel
  vertex_tangents   per-vertex tangent frames from the uv gradient
  project, transfer the covered texels projected on a source mesh (closest point, or along the normal), its attribute there
  encode_normal     a world-space normal in the texel's tangent frame, as a colour
  texels, scatter   the covered texels' positions and normals, and values put back into an image: the hook for any function
                    of a caller's own (the trained colour network is one)
  bake              all of it: position, normal, tangent_normal and color maps with a report

The definitions (the coverage rule, the texel box, the gutter order, the transfer formula, the tangent convention) are those of
include/recmv_hip.h and INTEGRATION.md §5.  Images are [H,W(,C)] with row 0 at v = 1, the OBJ convention.
"""
import numpy as np
import torch

from . import _lib as L

LANES = (8, 64)
# Mean texels per face box from which 64 lanes per face are launched.  Measured on an MI355X (profiles/bake_timing.json): 8 lanes
# are faster at a mean box of 21 and 67 texels (58 / 116 us and 148 / 162 us), 64 lanes at 455 and 1 747 (40 / 35 us and
# 114 / 88 us); 256 lies inside that bracket, the crossover itself is not measured.
LANES_SWITCH_AREA = 256.
MAPS = ('position', 'normal', 'tangent_normal', 'color')
PROJECTIONS = ('closest', 'normal')
HOW = {'closest': 0, 'forward': 1, 'backward': 2, 'fallback': 3}
MAX_CHANNELS = 16


def _size(size):
    H, W = (size, size) if isinstance(size, int) else tuple(int(x) for x in size)
    if H < 0 or W < 0 or H * W >= 2 ** 31:
        raise ValueError("size must be H, W >= 0 with fewer than 2^31 texels (got %r)" % (size,))
    return H, W


def _check_faces(faces):
    if not isinstance(faces, torch.Tensor) or faces.dtype != torch.int64 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be int64 of shape [F,3]")


def _check_uv(uv, V=None):
    if not isinstance(uv, torch.Tensor) or uv.dtype != torch.float64 or uv.dim() != 2 or uv.shape[1] != 2 or (
            V is not None and uv.shape[0] != V):
        raise ValueError("uv must be float64 of shape [%s,2]" % ("V" if V is None else V))


def _check_f32(t, cols, name, rows=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or (cols is not None and t.shape[1] != cols) or (
            rows is not None and t.shape[0] != rows):
        raise ValueError("%s must be float32 of shape [%s,%s]" % (name, "N" if rows is None else rows, "C" if cols is None else cols))


def _check_images(face, bary=None):
    if not isinstance(face, torch.Tensor) or face.dtype != torch.int32 or face.dim() != 2:
        raise ValueError("face must be int32 of shape [H,W]")
    if bary is not None and (not isinstance(bary, torch.Tensor) or bary.dtype != torch.float32 or bary.shape != face.shape + (3,)):
        raise ValueError("bary must be float32 of shape [H,W,3]")


def _cuda(*named):
    for t, name in named:
        L.require_cuda(t, name)


def fit_uv(uv, size, margin=0.):
    """uv [V,2] float64 -> unit coordinates [V,2] float64 on uv's device: one uniform scale in texels and a shift so that the
    chart keeps `margin` texels from every side of the H x W image and is centred in the rest (u = texel / W, v = texel / H).
    Host arithmetic in numpy float64, the restatement's."""
    H, W = _size(size)
    _check_uv(uv)
    a = uv.detach().cpu().numpy()
    margin = float(margin)
    avail = np.array([W - 2. * margin, H - 2. * margin])
    if a.shape[0] == 0 or not np.isfinite(a).all():
        raise ValueError("fit_uv: the chart must have finite vertices")
    lo = a.min(0)
    ext = a.max(0) - lo
    if not (margin >= 0 and avail.min() > 0 and ext.max() > 0):
        raise ValueError("fit_uv: the chart must not be a point and the margins must leave room (margin=%r, size=%r)" % (margin, (H, W)))
    s = min(avail[k] / ext[k] for k in range(2) if ext[k] > 0)
    off = margin + (avail - ext * s) / 2.
    return torch.from_numpy(((a - lo) * s + off) / np.array([float(W), float(H)])).to(uv.device)


def default_lanes(uv, faces, size):
    """8 or 64 lanes per face from the mean area of the faces' texel boxes; the choice changes the launch shape, never a bit."""
    H, W = _size(size)
    if faces.shape[0] == 0 or uv.shape[0] == 0:
        return 8
    c = uv[faces.clamp(0, uv.shape[0] - 1)]
    ext = (c.amax(1) - c.amin(1)).nan_to_num(0., 0., 0.)
    mean = float(((ext[:, 0] * W + 1.) * (ext[:, 1] * H + 1.)).clamp(max=float(H * W)).mean().item())
    return 64 if mean >= LANES_SWITCH_AREA else 8


@torch.no_grad()
def rasterize_uv(uv, faces, size, lanes=None):
    """recmv_bake_raster: (face [H,W] int32, -1 where no face covers the centre; bary [H,W,3] float32; count [H,W] int32) of the
    chart uv [V,2] float64 (unit coordinates), faces [F,3] int64.  The owner is the lowest covering face id."""
    H, W = _size(size)
    _check_uv(uv)
    _check_faces(faces)
    if lanes is not None and int(lanes) not in LANES:
        raise ValueError("lanes must be one of %r (got %r)" % (LANES, lanes))
    _cuda((uv, "uv"), (faces, "faces"))
    if uv.device != faces.device:
        raise ValueError("uv and faces must be on one device")
    uv, faces, dev = uv.contiguous(), faces.contiguous(), uv.device
    lanes = default_lanes(uv, faces, (H, W)) if lanes is None else int(lanes)
    face, count = L.scratch((H, W), torch.int32, dev), L.scratch((H, W), torch.int32, dev)
    bary = L.scratch((H, W, 3), torch.float32, dev)
    L.launch("bake_raster", dev, L.ptr(uv), uv.shape[0], L.ptr(faces), faces.shape[0], H, W, lanes, L.ptr(face), L.ptr(bary),
             L.ptr(count))
    return face, bary, count


@torch.no_grad()
def gutter(face, passes=4):
    """recmv_bake_gutter: src [H,W] int32, for every texel the linear index of the covered texel it copies (itself when covered),
    grown by `passes` rings in the order W, E, N, S, NW, NE, SW, SE; -1 beyond."""
    _check_images(face)
    if int(passes) < 0:
        raise ValueError("passes must not be negative (got %r)" % (passes,))
    _cuda((face, "face"))
    face, dev = face.contiguous(), face.device
    H, W = face.shape
    src = L.scratch((H, W), torch.int32, dev)
    tmp = L.scratch((H, W), torch.int32, dev) if int(passes) else None
    L.launch("bake_gutter", dev, L.ptr(face), H, W, int(passes), L.ptr(src), L.ptr(tmp))
    return src


_gutter = gutter                 # (bake() has a parameter of that name)


@torch.no_grad()
def pad(image, src):
    """recmv_bake_pad: image [H,W,C] (or [H,W]) float32 gathered through src [H,W]: zeros where src is -1."""
    if not isinstance(src, torch.Tensor) or src.dtype != torch.int32 or src.dim() != 2:
        raise ValueError("src must be int32 of shape [H,W]")
    if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() not in (2, 3) or image.shape[:2] != src.shape:
        raise ValueError("image must be float32 of shape [H,W] or [H,W,C] like src")
    _cuda((image, "image"), (src, "src"))
    image, src = image.contiguous(), src.contiguous()
    out = L.scratch(tuple(image.shape), torch.float32, image.device)
    T = src.numel()
    L.launch("bake_pad", image.device, L.ptr(image), L.ptr(src), T, image.numel() // T if T else 0, L.ptr(out))
    return out


@torch.no_grad()
def interpolate(face, bary, faces, attr, normalise=False):
    """recmv_bake_interpolate: the attribute attr [V,C] float32 (C <= 16) at every texel, [H,W,C] float32, (b0 a0 + b1 a1) + b2 a2
    in float32; zeros where there is no owner.  normalise: the first three channels to unit length (normals); zero stays zero."""
    _check_images(face, bary)
    _check_faces(faces)
    _check_f32(attr, None, "attr")
    C = attr.shape[1]
    if not 1 <= C <= MAX_CHANNELS or (normalise and C < 3):
        raise ValueError("attr must have 1 .. %d channels, at least 3 with normalise (got %d)" % (MAX_CHANNELS, C))
    _cuda((face, "face"), (bary, "bary"), (faces, "faces"), (attr, "attr"))
    face, bary, faces, attr, dev = face.contiguous(), bary.contiguous(), faces.contiguous(), attr.contiguous(), face.device
    out = L.scratch(tuple(face.shape) + (C,), torch.float32, dev)
    L.launch("bake_interpolate", dev, L.ptr(face), L.ptr(bary), face.numel(), L.ptr(faces), faces.shape[0], L.ptr(attr),
             attr.shape[0], C, int(bool(normalise)), L.ptr(out))
    return out


@torch.no_grad()
def vertex_tangents(verts, faces, uv, normals):
    """recmv_bake_vertex_tangents: [V,4] float32, the unit tangent (the direction of growing u, orthogonal to the vertex normal)
    and the handedness w = sign(cross(n, t) . bitangent): the bitangent is cross(n, t) w.  Area-weighted over the vertex's faces
    in the order of shading.vertex_face_adjacency; (0, 0, 0, 1) without a usable face."""
    _check_f32(verts, 3, "verts")
    _check_faces(faces)
    _check_uv(uv, verts.shape[0])
    _check_f32(normals, 3, "normals", verts.shape[0])
    _cuda((verts, "verts"), (faces, "faces"), (uv, "uv"), (normals, "normals"))
    from . import shading
    verts, faces, uv, normals = verts.contiguous(), faces.contiguous(), uv.contiguous(), normals.contiguous()
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    off, codes = shading.vertex_face_adjacency(faces, V)
    out = L.scratch((V, 4), torch.float32, dev)
    L.launch("bake_vertex_tangents", dev, L.ptr(verts), L.ptr(uv), L.ptr(normals), V, L.ptr(faces), F, L.ptr(off), L.ptr(codes),
             L.ptr(out))
    return out


@torch.no_grad()
def encode_normal(face, normal, frame_n, frame_t):
    """recmv_bake_encode_normal: the normals normal [H,W,3] in the frames (frame_t [H,W,4] = tangent and handedness, frame_n
    [H,W,3]; the tangent is made orthogonal to frame_n again) as 0.5 + 0.5 c, [H,W,3] float32; zeros where there is no owner."""
    _check_images(face)
    for t, c, name in ((normal, 3, "normal"), (frame_n, 3, "frame_n"), (frame_t, 4, "frame_t")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.shape != face.shape + (c,):
            raise ValueError("%s must be float32 of shape [H,W,%d]" % (name, c))
    _cuda((face, "face"), (normal, "normal"), (frame_n, "frame_n"), (frame_t, "frame_t"))
    dev = face.device
    out = L.scratch(tuple(face.shape) + (3,), torch.float32, dev)
    L.launch("bake_encode_normal", dev, L.ptr(face.contiguous()), L.ptr(normal.contiguous()), L.ptr(frame_n.contiguous()),
             L.ptr(frame_t.contiguous()), face.numel(), L.ptr(out))
    return out


def choose_hits(hit_f, t_f, hit_b, t_b):
    """The rule of project(..., 'normal') on boolean / float tensors or arrays: forward where it hits and is not farther than the
    backward hit (ties go forward), else backward where that hits, else the fallback."""
    forward = hit_f & (~hit_b | (t_f <= t_b))
    backward = hit_b & ~forward
    return forward, backward


def default_distance(src_verts):
    """project()'s default reach along the normal: 5 % of the diagonal of the source's bounding box."""
    return 0.05 * float((src_verts.amax(0) - src_verts.amin(0)).norm().item())


@torch.no_grad()
def project(positions, normals, src_verts, src_faces, projection='closest', max_distance=None, grid=None):
    """Where the points positions [P,3] (float32, with unit normals [P,3]) land on the source mesh: (src_face [P] int64,
    src_point [P,3] float32, how [P] uint8 with the codes of HOW).  'closest': MeshGrid.closest_point.  'normal': the first hits
    of the segments p -> p + d n and p -> p - d n (MeshGrid.segment_hits; d = max_distance, by default 5 % of the source's
    bounding-box diagonal); the nearer of the two, ties to the forward one; the closest point where neither hits."""
    if projection not in PROJECTIONS:
        raise ValueError("projection must be one of %r (got %r)" % (PROJECTIONS, projection))
    _check_f32(positions, 3, "positions")
    _check_f32(normals, 3, "normals", positions.shape[0])
    _check_f32(src_verts, 3, "src_verts")
    _check_faces(src_faces)
    if max_distance is not None and not float(max_distance) > 0:
        raise ValueError("max_distance must be positive (got %r)" % (max_distance,))
    _cuda((positions, "positions"), (normals, "normals"), (src_verts, "src_verts"), (src_faces, "src_faces"))
    from . import metrics
    grid = metrics.MeshGrid(src_verts, src_faces) if grid is None else grid
    positions = positions.contiguous()
    face, point, _ = grid.closest_point(positions)
    how = torch.full((positions.shape[0],), HOW['closest'], dtype=torch.uint8, device=positions.device)
    if projection == 'closest' or positions.shape[0] == 0:
        return face, point, how
    d = float(max_distance) if max_distance is not None else default_distance(src_verts)
    fwd = grid.segment_hits(positions, positions + d * normals)
    bwd = grid.segment_hits(positions, positions - d * normals)
    forward, backward = choose_hits(fwd['face'] >= 0, fwd['t'], bwd['face'] >= 0, bwd['t'])
    face = torch.where(forward, fwd['face'], torch.where(backward, bwd['face'], face))
    point = torch.where(forward[:, None], fwd['point'], torch.where(backward[:, None], bwd['point'], point))
    how.fill_(HOW['fallback'])
    how[forward] = HOW['forward']
    how[backward] = HOW['backward']
    return face, point.contiguous(), how


@torch.no_grad()
def transfer(src_face, src_point, src_verts, src_faces, src_attr, normalise=False, return_bary=False):
    """recmv_bake_transfer: the source attribute src_attr [SV,C] float32 at the hits (src_face [T] int64, src_point [T,3]
    float32): the point's barycentrics in its face (float64, the header's formula; a degenerate face gives (1, 0, 0)), then
    interpolate's mix.  [T,C] float32 (with return_bary: and the barycentrics [T,3])."""
    if not isinstance(src_face, torch.Tensor) or src_face.dtype != torch.int64 or src_face.dim() != 1:
        raise ValueError("src_face must be int64 of shape [T]")
    _check_f32(src_point, 3, "src_point", src_face.shape[0])
    _check_f32(src_verts, 3, "src_verts")
    _check_faces(src_faces)
    _check_f32(src_attr, None, "src_attr", src_verts.shape[0])
    C = src_attr.shape[1]
    if not 1 <= C <= MAX_CHANNELS or (normalise and C < 3):
        raise ValueError("src_attr must have 1 .. %d channels, at least 3 with normalise (got %d)" % (MAX_CHANNELS, C))
    _cuda((src_face, "src_face"), (src_point, "src_point"), (src_verts, "src_verts"), (src_faces, "src_faces"), (src_attr, "src_attr"))
    T, dev = src_face.shape[0], src_face.device
    bary, out = L.scratch((T, 3), torch.float32, dev), L.scratch((T, C), torch.float32, dev)
    L.launch("bake_transfer", dev, L.ptr(src_face.contiguous()), L.ptr(src_point.contiguous()), T, L.ptr(src_verts.contiguous()),
             src_verts.shape[0], L.ptr(src_faces.contiguous()), src_faces.shape[0], L.ptr(src_attr.contiguous()), C,
             int(bool(normalise)), L.ptr(bary), L.ptr(out))
    return (out, bary) if return_bary else out


@torch.no_grad()
def texels(face, bary, faces, verts, normals=None):
    """The covered texels: (index [T] int64, linear y W + x in row-major order; position [T,3]; normal [T,3] unit, or None
    without `normals` [V,3]).  Evaluate any function there and hand its values to scatter()."""
    position = interpolate(face, bary, faces, verts)
    index = torch.nonzero(face.reshape(-1) >= 0).reshape(-1)
    normal = None if normals is None else interpolate(face, bary, faces, normals, normalise=True).reshape(-1, 3)[index].contiguous()
    return index, position.reshape(-1, 3)[index].contiguous(), normal


@torch.no_grad()
def scatter(values, face, size=None):
    """values [T,C] (or [T]) of the covered texels in texels()' order -> an image [H,W,C] (or [H,W]), zeros elsewhere."""
    _check_images(face)
    if size is not None and _size(size) != tuple(face.shape):
        raise ValueError("size %r is not the face image's %r" % (size, tuple(face.shape)))
    if not isinstance(values, torch.Tensor) or values.dim() not in (1, 2):
        raise ValueError("values must have shape [T] or [T,C]")
    _cuda((values, "values"), (face, "face"))
    index = torch.nonzero(face.reshape(-1) >= 0).reshape(-1)
    if values.shape[0] != index.shape[0]:
        raise ValueError("values has %d rows, the image %d covered texels" % (values.shape[0], index.shape[0]))
    out = torch.zeros((face.numel(),) + tuple(values.shape[1:]), dtype=values.dtype, device=values.device)
    out[index] = values
    return out.reshape(tuple(face.shape) + tuple(values.shape[1:]))


def quantise(image):
    """round(255 clamp(x)) of a float image as a uint8 numpy array, the PNGs' values (float64 on the host; NaN -> 0)."""
    x = np.nan_to_num(image.detach().cpu().numpy().astype(np.float32), nan=0.)
    return np.rint(255. * np.clip(x, 0., 1.).astype(np.float64)).astype(np.uint8)


def uv_areas(uv, faces):
    """A of the coverage rule per face [F] float64 (torch, the same operations): < 0 flipped, 0 or not finite: covers nothing."""
    lo, hi = torch.minimum(faces[:, 0], faces[:, 1]), torch.maximum(faces[:, 0], faces[:, 1])
    a = (uv[hi, 0] - uv[lo, 0]) * (uv[faces[:, 2], 1] - uv[lo, 1]) - (uv[hi, 1] - uv[lo, 1]) * (uv[faces[:, 2], 0] - uv[lo, 0])
    return torch.where(faces[:, 0] > faces[:, 1], -a, a)


def _report(face, bary, count, verts, faces, uv, how):
    H, W = face.shape
    covered = face >= 0
    n = int(covered.sum().item())
    A = uv_areas(uv, faces) if faces.shape[0] else torch.zeros(0, dtype=torch.float64, device=face.device)
    per_face = torch.bincount(face[covered].long(), minlength=faces.shape[0]).double()
    p = verts.double()[faces] if faces.shape[0] else torch.zeros(0, 3, 3, dtype=torch.float64, device=face.device)
    area = 0.5 * torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=1)
    usable = torch.isfinite(area) & (area > 0)
    density = (per_face[usable] / area[usable])
    interior = covered & (bary.amin(-1) > 0)
    return {'size': [H, W], 'covered_texels': n, 'image_share': n / float(H * W) if H * W else 0.,
            'shared_texels': int((count > 1).sum().item()),
            # a texel strictly inside its owner that a second face covers too: not a shared edge or vertex but an overlap in the atlas
            'overlap_texels': int((interior & (count > 1)).sum().item()),
            'flipped_faces': int((torch.isfinite(A) & (A < 0)).sum().item()),
            'zero_area_faces': int((~torch.isfinite(A) | (A == 0)).sum().item()),
            'texels_per_area': ({'min': float(density.min().item()), 'median': float(density.median().item()),
                                 'max': float(density.max().item())} if density.numel() else None),
            'fallback_texels': None if how is None else int((how == HOW['fallback']).sum().item())}


@torch.no_grad()
def bake(verts, faces, uv, size, maps=MAPS, source=None, projection='closest', gutter=4, colors=None, lanes=None, fit=True,
         max_distance=None):
    """The maps of the mesh verts [V,3] float32 / faces [F,3] int64 with the chart uv [V,2] float64 (CUDA) on a `size` = H or
    (H, W) image.  `fit`: the chart is first fitted into the image (fit_uv, `gutter` texels from every side; flatten's uv have the
    pattern's scale), else uv are unit coordinates.  source = (verts, faces) or (verts, faces, colors): the normal and color
    maps come from that mesh, at the texels' projections (`projection`, project()).  colors [V,3]: the mesh's own vertex colours.
    A dict of float32 images [H,W,C], padded by `gutter` rings: 'position', 'normal' (object space, unit), 'tangent_normal' (the
    normal in the mesh's own tangent frames, 0.5 + 0.5 c), 'color' (if there are colours) — those of `maps` — and 'face', 'bary',
    'count', 'src', 'uv' (the fitted chart), 'lanes', 'report'."""
    H, W = _size(size)
    unknown = [m for m in maps if m not in MAPS]
    if unknown:
        raise ValueError("maps must be of %r (got %r)" % (MAPS, unknown))
    if projection not in PROJECTIONS:
        raise ValueError("projection must be one of %r (got %r)" % (PROJECTIONS, projection))
    if int(gutter) < 0:
        raise ValueError("gutter must not be negative (got %r)" % (gutter,))
    _check_f32(verts, 3, "verts")
    _check_faces(faces)
    _check_uv(uv, verts.shape[0])
    if colors is not None:
        _check_f32(colors, 3, "colors", verts.shape[0])
    if source is not None:
        if len(source) not in (2, 3):
            raise ValueError("source must be (verts, faces) or (verts, faces, colors)")
        _check_f32(source[0], 3, "source verts")
        _check_faces(source[1])
        if len(source) == 3 and source[2] is not None:
            _check_f32(source[2], 3, "source colors", source[0].shape[0])
    _cuda((verts, "verts"), (faces, "faces"), (uv, "uv"))
    from . import shading
    verts, faces = verts.contiguous(), faces.contiguous()
    uvf = fit_uv(uv, (H, W), float(gutter)) if fit else uv.contiguous()
    lanes = default_lanes(uvf, faces, (H, W)) if lanes is None else int(lanes)
    face, bary, count = rasterize_uv(uvf, faces, (H, W), lanes)
    src = _gutter(face, int(gutter))
    res = {'face': face, 'bary': bary, 'count': count, 'src': src, 'uv': uvf, 'lanes': lanes}
    vn = shading.verts_normals(verts, faces)
    frame_n = interpolate(face, bary, faces, vn, normalise=True)
    how, normal, color = None, frame_n, None
    if colors is not None:
        color = interpolate(face, bary, faces, colors.contiguous())
    if source is not None:
        sv, sf = source[0].contiguous(), source[1].contiguous()
        sc = source[2] if len(source) == 3 else None
        _cuda((sv, "source verts"), (sf, "source faces"))
        index, pos, nrm = texels(face, bary, faces, verts, vn)
        hit_face, hit_point, how = project(pos, nrm, sv, sf, projection, max_distance)
        if 'normal' in maps or 'tangent_normal' in maps:
            normal = scatter(transfer(hit_face, hit_point, sv, sf, shading.verts_normals(sv, sf), normalise=True), face)
        if sc is not None:
            color = scatter(transfer(hit_face, hit_point, sv, sf, sc.contiguous()), face)
    if 'position' in maps:
        res['position'] = pad(interpolate(face, bary, faces, verts), src)
    if 'normal' in maps:
        res['normal'] = pad(normal, src)
    if 'tangent_normal' in maps:
        frame_t = interpolate(face, bary, faces, vertex_tangents(verts, faces, uvf, vn), normalise=True)
        res['tangent_normal'] = pad(encode_normal(face, normal, frame_n, frame_t), src)
    if 'color' in maps and color is not None:
        res['color'] = pad(color, src)
    res['report'] = _report(face, bary, count, verts, faces, uvf, how)
    return res
