"""Mesh voxelisation (csrc/mesh_voxelize.hip) — an ADDITION to the reference, which never turns a mesh into a volume.

  Lattice           a regular lattice of cubic cells: origin, step, dims; node (i, j, k) sits at origin + (i, j, k) * step (formed
                    in f32, one multiply and one add), layout [NX, NY, NZ] with z contiguous — MCGpu.mc_gpu's volume layout
  lattice_for       a lattice around a mesh's bounding box, by step or by the number of nodes along the longest axis
  distance_field    per node the exact squared distance to and the id of the nearest face within a narrow band
                    (recmv_voxel_band_distance: one wave per face over the face's dilated box, the bits of
                    iso_remesh.closest_point), the inside flag and the signed, clamped distance (recmv_voxel_sign_fill)
  signed_distance   +-sqrt(dist2) of arbitrary points: the existing closest-point query and metrics.points_inside composed
  extract           MCGpu.mc_gpu on a field of a lattice
  remesh            lattice_for -> distance_field -> extract: a watertight manifold mesh of uniform resolution from a closed one
  solidify          a closed shell of a given thickness around an open surface: the iso-surface of the UNSIGNED distance at
                    thickness / 2 (no sign needed)
  occupancy, volume, volume_iou    the inside flags of a lattice's nodes, their count times step^3, and the volumetric
                    intersection over union of two closed meshes on one lattice around both

The in-band rule: a node is a band node when dist2 <= band * band, the product formed once in f32; elsewhere dist2 = +inf,
face = -1 and the field is clamped to +-band.
The sign is a CROSSING PARITY.  The band nodes, in ascending node order, go through metrics.points_inside unchanged — the
definition, directions and majority vote of metrics.penetration — and the column rule carries their flags to the other nodes:
walking a (j, k) column along +x, a node outside the band takes the flag of the last band node before it, outside if there is
none.  That is sound whenever band >= step (a lattice edge the surface crosses has both ends within one step of it);
distance_field asks for band >= 2 steps.  Consequences: the mesh must be CLOSED; overlapping closed pieces XOR instead of
uniting (a point inside two pieces crosses an even number of faces); a mesh with holes gives whatever the parities give.  Two
diagnostics, no errors, show a lost parity: `open_columns`, the number of columns that end inside, and `sign_conflicts`, the number
of lattice edges whose ends both lie outside the band and differ in their flag (with a correct sign an edge the surface crosses
has an end within one step of it, so there is none).  A hole that faces along x can leave every column closed — the open
cylinder of the tests does at some steps — but on the way out through the hole the flag must flip between nodes far from the
surface, which the second count sees.  remesh's callers should refuse a result where either is not 0.

sign='winding' (distance_field, remesh, occupancy, volume, volume_iou; the default stays 'parity') takes the sign from the
generalized winding number of recmv.winding instead: EVERY node's flag is |w| > 1/2 and the column rule is not used (it is unsound
through a hole).  w comes from the pyramid (winding_method='tree', recmv.winding.DEFAULT_BETA) by default and from every face with
winding_method='exact'; the nodes are queried in slices.  sdf = where(inside, -1, 1) * minimum(sqrt(dist2), band) as before.
`open_columns` and `sign_conflicts` are still reported, but under this sign they are information, not faults: where the mesh has
a hole the surface w = 1/2 passes between nodes that are clamped to +-band, marching cubes caps the hole there — a COARSE cap, a
staircase of the lattice's step and no smooth patch — and the cap shows up in both counts.  The result carries 'sign'.

What the first two items below used to say is therefore available through sign='winding':
  * a winding-number sign for meshes with holes;
  * a per-piece union of overlapping closed pieces (w = 2 inside two pieces is inside).
Out of scope here (none of it is attempted):
  * cavity filling, or an "outer surface" of a body plus its garments;
  * a GridSamplerMine collision loss on a body TSDF (distance_field's `sdf` is the lattice it would sample);
  * any change to MCGpu, metrics or the existing kernels.
"""
import ctypes as C
import math

import torch

from . import _lib as L
from . import metrics
from . import winding
from .mesh_args import check_mesh

MAX_NODES = 1 << 28            # recmv_mc_*'s limit
DEFAULT_BAND_STEPS = 3.        # a choice, not a measurement: marching cubes needs one step, the rest keeps its interpolation
                               # well inside exact values
DEFAULT_PAD_STEPS = 4          # the default band and one step: the lattice border is never cut
MIN_BAND_STEPS = 2.
DEFAULT_IOU_RESOLUTION = 129   # volume_iou without step and resolution
SIGNS = ('parity', 'winding')
DEFAULT_WINDING_METHOD = 'tree'  # measured against 'exact' at lattice sizes (tools/winding_timing.py)
WINDING_SLICE = 1 << 22        # lattice nodes per winding query


def _check_sign(sign, winding_method):
    if sign not in SIGNS:
        raise ValueError("sign must be 'parity' or 'winding' (got %r)" % (sign,))
    if winding_method is not None and winding_method not in winding.METHODS:
        raise ValueError("winding_method must be 'tree' or 'exact' (got %r)" % (winding_method,))
    if winding_method is not None and sign != 'winding':
        raise ValueError("winding_method belongs to sign='winding'")


def _winding_inside(verts, faces, lattice, winding_method):
    """|w| > 1/2 at every node of the lattice, [N] uint8, in slices of WINDING_SLICE nodes in node order."""
    N, dev = lattice.n_nodes, verts.device
    method = DEFAULT_WINDING_METHOD if winding_method is None else winding_method
    tree = winding.WindingTree(verts, faces) if method == 'tree' else None
    out = L.scratch((N,), torch.uint8, dev)
    for a in range(0, N, WINDING_SLICE):
        pts = lattice.points(torch.arange(a, min(a + WINDING_SLICE, N), device=dev))
        w = tree.query(pts) if tree is not None else winding.winding_number(pts, verts, faces)
        out[a:a + WINDING_SLICE] = winding.inside_from_winding(w)
    return out


def _f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


class Lattice:
    """origin (three floats), step and dims (nx, ny, nz); origin and step are rounded to float32, what the kernels get."""

    def __init__(self, origin, step, dims):
        self.origin = tuple(_f32(o) for o in origin)
        self.step = _f32(step)
        self.dims = tuple(int(d) for d in dims)
        if len(self.origin) != 3 or len(self.dims) != 3:
            raise ValueError("Lattice: origin and dims have three entries each")
        if not all(math.isfinite(o) for o in self.origin):
            raise ValueError("Lattice: the origin is not finite")
        if not (self.step > 0. and math.isfinite(self.step)):
            raise ValueError("Lattice: step must be positive and finite (got %r)" % (step,))
        if min(self.dims) < 0:
            raise ValueError("Lattice: dims must not be negative (got %r)" % (self.dims,))
        if self.n_nodes > MAX_NODES:
            raise ValueError("Lattice: %d x %d x %d nodes, at most 2^28" % self.dims)

    @property
    def n_nodes(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    def desc(self):
        d = L.Lattice()
        d.origin[:] = self.origin
        d.step = self.step
        d.nx, d.ny, d.nz = self.dims
        return d

    def axis(self, a, device):
        """The coordinates of the nodes along axis a, [dims[a]] f32: origin + idx.float() * step, the kernels' bits."""
        return self.origin[a] + torch.arange(self.dims[a], device=device).float() * self.step

    def points(self, index):
        """The coordinates [K,3] f32 of the nodes with the flat indices `index` [K] int64."""
        nx, ny, nz = self.dims
        ijk = (index // (ny * nz), (index // nz) % ny, index % nz)
        return torch.stack([self.origin[a] + ijk[a].float() * self.step for a in range(3)], 1)

    def nodes(self, device):
        """All node coordinates, [NX, NY, NZ, 3] f32."""
        x, y, z = (self.axis(a, device) for a in range(3))
        return torch.stack(torch.meshgrid(x, y, z, indexing='ij'), -1)

    def json(self):
        return {'origin': list(self.origin), 'step': self.step, 'dims': list(self.dims)}

    def __repr__(self):
        return "Lattice(origin=%r, step=%r, dims=%r)" % (self.origin, self.step, self.dims)


def _box(verts):
    """(lo, hi) of the vertices as python floats: the one read-back."""
    box = torch.stack([verts.amin(0), verts.amax(0)]).cpu()
    if not bool(torch.isfinite(box).all()):
        raise ValueError("the bounding box is not finite")
    return box[0].tolist(), box[1].tolist()


def lattice_from_box(lo, hi, step=None, resolution=None, pad_steps=DEFAULT_PAD_STEPS):
    """lattice_for on a given box.  `pad_steps`: an integer, or a function of the step that gives one."""
    if (step is None) == (resolution is None):
        raise ValueError("give step or resolution, not both and not neither")
    if not all(math.isfinite(x) for x in list(lo) + list(hi)):
        raise ValueError("the bounding box is not finite")
    ext = [max(b - a, 0.) for a, b in zip(lo, hi)]
    pad_of = pad_steps if callable(pad_steps) else (lambda s: pad_steps)
    if step is not None:
        step = _f32(step)
        if not (step > 0. and math.isfinite(step)):
            raise ValueError("step must be positive and finite (got %r)" % (step,))
        pad = int(pad_of(step))
    else:
        resolution = int(resolution)
        longest = max(ext)
        if not longest > 0.:
            raise ValueError("resolution needs a box with an extent")
        pad = 0
        for _ in range(64):                                # a larger pad gives a larger step, which never asks for a larger pad still
            cells = resolution - 1 - 2 * pad
            if cells < 1:
                raise ValueError("resolution %d leaves no cell for the box beside %d nodes of padding per side" % (resolution, pad))
            step = _f32(longest / cells)
            want = int(pad_of(step))
            if want <= pad:
                break
            pad = want
    if pad < 0:
        raise ValueError("pad_steps must not be negative")
    origin = [_f32(a - pad * step) for a in lo]
    dims = [int(math.ceil((b + pad * step - o) / step - 1e-6)) + 1 for b, o in zip(hi, origin)]
    if resolution is not None:                             # exactly `resolution` nodes along the longest axis, whatever the rounding
        k = ext.index(max(ext))
        dims[k] = resolution
    if dims[0] * dims[1] * dims[2] > MAX_NODES:
        raise ValueError("%d x %d x %d nodes, at most 2^28: choose a larger step" % tuple(dims))
    return Lattice(origin, step, dims)


def lattice_for(verts, step=None, resolution=None, pad_steps=DEFAULT_PAD_STEPS):
    """A lattice of cubic cells around the bounding box of verts [V,3] (CUDA): the box and `pad_steps` nodes beyond it on every
    side.  Give `step`, or `resolution`, the number of nodes along the longest axis (padding included).  One read-back, for the
    box.  ValueError for a box that is not finite and for more than 2^28 nodes."""
    L.require_cuda(verts, "verts")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] == 0:
        raise ValueError("verts must be of shape [V,3], V > 0")
    lo, hi = _box(verts)
    return lattice_from_box(lo, hi, step, resolution, pad_steps)


def _band_of(lattice, band):
    band = DEFAULT_BAND_STEPS * lattice.step if band is None else float(band)
    band = _f32(band)
    if not math.isfinite(band) or band < MIN_BAND_STEPS * lattice.step:
        raise ValueError("band %g is below 2 steps of %g: the column rule and marching cubes need the nodes beside the surface"
                         % (band, lattice.step))
    return band


@torch.no_grad()
def distance_field(verts, faces, lattice, band=None, signed=True, method='auto', sign='parity', winding_method=None):
    """The narrow-band distance field of the mesh verts [V,3] f32 / faces [F,3] int64 (CUDA) on `lattice`: a dict with `dist2`
    f32 and `face` int64 (+inf and -1 outside the band), `sdf` f32 = (inside ? -1 : +1) * min(sqrt(dist2), band), `inside` bool
    (each [NX, NY, NZ]), `band` (the float32 the kernels got), `band_nodes`, `open_columns` and `sign_conflicts` (python ints; the
    last two are 0 for a closed mesh well inside the lattice, see the module docstring).  `band`: a length, 3 steps by default,
    at least 2 steps.  `signed=False` skips the segment queries: every node is outside and sdf >= 0.
    `method`: metrics.points_inside's.  `sign`, `winding_method`: the module docstring; the result carries `sign`."""
    _check_sign(sign, winding_method)
    band = _band_of(lattice, band)
    metrics.use_grid_for_segments(method, 0, 0)
    verts, faces = check_mesh(verts, faces, allow_empty=False)
    dev, N, dims = verts.device, lattice.n_nodes, lattice.dims
    dist2 = L.scratch((N,), torch.float32, dev)
    face = L.scratch((N,), torch.int64, dev)
    sdf = L.scratch((N,), torch.float32, dev)
    inside = L.scratch((N,), torch.uint8, dev)
    open_columns = torch.zeros(1, dtype=torch.int64, device=dev)
    desc = lattice.desc()
    band_nodes = 0
    if N:
        ws = L.workspace(nbytes := int(L.lib().recmv_voxel_band_workspace_bytes(C.byref(desc))), dev, "voxel_band_workspace_bytes")
        L.launch("voxel_band_distance", dev, L.ptr(verts), verts.shape[0], L.ptr(faces), faces.shape[0], C.byref(desc), band,
                 L.ptr(dist2), L.ptr(face), L.ptr(ws), nbytes)
        del ws
        b = torch.tensor(band, dtype=torch.float32, device=dev)
        in_band = dist2 <= b * b
        inside_band = None
        if signed and sign == 'winding':
            inside = _winding_inside(verts, faces, lattice, winding_method)
            flag = inside.view(torch.bool)
            sdf = torch.where(flag, -1., 1.).to(torch.float32) * torch.minimum(dist2.sqrt(), b)
            counts = torch.stack([flag.view(dims)[-1].sum(), _sign_conflicts(flag.view(dims), in_band.view(dims)), in_band.sum()])
            n_open, n_conflicts, band_nodes = (int(x) for x in counts.cpu().tolist())
            return {'dist2': dist2.view(dims), 'face': face.view(dims), 'sdf': sdf.view(dims), 'inside': flag.view(dims),
                    'band': band, 'band_nodes': band_nodes, 'open_columns': n_open, 'sign_conflicts': n_conflicts, 'sign': sign}
        if signed:
            index = torch.nonzero(in_band)[:, 0]                                   # ascending node order (a read-back)
            band_nodes = int(index.shape[0])
            inside_band = torch.zeros(N, dtype=torch.uint8, device=dev)
            if band_nodes:
                inside_band[index] = metrics.points_inside(lattice.points(index), verts, faces, method=method).to(torch.uint8)
        L.launch("voxel_sign_fill", dev, L.ptr(dist2), L.ptr(inside_band), C.byref(desc), band, int(bool(signed)), L.ptr(sdf),
                 L.ptr(inside), L.ptr(open_columns))
        counts = [open_columns[0], _sign_conflicts(inside.view(dims), in_band.view(dims))]
        if not signed:
            counts.append(in_band.sum())
        counts = [int(x) for x in torch.stack(counts).cpu().tolist()]
        n_open, n_conflicts = counts[0], counts[1]
        if not signed:
            band_nodes = counts[2]
    else:
        n_open = n_conflicts = 0
    return {'dist2': dist2.view(dims), 'face': face.view(dims), 'sdf': sdf.view(dims), 'inside': inside.view(torch.bool).view(dims),
            'band': band, 'band_nodes': band_nodes, 'open_columns': n_open, 'sign_conflicts': n_conflicts, 'sign': sign}


def _sign_conflicts(inside, in_band):
    """The number of lattice edges (along any axis) whose two ends are BOTH outside the band and carry different inside flags, a
    device scalar.  With a correct sign there is none: an edge the surface crosses has an end within one step <= band of it.
    (Along x the column rule cannot make one; along y and z neighbouring columns disagree where the parity was lost — an open
    mesh whose hole faces along x ends no column inside, but it must flip the flag somewhere on the way out through the hole.)"""
    total = torch.zeros((), dtype=torch.int64, device=inside.device)
    for a in range(3):
        n = inside.shape[a]
        if n < 2:
            continue
        lo, hi = inside.narrow(a, 0, n - 1), inside.narrow(a, 1, n - 1)
        total = total + ((lo != hi) & ~in_band.narrow(a, 0, n - 1) & ~in_band.narrow(a, 1, n - 1)).sum()
    return total


@torch.no_grad()
def signed_distance(points, verts, faces, method='auto'):
    """-sqrt(dist2) for the points [P,3] f32 inside the closed mesh and +sqrt(dist2) for the others, [P] f32: the closest-point
    query of recmv.metrics and metrics.points_inside, composed (no kernel of its own).  `method` as in recmv.metrics."""
    inside = metrics.points_inside(points, verts, faces, method=method)
    if points.shape[0] == 0:
        return points.new_zeros(0)
    _, _, dist2 = metrics._nearest(points.contiguous(), verts.contiguous(), faces.contiguous(), method)
    d = dist2.sqrt()
    return torch.where(inside, -d, d)


def extract(sdf, lattice, iso=0.):
    """The iso-surface of a field [NX, NY, NZ] f32 on `lattice`: MCGpu.mc_gpu with the lattice's steps and origin, (verts [V,3]
    f32, faces [F,3] int64).  Its orientation is the one mc_gpu gives a field that is negative inside."""
    from . import MCGpu
    if tuple(sdf.shape) != lattice.dims:
        raise ValueError("the field has the shape %r, the lattice %r" % (tuple(sdf.shape), lattice.dims))
    out = MCGpu.mc_gpu(sdf.contiguous(), lattice.step, lattice.step, lattice.step, *lattice.origin, float(iso))
    if not out:
        raise ValueError("extract: marching cubes refused a volume of %r" % (lattice.dims,))
    return out[0], out[1]


def _steps_beyond(length):
    """pad_steps for lattice_from_box: the nodes that cover `length(step)` and one more."""
    return lambda step: int(math.ceil(length(step) / step - 1e-6)) + 1


@torch.no_grad()
def remesh(verts, faces, step=None, resolution=None, band=None, method='auto', sign='parity', winding_method=None):
    """Voxel remeshing of a CLOSED mesh: exact distances on a lattice (`step`, or `resolution` nodes along the longest axis),
    the crossing-parity sign, marching cubes at 0 — a watertight manifold mesh of uniform resolution whatever the input's
    self-intersections (overlapping pieces XOR, see the module docstring).  The lattice is padded by at least band + 1 step, so
    its border is never cut.  Returns (verts, faces, info); info: `lattice`, `band`, `band_nodes`, `open_columns` and
    `sign_conflicts` (either > 0: the input has holes or the parity was lost — the output then is not to be trusted), `faces_in`,
    `faces_out`, `sign`.  sign='winding' takes a mesh with holes (each capped coarsely where w = 1/2) or of overlapping pieces
    (their union); the two diagnostics then are information only."""
    _check_sign(sign, winding_method)
    check_mesh(verts, faces, allow_empty=False)
    lo, hi = _box(verts)
    length = (lambda s: DEFAULT_BAND_STEPS * s) if band is None else (lambda s: float(band))
    lattice = lattice_from_box(lo, hi, step, resolution, _steps_beyond(length))
    field = distance_field(verts, faces, lattice, band=band, signed=True, method=method, sign=sign, winding_method=winding_method)
    v, f = extract(field['sdf'], lattice, 0.)
    return v, f, {'lattice': lattice, 'band': field['band'], 'band_nodes': field['band_nodes'],
                  'open_columns': field['open_columns'], 'sign_conflicts': field['sign_conflicts'],
                  'faces_in': int(faces.shape[0]), 'faces_out': int(f.shape[0]), 'sign': sign}


@torch.no_grad()
def solidify(verts, faces, thickness, step=None, resolution=None):
    """A closed shell of `thickness` around the (open) surface verts / faces: the iso-surface at thickness / 2 of the UNSIGNED
    distance, taken in a band of thickness / 2 + 2 steps on a lattice padded by at least that band + 1 step.  ValueError for
    thickness < 3 steps (the slab would hold no interior node).  Returns (verts, faces, info) like remesh (`open_columns` is 0:
    nothing is signed)."""
    thickness = float(thickness)
    if not (thickness > 0. and math.isfinite(thickness)):
        raise ValueError("thickness must be positive and finite (got %r)" % (thickness,))
    if step is not None and thickness < 3. * _f32(step):
        raise ValueError("thickness %g is below 3 steps of %g: the slab would hold no interior node" % (thickness, _f32(step)))
    check_mesh(verts, faces, allow_empty=False)
    lo, hi = _box(verts)
    length = lambda s: 0.5 * thickness + 2. * s  # noqa: E731
    lattice = lattice_from_box(lo, hi, step, resolution, _steps_beyond(length))
    if thickness < 3. * lattice.step:
        raise ValueError("thickness %g is below 3 steps of %g: the slab would hold no interior node" % (thickness, lattice.step))
    field = distance_field(verts, faces, lattice, band=length(lattice.step), signed=False)
    v, f = extract(field['sdf'], lattice, 0.5 * thickness)
    return v, f, {'lattice': lattice, 'band': field['band'], 'band_nodes': field['band_nodes'], 'open_columns': 0,
                  'sign_conflicts': 0, 'thickness': thickness, 'faces_in': int(faces.shape[0]), 'faces_out': int(f.shape[0])}


def _occupancy(verts, faces, lattice, method='auto', sign='parity', winding_method=None):
    return distance_field(verts, faces, lattice, band=MIN_BAND_STEPS * lattice.step, signed=True, method=method, sign=sign,
                          winding_method=winding_method)


def occupancy(verts, faces, lattice, method='auto', sign='parity', winding_method=None):
    """Which nodes of `lattice` lie inside the closed mesh: bool [NX, NY, NZ] (distance_field's `inside` at a band of 2 steps).
    sign='winding': |w| > 1/2, the union of overlapping pieces."""
    return _occupancy(verts, faces, lattice, method, sign, winding_method)['inside']


def volume(verts, faces, lattice, method='auto', sign='parity', winding_method=None):
    """The volume of the closed mesh as the number of nodes inside times step^3 (a python float; one read-back for the count)."""
    return int(occupancy(verts, faces, lattice, method, sign, winding_method).sum().item()) * lattice.step ** 3


@torch.no_grad()
def volume_iou(a_v, a_f, b_v, b_f, step=None, resolution=None, method='auto', sign='parity', winding_method=None):
    """Volumetric intersection over union of two closed meshes on ONE lattice around both (`step`, or `resolution` nodes along
    the longest axis; 129 nodes when neither is given): {'iou', 'intersection', 'union', 'volume_a', 'volume_b', 'step'} — the
    two counts exact integers (one read-back for all the counts), the volumes count * step^3, iou = 0 for an empty union — and
    `open_columns_a`, `open_columns_b`, `sign_conflicts_a`, `sign_conflicts_b`: not 0 when that mesh is not closed, and the
    figures then mean nothing — under sign='parity'; under sign='winding' (`sign` in the result) they are information only."""
    _check_sign(sign, winding_method)
    check_mesh(a_v, a_f, allow_empty=False)
    check_mesh(b_v, b_f, allow_empty=False)
    if a_v.device != b_v.device:
        raise ValueError("the two meshes must be on one device")
    if step is None and resolution is None:
        resolution = DEFAULT_IOU_RESOLUTION
    lattice = lattice_for(torch.cat([a_v, b_v]), step, resolution, pad_steps=int(MIN_BAND_STEPS) + 1)
    fa, fb = (_occupancy(v, f, lattice, method, sign, winding_method) for v, f in ((a_v, a_f), (b_v, b_f)))
    a, b = fa['inside'], fb['inside']
    n = torch.stack([(a & b).sum(), (a | b).sum(), a.sum(), b.sum()]).cpu().tolist()
    cell = lattice.step ** 3
    return {'iou': n[0] / n[1] if n[1] else 0., 'intersection': int(n[0]), 'union': int(n[1]), 'volume_a': n[2] * cell,
            'volume_b': n[3] * cell, 'step': lattice.step, 'lattice': lattice, 'open_columns_a': fa['open_columns'],
            'open_columns_b': fb['open_columns'], 'sign_conflicts_a': fa['sign_conflicts'], 'sign_conflicts_b': fb['sign_conflicts'],
            'sign': sign}
