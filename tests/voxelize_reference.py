"""Float64 numpy restatement of recmv.voxelize (csrc/mesh_voxelize.hip): the lattice's nodes, the band distance, the inside
test of the nodes, the column rule and the volume.

  nodes          node (i, j, k) = origin + float32(idx) * step, formed in FLOAT32 with one multiply and one add — exactly the
                 kernels' coordinates — in the order (i * ny + j) * nz + k
  band_distance  collide_reference.nearest from those nodes in float64; a node is in the band when dist2 <= band^2
  inside         segment_mesh_reference.points_inside with the product's directions and segment lengths, and its `decided` flags
  column_fill    walking a (j, k) column along +x, a band node takes its own flag, a node outside the band the flag of the last
                 band node before it, outside if there is none; open_columns = the columns that end inside
  sign_conflicts lattice edges whose ends both lie outside the band and differ in their flag: none when the sign is right
  volume         count * step^3
"""
import numpy as np

import collide_reference as CR
import segment_mesh_reference as SR


def nodes(origin, step, dims):
    """[N,3] float32, N = nx ny nz, z fastest."""
    o, s = np.asarray(origin, np.float32), np.float32(step)
    ax = [(o[a] + np.arange(dims[a]).astype(np.float32) * s).astype(np.float32) for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing='ij'), -1)
    return np.ascontiguousarray(g.reshape(-1, 3))


def band_distance(points, v, f, band):
    """(dist2 [N] float64, face [N], in_band [N] bool) over the faces with valid indices and finite corners."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    ok = np.nonzero(((f >= 0) & (f < v.shape[0])).all(1))[0]
    ok = ok[np.isfinite(v[f[ok]]).all((1, 2))]
    face, d2, _, _ = CR.nearest(points, v, f[ok])
    return d2, ok[face], d2 <= float(band) ** 2


def reach(points, v):
    """recmv.metrics.points_inside's segment length in float64 (any length beyond the box does for the reference)."""
    v = np.asarray(v, np.float64)
    lo, hi = v.min(0), v.max(0)
    return 1.5 * np.linalg.norm(hi - lo) + np.linalg.norm(np.asarray(points, np.float64) - 0.5 * (lo + hi), axis=1)


def inside(points, v, f, directions):
    """(inside [N] bool, decided [N] bool): segment_mesh_reference.points_inside."""
    return SR.points_inside(points, v, f, directions, reach(points, v))


def column_fill(in_band, inside_band, dims):
    """(inside [nx, ny, nz] bool, open_columns) from the flags in_band and inside_band [N] (inside_band is read at band nodes only)."""
    nx, ny, nz = dims
    band = np.asarray(in_band, bool).reshape(nx, ny * nz)
    flag = np.asarray(inside_band, bool).reshape(nx, ny * nz)
    out = np.zeros((nx, ny * nz), bool)
    state = np.zeros(ny * nz, bool)
    for i in range(nx):
        state = np.where(band[i], flag[i], state)
        out[i] = state
    return out.reshape(nx, ny, nz), int(state.sum())


def sign_conflicts(inside_flags, in_band, dims):
    """The lattice edges, along any axis, whose two ends both lie outside the band and differ in their inside flag."""
    ins, band = np.asarray(inside_flags, bool).reshape(dims), np.asarray(in_band, bool).reshape(dims)
    total = 0
    for a in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        total += int(((ins[lo] != ins[hi]) & ~band[lo] & ~band[hi]).sum())
    return total


def volume(inside_flags, step):
    return int(np.asarray(inside_flags).sum()) * float(step) ** 3
