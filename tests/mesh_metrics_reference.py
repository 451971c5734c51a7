"""Float64 numpy restatement of the metric definitions of recmv.metrics.surface_distance, on samples that are given (the
sampling is not restated: the judge works on the very samples the kernel path drew).  The search is collide_reference.nearest
(brute force, the foot of the perpendicular or the nearest of the three edges).  Pinned on hand-computed cases by
tests/test_mesh_metrics_cpu.py and used as the judge of tests/test_gpu_mesh_metrics.py."""
import numpy as np

import collide_reference as CR


def face_normals(verts, faces):
    """Unit face normals [F,3], float64."""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)


def nearest(points, verts, faces, rows=512):
    """collide_reference.nearest's (face [N], squared distance [N]) without testing every pair: a face whose bounding
    sphere (centroid c, radius rho) is farther from the point than the nearest centroid cannot hold the minimum, since
    |p - c| - rho <= d(p, face) <= |p - c| — every other pair goes through collide_reference.closest_on_triangle.  Exact:
    the prefilter only drops pairs that cannot win or tie."""
    p, v, f = np.asarray(points, np.float64), np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cen = (a + b + c) / 3.
    rho = np.sqrt(np.maximum(np.maximum(((a - cen) ** 2).sum(1), ((b - cen) ** 2).sum(1)), ((c - cen) ** 2).sum(1)))
    face, best = np.zeros(p.shape[0], np.int64), np.zeros(p.shape[0])
    for s in range(0, p.shape[0], rows):
        q = p[s:s + rows]
        dc = np.sqrt(((q[:, None, :] - cen[None]) ** 2).sum(-1))                    # [rows, F]
        keep = (dc - rho[None]) * (1. - 1e-12) <= dc.min(1, keepdims=True)
        pi, fi = np.nonzero(keep)
        d, _ = CR.closest_on_triangle(q[pi], a[fi], b[fi], c[fi])
        dmin = np.full(q.shape[0], np.inf)
        np.minimum.at(dmin, pi, d)
        fmin = np.full(q.shape[0], f.shape[0], np.int64)
        tie = d == dmin[pi]
        np.minimum.at(fmin, pi[tie], fi[tie])
        face[s:s + rows], best[s:s + rows] = fmin, dmin
    return face, best


def direction(points, src_face, src_v, src_f, dst_v, dst_f, nearest_face=None):
    """One direction: the distance d [N] of every sample to the surface dst, the face found (the lowest index among equal
    minima), and |n_source_face . n_nearest_face| [N] — for `nearest_face` [N] instead of the found one when given."""
    face, d2 = nearest(points, dst_v, dst_f)
    use = face if nearest_face is None else np.asarray(nearest_face, np.int64)
    dots = np.abs((face_normals(src_v, src_f)[np.asarray(src_face, np.int64)] * face_normals(dst_v, dst_f)[use]).sum(-1))
    return np.sqrt(d2), face, dots


def combine(d_pred, dots_pred, d_gt, dots_gt, thresholds):
    """The dict of recmv.metrics.surface_distance from the two directions' distances and normal products."""
    out = {'accuracy': d_pred.mean(), 'accuracy_rms': np.sqrt((d_pred ** 2).mean()), 'accuracy_max': d_pred.max(),
           'completeness': d_gt.mean(), 'completeness_rms': np.sqrt((d_gt ** 2).mean()), 'completeness_max': d_gt.max(),
           'chamfer_l1': 0.5 * (d_pred.mean() + d_gt.mean()), 'chamfer_l2': (d_pred ** 2).mean() + (d_gt ** 2).mean(),
           'normal_consistency_pred_to_gt': dots_pred.mean(), 'normal_consistency_gt_to_pred': dots_gt.mean(),
           'normal_consistency': 0.5 * (dots_pred.mean() + dots_gt.mean())}
    for t in thresholds:
        pr, rc = (d_pred <= t).mean(), (d_gt <= t).mean()
        out['precision_%g' % t], out['recall_%g' % t] = pr, rc
        out['fscore_%g' % t] = 2. * pr * rc / (pr + rc) if pr + rc > 0 else 0.
    return {k: float(v) for k, v in out.items()}


def surface_distance(pred_pts, pred_src, pred_v, pred_f, gt_pts, gt_src, gt_v, gt_f, thresholds):
    """The metrics of the prediction's samples pred_pts [N,3] (drawn from its faces pred_src [N]) and the ground truth's."""
    d_p, _, n_p = direction(pred_pts, pred_src, pred_v, pred_f, gt_v, gt_f)
    d_g, _, n_g = direction(gt_pts, gt_src, gt_v, gt_f, pred_v, pred_f)
    return combine(d_p, n_p, d_g, n_g, thresholds)


def square(z=0., tilt=0., n=1):
    """The unit square [0,1]^2 at height z as 2 n^2 triangles, rotated by `tilt` radians about the x axis through its edge
    y = 0: (verts [.,3] float64, faces [.,3] int64)."""
    ax = np.linspace(0., 1., n + 1)
    x, y = np.meshgrid(ax, ax, indexing='xy')
    x, y = x.reshape(-1), y.reshape(-1)
    v = np.stack([x, y * np.cos(tilt), z + y * np.sin(tilt)], 1)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i + 1, i + n + 2, i + n + 1], 1)])
    return v, f.astype(np.int64)


def sample(verts, faces, count, seed):
    """Uniform samples of a mesh for the hand cases (numpy's generator; area-weighted faces, reflected uniforms):
    (points [count,3] float64, face [count])."""
    rng = np.random.RandomState(seed)
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    pick = np.minimum(np.searchsorted(np.cumsum(area), rng.rand(count) * area.sum()), f.shape[0] - 1)
    r = rng.rand(count, 2)
    r = np.abs(np.where(r.sum(1, keepdims=True) > 1., r - 1., r))
    return v[f[pick, 0]] + e1[pick] * r[:, :1] + e2[pick] * r[:, 1:], pick
