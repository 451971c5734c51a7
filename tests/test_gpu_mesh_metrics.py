"""recmv.metrics.surface_distance and eval_fl.py on the GPU, against the float64 restatement of tests/mesh_metrics_reference.py
evaluated on the very samples the device drew.

Bounds (eps32 = 2^-23, u = eps32 / 2 the unit round-off; the samples and meshes are exact float32 values, the judge works in
float64):
  distances     the kernel's squared distance is within BOUND_D2 = 16 eps32 (d + Lmax)^2 of the exact one
                (tests/test_gpu_animation.py), and |sqrt(a) - sqrt(b)| <= sqrt(|a - b|), so every distance is within
                sqrt(BOUND_D2) of the reference's: means and rms within the mean of that over the samples, the maximum
                within its maximum.
  normals       a face normal is cross(e1, e2) of rounded edges (relative u per component); a component is two products and
                a difference: |dn_c| <= 3 u (|e1y e2z| + |e1z e2y|) + u |n_c| <= 3 u |e1| |e2| + u |n_c|, in norm
                <= u |n| (3 sqrt(3) / s + 1) with s = |n| / (|e1| |e2|) the sine of the face's angle at its first corner.
                Normalising (squares, sum, root: 3 u; the division: u) gives a unit normal within u (5.2 / s + 5) of the
                exact one.  The product of two such normals is formed in float32 (u, its terms sum to at most 1) and summed
                in float64: |error| <= u (5.2 / s_src + 5.2 / s_dst + 11) <= eps32 (5.2 / s_min + 5.5) per sample, so for
                their mean too.  BOUND_NC = eps32 (11 / s_min + 11): the estimate with a factor of two in hand.
  thresholds    the kernel's count of d <= t differs from the reference's by at most the number of samples whose reference
                distance is within sqrt(BOUND_D2) of t.  THRESHOLDS are chosen so that this is at most 1 % of the samples
                (a condition on the inputs, decided by the reference alone and asserted).
"""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import collide_reference as CR  # noqa: E402
import mesh_metrics_reference as MR  # noqa: E402
from test_gpu_animation import _bound_d2, _irregular_body, _longest_edge  # noqa: E402

DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)
SAMPLES = 4000
# distances between the two bodies lie in 0.0456 .. 0.0572: none below the first, few around the second and third, all below the last
THRESHOLDS = (0.04, 0.046, 0.0565, 0.07)


def _min_sine(v, f):
    v, f = np.asarray(v, np.float64), np.asarray(f)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    return float((np.linalg.norm(np.cross(e1, e2), axis=1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))).min())


def _judge(got, samples, pred, gt, thresholds):
    """got: surface_distance's dict; samples: its return_samples; pred / gt: (verts, faces) float32 / int64 on the host."""
    sides = {}
    for name, (sv, sf), (dv, df) in (("pred", pred, gt), ("gt", gt, pred)):
        pts, src, near = (t.cpu().numpy() for t in samples[name])
        d, ref_face, _ = MR.direction(pts, src, sv.numpy(), sf.numpy(), dv.numpy(), df.numpy())
        bound = _bound_d2(d ** 2, _longest_edge(dv, df))
        # the faces the kernel chose are valid argmins: their float64 distance is within the bound of the minimum
        vv, tri = dv.double().numpy(), df.numpy()[near]
        d_named, _ = CR.closest_on_triangle(pts.astype(np.float64), vv[tri[:, 0]], vv[tri[:, 1]], vv[tri[:, 2]])
        assert (d_named <= d ** 2 + bound).all()
        _, _, dots = MR.direction(pts, src, sv.numpy(), sf.numpy(), dv.numpy(), df.numpy(), nearest_face=near)
        sides[name] = (d, dots, np.sqrt(bound))
    ref = MR.combine(sides["pred"][0], sides["pred"][1], sides["gt"][0], sides["gt"][1], thresholds)
    tol_p, tol_g = sides["pred"][2], sides["gt"][2]
    tol = {"accuracy": tol_p.mean(), "accuracy_rms": tol_p.mean(), "accuracy_max": tol_p.max(),
           "completeness": tol_g.mean(), "completeness_rms": tol_g.mean(), "completeness_max": tol_g.max(),
           "chamfer_l1": 0.5 * (tol_p.mean() + tol_g.mean())}
    for key, t in tol.items():
        print("%s: %.9g, reference %.9g, |difference| %.3g, bound %.3g" % (key, got[key], ref[key], abs(got[key] - ref[key]), t))
        assert abs(got[key] - ref[key]) <= t, key
    # chamfer_l2 is a sum of two mean squared distances: each within the mean of BOUND_D2
    t2 = (tol_p ** 2).mean() + (tol_g ** 2).mean()
    assert abs(got["chamfer_l2"] - ref["chamfer_l2"]) <= t2
    bound_nc = EPS32 * (11. / min(_min_sine(*pred), _min_sine(*gt)) + 11.)
    for key in ("normal_consistency_pred_to_gt", "normal_consistency_gt_to_pred", "normal_consistency"):
        print("%s: %.9g, reference %.9g, bound %.3g" % (key, got[key], ref[key], bound_nc))
        assert abs(got[key] - ref[key]) <= bound_nc, key
    for t in thresholds:
        for key, side in (("precision_%g" % t, "pred"), ("recall_%g" % t, "gt")):
            d, _, tol_d = sides[side]
            near_t = float((np.abs(d - t) <= tol_d).mean())
            assert near_t <= 0.01, (key, near_t)                 # the condition on the inputs
            assert abs(got[key] - ref[key]) <= near_t + 1e-12, key
        pr, rc = got["precision_%g" % t], got["recall_%g" % t]
        assert got["fscore_%g" % t] == (2. * pr * rc / (pr + rc) if pr + rc > 0 else 0.)
    tol.update({"chamfer_l2": t2, "normal_consistency": bound_nc})
    return ref, tol


@pytest.fixture(scope="module")
def bodies():
    pv, pf = _irregular_body(level=3, radius=0.50)
    gv, gf = _irregular_body(level=4, radius=0.55)
    return (pv, pf), (gv, gf)


def test_surface_distance_against_the_float64_reference(bodies):
    from recmv import metrics
    pred, gt = bodies
    args = [t.to(DEV) for t in pred + gt]
    got, samples = metrics.surface_distance(*args, samples=SAMPLES, seed=3, thresholds=THRESHOLDS, method='grid',
                                            return_samples=True)
    assert all(isinstance(x, float) for x in got.values())
    for name, (v, f) in (("pred", pred), ("gt", gt)):
        pts, src, near = samples[name]
        assert pts.shape == (SAMPLES, 3) and src.shape == (SAMPLES,) and near.shape == (SAMPLES,)
        # a sample lies on the face it was drawn from
        d, _ = CR.closest_on_triangle(pts.cpu().double().numpy(), *(v.double().numpy()[f.numpy()[src.cpu().numpy()][:, k]] for k in range(3)))
        assert float(d.max()) <= (4 * EPS32) ** 2
    ref, _ = _judge(got, samples, pred, gt, THRESHOLDS)
    assert 0.045 < ref["accuracy"] < 0.057 and ref["precision_0.04"] == 0. and ref["recall_0.07"] == 1.
    assert got["fscore_0.04"] == 0. and got["fscore_0.07"] == 1.


def test_grid_and_brute_force_give_identical_metrics(bodies):
    from recmv import metrics
    pred, gt = bodies
    args = [t.to(DEV) for t in pred + gt]
    a = metrics.surface_distance(*args, samples=SAMPLES, seed=5, thresholds=THRESHOLDS, method='grid')
    b = metrics.surface_distance(*args, samples=SAMPLES, seed=5, thresholds=THRESHOLDS, method='brute')
    c = metrics.surface_distance(*args, samples=SAMPLES, seed=5, thresholds=THRESHOLDS, method='auto')
    assert a == b == c
    assert a != metrics.surface_distance(*args, samples=SAMPLES, seed=6, thresholds=THRESHOLDS, method='grid')


def _square(z=0., tilt=0., n=1):
    v, f = MR.square(z, tilt, n)
    return torch.from_numpy(v).float().contiguous(), torch.from_numpy(f)


@pytest.mark.parametrize("method", ["grid", "brute"])
def test_hand_cases_on_the_device(method):
    """The closed forms of tests/test_mesh_metrics_cpu.py: parallel unit squares h apart, and a square against itself turned
    by theta about an edge (h and the turned vertices are exact in float32 or rounded once: the closed forms are taken on
    the float32 meshes by the reference, and compared with the formulas within the same bounds plus 1e-6 for that rounding)."""
    from recmv import metrics
    h = 0.125
    a, b = _square(0., n=3), _square(h, n=2)
    got, samples = metrics.surface_distance(a[0].to(DEV), a[1].to(DEV), b[0].to(DEV), b[1].to(DEV), samples=2000, seed=1,
                                            thresholds=(0.5 * h, 2 * h), method=method, return_samples=True)
    ref, tol = _judge(got, samples, a, b, (0.5 * h, 2 * h))
    for key in ("accuracy", "completeness", "chamfer_l1", "accuracy_max"):
        assert abs(ref[key] - h) < 1e-6 and abs(got[key] - h) <= tol[key] + 1e-6
    assert abs(got["chamfer_l2"] - 2 * h * h) <= tol["chamfer_l2"] + 1e-6
    assert abs(got["normal_consistency"] - 1.) <= tol["normal_consistency"] + 1e-6
    assert got["fscore_%g" % (2 * h)] == 1. and got["fscore_%g" % (0.5 * h)] == 0.
    theta = 0.3
    b = _square(0., tilt=theta, n=2)
    got, samples = metrics.surface_distance(a[0].to(DEV), a[1].to(DEV), b[0].to(DEV), b[1].to(DEV), samples=2000, seed=2,
                                            thresholds=(0.5,), method=method, return_samples=True)
    _, tol = _judge(got, samples, a, b, (0.5,))
    assert abs(got["normal_consistency"] - math.cos(theta)) <= tol["normal_consistency"] + 1e-6
    assert abs(got["completeness"] - float(samples["gt"][0][:, 2].double().mean())) <= tol["completeness"] + 1e-6
    assert abs(got["accuracy"] - float((samples["pred"][0][:, 1].double() * math.sin(theta)).mean())) <= tol["accuracy"] + 1e-6


def test_eval_fl_end_to_end(tmp_path):
    """Three pairs of one topology in two directories (plus a file without a partner): the JSON is written, the means are
    the per-pair means, the smoothness of the sequence is there, and a rerun with the same seed writes the same file."""
    import eval_fl
    from recmv.utils import write_obj
    pv, pf = _irregular_body(level=2, radius=0.50)
    gv, gf = _irregular_body(level=2, radius=0.52)
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    pred.mkdir()
    gt.mkdir()
    for k in range(3):
        write_obj(str(pred / ("frame_%03d.obj" % k)), pv * (1 + 0.01 * k * k), pf)
        write_obj(str(gt / ("frame_%03d.obj" % k)), gv, gf)
    write_obj(str(gt / "frame_009.obj"), gv, gf)
    argv = ["--gpu-ids", "0", "--pred", str(pred), "--gt", str(gt), "--samples", "2000", "--seed", "4", "--thresholds",
            "0.01", "0.05", "--method", "grid"]
    res = eval_fl.main(argv + ["--out", str(tmp_path / "m1.json")])
    eval_fl.main(argv + ["--out", str(tmp_path / "m2.json")])
    text = (tmp_path / "m1.json").read_text()
    assert text == (tmp_path / "m2.json").read_text()
    out = json.loads(text)
    assert sorted(out["pairs"]) == ["frame_000", "frame_001", "frame_002"]
    assert [Path(p).name for p in out["unmatched_gt"]] == ["frame_009.obj"] and out["unmatched_pred"] == []
    assert out["samples"] == 2000 and out["seed"] == 4 and out["method"] == "grid"
    for key, m in out["mean"].items():
        assert abs(m - sum(out["pairs"][s][key] for s in out["pairs"]) / 3) <= 1e-15 * max(1., abs(m))
    assert out["mean"] == res["mean"]
    # the prediction grows by 0, 1 and 4 %: the second difference of a vertex is 2 % of its position
    assert out["temporal_smoothness"] > 0
    assert abs(out["temporal_smoothness"] - 0.02 * float(pv.double().norm(dim=1).mean())) < 1e-5   # (%f: six decimals)
    assert out["pairs"]["frame_000"]["accuracy"] > 0.015 and out["pairs"]["frame_002"]["accuracy"] < 0.01
    brute = eval_fl.main(argv[:-1] + ["brute"])
    assert brute["pairs"] == res["pairs"]
