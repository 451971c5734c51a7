"""eval_fl.py — surface metrics between reconstructed garments and ground-truth (or reference-run) meshes: an addition, the
reference has no evaluation command (its tools/comparison_results.py stops after loading a mesh).

`--pred` and `--gt` are two `.obj` files or two directories of them; directories are paired by file stem, files without a
partner are listed in the output and skipped, and no pair at all is an error.  The two meshes of a pair are taken to be in one
frame unless `--align` is given (`--scale` multiplies the prediction, for captures in another unit).  `--align rigid` or
`--align similarity` first fits the prediction to the ground truth by ICP (recmv.align.icp, after `--scale` and before
everything else): a reconstruction from one monocular video is known only up to a similarity, so without it the distances
measure the frame offset, not the shape.  `--align-metric plane|point` chooses the residual, `--align-trim f` keeps the
share f of the pairs with the smallest distances, `--align-iters n` caps the steps, `--align-from first` estimates the
transform on the first pair by stem and applies it to every pair (the honest setting for a sequence with one global scale;
`each`, the default, fits every pair on its own), and `--align-out DIR` writes the aligned predictions as `.obj`.  The
output then holds `align` (the settings) and `alignment` (per stem: scale, R, t, iterations, converged, rms_before, rms_after,
pairs); with `--align none` it is what it was without these flags.  Per pair
recmv.metrics.surface_distance (accuracy, completeness, Chamfer, normal consistency, precision / recall / F-score at
`--thresholds`, definitions in INTEGRATION.md §5), then the means over the pairs.  When the prediction directory is a sequence
of one topology the output also holds infer_fl_animation.py's temporal smoothness figure of it.  `--intersections` adds per
pair the faces of the prediction that take part in a crossing of the prediction with itself and their share of its faces
(`self_intersecting_faces`, `self_intersection_ratio`), the same for the ground truth (`…_gt`), and with `--body` (a mesh or
a directory paired by stem, like `--gt`) the prediction's faces that cross that body (`body_intersecting_faces`,
`body_intersection_ratio`), and with `--penetration` besides the prediction's vertices inside that body and the largest
distance of one of them to its surface (`body_inside_vertices`, `body_max_depth`); definitions in INTEGRATION.md §5.
`--inside-rule winding` judges the vertices by the generalized winding number about the body instead of the crossing parity
(recmv.winding, |w| > 1/2: the body may have holes or consist of overlapping pieces; `body_inside: {rule}` records it).
`--drop-floaters FRAC` removes from the prediction, before alignment and metrics, every piece whose area is below FRAC times
its largest piece's (recmv.topology.keep_components; one floater decides `accuracy_max` and drags the precision down) and
records what went under `floaters` in the pair's entry; `--topology` adds `topology_pred` and `topology_gt`
(recmv.topology.report: pieces, boundary loops, Euler characteristic, watertightness, triangle quality) to it.  `mean` is
taken over the numeric entries.  `--repair` mends the prediction AND the ground truth before anything else (after `--scale`;
recmv.repair.repair: degenerate and duplicate faces dropped, non-manifold edges and pinch vertices taken apart, orientable pieces
oriented, unused vertices dropped), and `--weld-eps E` (a length, implies `--repair`) first welds the vertices within E of each
other: a scan exported with one vertex triple per face reads as F pieces until it is welded, and `--topology` and
`--drop-floaters` mean nothing for it.  The numbers of the two calls' info go into the pair's entry as `repair_pred` and
`repair_gt`.  `--volume` adds to every pair the volumetric intersection over union of the two meshes and their volumes
(`volume_iou`, `volume_pred`, `volume_gt`; recmv.voxelize.volume_iou on one lattice around both, of step `--volume-step` or with
129 nodes along the longest axis; the counts and the lattice under `volume`).  The sign is a crossing parity, so both meshes must
be closed (`--voxel-sign winding` takes the sign of the generalized winding number instead, which measures meshes with holes,
unites overlapping pieces and never withholds a figure): when a diagnostic of either says it is not (`open_columns`, `sign_conflicts`) the three figures are None, `volume`
holds the `reason`, and they have no `mean`.

    python rec-mv_amd/eval_fl.py --gpu-ids 0 --pred <obj|dir> --gt <obj|dir> [--samples N] [--seed S] [--thresholds t ...]
        [--scale s] [--method auto|grid|brute] [--intersections [--body <obj|dir> [--penetration]]] [--out metrics.json]
        [--align none|rigid|similarity [--align-metric plane|point] [--align-trim f] [--align-iters n]
         [--align-from each|first] [--align-out DIR]] [--drop-floaters FRAC] [--topology] [--repair] [--weld-eps E]
        [--volume [--volume-step S] [--voxel-sign parity|winding]] [--inside-rule parity|winding] [--fill-holes [--fill-max-edges N] [--fill-keep-largest K]]
        [--boundary-bands W1,W2,...]

`--fill-holes` closes the holes of the prediction AND the ground truth after `--repair` and before every metric
(recmv.holes.fill: least-area patches; `--fill-max-edges N` leaves loops of more than N edges open, `--fill-keep-largest K` the
K longest), so that `--volume` has something to measure on scans with missing patches; the two calls' info goes into the pair's
entry as `holes_pred` and `holes_gt`.

`--boundary-bands W1,W2,...` (ascending, positive, finite widths) reports the error where the method claims to be right: at the
feature curves.  Every pair gets a `boundary_bands` entry: the prediction's samples (those of surface_distance: same seed, same
points) are binned by their geodesic distance ALONG the prediction to the prediction's own border (recmv.geodesic.
boundary_distance, interpolated at each sample on its source face) into [0, W1), [W1, W2), ..., [Wn, inf), and every bin
reports its `count` and the `mean`, `rms` and `max` of the samples' distance to the ground truth (None for an empty bin); the
same for the ground truth's samples, binned along the ground truth, against the prediction.  A side whose mesh has no border is
None with the reason "closed".  Every other key of the pair keeps its value bit for bit.
"""
import argparse
import json
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))


def build_parser():
    parser = argparse.ArgumentParser(description='surface metrics between predicted and ground-truth meshes')
    parser.add_argument('--gpu-ids', nargs='+', type=int, default=[0], metavar='IDs', help='gpu ids (the first is used)')
    parser.add_argument('--pred', required=True, help='predicted mesh (.obj) or a directory of them')
    parser.add_argument('--gt', required=True, help='ground-truth mesh (.obj) or a directory of them')
    parser.add_argument('--samples', default=100000, type=int, help='surface samples per direction')
    parser.add_argument('--seed', default=0, type=int)
    parser.add_argument('--thresholds', nargs='+', type=float, default=None,
                        help='distances for precision / recall / F-score, in the meshes\' length unit')
    parser.add_argument('--scale', default=1.0, type=float, help='factor on the prediction (captures in another unit)')
    parser.add_argument('--method', default='auto', choices=['auto', 'grid', 'brute'])
    parser.add_argument('--intersections', action='store_true',
                        help='also count the self-crossing faces of both meshes (and the body-crossing ones with --body)')
    parser.add_argument('--body', default=None, help='body mesh (.obj) or a directory of them paired by stem; needs --intersections')
    parser.add_argument('--penetration', action='store_true',
                        help='with --intersections --body: also the vertices of the prediction inside the body and their largest depth')
    parser.add_argument('--out', default=None, help='metrics JSON (default: printed only)')
    parser.add_argument('--align', default='none', choices=['none', 'rigid', 'similarity'],
                        help='fit the prediction to the ground truth by ICP before the metrics')
    parser.add_argument('--align-metric', default='plane', choices=['plane', 'point'])
    parser.add_argument('--align-trim', default=1.0, type=float, help='share of the pairs with the smallest distances that takes part')
    parser.add_argument('--align-iters', default=50, type=int, help='at most this many ICP steps')
    parser.add_argument('--align-from', default='each', choices=['each', 'first'],
                        help='first: the transform of the first pair by stem is applied to every pair')
    parser.add_argument('--align-out', default=None, help='directory for the aligned predictions (.obj)')
    parser.add_argument('--topology', action='store_true',
                        help='add the topology report of the prediction and of the ground truth to every pair')
    parser.add_argument('--drop-floaters', default=None, type=float, metavar='FRAC',
                        help='drop the pieces of the prediction with less than FRAC of its largest piece\'s area, before everything else')
    parser.add_argument('--repair', action='store_true',
                        help='mend the prediction and the ground truth before everything else (recmv.repair.repair)')
    parser.add_argument('--weld-eps', default=None, type=float,
                        help='a length: weld the vertices within it of each other before the repair (implies --repair)')
    parser.add_argument('--volume', action='store_true',
                        help='add the volumetric IoU and the two volumes of every pair (closed meshes; recmv.voxelize.volume_iou)')
    parser.add_argument('--fill-holes', action='store_true',
                        help='close the holes of both meshes after --repair and before the metrics (recmv.holes.fill)')
    parser.add_argument('--fill-max-edges', default=None, type=int, metavar='N', help='with --fill-holes: longer loops stay open')
    parser.add_argument('--fill-keep-largest', default=None, type=int, metavar='K',
                        help='with --fill-holes: the K loops of longest perimeter stay open')
    parser.add_argument('--voxel-sign', default='parity', choices=('parity', 'winding'),
                        help='with --volume: the sign of the lattices; winding (the generalized winding number) measures meshes '
                             'with holes and unites overlapping pieces, and its figures are never withheld')
    parser.add_argument('--inside-rule', default='parity', choices=('parity', 'winding'),
                        help='with --penetration: how a vertex is judged inside the body; winding takes a body with holes')
    parser.add_argument('--volume-step', default=None, type=float, metavar='S',
                        help='with --volume: the lattice step (default: 129 nodes along the longest axis of the pair\'s box)')
    parser.add_argument('--boundary-bands', default=None, metavar='W1,W2,...',
                        help='per pair, the error binned by geodesic distance to the border (ascending widths)')
    return parser


def parse_bands(text):
    """'W1,W2,...' -> the widths as floats: at least one, ascending, positive, finite.  ValueError otherwise."""
    try:
        widths = [float(t) for t in text.split(',')]
    except ValueError:
        raise ValueError("--boundary-bands takes numbers separated by commas (got %r)" % (text,))
    if not widths or not all(0. < w < float('inf') for w in widths):
        raise ValueError("--boundary-bands: the widths must be positive and finite (got %r)" % (text,))
    if any(b <= a for a, b in zip(widths, widths[1:])):
        raise ValueError("--boundary-bands: the widths must ascend (got %r)" % (text,))
    return widths


def band_stats(g, d, widths):
    """The samples with geodesic border distance g [P] and error d [P] (tensors) binned by g into [0, W1), [W1, W2), ...,
    [Wn, inf): a list of {'lo', 'hi', 'count', 'mean', 'rms', 'max'} (hi None for the last; None figures for an empty bin).
    A sample whose g is +inf (no border reaches it) falls into the last bin; one whose g is NaN into none."""
    import torch
    g, d = g.double(), d.double()
    edges = [0.] + list(widths) + [float('inf')]
    out = []
    for k, (lo, hi) in enumerate(zip(edges, edges[1:])):
        last = k == len(edges) - 2
        x = d[(g >= lo) & ((g <= hi) if last else (g < hi))]
        n = int(x.shape[0])
        out.append({'lo': lo, 'hi': None if last else hi, 'count': n,
                    'mean': float(x.mean()) if n else None, 'rms': float((x * x).mean().sqrt()) if n else None,
                    'max': float(x.max()) if n else None})
    return out


def boundary_bands(side_v, side_f, points, src_face, other_v, other_f, widths, method):
    """One side of a pair's `boundary_bands`: (bands, reason) — (None, "closed") for a mesh without a border."""
    from recmv import geodesic, metrics
    field = geodesic.boundary_distance(side_v, side_f)
    if not bool((field == 0.).any()):
        return None, 'closed'
    g = geodesic.interpolate(field, side_v, side_f, src_face, points)
    d = metrics._nearest(points, other_v, other_f, method)[2].double().sqrt()
    return band_stats(g, d, widths), None


def _objs(path):
    if osp.isdir(path):
        return {osp.splitext(n)[0]: osp.join(path, n) for n in sorted(os.listdir(path)) if n.lower().endswith('.obj')}
    return None


def pair_files(pred, gt):
    """(pairs [(stem, pred file, gt file)] sorted by stem, unmatched prediction files, unmatched ground-truth files).  Two
    files are one pair whatever their names; two directories are paired by stem.  ValueError when nothing pairs."""
    p, g = _objs(pred), _objs(gt)
    if (p is None) != (g is None):
        raise ValueError("--pred and --gt must both be files or both be directories")
    if p is None:
        for f in (pred, gt):
            if not osp.isfile(f):
                raise ValueError("no such mesh: %s" % f)
        return [(osp.splitext(osp.basename(pred))[0], pred, gt)], [], []
    pairs = [(s, p[s], g[s]) for s in sorted(p) if s in g]
    if not pairs:
        raise ValueError("no .obj stem is in both %s (%d meshes) and %s (%d meshes)" % (pred, len(p), gt, len(g)))
    return pairs, [p[s] for s in sorted(p) if s not in g], [g[s] for s in sorted(g) if s not in p]


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    widths = None
    if args.boundary_bands is not None:
        try:
            widths = parse_bands(args.boundary_bands)
        except ValueError as e:
            parser.error(str(e))
    try:
        pairs, only_pred, only_gt = pair_files(args.pred, args.gt)
    except ValueError as e:
        parser.error(str(e))
    if args.body and not args.intersections:
        parser.error("--body needs --intersections")
    if args.penetration and not (args.intersections and args.body):
        parser.error("--penetration needs --intersections and --body")
    bodies = None
    if args.body:
        bodies = _objs(args.body)
        if bodies is None and not osp.isfile(args.body):
            parser.error("no such mesh: %s" % args.body)
        if bodies is not None and not all(stem in bodies for stem, _, _ in pairs):
            parser.error("--body %s has no mesh for: %s" % (args.body, ', '.join(s for s, _, _ in pairs if s not in bodies)))
    if args.align == 'none' and args.align_out:
        parser.error("--align-out needs --align rigid or --align similarity")
    if not (0. < args.align_trim <= 1.):
        parser.error("--align-trim must be in (0, 1]")
    if args.align_iters < 0:
        parser.error("--align-iters must not be negative")
    if args.drop_floaters is not None and not (0. <= args.drop_floaters <= 1.):
        parser.error("--drop-floaters must be in [0, 1]")
    if args.weld_eps is not None and not (0. <= args.weld_eps < float('inf')):
        parser.error("--weld-eps must be finite and not negative")
    repairing = args.repair or args.weld_eps is not None
    if args.voxel_sign != 'parity' and not args.volume:
        parser.error("--voxel-sign needs --volume")
    if args.inside_rule != 'parity' and not args.penetration:
        parser.error("--inside-rule needs --penetration")
    if args.volume_step is not None and not args.volume:
        parser.error("--volume-step needs --volume")
    if args.volume_step is not None and not (0. < args.volume_step < float('inf')):
        parser.error("--volume-step must be positive and finite")
    if (args.fill_max_edges is not None or args.fill_keep_largest is not None) and not args.fill_holes:
        parser.error("--fill-max-edges and --fill-keep-largest need --fill-holes")
    if (args.fill_max_edges is not None and args.fill_max_edges < 0) or (args.fill_keep_largest is not None
                                                                         and args.fill_keep_largest < 0):
        parser.error("--fill-max-edges and --fill-keep-largest must not be negative")
    import torch
    from infer_fl_animation import temporal_smoothness
    from recmv import align, metrics, topology
    from recmv.utils import read_obj, write_obj

    device = torch.device('cuda:%d' % args.gpu_ids[0])
    thresholds = tuple(args.thresholds) if args.thresholds else metrics.DEFAULT_THRESHOLDS
    per_pair, sequence, alignment, shared, floaters, repaired, filled = {}, [], {}, None, {}, {}, {}
    for stem, pf, gf in pairs:
        pv, pfaces = read_obj(pf)
        gv, gfaces = read_obj(gf)
        pv = pv * args.scale
        if repairing:
            from recmv import repair
            rv, rf, rp = repair.repair(pv.to(device), pfaces.to(device), weld_eps=args.weld_eps)
            pv, pfaces = rv.cpu(), rf.cpu()
            rv, rf, rg = repair.repair(gv.to(device), gfaces.to(device), weld_eps=args.weld_eps)
            gv, gfaces = rv.cpu(), rf.cpu()
            repaired[stem] = {'repair_pred': repair.info_json(rp), 'repair_gt': repair.info_json(rg)}
            print('%s: repaired, prediction %d vertices and %d faces, ground truth %d vertices and %d faces' % (
                stem, pv.shape[0], pfaces.shape[0], gv.shape[0], gfaces.shape[0]))
        if args.fill_holes:
            from recmv import holes
            filled[stem] = {}
            try:
                hv, hf, hi = holes.fill(pv.to(device), pfaces.to(device), max_edges=args.fill_max_edges,
                                        keep_largest=args.fill_keep_largest or 0)
                pv, pfaces, filled[stem]['holes_pred'] = hv.cpu(), hf.cpu(), holes.info_json(hi)
                hv, hf, hi = holes.fill(gv.to(device), gfaces.to(device), max_edges=args.fill_max_edges,
                                        keep_largest=args.fill_keep_largest or 0)
                gv, gfaces, filled[stem]['holes_gt'] = hv.cpu(), hf.cpu(), holes.info_json(hi)
            except ValueError as e:
                parser.error("%s: %s" % (stem, e))
            print('%s: holes filled, prediction %d of %d loops, ground truth %d of %d' % (
                stem, filled[stem]['holes_pred']['filled'], filled[stem]['holes_pred']['loops'],
                filled[stem]['holes_gt']['filled'], filled[stem]['holes_gt']['loops']))
        if args.drop_floaters is not None:
            kv, kf, kept = topology.keep_components(pv.to(device), pfaces.to(device), min_area_frac=args.drop_floaters)
            floaters[stem] = {'min_area_frac': args.drop_floaters, 'components': kept['components'],
                              'dropped_components': kept['dropped_components'], 'dropped_faces': kept['dropped_faces'],
                              'dropped_area': kept['dropped_area'], 'invalid_faces': kept['invalid_faces'],
                              'vertices': int(kv.shape[0]), 'faces': int(kf.shape[0])}
            pv, pfaces = kv.cpu(), kf.cpu()
            print('%s: dropped %d of %d pieces (%d faces)' % (stem, kept['dropped_components'], kept['components'],
                                                              kept['dropped_faces']))
        if args.align != 'none':
            fit = shared
            if fit is None:
                fit = align.icp(pv.to(device), pfaces.to(device), gv.to(device), gfaces.to(device), mode=args.align,
                                metric=args.align_metric, seed=args.seed,
                                iters=args.align_iters, trim=args.align_trim, method=args.method)
                if args.align_from == 'first':
                    shared = fit
            alignment[stem] = {k: fit[k] for k in ('scale', 'R', 't', 'iterations', 'converged', 'rms_before', 'rms_after',
                                                   'pairs')}
            pv = align.apply(fit, pv)
            print('%s: aligned (%s, %s): scale %.6g, rms %.6g -> %.6g in %d steps%s' % (
                stem, args.align, args.align_metric, fit['scale'], fit['rms_before'], fit['rms_after'], fit['iterations'],
                '' if args.align_from == 'each' or stem == pairs[0][0] else ' of ' + pairs[0][0]))
            if args.align_out:
                os.makedirs(args.align_out, exist_ok=True)
                write_obj(osp.join(args.align_out, stem + '.obj'), pv, pfaces)
        sequence.append((pv, pfaces))
        per_pair[stem] = metrics.surface_distance(pv.to(device), pfaces.to(device), gv.to(device), gfaces.to(device),
                                                  samples=args.samples, seed=args.seed, thresholds=thresholds,
                                                  method=args.method, return_samples=widths is not None)
        if widths is not None:
            per_pair[stem], drawn = per_pair[stem]
            dv, df, ev, ef = pv.to(device), pfaces.to(device), gv.to(device), gfaces.to(device)
            bp, why_p = boundary_bands(dv, df, drawn['pred'][0], drawn['pred'][1], ev, ef, widths, args.method)
            bg, why_g = boundary_bands(ev, ef, drawn['gt'][0], drawn['gt'][1], dv, df, widths, args.method)
            per_pair[stem]['boundary_bands'] = {'widths': widths, 'pred': bp, 'pred_reason': why_p, 'gt': bg, 'gt_reason': why_g}
        if args.intersections:
            own = metrics.self_intersections(pv.to(device), pfaces.to(device), method=args.method)
            own_gt = metrics.self_intersections(gv.to(device), gfaces.to(device), method=args.method)
            per_pair[stem].update({'self_intersecting_faces': int(own['faces'].shape[0]),
                                   'self_intersection_ratio': own['ratio'],
                                   'self_intersecting_faces_gt': int(own_gt['faces'].shape[0]),
                                   'self_intersection_ratio_gt': own_gt['ratio']})
            if args.body:
                bv, bfaces = read_obj(bodies[stem] if bodies is not None else args.body)
                hit = metrics.mesh_intersections(pv.to(device), pfaces.to(device), bv.to(device), bfaces.to(device),
                                                 method=args.method)
                per_pair[stem].update({'body_intersecting_faces': int(hit['faces_a'].shape[0]),
                                       'body_intersection_ratio': hit['ratio_a']})
                if args.penetration:
                    pen = metrics.penetration(pv.to(device), bv.to(device), bfaces.to(device), method=args.method,
                                              rule=args.inside_rule)
                    per_pair[stem].update({'body_inside_vertices': pen['count'], 'body_max_depth': pen['max_depth']})
                    if args.inside_rule != 'parity':
                        per_pair[stem]['body_inside'] = {'rule': args.inside_rule}
        if args.volume:
            from recmv import voxelize
            vol = voxelize.volume_iou(pv.to(device), pfaces.to(device), gv.to(device), gfaces.to(device), step=args.volume_step,
                                      method=args.method, sign=args.voxel_sign)
            closed = args.voxel_sign == 'winding' or not (vol['open_columns_a'] or vol['open_columns_b'] or vol['sign_conflicts_a']
                                                          or vol['sign_conflicts_b'])
            per_pair[stem].update({'volume_iou': vol['iou'] if closed else None, 'volume_pred': vol['volume_a'] if closed else None,
                                   'volume_gt': vol['volume_b'] if closed else None})
            per_pair[stem]['volume'] = {'step': vol['step'], 'lattice': vol['lattice'].json(), 'intersection': vol['intersection'],
                                        'union': vol['union'], 'open_columns_pred': vol['open_columns_a'],
                                        'open_columns_gt': vol['open_columns_b'], 'sign_conflicts_pred': vol['sign_conflicts_a'],
                                        'sign_conflicts_gt': vol['sign_conflicts_b'],
                                        'reason': None if closed else 'a mesh of the pair is not closed (open_columns or sign_conflicts > 0): '
                                                                      'a crossing parity gives it no volume'}
            if args.voxel_sign != 'parity':
                per_pair[stem]['volume']['sign'] = args.voxel_sign
        if stem in floaters:
            per_pair[stem]['floaters'] = floaters[stem]
        if stem in repaired:
            per_pair[stem].update(repaired[stem])
        if stem in filled:
            per_pair[stem].update(filled[stem])
        if args.topology:
            per_pair[stem]['topology_pred'] = topology.report(pv.to(device), pfaces.to(device))
            per_pair[stem]['topology_gt'] = topology.report(gv.to(device), gfaces.to(device))
        print('%s: chamfer_l1 %.6g, accuracy %.6g, completeness %.6g, normal consistency %.4f' % (
            stem, per_pair[stem]['chamfer_l1'], per_pair[stem]['accuracy'], per_pair[stem]['completeness'],
            per_pair[stem]['normal_consistency']))
    keys = [k for k, x in next(iter(per_pair.values())).items() if not isinstance(x, dict)]
    if args.volume:                                        # a figure that is None for a pair (a mesh that is not closed) has no mean
        keys = [k for k in keys if all(m[k] is not None for m in per_pair.values())]
    mean = {k: sum(m[k] for m in per_pair.values()) / len(per_pair) for k in keys}
    res = {'pairs': per_pair, 'mean': mean, 'samples': args.samples, 'seed': args.seed, 'method': args.method,
           'thresholds': list(thresholds), 'scale': args.scale, 'unmatched_pred': only_pred, 'unmatched_gt': only_gt}
    if repairing:                                          # (without these flags the output is what it always was)
        res['repair'] = {'weld_eps': args.weld_eps}
    if args.fill_holes:
        res['fill_holes'] = {'max_edges': args.fill_max_edges, 'keep_largest': args.fill_keep_largest}
    if args.align != 'none':                               # (not into pairs[stem]: `mean` sums every key there)
        res['align'] = {'mode': args.align, 'metric': args.align_metric, 'trim': args.align_trim, 'iters': args.align_iters,
                        'from': args.align_from}
        res['alignment'] = alignment
    v0, f0 = sequence[0]
    if osp.isdir(args.pred) and all(v.shape == v0.shape and torch.equal(f, f0) for v, f in sequence):
        res['temporal_smoothness'] = temporal_smoothness(torch.stack([v for v, _ in sequence]).numpy())
    print('mean over %d pairs: %s' % (len(per_pair), json.dumps(mean)))
    if only_pred or only_gt:
        print('skipped, without a partner: %s' % ', '.join(only_pred + only_gt))
    if args.out:
        os.makedirs(osp.dirname(osp.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
    return res


if __name__ == '__main__':
    main()
