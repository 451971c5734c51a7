"""clean_fl.py — what exported meshes are made of, and the same meshes without their floaters: an addition, the reference has
no such command (recmv.topology has the definitions).

`--in` is one `.obj` file or a directory of them.  Every mesh is described (recmv.topology.report: pieces, boundary loops, Euler
characteristic, watertightness, triangle quality, the largest pieces with their genus), cleaned
(recmv.topology.keep_components: a piece stays when it passes every rule given — `--largest N`: among the N largest by area,
`--min-area-frac X`: at least X times the largest piece's area, `--min-faces N`: at least N faces; invalid faces and vertices
that no kept face uses always go; `--connectivity edge` joins faces only across shared edges), described again and written to
`--out` under its own name.  `--simplify-faces N` or `--simplify-ratio R` and / or `--simplify-max-error E` then thin what is left
(recmv.simplify.simplify: quadric-error edge collapse down to N faces, or to the share R of the cleaned mesh's faces, never
moving the surface by more than E in the root-mean-square sense of the quadrics) before it is described and written; the mesh
must be edge-manifold by then.  `--smooth taubin|laplacian|bilateral` smooths what is left BEFORE it is simplified, so that the
quadrics see the de-noised planes (recmv.smooth.smooth; `--smooth-iters`, `--smooth-lambda`, `--smooth-mu`, `--smooth-weights
uniform|cotangent` for the first two, `--smooth-normal-iters`, `--smooth-vertex-iters`, `--smooth-sigma-s` for bilateral;
`--smooth-boundary fixed|curve|free`: open boundaries stay where they are by default).  `--repair` mends every mesh FIRST OF ALL,
before any of the above (recmv.repair.repair: degenerate and duplicate faces dropped, every edge with more than two faces and every
pinch vertex taken apart, every orientable piece consistently oriented, unused vertices dropped); `--weld-eps E` (a length; it
implies `--repair`) first welds the vertices within E of each other, 0 the coincident ones — without it nothing is welded.  That
is the way to an edge-manifold mesh; topology.json then holds `repair` per file, the numbers of that call's info.
`--voxel-remesh STEP` (or `--voxel-resolution N`, the nodes along the longest axis) remeshes what is left through a distance
lattice BEFORE it is smoothed or simplified (recmv.voxelize.remesh: exact distances in a narrow band, a crossing-parity sign,
marching cubes — a watertight manifold mesh of uniform resolution from a CLOSED mesh, whatever its self-intersections);
topology.json then holds `voxel` per file (lattice, band_nodes, open_columns, sign_conflicts, faces before and after).  A mesh
that is not closed shows as open_columns > 0 or sign_conflicts > 0 and the command refuses it, writing nothing, unless
`--voxel-force` is given.  `--voxel-sign winding` takes the sign from the generalized winding number instead
(recmv.winding, |w| > 1/2 at every node): a mesh with holes is capped coarsely where w = 1/2, overlapping pieces unite, the two
diagnostics are information only and nothing is refused; `voxel` then holds `sign`.  `--solidify T` takes the
unsigned route instead (recmv.voxelize.solidify: a closed shell of thickness T around an open garment; the voxel flag gives the
step).
`--fill-holes` closes the holes of what is left AFTER the repair and the floaters and BEFORE the voxel remesh, the smoothing and
the simplification (recmv.holes.fill: every boundary loop triangulated with the least area; the mesh must be edge-manifold and
consistently oriented, which `--repair` sees to).  Garments are open by design, so say which loops are holes: `--fill-max-edges N`
and `--fill-max-perimeter P` leave longer loops open, `--fill-keep-largest K` leaves the K longest open (a skirt has 2 openings,
trousers 3, a shirt 4).  `--fill-refine` splits and flips the patches' inner edges down to the length of their borders' and
`--fill-fair-iters N` (with it) then relaxes the new vertices.  topology.json then holds `holes` per file, that call's info, and
the per-file report shows the boundary loops before and after.  With it `--voxel-remesh` takes a holed mesh without
`--voxel-force`.
`--out`/topology.json holds per file
the report `before`, the report `after` and what was `dropped`, with a simplify flag `simplify`: that call's info, and with
`--smooth` `smooth`: that call's info, beside the smooth parameters at the top level.  With `--report-only` nothing is cleaned or written but
topology.json (with `before` alone; printed when there is no `--out`): on a registered run it is the check that `registry_<garment>.obj` is one piece with the expected number of boundary
loops — an upper garment with four feature lines has four.

    python rec-mv_amd/clean_fl.py --gpu-ids 0 --in <obj|dir> --out <dir> [--largest N] [--min-area-frac X] [--min-faces N]
        [--connectivity vertex|edge] [--simplify-faces N | --simplify-ratio R] [--simplify-max-error E] [--report-only]
        [--smooth taubin|laplacian|bilateral] [--smooth-iters N] [--smooth-lambda L] [--smooth-mu M]
        [--smooth-weights uniform|cotangent] [--smooth-boundary fixed|curve|free] [--smooth-normal-iters N]
        [--smooth-vertex-iters N] [--smooth-sigma-s S] [--repair] [--weld-eps E]
        [--voxel-remesh STEP | --voxel-resolution N] [--voxel-force] [--voxel-sign parity|winding] [--solidify T]
        [--fill-holes] [--fill-max-edges N] [--fill-max-perimeter P] [--fill-keep-largest K] [--fill-refine]
        [--fill-fair-iters N]
"""
import argparse
import json
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))


def build_parser():
    parser = argparse.ArgumentParser(description='topology report of meshes and removal of their small detached pieces')
    parser.add_argument('--gpu-ids', nargs='+', type=int, default=[0], metavar='IDs', help='gpu ids (the first is used)')
    parser.add_argument('--in', dest='inp', required=True, help='mesh (.obj) or a directory of them')
    parser.add_argument('--out', default=None, help='directory for the cleaned meshes and topology.json')
    parser.add_argument('--largest', default=None, type=int, help='keep at most this many pieces, the largest by area')
    parser.add_argument('--min-area-frac', default=None, type=float,
                        help='keep the pieces with at least this share of the largest piece\'s area')
    parser.add_argument('--min-faces', default=None, type=int, help='keep the pieces with at least this many faces')
    parser.add_argument('--connectivity', default='vertex', choices=['vertex', 'edge'],
                        help='what joins two faces into one piece: a shared vertex, or only a shared edge')
    parser.add_argument('--simplify-faces', default=None, type=int, help='after cleaning, simplify every mesh to this many faces')
    parser.add_argument('--simplify-ratio', default=None, type=float,
                        help='after cleaning, simplify every mesh to this share of its faces')
    parser.add_argument('--simplify-max-error', default=None, type=float,
                        help='no collapse whose quadric error (a length) is above this; alone: collapse until none is left')
    parser.add_argument('--smooth', default=None, choices=['taubin', 'laplacian', 'bilateral'],
                        help='after cleaning and before simplifying, smooth every mesh with this method')
    parser.add_argument('--smooth-iters', default=10, type=int, help='taubin / laplacian iterations')
    parser.add_argument('--smooth-lambda', default=0.5, type=float, help='the step, in (0, 1]')
    parser.add_argument('--smooth-mu', default=None, type=float, help='taubin\'s second step, < 0 (default: pass-band 0.1)')
    parser.add_argument('--smooth-weights', default='uniform', choices=['uniform', 'cotangent'], help='the neighbours\' weights')
    parser.add_argument('--smooth-boundary', default='fixed', choices=['fixed', 'curve', 'free'],
                        help='boundary vertices stay, move along their curve, or move like the interior')
    parser.add_argument('--smooth-normal-iters', default=5, type=int, help='bilateral: iterations of the normal filter')
    parser.add_argument('--smooth-vertex-iters', default=10, type=int, help='bilateral: iterations of the vertex update')
    parser.add_argument('--smooth-sigma-s', default=0.35, type=float, help='bilateral: the normal difference that still counts')
    parser.add_argument('--repair', action='store_true',
                        help='first of all mend every mesh: drop degenerate faces, split non-manifold edges and vertices, orient')
    parser.add_argument('--weld-eps', default=None, type=float,
                        help='a length: weld the vertices within it of each other before the repair (implies --repair)')
    parser.add_argument('--voxel-remesh', default=None, type=float, metavar='STEP',
                        help='after cleaning and before smoothing, remesh every (closed) mesh through a distance lattice of this step')
    parser.add_argument('--voxel-resolution', default=None, type=int, metavar='N',
                        help='the same with the step chosen so that the lattice has N nodes along the longest axis')
    parser.add_argument('--voxel-force', action='store_true',
                        help='write the voxel remesh even when columns of the lattice end inside (the mesh is not closed)')
    parser.add_argument('--voxel-sign', default='parity', choices=('parity', 'winding'),
                        help='the sign of the voxel remesh: the crossing parity (closed meshes only), or the generalized winding '
                             'number, which takes holes and overlapping pieces and never refuses')
    parser.add_argument('--solidify', default=None, type=float, metavar='T',
                        help='instead of the signed remesh: a closed shell of thickness T around every (open) mesh; '
                             '--voxel-remesh or --voxel-resolution gives the step')
    parser.add_argument('--fill-holes', action='store_true',
                        help='after the repair and the floaters and before every later stage, close the holes (least-area patches)')
    parser.add_argument('--fill-max-edges', default=None, type=int, metavar='N', help='loops of more than N edges stay open')
    parser.add_argument('--fill-max-perimeter', default=None, type=float, metavar='P', help='loops longer than P stay open')
    parser.add_argument('--fill-keep-largest', default=None, type=int, metavar='K',
                        help='the K loops of longest perimeter stay open (the openings of a garment)')
    parser.add_argument('--fill-refine', action='store_true', help='split and flip the inner edges of the patches')
    parser.add_argument('--fill-fair-iters', default=None, type=int, metavar='N',
                        help='with --fill-refine: Laplacian iterations on the new vertices')
    parser.add_argument('--report-only', action='store_true', help='describe the meshes, clean and write none')
    return parser


def check_fill_flags(parser, args):
    """The parser errors of the --fill-* flags."""
    given = [flag for flag, x in (('--fill-max-edges', args.fill_max_edges), ('--fill-max-perimeter', args.fill_max_perimeter),
                                  ('--fill-keep-largest', args.fill_keep_largest), ('--fill-refine', args.fill_refine or None),
                                  ('--fill-fair-iters', args.fill_fair_iters)) if x is not None]
    if given and not args.fill_holes:
        parser.error("%s needs --fill-holes" % given[0])
    if args.fill_holes and args.report_only:
        parser.error("--report-only writes no mesh: --fill-holes needs --out")
    if args.fill_max_edges is not None and args.fill_max_edges < 0:
        parser.error("--fill-max-edges must not be negative")
    if args.fill_max_perimeter is not None and not (0. <= args.fill_max_perimeter < float('inf')):
        parser.error("--fill-max-perimeter must be finite and not negative")
    if args.fill_keep_largest is not None and args.fill_keep_largest < 0:
        parser.error("--fill-keep-largest must not be negative")
    if args.fill_fair_iters is not None and args.fill_fair_iters < 0:
        parser.error("--fill-fair-iters must not be negative")
    if args.fill_fair_iters and not args.fill_refine:
        parser.error("--fill-fair-iters needs --fill-refine: without it a patch has no vertex of its own")


def mesh_files(path):
    """[(name, file)] of the `.obj` files of a directory sorted by name, or of the one file."""
    if osp.isdir(path):
        return [(n, osp.join(path, n)) for n in sorted(os.listdir(path)) if n.lower().endswith('.obj')]
    if osp.isfile(path):
        return [(osp.basename(path), path)]
    raise ValueError("no such mesh or directory: %s" % path)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.min_area_frac is not None and not (0. <= args.min_area_frac <= 1.):
        parser.error("--min-area-frac must be in [0, 1]")
    if args.largest is not None and args.largest < 1:
        parser.error("--largest must be at least 1")
    if args.min_faces is not None and args.min_faces < 0:
        parser.error("--min-faces must not be negative")
    if args.simplify_faces is not None and args.simplify_ratio is not None:
        parser.error("give --simplify-faces or --simplify-ratio, not both")
    if args.simplify_faces is not None and args.simplify_faces < 0:
        parser.error("--simplify-faces must not be negative")
    if args.simplify_ratio is not None and not (0. <= args.simplify_ratio <= 1.):
        parser.error("--simplify-ratio must be in [0, 1]")
    if args.simplify_max_error is not None and not (args.simplify_max_error >= 0.):
        parser.error("--simplify-max-error must not be negative")
    simplifying = not (args.simplify_faces is None and args.simplify_ratio is None and args.simplify_max_error is None)
    if simplifying and args.report_only:
        parser.error("--report-only writes no mesh: the simplify flags need --out")
    if args.smooth is not None:
        if args.report_only:
            parser.error("--report-only writes no mesh: --smooth needs --out")
        if args.smooth_iters < 0 or args.smooth_normal_iters < 0 or args.smooth_vertex_iters < 0:
            parser.error("the --smooth-*-iters must not be negative")
        if not (0. < args.smooth_lambda <= 1.):
            parser.error("--smooth-lambda must be in (0, 1]")
        if args.smooth_mu is not None and not (-float('inf') < args.smooth_mu < 0.):
            parser.error("--smooth-mu must be finite and below 0")
        if not (0. < args.smooth_sigma_s < float('inf')):
            parser.error("--smooth-sigma-s must be finite and above 0")
    if args.weld_eps is not None and not (0. <= args.weld_eps < float('inf')):
        parser.error("--weld-eps must be finite and not negative")
    repairing = args.repair or args.weld_eps is not None
    if repairing and args.report_only:
        parser.error("--report-only writes no mesh: --repair and --weld-eps need --out")
    voxelising = args.voxel_remesh is not None or args.voxel_resolution is not None
    if args.voxel_remesh is not None and args.voxel_resolution is not None:
        parser.error("give --voxel-remesh or --voxel-resolution, not both")
    if args.voxel_remesh is not None and not (0. < args.voxel_remesh < float('inf')):
        parser.error("--voxel-remesh must be a positive, finite step")
    if args.voxel_resolution is not None and args.voxel_resolution < 2:
        parser.error("--voxel-resolution must be at least 2")
    if args.solidify is not None:
        if not voxelising:
            parser.error("--solidify needs --voxel-remesh or --voxel-resolution for the step")
        if not (0. < args.solidify < float('inf')):
            parser.error("--solidify must be a positive, finite thickness")
    if args.voxel_force and not voxelising:
        parser.error("--voxel-force needs --voxel-remesh or --voxel-resolution")
    if args.voxel_sign != 'parity' and not voxelising:
        parser.error("--voxel-sign needs --voxel-remesh or --voxel-resolution")
    if args.voxel_sign != 'parity' and args.solidify is not None:
        parser.error("--solidify is unsigned: --voxel-sign does not apply")
    if voxelising and args.report_only:
        parser.error("--report-only writes no mesh: the voxel flags need --out")
    check_fill_flags(parser, args)
    if not args.report_only and not args.out:
        parser.error("--out is needed unless --report-only is given")
    try:
        files = mesh_files(args.inp)
    except ValueError as e:
        parser.error(str(e))
    if not files:
        parser.error("no .obj file in %s" % args.inp)
    import torch
    from recmv import topology
    from recmv.utils import read_obj, write_obj

    device = torch.device('cuda:%d' % args.gpu_ids[0])
    res = {}
    for name, path in files:
        v, f = read_obj(path)
        v, f = v.to(device), f.to(device)
        entry = {'before': topology.report(v, f)}
        b = entry['before']
        print('%s: %d faces, %d pieces (%d by edges), %d boundary loops, euler characteristic %d, watertight %s' % (
            name, b['faces'], b['components_vertex'], b['components_edge'], b['boundary_loops'], b['euler_characteristic'],
            b['watertight']))
        if repairing:                                      # first of all: every later stage sees the mended mesh
            from recmv import repair
            faces_before = int(f.shape[0])
            v, f, ri = repair.repair(v, f, weld_eps=args.weld_eps)
            entry['repair'] = ri = repair.info_json(ri)
            print('%s: repaired, %d vertices welded, %d of %d faces dropped, %d vertices added at non-manifold places, %d faces '
                  'flipped, %d pieces not orientable' % (
                      name, ri['weld']['merged_vertices'] if 'weld' in ri else 0, faces_before - int(f.shape[0]), faces_before,
                      ri['split_nonmanifold']['added_vertices'], ri['orient']['flipped_faces'],
                      ri['orient']['non_orientable_pieces']))
        if not args.report_only:
            kv, kf, info = topology.keep_components(v, f, largest=args.largest, min_area_frac=args.min_area_frac,
                                                    min_faces=args.min_faces, connectivity=args.connectivity)
            if args.fill_holes:                            # behind the repair and the floaters, before every later stage
                from recmv import holes
                try:
                    kv, kf, hi = holes.fill(kv, kf, max_edges=args.fill_max_edges, max_perimeter=args.fill_max_perimeter,
                                            keep_largest=args.fill_keep_largest or 0, refine=args.fill_refine,
                                            fair_iterations=args.fill_fair_iters or 0)
                except ValueError as e:
                    parser.error("%s: %s" % (name, e))
                entry['holes'] = hi = holes.info_json(hi)
                print('%s: %d boundary loops, %d filled with %d faces and %d vertices, %d left open' % (
                    name, hi['loops'], hi['filled'], sum(hi['faces_added']), sum(hi['verts_added']), hi['loops'] - hi['filled']))
            if voxelising:                                 # behind the repair and the floaters, before smoothing and simplifying
                from recmv import voxelize
                try:
                    if args.solidify is not None:
                        kv, kf, vi = voxelize.solidify(kv, kf, args.solidify, step=args.voxel_remesh,
                                                       resolution=args.voxel_resolution)
                    else:
                        kv, kf, vi = voxelize.remesh(kv, kf, step=args.voxel_remesh, resolution=args.voxel_resolution,
                                                     sign=args.voxel_sign)
                except ValueError as e:
                    parser.error("%s: %s" % (name, e))
                if (vi['open_columns'] > 0 or vi['sign_conflicts'] > 0) and not args.voxel_force and args.voxel_sign == 'parity':
                    parser.error("%s: open_columns = %d, sign_conflicts = %d: columns of the lattice end inside the mesh, or nodes far "
                                 "from the surface disagree about their side, so the mesh is not closed (or a parity was lost) and "
                                 "its voxel remesh is not to be trusted; nothing written.  --solidify is for open surfaces; "
                                 "--voxel-force writes the remesh all the same" % (name, vi['open_columns'], vi['sign_conflicts']))
                entry['voxel'] = {'mode': 'solidify' if args.solidify is not None else 'remesh', 'lattice': vi['lattice'].json(),
                                  'band': vi['band'], 'band_nodes': vi['band_nodes'], 'open_columns': vi['open_columns'],
                                  'sign_conflicts': vi['sign_conflicts'], 'faces_before': vi['faces_in'], 'faces_after': vi['faces_out']}
                if args.solidify is None:
                    entry['voxel']['sign'] = vi['sign']
                print('%s: voxel %s on %d x %d x %d nodes of step %g: %d -> %d faces, %d band nodes, %d open columns, %d sign '
                      'conflicts' % (name, entry['voxel']['mode'], *vi['lattice'].dims, vi['lattice'].step, vi['faces_in'],
                                     vi['faces_out'], vi['band_nodes'], vi['open_columns'], vi['sign_conflicts']))
            if args.smooth is not None:                   # before the quadrics are built: they then see the de-noised planes
                from recmv import smooth
                kv, entry['smooth'] = smooth.smooth(kv, kf, method=args.smooth, iterations=args.smooth_iters, lam=args.smooth_lambda,
                                                    mu=args.smooth_mu, weights=args.smooth_weights, boundary=args.smooth_boundary,
                                                    normal_iterations=args.smooth_normal_iters,
                                                    vertex_iterations=args.smooth_vertex_iters, sigma_s=args.smooth_sigma_s)
                si = entry['smooth']
                print('%s: smoothed (%s), %d vertices moved by at most %.3g, roughness %.4f -> %.4f' % (
                    name, args.smooth, si['moved'], si['displacement_max'], si['roughness_before'], si['roughness_after']))
            if simplifying:
                from recmv import simplify
                kept = int(kf.shape[0])
                kv, kf, entry['simplify'] = simplify.simplify(kv, kf, target_faces=args.simplify_faces, ratio=args.simplify_ratio,
                                                              max_error=args.simplify_max_error)
            entry['after'] = topology.report(kv, kf)
            entry['dropped'] = {'components': info['dropped_components'], 'faces': info['dropped_faces'],
                                'area': info['dropped_area'], 'invalid_faces': info['invalid_faces'],
                                'vertices': int(v.shape[0] - kv.shape[0])}
            os.makedirs(args.out, exist_ok=True)
            write_obj(osp.join(args.out, name), kv, kf)
            print('%s: dropped %d of %d pieces (%d faces, %d vertices)' % (name, info['dropped_components'], info['components'],
                                                                          info['dropped_faces'], entry['dropped']['vertices']))
            if simplifying:
                si = entry['simplify']
                print('%s: simplified %d -> %d faces in %d rounds (%s), largest error %.3g' % (
                    name, kept, si['faces_after'], si['rounds'], si['stopped'], si['max_error']))
        res[name] = entry
    out = {'files': res, 'connectivity': args.connectivity, 'largest': args.largest, 'min_area_frac': args.min_area_frac,
           'min_faces': args.min_faces, 'report_only': args.report_only}
    if simplifying:                                        # (without these flags topology.json is what it always was)
        out.update({'simplify_faces': args.simplify_faces, 'simplify_ratio': args.simplify_ratio,
                    'simplify_max_error': args.simplify_max_error})
    if repairing:                                          # (likewise)
        out.update({'repair': True, 'weld_eps': args.weld_eps})
    if voxelising:                                         # (likewise)
        out.update({'voxel_remesh': args.voxel_remesh, 'voxel_resolution': args.voxel_resolution, 'voxel_force': args.voxel_force,
                    'solidify': args.solidify})
    if args.fill_holes:                                    # (likewise)
        out.update({'fill_holes': True, 'fill_max_edges': args.fill_max_edges, 'fill_max_perimeter': args.fill_max_perimeter,
                    'fill_keep_largest': args.fill_keep_largest, 'fill_refine': args.fill_refine,
                    'fill_fair_iters': args.fill_fair_iters})
    if args.smooth is not None:                            # (likewise)
        out.update({'smooth': args.smooth, 'smooth_iters': args.smooth_iters, 'smooth_lambda': args.smooth_lambda,
                    'smooth_mu': args.smooth_mu, 'smooth_weights': args.smooth_weights, 'smooth_boundary': args.smooth_boundary,
                    'smooth_normal_iters': args.smooth_normal_iters, 'smooth_vertex_iters': args.smooth_vertex_iters,
                    'smooth_sigma_s': args.smooth_sigma_s})
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(osp.join(args.out, 'topology.json'), 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
    else:
        print(json.dumps(out, indent=1, sort_keys=True))
    return out


if __name__ == '__main__':
    main()
