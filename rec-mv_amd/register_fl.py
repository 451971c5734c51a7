"""register_fl.py — garment-template registration of a trained run (the `registration` step of the reference's
`infer_garment`, engineer/networks/OptimGarmentNetwork.py:2316-2514, on recmv.registration).

Loads the run the way infer_fl.py does, extracts the canonical garment meshes at the `fine` pyramid, fits each garment's
template (`--template <garment>=<obj>`, one per garment) to its mesh by NR-ICP and writes `<rec-root>/registry_<garment>.obj`.
When every registry file exists they are kept (the reference's cache).  Then `infer_fl.py --registry` poses them.
`--align-curves` first deforms each template so that its boundary loops land on the run's feature curves (the reference's
`fl_init_registry`, recmv.engineer.optimizer.Laplacian_Optimizer); the run must have been trained with the curve branch.
`--iso-remesh` iso-remeshes the coarse NR-ICP result before the refine pass (the reference's `remesh_garment_mesh`:
isotropic remeshing, then Loop subdivision; recmv.iso_remesh).

    python rec-mv_amd/register_fl.py --gpu-ids 0 --rec-root <capture>/<save-folder> --data-type scene \\
        --template short_sleeve_upper=upper.obj --template short_pants=pants.obj
"""
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))

from infer_fl import build_parser as _infer_parser  # noqa: E402


def build_parser():
    parser = _infer_parser()
    parser.description = 'garment template registration (Laplacian alignment to the feature curves, NR-ICP)'
    parser.add_argument('--template', action='append', default=[], metavar='GARMENT=OBJ',
                        help='template mesh of a garment (repeat for every garment)')
    parser.add_argument('--fit-epochs', type=int, default=None, help='epochs of the coarse pass (default 200)')
    parser.add_argument('--refine-epochs', type=int, default=None, help='epochs of the refine pass (default 100)')
    parser.add_argument('--inner-iter', type=int, default=None, help='inner iterations after the first epoch (default 50)')
    parser.add_argument('--dense-pcl', type=float, default=None, help='subdivide templates to this many vertices (default 4e4)')
    parser.add_argument('--torch-path', action='store_true',
                        help='fit with the plain-torch NR-ICP (and the dense Laplacian solve, the torch iso-remesh) instead of the '
                             'kernels')
    parser.add_argument('--align-curves', action='store_true',
                        help="first align each template's boundary loops to the run's feature curves (Laplacian deformation)")
    parser.add_argument('--align-epochs', type=int, default=None, help='epochs of the curve alignment (default 3)')
    parser.add_argument('--iso-remesh', action='store_true',
                        help='iso-remesh the coarse result (isotropic remeshing, then Loop subdivision) before the refine pass')
    parser.add_argument('--iso-remesh-iters', type=int, default=None, help='isotropic remeshing iterations (default 3)')
    parser.add_argument('--iso-remesh-len', type=float, default=None,
                        help='target edge length as a fraction of the bounding-box diagonal (default 0.01)')
    parser.add_argument('--iso-remesh-subdiv', type=int, default=None, help='Loop subdivision levels (default 1)')
    return parser


def _templates(specs, names):
    out = {}
    for spec in specs:
        if '=' not in spec:
            raise SystemExit("--template expects GARMENT=OBJ, got %r" % spec)
        name, path = spec.split('=', 1)
        out[name] = path
    unknown = sorted(set(out) - set(names))
    if unknown:
        raise SystemExit("--template: unknown garment(s) %s (this run has %s)" % (", ".join(unknown), ", ".join(names)))
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    from recmv import metrics, registration, utils
    from infer_fl import load_run

    rec_root = osp.normpath(args.rec_root)
    if args.align_epochs is not None and not args.align_curves:
        raise SystemExit("--align-epochs needs --align-curves")
    for flag in ('iters', 'len', 'subdiv'):
        if getattr(args, 'iso_remesh_' + flag) is not None and not args.iso_remesh:
            raise SystemExit("--iso-remesh-%s needs --iso-remesh" % flag)
    optNet, _, _, TmpVs_list, Tmpfs_list = load_run(args, curves=args.align_curves)
    names = list(optNet.garment_names)
    paths = [registration.registry_path(rec_root, n) for n in names]
    if all(osp.isfile(p) for p in paths):
        print('registry meshes exist, loading: ' + ', '.join(paths))
        return registration.register_garments(optNet, None, None, None, rec_root)
    given = _templates(args.template, names)
    missing = [n for n in names if n not in given]
    if missing:
        raise SystemExit("--template needed for garment(s) %s" % ", ".join(missing))
    templates = [utils.read_obj(given[n]) for n in names]
    over = {}
    if args.inner_iter is not None:
        over['inner_iter'] = args.inner_iter
    if args.dense_pcl is not None:
        over['dense_pcl'] = args.dense_pcl
    fit = dict(over, **({'epoch': args.fit_epochs} if args.fit_epochs is not None else {}))
    refine = dict(over, **({'epoch': args.refine_epochs} if args.refine_epochs is not None else {}))
    curves, align = None, None
    if args.align_curves:
        pts = optNet.inter_free_curve.inference()
        curves = {n: pts[i] for i, n in enumerate(optNet.fl_names)}
        align = {'epoch': args.align_epochs} if args.align_epochs is not None else None
    iso = None
    if args.iso_remesh:
        iso = {k: v for k, v in (('iterations', args.iso_remesh_iters), ('target_len_frac', args.iso_remesh_len),
                                 ('subdiv_levels', args.iso_remesh_subdiv)) if v is not None}
    meshes = registration.register_garments(optNet, templates, TmpVs_list[1:], Tmpfs_list[1:], rec_root, fit=fit,
                                            refine=refine, use_kernels=not args.torch_path, curves=curves, align=align,
                                            iso_remesh=iso)
    for n, p, (v, f) in zip(names, paths, meshes):
        print('%s: %d vertices, %d faces -> %s' % (n, v.shape[0], f.shape[0], p))
        if v.shape[0] and f.shape[0]:                      # a fit or a remesh can fold the template: say so (a log line only)
            dev = TmpVs_list[0].device
            own = metrics.self_intersections(v.detach().to(dev).float(), f.to(dev).long())
            print('%s: %d of %d faces take part in a self-intersection (%d crossing pairs)' % (
                n, own['faces'].shape[0], f.shape[0], own['n_pairs']))
    return meshes


if __name__ == '__main__':
    main()
