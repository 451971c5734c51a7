"""infer_fl_curve.py — the reference's feature-curve driver (infer_fl_curve.py:1-250) on the MI355X kernels.

Loads a trained run `<rec-root>` with its capture `<rec-root>/..` (as infer_fl.py does, with the feature-curve branch, so the
checkpoint must hold `inter_free_curve.*`), turns every trained feature curve (neck, cuffs, hems) into a thin tube mesh
(`Intersect_Free_Curve.curve_to_mesh`, csrc/curve_tubes.hip) and, for every frame (up to `--frames`), poses the tubes with
the deformer (`OptimGarmentNetwork.infer_garment_fl`, :2861-2935, recmv/inference.py).  Writes what the reference writes:

  tmp_body.ply                  canonical body mesh
  fl_meshs/{fid:06d}.obj        the posed tubes of all garments' feature curves, one mesh

`modified.ply`, when present in the run folder, stands for the first garment's mesh, as in the reference (the tubes do not
depend on the garment meshes).  `--nV --nI --C --nColor` only drive rendering in the other drivers: accepted and ignored.

Additions, all opt-in: `--fit-registry` first fits the curves to the boundary loops of the registered meshes
`<rec-root>/registry_<garment>.obj` (register_fl.py), so that the tubes sit on those meshes — the fit branch of
`curve_to_mesh` (garment_structure.py:179-212) on the fused step of csrc/curve_tubes.hip, `--fit-iters` AdamW steps (the
reference: 20000); it writes fl_meshs/fit.json.  `--curve-radius` / `--curve-joints` set the tube's radius and ring size.

Deviations: which loop stands for which feature line is decided by centroid (recmv.lap_align.assign_loops)
where the reference hard-codes `curve_idx` / `target_idx` for one garment, and registration stays register_fl.py's job.

    python rec-mv_amd/infer_fl_curve.py --gpu-ids 0 --rec-root <capture>/<save-folder> --data-type scene [--fit-registry]
"""
import argparse
import json
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))

FIT_SAMPLES = 2000            # points every boundary loop is resampled to (OptimGarmentNetwork.py:2874)


def build_parser():
    parser = argparse.ArgumentParser(description='neu video body infer')
    parser.add_argument('--gpu-ids', nargs='+', type=int, metavar='IDs', help='gpu ids')
    parser.add_argument('--batch-size', default=1, type=int, metavar='IDs', help='batch size')
    parser.add_argument('--rec-root', default=None, metavar='M', help='data root')
    parser.add_argument('--frames', default=-1, type=int, metavar='frames', help='render frame nums')
    parser.add_argument('--nV', action='store_true', help='not save video')
    parser.add_argument('--data-type', default='synthe', help='the type of inference dataset')
    parser.add_argument('--nI', action='store_true', help='not save image')
    parser.add_argument('--C', action='store_true', help='overlay on gtimg')
    parser.add_argument('--nColor', action='store_true', help='not render images')
    parser.add_argument('--a_pose', action='store_true', help='using a-pose images to extract garment_meshes')
    parser.add_argument('--conf', default=None, metavar='M', help='config file (default: <rec-root>/config.conf)')
    parser.add_argument('--fit-registry', action='store_true',
                        help='first fit the curves to the boundary loops of <rec-root>/registry_*.obj (register_fl.py)')
    parser.add_argument('--fit-iters', default=20000, type=int, help='AdamW steps of --fit-registry (default 20000)')
    parser.add_argument('--curve-radius', default=0.002, type=float, help='radius of the tubes (default 0.002)')
    parser.add_argument('--curve-joints', default=6, type=int, help='vertices per tube ring; must divide 360 (default 6)')
    return parser


def registry_loops(optNet, rec_root, log=print):
    """The boundary loops of the registered meshes, one per feature line: ([polyline [FIT_SAMPLES-ish, 3] float32], [index of
    its curve in optNet.fl_names]).  Every garment's loops are assigned to its feature lines by centroid; a line without a
    loop (or a garment without a registry file) is logged and skipped."""
    import numpy as np
    import torch
    from recmv import lap_align, registration, utils
    from recmv.curves import FL_EXTRACT
    from recmv.engineer.utils.polygons import uniformsample3d

    names = list(optNet.garment_names)
    paths = [registration.registry_path(rec_root, n) for n in names]
    if not any(osp.isfile(p) for p in paths):
        raise FileNotFoundError("--fit-registry: none of %s exists (run register_fl.py first)" % ", ".join(paths))
    pts = optNet.inter_free_curve.inference().detach().cpu()
    curves = {n: pts[i] for i, n in enumerate(optNet.fl_names)}
    extract = getattr(optNet, 'fl_extract', None) or {}
    polylines, target_idx = [], []
    for name, path in zip(names, paths):
        if not osp.isfile(path):
            log('%s: no %s, its feature lines are not fitted' % (name, path))
            continue
        verts, faces = utils.read_obj(path)
        loops = lap_align.boundary_loops(faces, verts.shape[0])
        fields = [f for f in (extract[name] if name in extract else FL_EXTRACT[name]) if f not in
                  [optNet.fl_names[t] for t in target_idx]]
        assigned = lap_align.assign_loops(loops, verts, curves, fields, log=log, garment=name)
        for field in fields:
            if field not in assigned:
                log('%s: no boundary loop for %s, not fitted' % (name, field))
                continue
            loop_pts = verts[torch.tensor(loops[assigned[field]], dtype=torch.int64)].numpy().astype(np.float64)
            polylines.append(np.asarray(uniformsample3d(loop_pts, FIT_SAMPLES), dtype=np.float32))
            target_idx.append(optNet.fl_names.index(field))
    return polylines, target_idx


def _same_length(polylines):
    """The fused step takes one point count for all pairs: a loop that resampled to a few points less (uniformsample3d
    rounds per edge) is padded by repeating its last point.  A duplicate changes no nearest neighbour, but it counts twice in
    the polyline-to-curve mean: a deviation from the chamfer on the unpadded loop of a few parts in M."""
    import numpy as np
    M = max(p.shape[0] for p in polylines)
    return [np.concatenate([p, np.repeat(p[-1:], M - p.shape[0], axis=0)], axis=0) for p in polylines]


def main(argv=None):
    args = build_parser().parse_args(argv)
    assert not (args.nV and args.nI)
    from infer_fl import RATIO, load_run
    from recmv import utils

    rec_root = osp.normpath(args.rec_root)
    optNet, dataset, dataloader, TmpVs_list, Tmpfs_list = load_run(args, curves=True)
    device = TmpVs_list[0].device
    batch_size = args.batch_size
    utils.write_ply(osp.join(rec_root, 'tmp_body.ply'), TmpVs_list[0], Tmpfs_list[0])
    modified = osp.join(rec_root, 'modified.ply')
    if osp.exists(modified):
        verts, faces = utils.read_ply(modified)
        TmpVs_list[1], Tmpfs_list[1] = verts.to(device), faces.to(device)
    garment_TmpVs, garment_Tmpfs = TmpVs_list[1:], Tmpfs_list[1:]
    out_dir = osp.join(rec_root, 'fl_meshs')
    os.makedirs(out_dir, exist_ok=True)

    fit = None
    if args.fit_registry:
        polylines, target_idx = registry_loops(optNet, rec_root)
        if not polylines:
            raise SystemExit("--fit-registry: no boundary loop of the registered meshes matches a feature line")
        fit = {}
        optNet.fl_curve_meshes = optNet.inter_free_curve.curve_to_mesh(
            curve_radius=args.curve_radius, num_joints=args.curve_joints, curve_verts=_same_length(polylines),
            curve_idx=list(range(len(polylines))), target_idx=target_idx, iters=args.fit_iters, log=fit)
        fit['curves'] = [optNet.fl_names[t] for t in fit['target_idx']]
        with open(osp.join(out_dir, 'fit.json'), 'w') as fh:
            json.dump(fit, fh, indent=1)
        for name, a, b in zip(fit['curves'], fit['first_loss'], fit['last_loss']):
            print('fit %s: loss %.6f -> %.6f in %d steps' % (name, a, b, fit['iters']))

    n_frames = 0
    for data_index, (frame_ids, outs) in enumerate(dataloader):
        if (data_index * batch_size > args.frames) if args.frames >= 0 else False:
            break
        frame_ids = frame_ids.long().to(device)
        curve_mesh = optNet.infer_garment_fl(garment_TmpVs, garment_Tmpfs, dataset.H, dataset.W, RATIO, frame_ids, args.nColor,
                                             None, rec_root, curve_radius=args.curve_radius, num_joints=args.curve_joints)
        fid = frame_ids[0].item()
        path = osp.join(out_dir, '{:06d}.obj'.format(fid))
        curve_mesh.export(path)
        print(path)
        n_frames += 1
    return {'frames': n_frames, 'fit': fit}


if __name__ == '__main__':
    main()
