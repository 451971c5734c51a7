"""infer_fl_animation.py — the reference's animation driver (infer_fl_animation.py:1-283) on the MI355X kernels.

Loads a trained run `<rec-root>` with its capture `<rec-root>/..` (as infer_fl.py does) and drives its garments with the
poses of a motion file the capture never saw (`OptimGarmentNetwork.infer_garment_animation`, :2729-2859,
recmv/inference.py): the deformer codes, translation and colour code are the capture's means, the meshes are the registered
templates `<rec-root>/registry_<garment>.obj` when register_fl.py has written them, else the marching-cubes meshes.  Writes
what the reference writes:

  tmp_body.ply, tmp_<garment>.ply                            canonical meshes at the fine pyramid
  animation/<data-type>/meshs/<garment>_<fid:06d>.npy        posed garment vertices [V,3] float32
  animation/<data-type>/meshs/<garment>_<fid:06d>.png        Phong renders, posed body | posed garment (not with --nI)
  animation/<data-type>/colors/<garment>_<fid:06d>.png       colour render (not with --nColor / --nI)

and three additions:

  animation/<data-type>/smoothness.json   per garment the reference's temporal smoothness figure (tools/compute_CSI.py): the
                                          mean over the inner frames of the mean vertex norm of the second difference
  animation/<data-type>/collisions.json   with --fix-collisions: per garment and frame the vertices moved, the vertices left
                                          unresolved and the passes run by the body-collision repair (recmv/collide.py)

  animation/<data-type>/intersections.json  with --report-intersections: per frame and garment the garment faces that cross
                                          the posed body, those that cross the garment itself, and per pair of garments
                                          the faces that cross each other (recmv.collide.intersection_report), on the meshes
                                          written — after the repair when --fix-collisions is given too; with --penetration
                                          also the garment vertices inside the body (`inside_vertices`) and the largest
                                          distance of one of them to the body's surface (`max_depth`)

Deviations: the motion is an input (`--motion`; the reference reads ../snug/assets/CMU/131/131_11_poses.npz),
registration is register_fl.py's job (the reference registers on the first frame), and the collision repair is not in the
reference (off unless asked for).  `--nV` is accepted and ignored (the reference writes no video either).

    python rec-mv_amd/infer_fl_animation.py --gpu-ids 0 --rec-root <capture>/<save-folder> --data-type snug \\
        --motion <motion.npz> [--fix-collisions] [--report-intersections [--penetration]]
"""
import argparse
import json
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))


def build_parser():
    parser = argparse.ArgumentParser(description='neu video body infer')
    parser.add_argument('--gpu-ids', nargs='+', type=int, metavar='IDs', help='gpu ids')
    parser.add_argument('--batch-size', default=1, type=int, metavar='IDs', help='batch size')
    parser.add_argument('--rec-root', default=None, metavar='M', help='data root')
    parser.add_argument('--frames', default=-1, type=int, metavar='frames', help='render frame nums')
    parser.add_argument('--data-type', type=str, required=True)
    parser.add_argument('--nV', action='store_true', help='not save video')
    parser.add_argument('--nI', action='store_true', help='not save image')
    parser.add_argument('--C', action='store_true', help='overlay on gtimg')
    parser.add_argument('--nColor', action='store_true', help='not render images')
    parser.add_argument('--conf', default=None, metavar='M', help='config file (default: <rec-root>/config.conf)')
    parser.add_argument('--motion', default=None, metavar='NPZ',
                        help='AMASS / CMU style motion file (poses, trans, mocap_framerate); required with --data-type snug')
    parser.add_argument('--fix-collisions', action='store_true',
                        help='push garment vertices that sank into the posed body back out (not in the reference)')
    parser.add_argument('--collision-eps', default=None, type=float,
                        help='margin kept between garment and body, in the capture\'s length unit (default 2e-3)')
    parser.add_argument('--collision-iters', default=None, type=int, help='passes of the collision repair (default 3)')
    parser.add_argument('--report-intersections', action='store_true',
                        help='write intersections.json: garment faces crossing the body, themselves and each other')
    parser.add_argument('--penetration', action='store_true',
                        help='with --report-intersections: also the garment vertices inside the body and their largest depth')
    parser.set_defaults(a_pose=False)
    return parser


def temporal_smoothness(frames):
    """tools/compute_CSI.py of the reference: over the inner frames i of a sequence of meshes [T,V,3] with one topology, the
    mean over vertices of |(v_i - v_{i-1}) - (v_{i+1} - v_i)|, averaged over those frames (None for fewer than 3 frames or an empty mesh)."""
    import numpy as np
    v = np.asarray(frames, np.float64)
    if v.shape[0] < 3 or v.shape[1] == 0:               # (a garment whose extraction found no surface has no vertices)
        return None
    second = (v[1:-1] - v[:-2]) - (v[2:] - v[1:-1])
    return float(np.sqrt((second ** 2).sum(-1)).mean(-1).mean())


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    assert not (args.nV and args.nI)
    if args.data_type != 'snug':
        parser.error("--data-type %s: only the snug loader yields the poses an animation is driven with" % args.data_type)
    if args.penetration and not args.report_intersections:
        parser.error("--penetration needs --report-intersections")
    if not args.motion:
        parser.error("--data-type snug needs --motion <npz>")
    import numpy as np
    from infer_fl import RATIO, load_run
    from recmv import utils
    from recmv.dataset import write_image_bgr

    rec_root = osp.normpath(args.rec_root)
    optNet, dataset, dataloader, TmpVs_list, Tmpfs_list = load_run(args)
    device = TmpVs_list[0].device
    batch_size = args.batch_size
    H, W = dataset.H, dataset.W
    utils.write_ply(osp.join(rec_root, 'tmp_body.ply'), TmpVs_list[0], Tmpfs_list[0])
    garment_TmpVs, garment_Tmpfs = TmpVs_list[1:], Tmpfs_list[1:]
    names = list(optNet.garment_names)
    for TmpVs, Tmpfs, name in zip(garment_TmpVs, garment_Tmpfs, names):
        utils.write_ply(osp.join(rec_root, 'tmp_{}.ply'.format(name)), TmpVs, Tmpfs)
    save_path = osp.join(rec_root, 'animation/{}'.format(args.data_type))
    os.makedirs(osp.join(save_path, 'colors'), exist_ok=True)
    os.makedirs(osp.join(save_path, 'meshs'), exist_ok=True)

    sequences = {name: {} for name in names}
    collisions = {name: {} for name in names}
    intersections = {}
    n_frames = 0
    for data_index, (frame_ids, outs) in enumerate(dataloader):
        if (data_index * batch_size > args.frames) if args.frames >= 0 else False:
            break
        frame_ids = frame_ids.long().to(device)
        stats = {}
        extra = {'intersection_stats': []} if args.report_intersections else {}
        if args.penetration:
            extra['intersection_penetration'] = True
        colors_list, imgs_list, defVs_list = optNet.infer_garment_animation(
            garment_TmpVs, garment_Tmpfs, outs['poses_y'], H, W, RATIO, frame_ids, rec_root, notcolor=args.nColor,
            fix_collisions=args.fix_collisions, collision_eps=args.collision_eps, collision_iters=args.collision_iters,
            collision_stats=stats, **extra)
        fids = frame_ids.cpu().numpy().reshape(-1)
        for fid, frame in zip(fids, extra.get('intersection_stats', [])):
            intersections[str(int(fid))] = frame
        for colors, imgs, defVs, name in zip(colors_list, imgs_list, defVs_list, names):
            for j, (fid, img, defV) in enumerate(zip(fids, imgs, defVs)):
                np.save(osp.join(save_path, 'meshs/{}_{:06d}.npy'.format(name, fid)), defV.reshape(-1, 3))
                sequences[name][int(fid)] = defV.reshape(-1, 3)
                if not args.nI:
                    write_image_bgr(osp.join(save_path, 'meshs/{}_{:06d}.png'.format(name, fid)), img[:, :, [2, 1, 0]])
                if name in stats:
                    collisions[name][str(int(fid))] = {'moved': int(stats[name]['moved'][j]),
                                                       'unresolved': int(stats[name]['unresolved'][j]),
                                                       'passes': int(stats[name]['passes'])}
            if colors is not None and not args.nI:
                for fid, color in zip(fids, colors):
                    write_image_bgr(osp.join(save_path, 'colors/{}_{:06d}.png'.format(name, fid)), color)
        n_frames += len(fids)
    smooth = {name: temporal_smoothness([seq[k] for k in sorted(seq)]) for name, seq in sequences.items()}
    for name in names:
        print('temporal smoothness of %s over %d frames: %s' % (name, len(sequences[name]), smooth[name]))
    with open(osp.join(save_path, 'smoothness.json'), 'w') as fh:
        json.dump({'frames': n_frames, 'smoothness': smooth}, fh, indent=1)
    if args.fix_collisions:
        with open(osp.join(save_path, 'collisions.json'), 'w') as fh:
            json.dump(collisions, fh, indent=1)
        for name in names:
            c = collisions[name].values()
            print('collision repair of %s: %d vertices moved, %d unresolved over %d frames' % (
                name, sum(v['moved'] for v in c), sum(v['unresolved'] for v in c), len(c)))
    if args.report_intersections:
        with open(osp.join(save_path, 'intersections.json'), 'w') as fh:
            json.dump(intersections, fh, indent=1)
        for name in names:
            c = [f[name] for f in intersections.values()]
            print('crossing faces of %s over %d frames: %d against the body, %d against itself' % (
                name, len(c), sum(v['body_faces'] for v in c), sum(v['self_faces'] for v in c)))
    print('done')
    res = {'frames': n_frames, 'smoothness': smooth, 'collisions': collisions if args.fix_collisions else None}
    if args.report_intersections:
        res['intersections'] = intersections
    return res


if __name__ == '__main__':
    main()
