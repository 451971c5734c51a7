"""infer_fl.py — the reference's inference driver (infer_fl.py:1-283) on the MI355X kernels.

Loads a trained run `<rec-root>` (its `config.conf` and `latest.pth`, written by train.py) with the capture `<rec-root>/..`,
extracts the canonical meshes at the `fine` pyramid, and for every frame (up to `--frames`) writes what the reference's
`OptimGarmentNetwork.infer` produces (engineer/networks/OptimGarmentNetwork.py:3216-3306, recmv/inference.py):

  tmp_body.ply                          canonical body mesh
  meshs/{garment}_{fid:06d}.obj / .png  posed MC garment mesh, its Phong render (ground-truth background with --C)
  def1meshs/{garment}_{fid:06d}.png     canonical-pose mesh rendered from behind
  colors/{garment}_{fid:06d}.png        colour render (not with --nColor)
  smpl_meshs/smpl_{fid:06d}.obj         body template posed by the skinner
  mask_error.json                       1 - IoU of each garment's silhouette with the frame's mask

With `--registry` the garments posed are the registered template meshes `<rec-root>/registry_<garment>.obj` that
register_fl.py writes (`infer_garment`, :2960-3120) instead of the MC meshes; the per-garment files keep their names, and
every frame also gets the merged render of all garments in flat colours, render/{fid:06d}.png.

Not provided: the template cut from the SMPL assets.  The feature-curve tubes of `infer_garment_fl` are
infer_fl_curve.py's.  `--nV` is accepted and ignored
(the reference writes no video either).  The capture is read in this process (no loader workers).

    python rec-mv_amd/infer_fl.py --gpu-ids 0 --rec-root <capture>/<save-folder> --data-type scene [--registry]
"""
import argparse
import json
import os
import os.path as osp
import sys
import time

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))


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
    parser.add_argument('--registry', action='store_true',
                        help='pose the registered meshes <rec-root>/registry_*.obj (register_fl.py) and write render/*.png')
    return parser


def _check_curves(path, optNet):
    """The checkpoint must hold the feature curves (`inter_free_curve.*`) in the shapes this run builds."""
    import torch
    state = torch.load(path, map_location='cpu')['model_state_dict']
    keys = sorted(k for k in state if k.startswith('inter_free_curve.'))
    if not keys:
        raise ValueError("%s holds no feature curves (no inter_free_curve.* keys): the run was trained without the curve "
                         "branch" % path)
    mine = optNet.inter_free_curve.state_dict()
    for k in keys:
        name = k[len('inter_free_curve.'):]
        if name in mine and tuple(mine[name].shape) != tuple(state[k].shape):
            raise ValueError("%s: %s has shape %s, this run builds %s ([curves, samples, ...]: the curve count or sample "
                             "count differs)" % (path, k, tuple(state[k].shape), tuple(mine[name].shape)))


def load_run(args, curves=False):
    """The trained run of `args` and its canonical meshes at the fine pyramid: (optNet, dataset, dataloader, TmpVs_list,
    Tmpfs_list), index 0 the body, then the garments.  `curves=True` builds the loop with its feature-curve branch, so that
    `optNet.inter_free_curve` is restored from the checkpoint (which must hold it)."""
    import torch
    from recmv import utils
    from recmv.dataset import getDatasetAndLoader
    from recmv.hocon import ConfigFactory
    from recmv.loop import RESOLUTIONS
    from recmv.model.network import getOptNet
    from recmv.utils.constant import TEMPLATE_GARMENT

    assert torch.cuda.is_available(), "infer_fl.py needs a GPU (librecmv_hip.so has no CPU fallback)"
    rec_root = osp.normpath(args.rec_root)
    config = ConfigFactory.parse_file(args.conf or osp.join(rec_root, 'config.conf'))
    device = torch.device('cuda', args.gpu_ids[0] if args.gpu_ids else 0)
    torch.cuda.set_device(device)
    batch_size = args.batch_size
    garment_type = config.get_string('train.garment_type')
    condlen = {'deformer': int(config.get_int('mlp_deformer.condlen') * (1 + len(TEMPLATE_GARMENT[garment_type]))),
               'renderer': config.get_int('render_net.condlen')}
    dataset, dataloader = getDatasetAndLoader(osp.normpath(osp.join(rec_root, osp.pardir)), condlen, batch_size, False, 0,
                                              config.get_bool('train.opt_pose'), config.get_bool('train.opt_trans'),
                                              config.get_config('train.opt_camera'), garment_type, data_type=args.data_type,
                                              a_pose=args.a_pose, **({'motion': args.motion} if getattr(args, 'motion', None) else {}))
    for t in dataset.conds + [dataset.poses, dataset.trans, dataset.shape] + list(dataset.camera_params.values()):
        t.data = t.data.to(device)
    resolutions = RESOLUTIONS['fine']                      # the script's own table, `fine` (infer_fl.py:42-63)
    optNet, _ = getOptNet(dataset, osp.basename(rec_root), batch_size, None, None, resolutions, device, config,
                          **({'curves': True} if curves else {}))
    optNet, dataloader = utils.set_hierarchical_config(config, 'fine', optNet, dataloader, resolutions)
    align = osp.join(rec_root, 'fl_init', 'init_trans_matrix.pth')
    if getattr(optNet, 'curves', False) and osp.isfile(align):
        optNet.align_fl(align)
    if curves:
        _check_curves(osp.join(rec_root, 'latest.pth'), optNet)
    print('load model: ' + osp.join(rec_root, 'latest.pth'))
    optNet, dataset, _ = utils.load_model(osp.join(rec_root, 'latest.pth'), optNet, dataset, device)
    optNet.dataset = dataset
    optNet.eval()
    with torch.no_grad():
        TmpVs_list, Tmpfs_list = optNet.discretizeSDF(RATIO, None, 0.)
    return optNet, dataset, dataloader, TmpVs_list, Tmpfs_list


RATIO = {'sdfRatio': 1., 'deformerRatio': 1., 'renderRatio': 1.}


def main(argv=None):
    args = build_parser().parse_args(argv)
    assert not (args.nV and args.nI)
    import torch
    from recmv import inference, registration, utils
    from recmv.dataset import write_image_bgr
    from recmv.utils.constant import render_colors

    rec_root = osp.normpath(args.rec_root)
    optNet, dataset, dataloader, TmpVs_list, Tmpfs_list = load_run(args)
    device = TmpVs_list[0].device
    batch_size = args.batch_size
    H, W = dataset.H, dataset.W
    ratio = RATIO
    utils.write_ply(osp.join(rec_root, 'tmp_body.ply'), TmpVs_list[0], Tmpfs_list[0])
    garment_TmpVs, garment_Tmpfs = TmpVs_list[1:], Tmpfs_list[1:]
    subs = ('colors', 'meshs', 'smpl_meshs', 'def1meshs')
    if args.registry:
        paths = [registration.registry_path(rec_root, name) for name in optNet.garment_names]
        missing = [p for p in paths if not osp.isfile(p)]
        if missing:
            raise FileNotFoundError("--registry: %s missing (run register_fl.py first)" % ", ".join(missing))
        meshes = registration.register_garments(optNet, None, None, None, rec_root)
        garment_TmpVs, garment_Tmpfs = [v for v, _ in meshes], [f for _, f in meshes]
        colors_rgb = render_colors(optNet.garment_type, len(optNet.garment_names))
        subs = subs + ('render',)
    garment_fs_host = [f.cpu() for f in garment_Tmpfs]
    for sub in subs:
        os.makedirs(osp.join(rec_root, sub), exist_ok=True)

    errors = {name: {} for name in optNet.garment_names}
    timings = {}
    gts = {}
    n_frames = 0
    for data_index, (frame_ids, outs) in enumerate(dataloader):
        if (data_index * batch_size > args.frames) if args.frames >= 0 else False:
            break
        print(data_index * batch_size)
        frame_ids = frame_ids.long().to(device)
        gts['mask'] = outs['mask'].to(device)
        if args.C:
            gts['image'] = (outs['img'].to(device) + 1.) / 2.
        r = optNet.infer_garments(garment_TmpVs, garment_Tmpfs, H, W, ratio, frame_ids, args.nColor, gts, timings=timings)
        t0 = time.perf_counter()
        fids = frame_ids.cpu().numpy().reshape(-1)
        for g_i, name in enumerate(optNet.garment_names):
            colors, imgs, def1imgs, defVs, maskE = (r[k][g_i] for k in ('colors', 'imgs', 'def1imgs', 'defMeshVs', 'maskE'))
            for j, (fid, img, def1img, defV) in enumerate(zip(fids, imgs, def1imgs, defVs)):
                utils.write_obj(osp.join(rec_root, 'meshs/{}_{:06d}.obj'.format(name, fid)), defV, garment_fs_host[g_i])
                if not args.nI:
                    write_image_bgr(osp.join(rec_root, 'meshs/{}_{:06d}.png'.format(name, fid)), img[:, :, [2, 1, 0]])
                    write_image_bgr(osp.join(rec_root, 'def1meshs/{}_{:06d}.png'.format(name, fid)), def1img[:, :, [2, 1, 0]])
                errors[name][int(fid)] = float(maskE[j])
            if colors is not None and not args.nI:
                for fid, color in zip(fids, colors):
                    write_image_bgr(osp.join(rec_root, 'colors/{}_{:06d}.png'.format(name, fid)), color)
        if args.registry:
            merged, _ = inference.merged_render(optNet, r['defMeshVs'], garment_Tmpfs, colors_rgb, H, W)
            for fid, img in zip(fids, merged):
                write_image_bgr(osp.join(rec_root, 'render/{:06d}.png'.format(fid)), img[:, :, [2, 1, 0]])
        body_vs, body_fs = inference.posed_body(optNet, frame_ids, ratio)
        body_vs, body_fs = body_vs.cpu(), body_fs.cpu()
        for fid, vs in zip(fids, body_vs):
            utils.write_obj(osp.join(rec_root, 'smpl_meshs/smpl_{:06d}.obj'.format(fid)), vs, body_fs)
        timings['files'] = timings.get('files', 0.0) + time.perf_counter() - t0
        n_frames += len(fids)
    with open(osp.join(rec_root, 'mask_error.json'), 'w') as fh:
        json.dump({'maskE': {name: {str(k): v for k, v in sorted(e.items())} for name, e in errors.items()}}, fh, indent=1)
    per_frame = {k: v / max(n_frames, 1) for k, v in sorted(timings.items())}
    print('frames %d; wall seconds per frame: %s' % (n_frames, ', '.join('%s %.4f' % kv for kv in per_frame.items())))
    return {'frames': n_frames, 'seconds_per_frame': per_frame, 'mask_error': errors}


if __name__ == '__main__':
    main()
