"""A small trained run folder for infer_fl.py: a synthetic capture directory (tests/capture_fixture.py, the loop's pinhole),
two optimiser iterations of the loop on it, and `<capture>/result/{latest.pth, config.conf}` as train.py leaves them.

    python tools/make_infer_run.py OUT_DIR [--size 512] [--curves]
    python rec-mv_amd/infer_fl.py --gpu-ids 0 --rec-root OUT_DIR/capture/result --data-type scene --frames 2
"""
import argparse
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(REPO / "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--size", type=int, default=512, help="image height = width of the capture")
    ap.add_argument("--iters", type=int, default=2, help="optimiser iterations before the checkpoint (0: the initial surfaces)")
    ap.add_argument("--curves", action="store_true",
                    help="train with the feature-curve branch on, so that latest.pth holds inter_free_curve.*")
    args = ap.parse_args(argv)
    import torch
    import capture_fixture as cf
    from recmv import utils
    from recmv.dataset import getDatasetAndLoader
    from recmv.hocon import ConfigFactory, HOCONConverter
    from recmv.model.network import getOptNet
    dev = torch.device("cuda:0")
    root = cf.write_capture(os.path.join(args.out, "capture"), H=args.size, W=args.size, loop_camera=True)
    conf = ConfigFactory.parse_file(str(REPO / "configs" / "synthetic" / "people_snapshot_like.conf"))
    conf.put('train.sample_pix_num', 256)
    conds_lens = {'deformer': conf.get_int('mlp_deformer.condlen') * 3, 'renderer': conf.get_int('render_net.condlen')}
    torch.manual_seed(3)
    ds, _ = getDatasetAndLoader(root, conds_lens, 3, True, 0, True, True, conf.get_config('train.opt_camera'), cf.GARMENT_TYPE,
                                data_type='scene')
    for t in ds.conds + [ds.poses, ds.trans, ds.shape] + list(ds.camera_params.values()):
        t.data = t.data.to(dev)
    res = [(9, 13, 7), (17, 25, 13), (33, 49, 25), (65, 97, 49)]
    optNet, _ = getOptNet(ds, 'result', 3, None, None, res, dev, conf, skin_grid=(17, 33, 17),
                          **({'curves': True} if args.curves else {}))
    optNet, _ = utils.set_hierarchical_config(conf, 'coarse', optNet, None, res)
    optimizer = optNet.rebuild_optimizer()
    for frames in ([0, 2, 3], [5, 6, 8], [1, 4, 7], [9, 10, 11])[:args.iters]:
        datas = torch.utils.data.default_collate([ds[i][1] for i in frames])
        frame_ids = torch.tensor(frames, device=dev)
        ratio = {'sdfRatio': 1., 'deformerRatio': optNet.opt_times / 2500. + 0.5, 'renderRatio': 1.}
        optimizer.zero_grad()
        loss = optNet(datas, 256, ratio, frame_ids, args.out, global_optimizer=optimizer)
        loss.backward()
        optNet.propagateTmpPsGrad(frame_ids, ratio)
        optimizer.step()
        optNet.opt_times += 1.
    run = os.path.join(root, 'result')
    os.makedirs(run, exist_ok=True)
    utils.save_model(os.path.join(run, 'latest.pth'), 0, optNet, ds)
    with open(os.path.join(run, 'config.conf'), 'w') as fh:
        fh.write(HOCONConverter.convert(conf, 'hocon'))
    print(run)


if __name__ == "__main__":
    main()
