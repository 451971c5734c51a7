"""flatten_fl.py — garments laid flat: an addition, the reference has no such command (recmv.param has the definitions).

`--in` is one `.obj` file or a directory of them.  Every mesh is cut into a disk along shortest paths between its boundary loops
(recmv.param.cut_to_disk: a shirt has 4 loops and gets 3 seams, a skirt 2 and 1), mapped to the plane (`--method arap`: as rigid
as possible from the cotangent harmonic map, `--arap-iters N` local/global iterations; `--method harmonic` with `--weights
cotangent|uniform`) and scaled so that the pattern's area is the surface's (`--no-normalise` leaves the map's own scale).  Per
input `--out` gets `<name>.obj`, the cut mesh with `vt` lines and `f v/vt` faces, and `<name>_flat.obj`, the pattern as a planar
mesh (z = 0) with the same faces.  `--out`/flatten.json holds per file the distortion summary, the seams (lengths, vertex
counts), the solver's iterations and the route it took; a mesh that cannot be cut (closed, several pieces, genus > 0,
non-manifold) is recorded with its reason under `refused` and the run goes on.

    python rec-mv_amd/flatten_fl.py --gpu-ids 0 --in <obj|dir> --out <dir> [--method arap|harmonic]
        [--weights cotangent|uniform] [--arap-iters N] [--no-normalise]
"""
import argparse
import json
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))


def build_parser():
    parser = argparse.ArgumentParser(description='cut garment meshes into disks and flatten them')
    parser.add_argument('--gpu-ids', nargs='+', type=int, default=[0], metavar='IDs', help='gpu ids (the first is used)')
    parser.add_argument('--in', dest='inp', required=True, help='mesh (.obj) or a directory of them')
    parser.add_argument('--out', required=True, help='directory for the cut meshes, the patterns and flatten.json')
    parser.add_argument('--method', default='arap', choices=['arap', 'harmonic'], help='the map')
    parser.add_argument('--weights', default='cotangent', choices=['cotangent', 'uniform'], help='weights of --method harmonic')
    parser.add_argument('--arap-iters', default=20, type=int, help='local/global iterations of --method arap')
    parser.add_argument('--no-normalise', action='store_true', help='keep the map\'s own scale')
    return parser


def _inputs(path):
    if osp.isdir(path):
        return [(n, osp.join(path, n)) for n in sorted(os.listdir(path)) if n.lower().endswith('.obj')]
    if osp.isfile(path):
        return [(osp.basename(path), path)]
    raise ValueError("no such mesh or directory: %s" % path)


def write_obj_uv(name, verts, uv, faces):
    """`v %f %f %f` lines, `vt %f %f` lines (one per vertex), then `f a/a b/b c/c` with 1-based indices."""
    v = verts.detach().cpu().float().tolist()
    t = uv.detach().cpu().double().tolist()
    f = (faces.detach().cpu().long() + 1).tolist()
    with open(name, 'w') as fh:
        fh.write("".join("v %f %f %f\n" % tuple(r) for r in v))
        fh.write("".join("vt %f %f\n" % tuple(r) for r in t))
        fh.write("".join("f %d/%d %d/%d %d/%d\n" % (a, a, b, b, c, c) for a, b, c in f))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.arap_iters < 0:
        parser.error("--arap-iters must not be negative")
    try:
        files = _inputs(args.inp)
    except ValueError as e:
        parser.error(str(e))
    import torch
    from recmv import param
    from recmv.utils.utils import read_obj, write_obj
    device = torch.device('cuda:%d' % args.gpu_ids[0])
    os.makedirs(args.out, exist_ok=True)
    res = {'method': args.method, 'weights': args.weights, 'arap_iters': args.arap_iters, 'normalise': not args.no_normalise,
           'files': {}}
    for name, path in files:
        v, f = read_obj(path)
        try:
            r = param.flatten(v.to(device), f.to(device), method=args.method, normalise=not args.no_normalise,
                              weights=args.weights, iterations=args.arap_iters)
        except ValueError as e:
            res['files'][name] = {'refused': str(e)}
            print("%s: refused: %s" % (name, e))
            continue
        stem = osp.splitext(name)[0]
        write_obj_uv(osp.join(args.out, stem + '.obj'), r['verts'], r['uv'], r['faces'])
        flat = torch.cat([r['uv'], torch.zeros_like(r['uv'][:, :1])], 1)
        write_obj(osp.join(args.out, stem + '_flat.obj'), flat, r['faces'])
        res['files'][name] = {'vertices': int(v.shape[0]), 'cut_vertices': int(r['verts'].shape[0]), 'faces': int(f.shape[0]),
                              'distortion': r['distortion'],
                              'seams': [{'length': s['length'], 'vertices': len(s['vertices'])} for s in r['seams']],
                              'iterations': r['info']['cg_iterations'], 'route': r['info']['route']}
        d = r['distortion']
        print("%s: %d seams, %d flipped, conformal %.4f, area %.4f, isometric max %.4f, route %s" % (
            name, len(r['seams']), d['flipped'], d['conformal'] or 0., d['area'] or 0., d['isometric_max'] or 0., r['info']['route']))
    with open(osp.join(args.out, 'flatten.json'), 'w') as fh:
        json.dump(res, fh, indent=1)
    return res


if __name__ == '__main__':
    main()
