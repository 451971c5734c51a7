"""flatten_fl.py — garments laid flat: an addition, the reference has no such command (recmv.param has the definitions).

`--in` is one `.obj` file or a directory of them.  Every mesh is cut into a disk along shortest paths between its boundary loops
(recmv.param.cut_to_disk: a shirt has 4 loops and gets 3 seams, a skirt 2 and 1), mapped to the plane (`--method arap`: as rigid
as possible from the cotangent harmonic map, `--arap-iters N` local/global iterations; `--method harmonic` with `--weights
cotangent|uniform`) and scaled so that the pattern's area is the surface's (`--no-normalise` leaves the map's own scale).  Per
input `--out` gets `<name>.obj`, the cut mesh with `vt` lines and `f v/vt` faces, and `<name>_flat.obj`, the pattern as a planar
mesh (z = 0) with the same faces.  `--out`/flatten.json holds per file the distortion summary, the seams (lengths, vertex
counts), the solver's iterations and the route it took; a mesh that cannot be cut (closed, several pieces, genus > 0,
non-manifold) is recorded with its reason under `refused` and the run goes on.

`--bake SIZE` also bakes textures on a SIZE x SIZE image (recmv.bake): the chart is fitted into the unit square, `<name>.obj`
carries those unit `vt` with `mtllib` / `usemtl` lines, `<name>.mtl` names the maps, `<name>_normal.png` (object space, 0.5 +
0.5 n), `<name>_tangent_normal.png` and `<name>_color.png` (when the mesh or its source has vertex colours, `v x y z r g b`) are
8-bit, round(255 clamp(x)), and `<name>_position.npy` is float32 [SIZE,SIZE,3]; flatten.json gains `bake` per file.
`--bake-source <obj|dir>` takes normals and colours from a detailed mesh (a directory is paired by file name),
`--bake-projection closest|normal` chooses how texels find it, `--bake-maps` which maps are written, `--bake-gutter N` the rings
of edge padding, `--bake-lanes 8|64` the rasteriser's launch shape.  Without `--bake` the command writes what it always wrote.

    python rec-mv_amd/flatten_fl.py --gpu-ids 0 --in <obj|dir> --out <dir> [--method arap|harmonic]
        [--weights cotangent|uniform] [--arap-iters N] [--no-normalise]
        [--bake SIZE [--bake-source <obj|dir>] [--bake-maps position,normal,tangent_normal,color] [--bake-gutter N]
         [--bake-projection closest|normal] [--bake-lanes 8|64]]
"""
import argparse
import json
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))

BAKE_MAPS = ('position', 'normal', 'tangent_normal', 'color')


def build_parser():
    parser = argparse.ArgumentParser(description='cut garment meshes into disks and flatten them')
    parser.add_argument('--gpu-ids', nargs='+', type=int, default=[0], metavar='IDs', help='gpu ids (the first is used)')
    parser.add_argument('--in', dest='inp', required=True, help='mesh (.obj) or a directory of them')
    parser.add_argument('--out', required=True, help='directory for the cut meshes, the patterns and flatten.json')
    parser.add_argument('--method', default='arap', choices=['arap', 'harmonic'], help='the map')
    parser.add_argument('--weights', default='cotangent', choices=['cotangent', 'uniform'], help='weights of --method harmonic')
    parser.add_argument('--arap-iters', default=20, type=int, help='local/global iterations of --method arap')
    parser.add_argument('--no-normalise', action='store_true', help='keep the map\'s own scale')
    parser.add_argument('--bake', default=None, type=int, metavar='SIZE', help='bake textures on a SIZE x SIZE image')
    parser.add_argument('--bake-source', default=None, metavar='OBJ|DIR', help='detailed mesh(es) the normals and colours come from')
    parser.add_argument('--bake-maps', default=','.join(BAKE_MAPS), help='comma-separated: ' + ', '.join(BAKE_MAPS))
    parser.add_argument('--bake-gutter', default=4, type=int, metavar='N', help='rings of edge padding')
    parser.add_argument('--bake-projection', default='closest', choices=['closest', 'normal'], help='how texels find the source')
    parser.add_argument('--bake-lanes', default=None, type=int, choices=[8, 64], help='lanes per face of the UV rasteriser')
    return parser


def _bake_source(path, name):
    """The source mesh of input `name`: the file itself, or the file of that name in the directory (None when there is none)."""
    if path is None:
        return None
    full = osp.join(path, name) if osp.isdir(path) else path
    return full if osp.isfile(full) else None


def _bake_one(args, maps, name, path, r, out_dir, device):
    """Bake the flattened mesh `r` of input `name` and write its files; the `bake` entry of flatten.json."""
    import numpy as np
    import torch
    from recmv import bake
    from recmv.dataset.dataset import write_image_bgr
    from recmv.utils.utils import read_obj_uv, write_obj_uv_mtl
    colors = read_obj_uv(path)['colors']
    colors = None if colors is None else colors.to(device)[r['origin']].contiguous()
    source, source_path = None, _bake_source(args.bake_source, name)
    if source_path is not None:
        s = read_obj_uv(source_path)
        source = (s['verts'].to(device), s['faces'].to(device), None if s['colors'] is None else s['colors'].to(device))
    b = bake.bake(r['verts'], r['faces'], r['uv'], args.bake, maps=maps, source=source, projection=args.bake_projection,
                  gutter=args.bake_gutter, colors=colors, lanes=args.bake_lanes)
    stem = osp.splitext(name)[0]
    files = {}
    filled = (b['src'] >= 0)[:, :, None]
    for kind in maps:
        if kind not in b:
            continue
        if kind == 'position':
            files[kind] = stem + '_position.npy'
            np.save(osp.join(out_dir, files[kind]), b[kind].cpu().numpy())
            continue
        image = torch.where(filled, 0.5 + 0.5 * b[kind], torch.zeros_like(b[kind])) if kind == 'normal' else b[kind]
        files[kind] = '%s_%s.png' % (stem, kind)
        write_image_bgr(osp.join(out_dir, files[kind]), bake.quantise(image)[:, :, ::-1])
    write_obj_uv_mtl(osp.join(out_dir, stem + '.obj'), r['verts'], b['uv'], r['faces'], files, colors=colors)
    return {'size': [args.bake, args.bake], 'lanes': b['lanes'], 'gutter': args.bake_gutter, 'projection': args.bake_projection,
            'source': source_path, 'files': files, 'report': b['report']}


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
    maps = tuple(m for m in args.bake_maps.split(',') if m)
    if args.bake is not None:
        if args.bake < 1 or args.bake >= 32768:
            parser.error("--bake SIZE must be 1 .. 32767")
        if args.bake_gutter < 0 or 2 * args.bake_gutter >= args.bake:
            parser.error("--bake-gutter must not be negative and must leave room in the image")
        if not maps or any(m not in BAKE_MAPS for m in maps):
            parser.error("--bake-maps must name some of " + ", ".join(BAKE_MAPS))
        if args.bake_source is not None and not osp.exists(args.bake_source):
            parser.error("no such source mesh or directory: %s" % args.bake_source)
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
        baked = _bake_one(args, maps, name, path, r, args.out, device) if args.bake is not None else None
        if baked is None:
            write_obj_uv(osp.join(args.out, stem + '.obj'), r['verts'], r['uv'], r['faces'])
        flat = torch.cat([r['uv'], torch.zeros_like(r['uv'][:, :1])], 1)
        write_obj(osp.join(args.out, stem + '_flat.obj'), flat, r['faces'])
        res['files'][name] = {'vertices': int(v.shape[0]), 'cut_vertices': int(r['verts'].shape[0]), 'faces': int(f.shape[0]),
                              'distortion': r['distortion'],
                              'seams': [{'length': s['length'], 'vertices': len(s['vertices'])} for s in r['seams']],
                              'iterations': r['info']['cg_iterations'], 'route': r['info']['route']}
        if baked is not None:
            res['files'][name]['bake'] = baked
        d = r['distortion']
        print("%s: %d seams, %d flipped, conformal %.4f, area %.4f, isometric max %.4f, route %s" % (
            name, len(r['seams']), d['flipped'], d['conformal'] or 0., d['area'] or 0., d['isometric_max'] or 0., r['info']['route']))
    with open(osp.join(args.out, 'flatten.json'), 'w') as fh:
        json.dump(res, fh, indent=1)
    return res


if __name__ == '__main__':
    main()
