"""Animation on novel poses on the GPU: recmv_point_mesh_nearest and recmv_collision_push / collide.resolve against the float64
restatement of tests/collide_reference.py, infer_garment_animation on a loop trained for two iterations on a capture
directory, and infer_fl_animation.py end to end on a run folder with a 4-frame synthetic motion.

Bounds (eps32 = 2^-23, u = eps32 / 2 the unit round-off; inputs are exact float32 values, the judge works in float64):
  squared distance  The kernel forms ap = p - a, ab, ac (one rounding each, relative u), six dot products, the closest point's
                    parameters and the residual r = ap - s ab - t ac, |r|^2 = d^2.  An error of the parameters moves the
                    closest point inside the face or along an edge, at right angles to r, so it enters d^2 in second order
                    only; the first-order error is that of evaluating r (three terms of magnitude <= R, the largest distance
                    from p to a corner of the face: <= 4 u R per component, <= 7 u R in norm) times 2 d, plus 3 u d^2 for the
                    squares and their sum: <= 14 u R d + 3 u d^2 <= 17 u R^2 = 8.5 eps32 R^2 because d <= R.  The face the
                    kernel picks has a corner within d + Lmax of p (Lmax the longest edge), so R <= d + Lmax.
                    BOUND_D2 = 16 eps32 (d + Lmax)^2: the estimate with a factor of two in hand.
  signed distance   p_out = p + (eps - s) n: s carries the residual's error (<= 7 u R) and the normal's (interpolation and
                    normalisation, <= 4 u |s|), the step's product and sum round once more each, and every coordinate of p_out
                    is rounded to float32 (<= u P per coordinate, P the largest coordinate magnitude: <= 1.8 u P in norm).
                    With R, |s| <= Lmax + max_depth + eps =: Rs that is <= u (1.8 P + 13 Rs) < eps32 (P + 7 Rs).
                    BOUND_S = 2 eps32 (P + 7 Rs), again a factor of two in hand.
"""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
REPO = HERE.parent
CONF = str(REPO / "configs" / "synthetic" / "people_snapshot_like.conf")
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import collide_reference as CR  # noqa: E402

DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)
RATIO = {'sdfRatio': 1., 'deformerRatio': 1., 'renderRatio': 1.}


def _longest_edge(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces)
    return max(float(np.linalg.norm(v[f[:, i]] - v[f[:, (i + 1) % 3]], axis=1).max()) for i in range(3))


def _bound_d2(d2, lmax):
    return 16. * EPS32 * (np.sqrt(d2) + lmax) ** 2


def _irregular_body(level=4, radius=0.5, seed=3):
    """A closed mesh with unequal triangles and varying curvature: an icosphere whose vertices are shifted along the surface
    by up to a tenth of an edge and whose radius varies smoothly by +-6 % (float32 [V,3], int64 [F,3])."""
    from test_nricp_cpu import icosphere
    v, f = icosphere(level)
    g = torch.Generator().manual_seed(seed)
    edge = float((v[f[:, 0]] - v[f[:, 1]]).norm(dim=1).mean())
    v = v + 0.1 * edge * (torch.rand(v.shape, generator=g) * 2 - 1)
    v = v / v.norm(dim=1, keepdim=True)
    bump = 1 + 0.06 * torch.sin(3 * v[:, 0] + 1) * torch.cos(2 * v[:, 1]) + 0.03 * torch.sin(5 * v[:, 2])
    return (radius * bump[:, None] * v).float().contiguous(), f.contiguous()


def _shell(verts, faces, n, offsets, seed, min_height=0.):
    """`n` points beside the mesh: a random point well inside a random face (every barycentric weight >= 0.15), moved along
    that face's normal by the signed `offsets` [n] — points whose nearest triangle is unambiguous, like those of a garment
    that lies on a body much more finely tessellated than the distance between the two.  `min_height`: only faces whose
    smallest height is at least that (a marching-cubes mesh has slivers narrower than any offset).  float32 [n,3], the
    faces [n]."""
    rng = np.random.RandomState(seed)
    v, f = np.asarray(verts, np.float64), np.asarray(faces)
    e = [np.linalg.norm(v[f[:, (i + 1) % 3]] - v[f[:, i]], axis=1) for i in range(3)]
    area2 = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    wide = np.nonzero(area2 / np.maximum(np.maximum(e[0], e[1]), e[2]) >= min_height)[0]
    pick = wide[rng.randint(0, wide.shape[0], n)]
    w = rng.dirichlet(np.ones(3), n) * 0.55 + 0.15
    a, b, c = v[f[pick, 0]], v[f[pick, 1]], v[f[pick, 2]]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c + np.asarray(offsets)[:, None] * nrm
    return torch.from_numpy(p.astype(np.float32)), pick


def _check_nearest(p, verts, faces, face_gpu, d_gpu, cap=0.01):
    """One frame against the restatement; returns the share of points whose face is left out by the ambiguity rule."""
    lmax = _longest_edge(verts, faces)
    face, d1, d2, _ = CR.nearest(p.numpy(), verts.numpy(), faces.numpy())
    bound = _bound_d2(d1, lmax)
    err = np.abs(d_gpu.double().numpy() - d1)
    assert (err <= bound).all(), (float(err.max()), float(bound[err.argmax()]))
    clear = (d2 - d1) > bound
    assert np.array_equal(face_gpu.numpy()[clear], face[clear])
    # whichever face the kernel names is one of the nearest ones: its float64 distance is within the bound of the minimum
    v = verts.double().numpy()
    tri = faces.numpy()[face_gpu.numpy()]
    d_named, _ = CR.closest_on_triangle(p.double().numpy(), v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]])
    assert (d_named <= d1 + bound).all()
    left_out = 1. - clear.mean()
    print("nearest: %d points, %d faces, largest |d2 error| / bound %.3g, faces left out %.4f" % (
        p.shape[0], faces.shape[0], float((err / bound).max()), left_out))
    if cap is not None:
        assert left_out <= cap, left_out                 # a condition on the inputs (the restatement alone decides it)
    return left_out


def test_point_mesh_nearest_on_an_irregular_closed_mesh():
    from recmv import collide
    bv, bf = _irregular_body()
    B, N = 3, 2731                                        # N is not a multiple of 512 points, F = 5120 + 7 not of 512 faces
    frames = torch.stack([bv, bv * 1.07 + 0.02, bv[:, [1, 2, 0]] * 0.93 - 0.01]).contiguous()   # (an even permutation of the axes)
    # seven more faces, copies of existing ones: exact ties that must go to the lower index
    bf = torch.cat([bf, bf[[5, 77, 901, 2000, 3333, 4444, 5119]]]).contiguous()
    rng = np.random.RandomState(1)
    pts = []
    for b in range(B):
        off = rng.uniform(0.002, 0.012, N) * rng.choice([-1., 1.], N)
        p, _ = _shell(frames[b], bf[:5120], N, off, seed=10 + b)
        far = torch.from_numpy(rng.randn(20, 3).astype(np.float32))          # a few points anywhere (edge / corner regions)
        p[:20] = far * 0.5
        pts.append(p)
    pts = torch.stack(pts)
    face, d = collide.point_mesh_nearest(pts.to(DEV), frames.to(DEV), bf.to(DEV))
    assert face.shape == (B, N) and face.dtype == torch.int64 and d.shape == (B, N) and d.dtype == torch.float32
    face, d = face.cpu(), d.cpu()
    assert int(face.max()) < 5120                         # a duplicated face never wins over its original
    for b in range(B):
        _check_nearest(pts[b], frames[b], bf, face[b], d[b])
    # bitwise reproducible; frames are independent (one frame alone gives the same bits); empty inputs
    face2, d2 = collide.point_mesh_nearest(pts.to(DEV), frames.to(DEV), bf.to(DEV))
    assert torch.equal(face2.cpu(), face) and torch.equal(d2.cpu(), d)
    f1, d1 = collide.point_mesh_nearest(pts[1:2].to(DEV), frames[1:2].to(DEV), bf.to(DEV))
    assert torch.equal(f1.cpu(), face[1:2]) and torch.equal(d1.cpu(), d[1:2])
    f0, d0 = collide.point_mesh_nearest(torch.zeros(2, 0, 3, device=DEV), frames[:2].to(DEV), bf.to(DEV))
    assert f0.shape == (2, 0) and d0.shape == (2, 0)
    # the single-mesh kernel of the remesher computes the same distances bit for bit (one shared point-triangle routine)
    from recmv.iso_remesh import closest_point
    fc, _, dc = closest_point(pts[0].to(DEV), frames[0].to(DEV), bf.to(DEV))
    assert torch.equal(fc.cpu(), face[0]) and torch.equal(dc.cpu(), d[0])
    # a face with an index outside the mesh is skipped
    bad = bf.clone()
    bad[int(face[0, 100])] = torch.tensor([0, 1, bv.shape[0]])
    fb, _ = collide.point_mesh_nearest(pts[:1].to(DEV), frames[:1].to(DEV), bad.to(DEV))
    assert int(fb[0, 100]) != int(face[0, 100]) and int(fb[0, 100]) >= 0


def test_collision_push_and_resolve_against_the_restatement():
    from recmv import collide, shading
    bv, bf = _irregular_body()
    eps, md = 2e-3, 3e-2
    B, N = 2, 1500
    frames = torch.stack([bv, bv * 1.05 - 0.01])
    lmax = max(_longest_edge(frames[b], bf) for b in range(B))
    P = float(frames.abs().max()) + md
    bound_s = 2. * EPS32 * (P + 7. * (lmax + md + eps))
    rng = np.random.RandomState(5)
    garments, kinds = [], []
    for b in range(B):
        # 0: clear of the body (4-12 mm above it); 1: planted 0.5-25 mm inside; 2: nearer than eps but outside;
        # 3: planted 40-45 mm inside, deeper than max_depth
        kind = rng.choice([0, 1, 2, 3], N, p=[0.55, 0.3, 0.1, 0.05])
        off = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                        [rng.uniform(0.004, 0.012, N), -rng.uniform(0.0005, 0.025, N), rng.uniform(0.0002, 0.0015, N),
                         -rng.uniform(0.040, 0.045, N)])
        p, _ = _shell(frames[b], bf, N, off, seed=20 + b)
        garments.append(p)
        kinds.append(kind)
    g = torch.stack(garments)
    faces_before = bf.clone()
    out, stats = collide.resolve(g.to(DEV), frames.to(DEV), bf.to(DEV), eps=eps, max_depth=md, iters=3)
    out2, stats2 = collide.resolve(g.to(DEV), frames.to(DEV), bf.to(DEV), eps=eps, max_depth=md, iters=3)
    assert torch.equal(out, out2) and stats == stats2                    # two runs: the same bits
    assert torch.equal(bf, faces_before) and out.shape == g.shape and out.dtype == torch.float32
    out = out.cpu()
    assert stats['passes'] <= 3 and len(stats['moved_per_pass']) == stats['passes']
    for b in range(B):
        v, f = frames[b].numpy(), bf.numpy()
        s_before, _, _ = CR.signed_distance(g[b].numpy(), v, f)
        margin = 100 * bound_s
        # the fixture's classes are what the restatement sees, clear of every threshold
        assert (s_before[kinds[b] == 0] >= eps + margin).all() and (s_before[kinds[b] == 3] < -md - margin).all()
        assert ((s_before[(kinds[b] == 1) | (kinds[b] == 2)] < eps - margin)
                & (s_before[(kinds[b] == 1) | (kinds[b] == 2)] > -md + margin)).all()
        # the restatement itself converges within the three passes
        ref_out, ref_moved, ref_unres, _ = CR.resolve(g[b].numpy(), v, f, eps, md, iters=3)
        s_ref = CR.signed_distance(ref_out, v, f)[0]
        assert (s_ref[~ref_unres] >= eps - bound_s).all()
        # the kernel's result, judged by the restatement
        s_after = CR.signed_distance(out[b].numpy(), v, f)[0]
        deep = kinds[b] == 3
        assert (s_after[~deep] >= eps - bound_s).all(), float(s_after[~deep].min())
        keep = s_before >= eps
        assert torch.equal(out[b][torch.from_numpy(keep)], g[b][torch.from_numpy(keep)])       # bit for bit
        assert torch.equal(out[b][torch.from_numpy(deep)], g[b][torch.from_numpy(deep)])       # too deep: unmoved ...
        assert stats['unresolved'][b] == int(deep.sum()) == int(ref_unres.sum())               # ... and counted
        assert stats['moved'][b] == int(ref_moved.sum()) == int(((kinds[b] == 1) | (kinds[b] == 2)).sum())
        assert stats['moved_per_pass'][0][b] == stats['moved'][b]
        moved_mask = (out[b] != g[b]).any(-1).numpy()
        assert np.array_equal(moved_mask, ref_moved)
        assert np.abs(out[b].numpy()[ref_moved] - ref_out[ref_moved]).max() <= 4 * bound_s
    # one push by hand: counts and the copy-through of a single call; N = 0 and an input left untouched
    normals = shading.verts_normals(frames.to(DEV), bf.to(DEV))
    face, _ = collide.point_mesh_nearest(g.to(DEV), frames.to(DEV), bf.to(DEV))
    gd = g.to(DEV)
    once, moved, unres = collide.collision_push(gd, frames.to(DEV), normals, bf.to(DEV), face, eps, md)
    assert torch.equal(gd.cpu(), g) and moved.dtype == torch.int32
    assert moved.cpu().tolist() == stats['moved_per_pass'][0] and unres.cpu().tolist() == stats['unresolved']
    empty, m0, u0 = collide.collision_push(torch.zeros(2, 0, 3, device=DEV), frames.to(DEV), normals, bf.to(DEV),
                                           torch.zeros(2, 0, dtype=torch.int64, device=DEV), eps, md)
    assert empty.shape == (2, 0, 3) and m0.tolist() == [0, 0] and u0.tolist() == [0, 0]


def _trained_capture_loop(tmp_path):
    """tests/test_gpu_infer.py's helper: a capture directory read by recmv.dataset, two optimiser iterations."""
    import capture_fixture as cf
    from recmv import utils
    from recmv.dataset import getDatasetAndLoader
    from recmv.hocon import ConfigFactory
    from recmv.model.network import getOptNet
    root = cf.write_capture(str(tmp_path / "capture"), H=160, W=128, loop_camera=True)
    conf = ConfigFactory.parse_file(CONF)
    conf.put('train.sample_pix_num', 256)
    conds_lens = {'deformer': conf.get_int('mlp_deformer.condlen') * 3, 'renderer': conf.get_int('render_net.condlen')}
    torch.manual_seed(3)
    ds, _ = getDatasetAndLoader(root, conds_lens, 3, True, 0, True, True, conf.get_config('train.opt_camera'),
                                cf.GARMENT_TYPE, data_type='scene')
    for t in ds.conds + [ds.poses, ds.trans, ds.shape] + list(ds.camera_params.values()):
        t.data = t.data.to(DEV)
    res = [(9, 13, 7), (17, 25, 13), (33, 49, 25), (65, 97, 49)]
    optNet, _ = getOptNet(ds, 'result', 3, None, None, res, torch.device(DEV), conf, skin_grid=(17, 33, 17))
    optNet, _ = utils.set_hierarchical_config(conf, 'coarse', optNet, None, res)
    optimizer = optNet.rebuild_optimizer()
    for frames in ([0, 2, 3], [5, 6, 8]):
        datas = torch.utils.data.default_collate([ds[i][1] for i in frames])
        frame_ids = torch.tensor(frames, device=DEV)
        ratio = {'sdfRatio': 1., 'deformerRatio': optNet.opt_times / 2500. + 0.5, 'renderRatio': 1.}
        optimizer.zero_grad()
        loss = optNet(datas, 256, ratio, frame_ids, str(tmp_path), global_optimizer=optimizer)
        loss.backward()
        optNet.propagateTmpPsGrad(frame_ids, ratio)
        optimizer.step()
        optNet.opt_times += 1.
    torch.cuda.synchronize()
    return optNet, ds, conf, root


def _motion_poses(n, seed=2):
    g = torch.Generator().manual_seed(seed)
    return (0.15 * torch.randn(1, 72, generator=g) + 0.05 * torch.randn(n, 72, generator=g).cumsum(0)).float()


def test_infer_garment_animation_and_the_cli(tmp_path):
    import capture_fixture as cf
    from recmv import collide, inference, shading, utils
    from recmv.dataset import read_image_bgr
    from recmv.hocon import HOCONConverter
    optNet, ds, conf, root = _trained_capture_loop(tmp_path)
    TmpVs_list, Tmpfs_list = optNet.discretizeSDF(RATIO, None, 0.)
    gv, gf = TmpVs_list[1:], Tmpfs_list[1:]
    N, H, W = 3, ds.H, ds.W
    poses_y = _motion_poses(N)
    frame_ids = torch.arange(N, device=DEV)
    colors, imgs, defVs = optNet.infer_garment_animation(gv, gf, poses_y, H, W, RATIO, frame_ids)
    names = optNet.garment_names
    assert len(colors) == len(imgs) == len(defVs) == len(names) == 2
    # by hand: the conditions averaged over ALL capture frames, the body posed by the skinner and shaded
    all_ids = torch.arange(cf.FRAMES, device=DEV)
    d_all, _, trans_all, _ = optNet.get_grad_parameters(all_ids, DEV)
    poses = poses_y.to(DEV).view(N, 24, 3)
    trans = trans_all.detach().mean(0, keepdim=True).expand(N, -1).contiguous()
    cams = optNet._cameras()
    with torch.no_grad():
        optNet._ensure_body_template()
        body = optNet.deformer.defs[1](optNet.tmpBodyVs.view(1, -1, 3).expand(N, -1, 3), [poses, trans]).contiguous()
        bm = shading.Meshes(body, optNet.tmpBodyFs, shading.TexturesVertex(torch.ones_like(optNet.tmpBodyVs)[None]))
        left = inference._to_uint8(inference._render(bm, cams, H, W, shading.PointLights())[0][..., :3])
    assert (left != 255).any()
    for g_i, name in enumerate(names):
        assert imgs[g_i].shape == (N, H, 2 * W, 3) and colors[g_i].shape == (N, H, W, 3)
        assert imgs[g_i].dtype == colors[g_i].dtype == np.uint8
        assert defVs[g_i].shape == (N, gv[g_i].shape[0], 3) and defVs[g_i].dtype == np.float32
        assert np.array_equal(imgs[g_i][:, :, :W], left)
        assert (imgs[g_i][:, :, W:] != 255).any() and (colors[g_i] != 255).any()
        d_mean = d_all[g_i + 1].detach().mean(0, keepdim=True).expand(N, -1).contiguous()
        d_one = d_all[g_i + 1].detach()[4:5].expand(N, -1).contiguous()
        with torch.no_grad():
            direct = optNet.deformer(gv[g_i][None].expand(N, -1, 3), [d_mean, [poses, trans]], ratio=RATIO, offset_type=name)
            one = optNet.deformer(gv[g_i][None].expand(N, -1, 3), [d_one, [poses, trans_all.detach()[4:5].expand(N, -1)]],
                                  ratio=RATIO, offset_type=name)
        assert np.array_equal(defVs[g_i], direct.cpu().numpy())
        assert not np.array_equal(defVs[g_i], one.cpu().numpy())          # one frame's conditions give another mesh
    # [N,24,3] poses are accepted; --nColor's path returns no colours; the repair only moves what it reports
    c2, i2, v2 = optNet.infer_garment_animation(gv, gf, poses_y.view(N, 24, 3), H, W, RATIO, frame_ids, notcolor=True)
    assert c2 == [None, None] and all(np.array_equal(a, b) for a, b in zip(i2, imgs))
    assert all(np.array_equal(a, b) for a, b in zip(v2, defVs))
    stats = {}
    _, _, v3 = optNet.infer_garment_animation(gv, gf, poses_y, H, W, RATIO, frame_ids, notcolor=True, fix_collisions=True,
                                              collision_stats=stats)
    for g_i, name in enumerate(names):
        changed = (v3[g_i] != defVs[g_i]).any(-1).sum(1)
        assert changed.tolist() == stats[name]['moved'] and 1 <= stats[name]['passes'] <= collide.COLLISION_ITERS
        # the garments of this loop on its posed body, without the 1 % condition: distances and named faces
        face, d = collide.point_mesh_nearest(torch.from_numpy(defVs[g_i][:1]).to(DEV), body[:1], optNet.tmpBodyFs)
        _check_nearest(torch.from_numpy(defVs[g_i][0]), body[0].cpu(), optNet.tmpBodyFs.cpu(), face[0].cpu(), d[0].cpu(),
                       cap=None)
    # the posed body of the capture with a garment of a few thousand vertices lying 0.3-1.5 mm off those of its faces that are
    # at least 8 mm wide (the body is a marching-cubes mesh: over its slivers every point is ambiguous)
    shell, _ = _shell(body[0].cpu(), optNet.tmpBodyFs.cpu(), 3000, np.random.RandomState(4).uniform(0.0003, 0.0015, 3000), seed=6,
                      min_height=0.008)
    face, d = collide.point_mesh_nearest(shell[None].to(DEV), body[:1], optNet.tmpBodyFs)
    _check_nearest(shell, body[0].cpu(), optNet.tmpBodyFs.cpu(), face[0].cpu(), d[0].cpu())

    # ---- the CLI on a run folder beside the capture, driven by a 4-frame motion file
    run = os.path.join(root, 'result')
    os.makedirs(run, exist_ok=True)
    utils.save_model(os.path.join(run, 'latest.pth'), 0, optNet, ds)
    with open(os.path.join(run, 'config.conf'), 'w') as fh:
        fh.write(HOCONConverter.convert(conf, 'hocon'))
    motion = os.path.join(str(tmp_path), 'motion.npz')
    raw = np.zeros((4, 156))
    raw[:, :72] = _motion_poses(4, seed=9).numpy()
    np.savez(motion, poses=raw, trans=np.zeros((4, 3)), mocap_framerate=np.float64(30.))
    import importlib.util
    spec = importlib.util.spec_from_file_location("infer_fl_animation", REPO / "rec-mv_amd" / "infer_fl_animation.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ['--gpu-ids', '0', '--rec-root', run, '--data-type', 'snug', '--motion', motion]
    res = cli.main(base)
    anim = os.path.join(run, 'animation', 'snug')
    fids = [0, 1, 2, 3]
    expect = {'smoothness.json'}
    for fid in fids:
        for name in names:
            expect |= {'meshs/%s_%06d.npy' % (name, fid), 'meshs/%s_%06d.png' % (name, fid), 'colors/%s_%06d.png' % (name, fid)}
    written = {os.path.relpath(os.path.join(d, f), anim) for d, _, fs in os.walk(anim) for f in fs}
    assert written == expect, sorted(written ^ expect)
    assert all(os.path.isfile(os.path.join(run, f)) for f in ['tmp_body.ply'] + ['tmp_%s.ply' % n for n in names])
    assert res['frames'] == 4 and res['collisions'] is None
    plain = {}
    for name in names:
        tv, _ = utils.read_ply(os.path.join(run, 'tmp_%s.ply' % name))
        for fid in fids:
            m = np.load(os.path.join(anim, 'meshs/%s_%06d.npy' % (name, fid)))
            assert m.shape == (tv.shape[0], 3) and m.dtype == np.float32
            plain[name, fid] = m
            assert read_image_bgr(os.path.join(anim, 'meshs/%s_%06d.png' % (name, fid))).shape == (H, 2 * W, 3)
            assert read_image_bgr(os.path.join(anim, 'colors/%s_%06d.png' % (name, fid))).shape == (H, W, 3)
        assert res['smoothness'][name] == pytest.approx(cli.temporal_smoothness([plain[name, k] for k in fids]))
    with open(os.path.join(anim, 'smoothness.json')) as fh:
        assert json.load(fh)['smoothness'] == res['smoothness']
    res2 = cli.main(base + ['--fix-collisions', '--nColor'])
    with open(os.path.join(anim, 'collisions.json')) as fh:
        col = json.load(fh)
    assert set(col) == set(names) and res2['collisions'] == col
    for name in names:
        assert set(col[name]) == {'0', '1', '2', '3'}
        for fid in fids:
            m = np.load(os.path.join(anim, 'meshs/%s_%06d.npy' % (name, fid)))
            entry = col[name][str(fid)]
            assert set(entry) == {'moved', 'unresolved', 'passes'}
            assert int((m != plain[name, fid]).any(-1).sum()) == entry['moved']
