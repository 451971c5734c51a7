"""Texture baking on the GPU: the UV rasteriser (owner, barycentrics, count) and the gutter against the numpy restatement
(tests/bake_reference.py) bit for bit on every case of tests/bake_cases.py, with 8 and with 64 lanes per face; interpolation,
transfer, vertex tangents and the normal-map encoding bit for bit on a spherical cap; the transfer from a finer source mesh fed
with MeshGrid.closest_point's own outputs; the 'normal' projection's choice per texel; a mesh baked onto itself within a
derived float32 margin; recmv.bake.bake end to end; and rec-mv_amd/flatten_fl.py --bake.
"""
import functools
import json
import os.path as osp
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE.parent / "rec-mv_amd")]
import bake_cases as BC  # noqa: E402
import bake_reference as BR  # noqa: E402
import param_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = (48, 64)                                            # 64 x 48: H = 48 rows, W = 64 columns


def gpu(*arrays):
    return tuple(torch.from_numpy(np.array(a)).to(DEV) for a in arrays)


def same(t, a):
    return np.array_equal(t.detach().cpu().numpy(), a, equal_nan=True)


@functools.lru_cache(maxsize=None)
def raster_ref(name):
    """The restatement's images of a case: (uv, faces, size, face, bary, count, src after 4 passes); computed once, never written to."""
    make, size, _ = BC.RASTER[name]
    uv, f = make()
    face, bary, count = BR.rasterize(uv, f, size)
    out = (uv, f, size, face, bary, count, BR.gutter(face, 4))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cap_chart():
    """cap(9) as the baked mesh with the planar uv of its grid fitted into 64 x 48, its GPU vertex normals, and the restated
    images: a dict of numpy arrays, never written to."""
    from recmv import shading
    v, f = PC.cap(9)
    uv = BR.fit_uv(v[:, :2].astype(np.float64), SIZE, 2.)
    tv, tf = gpu(v, f)
    vn = shading.verts_normals(tv, tf).cpu().numpy()
    face, bary, count = BR.rasterize(uv, f, SIZE)
    c = dict(v=v, f=f, uv=uv, vn=vn, face=face, bary=bary, count=count, tan=BR.vertex_tangents(v, f, uv, vn))
    for a in c.values():
        a.setflags(write=False)
    return c


def cap_images():
    c = cap_chart()
    return c, gpu(c["v"], c["f"], c["uv"], c["vn"], c["face"], c["bary"])


# ------------------------------------------------------------------------------------------------------- the rasteriser
@pytest.mark.parametrize("name", sorted(BC.RASTER))
def test_rasteriser_and_gutter_have_the_restatements_bits_with_8_and_64_lanes(name):
    from recmv import bake
    uv, f, size, face, bary, count, src = raster_ref(name)
    tuv, tf = gpu(uv, f)
    got = {}
    for lanes in bake.LANES:
        g_face, g_bary, g_count = bake.rasterize_uv(tuv, tf, size, lanes=lanes)
        assert g_face.dtype == torch.int32 and g_bary.dtype == torch.float32 and g_count.dtype == torch.int32
        assert same(g_face, face) and same(g_count, count) and same(g_bary, bary), (name, lanes)
        got[lanes] = (g_face, g_bary, g_count)
    for a, b in zip(got[8], got[64]):
        assert torch.equal(a, b) or same(a, b.cpu().numpy())                       # the launch shape changes no bit
    auto = bake.rasterize_uv(tuv, tf, size)
    assert same(auto[0], face) and same(auto[2], count)
    assert same(bake.gutter(got[8][0], 4), src)
    print(name, size, "covered", int((face >= 0).sum()), "shared", int((count > 1).sum()), "padded", int((src >= 0).sum()))


def test_gutter_passes_and_padding():
    from recmv import bake
    face = BC.island()
    tface, = gpu(face)
    image = np.random.RandomState(0).rand(face.shape[0], face.shape[1], 3).astype(np.float32)
    timage, = gpu(image)
    for n in (0, 1, 2, 3, 4, 9):                           # both parities of the ping-pong
        src = bake.gutter(tface, n)
        want = BR.gutter(face, n)
        assert src.dtype == torch.int32 and same(src, want), n
        assert same(bake.pad(timage, src), BR.pad(image, want))
        assert same(bake.pad(timage[:, :, 0].contiguous(), src), BR.pad(image[:, :, 0], want))
    full, = gpu(np.zeros((5, 7), np.int32))
    for n in (0, 1, 3):
        assert same(bake.gutter(full, n), np.arange(35, dtype=np.int32).reshape(5, 7))
    for name in ("planar97x61", "outside", "one_texel", "empty"):
        face = raster_ref(name)[3]
        for n in (0, 1, 3):
            assert same(bake.gutter(gpu(face)[0], n), BR.gutter(face, n)), (name, n)


# -------------------------------------------------------------------------------------------------------- interpolation
@pytest.mark.parametrize("channels", [1, 3, 16])
def test_interpolation_has_the_restatements_bits(channels):
    from recmv import bake
    c, (tv, tf, tuv, tvn, tface, tbary) = cap_images()
    attr = np.random.RandomState(channels).randn(c["v"].shape[0], channels).astype(np.float32)
    attr[7] = 0.                                            # a zero vector stays zero under normalise
    tattr, = gpu(attr)
    for normalise in ([False, True] if channels >= 3 else [False]):
        got = bake.interpolate(tface, tbary, tf, tattr, normalise=normalise)
        assert got.shape == SIZE + (channels,) and same(got, BR.interpolate(c["face"], c["bary"], c["f"], attr, normalise))
        assert (got[tface < 0] == 0).all()
    on_zero = np.zeros((1, 1), np.int32), np.array([[[1., 0., 0.]]], np.float32), np.array([[7, 7 + 9, 7 + 10]])
    if channels >= 3:                                       # a texel at the zero vertex itself: 0 / 0 is not taken
        out = bake.interpolate(*gpu(on_zero[0], on_zero[1], on_zero[2].astype(np.int64), attr), normalise=True)
        assert (out[0, 0, :3] == 0).all()


def test_tangents_and_the_encoding_have_the_restatements_bits():
    from recmv import bake
    c, (tv, tf, tuv, tvn, tface, tbary) = cap_images()
    tan = bake.vertex_tangents(tv, tf, tuv, tvn)
    assert tan.shape == (81, 4) and same(tan, c["tan"]) and (tan[:, 3] == 1).all()
    mirrored = c["uv"].copy()
    mirrored[:, 0] = 1. - mirrored[:, 0]
    flipped = bake.vertex_tangents(tv, tf, gpu(mirrored)[0], tvn)
    assert same(flipped, BR.vertex_tangents(c["v"], c["f"], mirrored, c["vn"])) and (flipped[:, 3] == -1).all()
    frame_n = bake.interpolate(tface, tbary, tf, tvn, normalise=True)
    frame_t = bake.interpolate(tface, tbary, tf, tan, normalise=True)
    want_n = BR.interpolate(c["face"], c["bary"], c["f"], c["vn"], True)
    want_t = BR.interpolate(c["face"], c["bary"], c["f"], c["tan"], True)
    assert same(frame_n, want_n) and same(frame_t, want_t)
    other = np.random.RandomState(3).randn(*SIZE, 3).astype(np.float32)             # any normal, not only the frame's own
    other /= np.linalg.norm(other, axis=2, keepdims=True)
    for normal in (want_n, other.astype(np.float32)):
        got = bake.encode_normal(tface, gpu(normal)[0], frame_n, frame_t)
        assert same(got, BR.encode_normal(c["face"], normal, want_n, want_t))
    own = bake.encode_normal(tface, frame_n, frame_n, frame_t).cpu().numpy()[c["face"] >= 0]
    assert np.abs(own - [0.5, 0.5, 1.]).max() < 1e-6       # a surface's own normals are the flat normal map


# ------------------------------------------------------------------------------------------------------------- transfer
@functools.lru_cache(maxsize=None)
def source():
    """cap(33) with a per-vertex attribute (3 smooth channels and a rough one) and vertex colours."""
    v, f = PC.cap(33)
    rng = np.random.RandomState(11)
    attr = np.concatenate([np.sin(3. * v), rng.rand(v.shape[0], 1)], 1).astype(np.float32)
    colors = (0.5 + 0.5 * np.cos(5. * v)).astype(np.float32)
    for a in (v, f, attr, colors):
        a.setflags(write=False)
    return v, f, attr, colors


def test_transfer_from_a_finer_source_has_the_restatements_bits():
    from recmv import bake, metrics
    c, (tv, tf, tuv, tvn, tface, tbary) = cap_images()
    sv, sf, attr, _ = source()
    tsv, tsf, tattr = gpu(sv, sf, attr)
    index, pos, nrm = bake.texels(tface, tbary, tf, tv, tvn)
    want_index = np.nonzero(c["face"].reshape(-1) >= 0)[0]
    assert same(index, want_index) and same(pos, BR.interpolate(c["face"], c["bary"], c["f"], c["v"]).reshape(-1, 3)[want_index])
    assert same(nrm, BR.interpolate(c["face"], c["bary"], c["f"], c["vn"], True).reshape(-1, 3)[want_index])
    hit_face, hit_point, _ = metrics.MeshGrid(tsv, tsf).closest_point(pos)           # the query's own outputs feed both sides
    for normalise in (False, True):
        out, bary = bake.transfer(hit_face, hit_point, tsv, tsf, tattr, normalise=normalise, return_bary=True)
        want_bary, want = BR.transfer(hit_face.cpu().numpy(), hit_point.cpu().numpy(), sv, sf, attr, normalise)
        assert same(bary, want_bary) and same(out, want)
    assert float(bary.min()) > -1e-4 and float((bary.sum(1) - 1).abs().max()) < 1e-6   # the closest points lie in their faces
    flawed = hit_face.clone()
    flawed[::7] = -1
    flawed[3::7] = sf.shape[0] + 1                          # beyond the face table below
    sf2 = sf.copy()
    sf2[int(hit_face[1])] = sf2[int(hit_face[1])][[0, 0, 1]]                         # a repeated corner: no valid face
    n = sv.shape[0]                                         # a face over three points of one line: no area, (1, 0, 0)
    sv2 = np.concatenate([sv, np.array([[0, 0, 2], [1, 0, 2], [2, 0, 2]], np.float32)], 0)
    attr2 = np.concatenate([attr, np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], np.float32)], 0)
    sf2 = np.concatenate([sf2, np.array([[n, n + 1, n + 2]], np.int64)], 0)
    flawed[5::7] = sf2.shape[0] - 1
    out, bary = bake.transfer(flawed, hit_point, *gpu(sv2, sf2, attr2), return_bary=True)
    want_bary, want = BR.transfer(flawed.cpu().numpy(), hit_point.cpu().numpy(), sv2, sf2, attr2)
    assert same(bary, want_bary) and same(out, want) and (out[::7] == 0).all() and (bary[3::7] == 0).all()
    assert (bary[5::7].cpu().numpy() == [1., 0., 0.]).all() and (out[5::7].cpu().numpy() == [1., 2., 3., 4.]).all()
    image = bake.scatter(out, tface, SIZE)
    assert image.shape == SIZE + (4,) and same(image.reshape(-1, 4)[index], want) and (image[tface < 0] == 0).all()


def test_bake_end_to_end_with_a_source():
    from recmv import bake
    c, (tv, tf, tuv, tvn, tface, tbary) = cap_images()
    sv, sf, _, colors = source()
    tsv, tsf, tcolors = gpu(sv, sf, colors)
    flat = torch.from_numpy(c["v"][:, :2].astype(np.float64)).to(DEV)               # pattern-scale uv: bake fits them itself
    res = bake.bake(tv, tf, flat, SIZE, source=(tsv, tsf, tcolors), gutter=2)
    assert set(res) == {"face", "bary", "count", "src", "uv", "lanes", "report", "position", "normal", "tangent_normal", "color"}
    assert same(res["uv"], c["uv"]) and same(res["face"], c["face"]) and same(res["bary"], c["bary"]) and same(res["count"], c["count"])
    src = BR.gutter(c["face"], 2)
    assert same(res["src"], src) and res["lanes"] in bake.LANES
    assert same(res["position"], BR.pad(BR.interpolate(c["face"], c["bary"], c["f"], c["v"]), src))
    index, pos, nrm = bake.texels(tface, tbary, tf, tv, tvn)
    hit_face, hit_point, how = bake.project(pos, nrm, tsv, tsf)
    assert (how == bake.HOW["closest"]).all()
    want = np.zeros(SIZE + (3,), np.float32)
    want.reshape(-1, 3)[index.cpu().numpy()] = BR.transfer(hit_face.cpu().numpy(), hit_point.cpu().numpy(), sv, sf, colors)[1]
    assert same(res["color"], BR.pad(want, src))
    filled = src >= 0
    normal = res["normal"].cpu().numpy()
    assert np.abs(np.linalg.norm(normal[filled], axis=1) - 1).max() < 1e-6 and (normal[~filled] == 0).all()
    # both meshes sample one sphere: the source's normals at the closest points are the positions' directions, within the meshes' chords
    # (away from the source's border, where a vertex normal averages faces of one side only)
    position = res["position"].cpu().numpy()
    inner = filled & (np.abs(position[:, :, :2]).max(-1) < 0.6)
    radial = position[inner] / np.linalg.norm(position[inner], axis=1, keepdims=True)
    assert inner.sum() > 1000 and np.abs(normal[inner] - radial).max() < 0.05
    tn = res["tangent_normal"].cpu().numpy()
    assert np.abs(tn[inner] - [0.5, 0.5, 1.]).max() < 0.05 and tn[filled].min() >= 0 and (tn[~filled] == 0).all()
    r = res["report"]
    assert r["size"] == list(SIZE) and r["covered_texels"] == int((c["face"] >= 0).sum()) and r["fallback_texels"] == 0
    assert abs(r["image_share"] - r["covered_texels"] / (SIZE[0] * SIZE[1])) < 1e-12
    assert r["shared_texels"] == int((c["count"] > 1).sum()) and r["overlap_texels"] == 0
    assert r["flipped_faces"] == 0 and r["zero_area_faces"] == 0
    d = r["texels_per_area"]
    assert 0 < d["min"] <= d["median"] <= d["max"]
    json.dumps(r)
    own = bake.bake(tv, tf, tuv, SIZE, maps=("normal", "color"), colors=tcolors[:81].contiguous(), gutter=0, fit=False, lanes=64)
    assert "position" not in own and "tangent_normal" not in own and own["report"]["fallback_texels"] is None
    assert same(own["normal"], BR.interpolate(c["face"], c["bary"], c["f"], c["vn"], True))
    assert same(own["color"], BR.interpolate(c["face"], c["bary"], c["f"], colors[:81]))
    twice = torch.cat([tf, tf], 0)                          # the atlas laid on itself: every interior texel is an overlap
    over = bake.bake(tv, twice, tuv, SIZE, maps=("position",), gutter=0, fit=False)["report"]
    assert over["overlap_texels"] == int(((c["count"] > 0) & (c["bary"].min(-1) > 0)).sum()) > 0


# ------------------------------------------------------------------------------------------------- the 'normal' projection
def test_normal_projection_hits_forward_backward_and_falls_back():
    """The source is a smaller cap tilted through the baked one: texels on one side find it along +n, on the other along -n, and
    those of the overhanging border find nothing and fall back to the closest point."""
    from recmv import bake, metrics
    c, (tv, tf, tuv, tvn, tface, tbary) = cap_images()
    sv, sf = PC.cap(33)
    sv = sv.astype(np.float64)
    sv[:, :2] *= 0.8
    sv[:, 2] = np.sqrt(1. - (sv[:, :2] ** 2).sum(1)) + 0.03 * sv[:, 0] / 0.56
    tsv, tsf = gpu(sv.astype(np.float32), sf)
    index, pos, nrm = bake.texels(tface, tbary, tf, tv, tvn)
    grid = metrics.MeshGrid(tsv, tsf)
    d = bake.default_distance(tsv)
    assert abs(d - 0.05 * np.linalg.norm(np.ptp(sv, 0))) < 1e-6
    hit_face, hit_point, how = bake.project(pos, nrm, tsv, tsf, projection="normal", grid=grid)
    fwd = grid.segment_hits(pos, pos + d * nrm)
    bwd = grid.segment_hits(pos, pos - d * nrm)
    near = grid.closest_point(pos)
    ff, ft, bf, bt = (x.cpu().numpy() for x in (fwd["face"], fwd["t"], bwd["face"], bwd["t"]))
    want = BR.project_how(ff >= 0, ft, bf >= 0, bt)
    counts = np.bincount(want, minlength=4)
    print("closest, forward, backward, fallback:", counts.tolist(), "of", want.shape[0], "d", d)
    assert counts[0] == 0 and counts[1] > 50 and counts[2] > 50 and counts[3] > 50
    assert same(how, want)
    want_face = np.where(want == 1, ff, np.where(want == 2, bf, near[0].cpu().numpy()))
    want_point = np.where((want == 1)[:, None], fwd["point"].cpu().numpy(),
                          np.where((want == 2)[:, None], bwd["point"].cpu().numpy(), near[1].cpu().numpy()))
    assert same(hit_face, want_face) and same(hit_point, want_point) and (hit_face >= 0).all()
    again = bake.project(pos, nrm, tsv, tsf, projection="normal", max_distance=d)    # the default distance, given
    assert torch.equal(again[0], hit_face) and torch.equal(again[2], how)
    short = bake.project(pos, nrm, tsv, tsf, projection="normal", max_distance=1e-4)[2]
    assert int((short == bake.HOW["fallback"]).sum()) > counts[3]
    res = bake.bake(tv, tf, tuv, SIZE, maps=("normal",), source=(tsv, tsf), projection="normal", fit=False)
    assert res["report"]["fallback_texels"] == int(counts[3])


# ------------------------------------------------------------------------------------------------------------ self bake
def test_a_mesh_baked_onto_itself_returns_its_own_attribute():
    """The margin, derived, with u = 2^-24 and g = 3 u / (1 - 3 u) the bound of a three-term float32 sum of products (three
    roundings on the longest path):
      * the interpolated position p is within g P sqrt(3) of the exact point p* of the texel (P = max |coordinate|; every
        coordinate is such a sum with weights that add up to 1);
      * p* lies on the surface, so the closest point q is no farther from p than p* is: |q - p*| <= 2 g P sqrt(3); the query
        forms q as a three-term combination in float32 itself and rounds it: another g P sqrt(3), D = 3 sqrt(3) g P in all;
      * the attribute is linear on every face with gradient at most G (computed per channel from the mesh in float64), and
        continuous across edges; a path on the surface between two points D apart, D a 10^-6 th of an edge, is shorter than
        2 D on a mesh whose dihedral angles are below 120 degrees: |a(q) - a(p*)| <= 2 G D;
      * the transfer rounds the float64 barycentrics to float32 and mixes in float32: 2 g M (M = max |attribute|), and the
        float32 barycentrics of the image, which the reference takes as they are, add nothing.
    margin = 2 G D + 2 g M per channel."""
    from recmv import bake
    c, (tv, tf, tuv, tvn, tface, tbary) = cap_images()
    v, f = c["v"].astype(np.float64), c["f"]
    attr = np.stack([np.sin(2. * v[:, 0]) + v[:, 1], v[:, 2] * v[:, 0], np.cos(3. * v[:, 1])], 1).astype(np.float32)
    index, pos, nrm = bake.texels(tface, tbary, tf, tv, tvn)
    hit_face, hit_point, how = bake.project(pos, nrm, tv, tf)
    got = bake.transfer(hit_face, hit_point, tv, tf, gpu(attr)[0]).cpu().numpy().astype(np.float64)
    covered = c["face"].reshape(-1) >= 0
    rows = f[c["face"].reshape(-1)[covered]]
    b = c["bary"].reshape(-1, 3)[covered].astype(np.float64)
    a64 = attr.astype(np.float64)
    want = b[:, 0:1] * a64[rows[:, 0]] + b[:, 1:2] * a64[rows[:, 1]] + b[:, 2:3] * a64[rows[:, 2]]
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    det = g11 * g22 - g12 * g12
    d1, d2 = a64[f[:, 1]] - a64[f[:, 0]], a64[f[:, 2]] - a64[f[:, 0]]
    grad2 = (g22[:, None] * d1 * d1 - 2. * g12[:, None] * d1 * d2 + g11[:, None] * d2 * d2) / det[:, None]
    G = np.sqrt(grad2.max(0))
    u = 2. ** -24
    g = 3. * u / (1. - 3. * u)
    D = 3. * np.sqrt(3.) * g * np.abs(v).max()
    margin = 2. * G * D + 2. * g * np.abs(a64).max(0)
    err = np.abs(got - want).max(0)
    print("error per channel", err, "margin", margin, "gradient bound", G)
    assert (err <= margin).all()
    assert (how == bake.HOW["closest"]).all() and got.shape == want.shape


# --------------------------------------------------------------------------------------------------------- the command
def parents_outputs(args_in, out, method, weights):
    """What flatten_fl.py wrote before it knew --bake, restated from the same pieces: the files a run without --bake must equal."""
    import os
    import flatten_fl
    from recmv import param
    from recmv.utils.utils import read_obj, write_obj
    os.makedirs(out, exist_ok=True)
    res = {'method': method, 'weights': weights, 'arap_iters': 20, 'normalise': True, 'files': {}}
    for name, path in flatten_fl._inputs(args_in):
        v, f = read_obj(path)
        r = param.flatten(v.to(DEV), f.to(DEV), method=method, normalise=True, weights=weights, iterations=20)
        stem = osp.splitext(name)[0]
        flatten_fl.write_obj_uv(osp.join(out, stem + '.obj'), r['verts'], r['uv'], r['faces'])
        write_obj(osp.join(out, stem + '_flat.obj'), torch.cat([r['uv'], torch.zeros_like(r['uv'][:, :1])], 1), r['faces'])
        res['files'][name] = {'vertices': int(v.shape[0]), 'cut_vertices': int(r['verts'].shape[0]), 'faces': int(f.shape[0]),
                              'distortion': r['distortion'],
                              'seams': [{'length': s['length'], 'vertices': len(s['vertices'])} for s in r['seams']],
                              'iterations': r['info']['cg_iterations'], 'route': r['info']['route']}
    with open(osp.join(out, 'flatten.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


def test_flatten_fl_bake(tmp_path):
    import flatten_fl
    from PIL import Image
    from recmv.utils.utils import read_obj_uv, write_obj, write_obj_uv_mtl
    src, fine, out, plain, parent = (tmp_path / n for n in ("in", "fine", "out", "plain", "parent"))
    src.mkdir()
    fine.mkdir()
    v, f = PC.cap(9)
    colors = (0.5 + 0.5 * np.cos(4. * v)).astype(np.float32)
    write_obj_uv_mtl(str(src / "cap.obj"), torch.from_numpy(v), torch.zeros(81, 2, dtype=torch.float64), torch.from_numpy(f), {},
                     colors=torch.from_numpy(colors))      # the input has vertex colours of its own and no source
    (src / "cap.mtl").unlink()
    write_obj(str(src / "tube.obj"), *map(torch.from_numpy, PC.cylinder()))
    sv, sf = PC.cylinder(48, 17, 0.125)
    write_obj(str(fine / "tube.obj"), torch.from_numpy(sv), torch.from_numpy(sf))  # paired by name; cap.obj has no partner
    common = ["--gpu-ids", "0", "--in", str(src), "--method", "harmonic", "--weights", "uniform"]
    res = flatten_fl.main(common + ["--out", str(out), "--bake", "32", "--bake-source", str(fine), "--bake-gutter", "2"])
    report = json.loads((out / "flatten.json").read_text())
    assert report == json.loads(json.dumps(res)) and sorted(report["files"]) == ["cap.obj", "tube.obj"]
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted(["flatten.json", "cap.obj", "cap.mtl", "cap_flat.obj", "cap_normal.png", "cap_tangent_normal.png",
                            "cap_color.png", "cap_position.npy", "tube.obj", "tube.mtl", "tube_flat.obj", "tube_normal.png",
                            "tube_tangent_normal.png", "tube_position.npy"])        # no colours anywhere for the tube: no colour map
    for name, stem in (("cap.obj", "cap"), ("tube.obj", "tube")):
        entry = report["files"][name]["bake"]
        assert entry["size"] == [32, 32] and entry["lanes"] in (8, 64) and entry["gutter"] == 2 and entry["projection"] == "closest"
        assert entry["source"] == (str(fine / "tube.obj") if stem == "tube" else None)
        rep = entry["report"]
        assert 0 < rep["covered_texels"] < 32 * 32 and rep["flipped_faces"] == 0 and rep["overlap_texels"] == 0
        assert rep["fallback_texels"] == (0 if stem == "tube" else None)
        mesh = read_obj_uv(str(out / name))
        assert mesh["mtllib"] == stem + ".mtl" and mesh["usemtl"] == "baked" and torch.equal(mesh["faces"], mesh["faces_uv"])
        uv = mesh["uv"]
        assert uv.shape[0] == mesh["verts"].shape[0] == report["files"][name]["cut_vertices"]
        assert float(uv.min()) >= 2. / 32 - 1e-7 and float(uv.max()) <= 30. / 32 + 1e-7     # inside [0,1], the gutter's width off the sides
        mtl = (out / (stem + ".mtl")).read_text()
        assert ("norm %s_tangent_normal.png" % stem) in mtl and ("# normal %s_normal.png" % stem) in mtl
        assert ("map_Kd cap_color.png" in mtl) == (stem == "cap")
        position = np.load(str(out / (stem + "_position.npy")))
        assert position.dtype == np.float32 and position.shape == (32, 32, 3)
        # the same bake in this process (every step is pinned to the bit): the PNGs reload to its quantised images
        from recmv import bake, param
        from recmv.utils.utils import read_obj
        iv, jf = read_obj(str(src / name))
        r = param.flatten(iv.to(DEV), jf.to(DEV), method="harmonic", weights="uniform")
        own = None if stem == "tube" else read_obj_uv(str(src / name))["colors"].to(DEV)[r["origin"]].contiguous()    # 6 decimals
        fine_mesh = tuple(x.to(DEV) for x in read_obj(str(fine / "tube.obj"))) if stem == "tube" else None      # 6 decimals
        b = bake.bake(r["verts"], r["faces"], r["uv"], 32, source=fine_mesh, gutter=2, colors=own)
        assert b["report"] == rep and b["lanes"] == entry["lanes"]
        assert np.abs(uv.numpy() - b["uv"].cpu().numpy()).max() <= 0.5e-8         # the file's 8 decimals
        filled = (b["src"] >= 0).cpu().numpy()
        assert np.array_equal(position, b["position"].cpu().numpy())
        for kind, file_name in entry["files"].items():
            if kind == "position":
                continue
            image = b[kind].cpu().numpy()
            if kind == "normal":
                image = np.where(filled[:, :, None], np.float32(0.5) + np.float32(0.5) * image, np.float32(0))
            png = np.asarray(Image.open(str(out / file_name)))
            assert png.dtype == np.uint8 and png.shape == (32, 32, 3) and np.array_equal(png, BR.quantise(image)), (name, kind)
            assert (png[~filled] == 0).all() and png[filled].any()
        if stem == "cap":                                   # baked from itself: the flat normal map, and its own colours
            tn = np.asarray(Image.open(str(out / "cap_tangent_normal.png"))).astype(np.int32)[filled]
            assert np.abs(tn - [128, 128, 255]).max() <= 1
            assert torch.allclose(mesh["colors"], torch.from_numpy(colors)[r["origin"].cpu()], atol=1e-6)
    # without --bake: the bytes the parent's command wrote
    flatten_fl.main(common + ["--out", str(plain)])
    parents_outputs(str(src), str(parent), "harmonic", "uniform")
    assert sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in parent.iterdir()) == [
        "cap.obj", "cap_flat.obj", "flatten.json", "tube.obj", "tube_flat.obj"]
    for p in plain.iterdir():
        assert p.read_bytes() == (parent / p.name).read_bytes(), p.name
    assert "mtllib" not in (plain / "cap.obj").read_text()
