"""The render side of the loop — the five camera entry points (csrc/camera.hip), the vertex normals and the hard Phong shader
(csrc/shade_meshes.hip) and the point-splat compositor (csrc/rasterize_points.hip) — through the C ABI, and once each through the
autograd wrappers, against the float64 references of tests/render_reference.py.

Every bounded test prints `ratio name: ...` (largest error / bound) and asserts <= 1; the bounds are derived in the docstring of
render_reference and never fitted.  Exact outputs (integer inputs, zero normals, the background, counters, copies, tiled repeats
across a grid-stride wrap, the same sums with and without an optional output) are compared bit for bit.  Outputs are pre-filled
with NaN and guarded by sentinels on both sides.
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
import render_reference as R  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
SENT = -7.0
GUARD = 8
ERR_ARG = -1


def _lib():
    from recmv import _lib as L
    return L, L.lib()


def _stream():
    L, _ = _lib()
    return L.stream_ptr(torch.device(DEV))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _sentinel(dtype):
    return SENT if dtype.is_floating_point else 121


def _out(*shape, dtype=torch.float32, fill=NAN):
    """An output buffer full of `fill` between two rows of sentinels."""
    n = int(np.prod(shape)) if shape else 1
    base = torch.full((n + 2 * GUARD,), _sentinel(dtype), dtype=dtype, device=DEV)
    base[GUARD:GUARD + n] = fill
    return base[GUARD:GUARD + n].view(*shape)


def _guards_ok(*views):
    for v in views:
        if v is None:
            continue
        base = v._base
        s = _sentinel(base.dtype)
        assert bool((base[:GUARD] == s).all()) and bool((base[-GUARD:] == s).all()), "wrote outside its output"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _report(name, **ratios):
    print("ratio %s: %s" % (name, "  ".join("%s %.3g" % kv for kv in ratios.items())))
    for k, v in ratios.items():
        assert v <= 1.0, "%s: %s error / bound = %.4g" % (name, k, v)


def _ratio(got, ref, rows=None):
    got = got.detach().cpu().double().reshape(ref.v.shape)
    err, bound = (got - ref.v).abs(), ref.e
    if rows is not None:
        err, bound = err[rows], bound[rows]
    return R.ratio(err, bound)


def _dev(t):
    return t.to(DEV).contiguous() if t is not None else None


# ---------------------------------------------------------------------------------------------------------------- camera
def _project(cam, pts, mode):
    L, lib = _lib()
    P = pts.shape[0]
    out = _out(P, 2 if mode == 2 else 3)
    hold = [_dev(pts), _dev(cam["cam16"])]
    L.check(lib.recmv_cam_project(_p(hold[0]), P, _p(hold[1]), cam["W"], cam["H"], mode, _p(out), _stream()), "cam_project")
    torch.cuda.synchronize()
    _guards_ok(out)
    return out


def _project_backward(cam, pts, g, mode, with_pts=True):
    L, lib = _lib()
    P = pts.shape[0]
    nf = int(lib.recmv_cam_partial_floats(P))
    assert nf == 7 * R.bwd_blocks(P)
    g_pts = _out(P, 3) if with_pts else None
    g7, part = _out(7), _out(nf)
    hold = [_dev(pts), _dev(g), _dev(cam["cam16"])]
    L.check(lib.recmv_cam_project_backward(_p(hold[0]), _p(hold[1]), P, _p(hold[2]), cam["W"], cam["H"], mode, _p(g_pts), _p(g7),
                                           _p(part), nf, _stream()), "cam_project_backward")
    torch.cuda.synchronize()
    _guards_ok(g_pts, g7, part)
    return g_pts, g7


def _rays(cam, P, pix=None, col=None, row=None):
    L, lib = _lib()
    out = _out(P, 3)
    hold = [_dev(pix), _dev(col), _dev(row), _dev(cam["cam16"])]
    L.check(lib.recmv_cam_rays(_p(hold[0]), _p(hold[1]), _p(hold[2]), P, _p(hold[3]), _p(out), _stream()), "cam_rays")
    torch.cuda.synchronize()
    _guards_ok(out)
    return out


def _rays_backward(cam, g, pix=None, col=None, row=None):
    L, lib = _lib()
    P = g.shape[0]
    nf = 4 * R.bwd_blocks(P)
    g4, part = _out(4), _out(nf)
    hold = [_dev(pix), _dev(col), _dev(row), _dev(g), _dev(cam["cam16"])]
    L.check(lib.recmv_cam_rays_backward(_p(hold[0]), _p(hold[1]), _p(hold[2]), _p(hold[3]), P, _p(hold[4]), _p(g4), _p(part), nf,
                                        _stream()), "cam_rays_backward")
    torch.cuda.synchronize()
    _guards_ok(g4, part)
    return g4


@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("name", R.CAM_NAMES)
def test_cam_project_forward_and_backward(name, mode):
    """Every size of CAM_P (0, one thread, around a block, several blocks of the backward, several terms per thread): the
    projection, g_pts and the seven reduced gradients; the sums are the same bits with and without g_pts."""
    cam = R.make_camera(name)
    worst = {"out": 0.0, "g_pts": 0.0, "sums": 0.0}
    for P in R.CAM_P:
        pts, g = R.make_points(cam, P)
        g = g[:, :2].contiguous() if mode == 2 else g
        ref_bw = R.project_backward(cam["cam16"], pts, g, cam["W"], cam["H"], mode)
        g_pts, g7 = _project_backward(cam, pts, g, mode)
        _, g7_alone = _project_backward(cam, pts, g, mode, with_pts=False)
        assert _same_bits(g7, g7_alone), "the sums depend on g_pts being asked for (P = %d)" % P
        if P == 0:
            assert bool((g7 == 0).all()), "P == 0 must zero the sums"
            continue
        out = _project(cam, pts, mode)
        worst["out"] = max(worst["out"], _ratio(out, R.project(cam["cam16"], pts, cam["W"], cam["H"], mode)))
        worst["g_pts"] = max(worst["g_pts"], _ratio(g_pts, ref_bw["g_pts"]))
        worst["sums"] = max(worst["sums"], _ratio(g7, ref_bw["sums"]))
    _report("cam_project %s mode %d" % (name, mode), **worst)


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_cam_project_exact_integers(mode):
    """Signed permutation R, integer T and pp, power-of-two f, W / 2, H / 2 and z: every operation is exact."""
    cam = R.make_camera("exact")
    pts, g = R.make_points(cam, 257)
    g = g[:, :2].contiguous() if mode == 2 else g
    ref = R.project_backward(cam["cam16"], pts, g, cam["W"], cam["H"], mode)
    out = _project(cam, pts, mode)
    g_pts, g7 = _project_backward(cam, pts, g, mode)
    assert torch.equal(out.cpu(), R.project(cam["cam16"], pts, cam["W"], cam["H"], mode).v.float())
    assert torch.equal(g_pts.cpu(), ref["g_pts"].v.float())
    assert torch.equal(g7.cpu(), ref["sums"].v.float())


@pytest.mark.parametrize("form", ("int", "float"))
@pytest.mark.parametrize("name", R.CAM_NAMES)
def test_cam_rays_forward_and_backward(name, form):
    """The (col, row) int64 form and the float [P,3] form with w in {1, 0.5, 2, -1} mixed in one call."""
    cam = R.make_camera(name)
    worst = {"out": 0.0, "sums": 0.0}
    for P in R.CAM_P:
        col, row, pix, g = R.make_pixels(cam, P)
        if form == "int":
            args = {"col": col, "row": row}
            x, y, w = col.float(), row.float(), torch.ones(P)
        else:
            args = {"pix": pix}
            x, y, w = pix[:, 0], pix[:, 1], pix[:, 2]
        g4 = _rays_backward(cam, g, **args)
        if P == 0:
            assert bool((g4 == 0).all())
            continue
        out = _rays(cam, P, **args)
        worst["out"] = max(worst["out"], _ratio(out, R.rays(cam["cam16"], x, y, w)))
        worst["sums"] = max(worst["sums"], _ratio(g4, R.rays_backward(cam["cam16"], x, y, w, g)["sums"]))
    _report("cam_rays %s %s" % (name, form), **worst)


@functools.lru_cache(maxsize=None)
def _wrap_tile(name):
    cam = R.make_camera(name)
    pts, g = R.make_points(cam, R.WRAP_TILE)
    _, _, pix, gr = R.make_pixels(cam, R.WRAP_TILE)
    return cam, pts, g, pix, gr


def _tile_rows(P):
    idx = torch.arange(P) % R.WRAP_TILE
    return idx, torch.bincount(idx, minlength=R.WRAP_TILE)


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_cam_project_grid_stride_wrap_repeats_the_tile_bit_for_bit(mode):
    """P = 524 288 + 300 > 2048 * 256: the threads are independent, so rows i and i mod 4096 carry the same bits — the 300 rows
    behind the wrap repeat rows 0..299 — and the first 4096 rows are judged against float64."""
    cam, pts, _, _, _ = _wrap_tile("general")
    idx, _ = _tile_rows(R.FWD_WRAP_P)
    out = _project(cam, pts[idx], mode)
    assert _same_bits(out[-R.WRAP_ROWS:], out[:R.WRAP_ROWS])
    assert _same_bits(out, out[:R.WRAP_TILE][idx.to(DEV)])
    _report("cam_project across the wrap, mode %d" % mode, out=_ratio(out[:R.WRAP_TILE], R.project(cam["cam16"], pts, cam["W"], cam["H"], mode)))


def test_cam_rays_grid_stride_wrap_repeats_the_tile_bit_for_bit():
    cam, _, _, pix, _ = _wrap_tile("loop")
    idx, _ = _tile_rows(R.FWD_WRAP_P)
    out = _rays(cam, R.FWD_WRAP_P, pix=pix[idx])
    assert _same_bits(out[-R.WRAP_ROWS:], out[:R.WRAP_ROWS])
    assert _same_bits(out, out[:R.WRAP_TILE][idx.to(DEV)])
    _report("cam_rays across the wrap", out=_ratio(out[:R.WRAP_TILE], R.rays(cam["cam16"], pix[:, 0], pix[:, 1], pix[:, 2])))


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_cam_project_backward_wrap(mode):
    """P = 1 048 576 + 300 > 1024 * 256 * 4: g_pts repeats the tile bit for bit; the sums are judged against float64 on the tiled
    input (every tile row counted as often as it occurs)."""
    cam, pts, g, _, _ = _wrap_tile("general")
    g = g[:, :2].contiguous() if mode == 2 else g
    idx, counts = _tile_rows(R.BWD_WRAP_P)
    g_pts, g7 = _project_backward(cam, pts[idx], g[idx], mode)
    assert _same_bits(g_pts[-R.WRAP_ROWS:], g_pts[:R.WRAP_ROWS])
    assert _same_bits(g_pts, g_pts[:R.WRAP_TILE][idx.to(DEV)])
    ref = R.project_backward(cam["cam16"], pts, g, cam["W"], cam["H"], mode, counts=counts)
    _report("cam_project_backward across the wrap, mode %d" % mode, g_pts=_ratio(g_pts[:R.WRAP_TILE], ref["g_pts"]),
            sums=_ratio(g7, ref["sums"]))


def test_cam_rays_backward_wrap():
    cam, _, _, pix, g = _wrap_tile("loop")
    idx, counts = _tile_rows(R.BWD_WRAP_P)
    g4 = _rays_backward(cam, g[idx], pix=pix[idx])
    ref = R.rays_backward(cam["cam16"], pix[:, 0], pix[:, 1], pix[:, 2], g, counts=counts)
    _report("cam_rays_backward across the wrap", sums=_ratio(g4, ref["sums"]))


def test_cam_argument_errors_return_without_a_launch():
    L, lib = _lib()
    cam = R.make_camera("loop")
    c16, x = _dev(cam["cam16"]), _dev(torch.zeros(1100, 3))
    out, g7, g4 = _out(1100, 3), _out(7), _out(4)
    nf = int(lib.recmv_cam_partial_floats(1100))
    assert nf == 14
    part = _out(nf)
    s = _stream()
    assert lib.recmv_cam_project(_p(x), 4, _p(c16), 64.0, 64.0, 3, _p(out), s) == ERR_ARG
    assert lib.recmv_cam_project(_p(x), -1, _p(c16), 64.0, 64.0, 0, _p(out), s) == ERR_ARG
    assert lib.recmv_cam_project(_p(x), 4, _p(c16), 0.0, 64.0, 0, _p(out), s) == ERR_ARG
    assert lib.recmv_cam_project(_p(x), 4, None, 64.0, 64.0, 0, _p(out), s) == ERR_ARG
    assert lib.recmv_cam_project(_p(x), 4, _p(c16), 64.0, 64.0, 0, None, s) == ERR_ARG
    assert lib.recmv_cam_project_backward(_p(x), _p(x), 1100, _p(c16), 64.0, 64.0, 0, _p(out), _p(g7), _p(part), nf - 1, s) == ERR_ARG
    assert lib.recmv_cam_project_backward(_p(x), _p(x), 1100, _p(c16), 64.0, 64.0, 0, _p(out), None, _p(part), nf, s) == ERR_ARG
    assert lib.recmv_cam_project_backward(_p(x), _p(x), 1100, _p(c16), 64.0, 64.0, -1, _p(out), _p(g7), _p(part), nf, s) == ERR_ARG
    assert lib.recmv_cam_project_backward(_p(x), None, 1100, _p(c16), 64.0, 64.0, 0, _p(out), _p(g7), _p(part), nf, s) == ERR_ARG
    assert lib.recmv_cam_rays(None, None, None, 4, _p(c16), _p(out), s) == ERR_ARG
    assert lib.recmv_cam_rays(_p(x), None, None, -4, _p(c16), _p(out), s) == ERR_ARG
    assert lib.recmv_cam_rays_backward(_p(x), None, None, _p(x), 1100, _p(c16), _p(g4), _p(part), 4 * 2 - 1, s) == ERR_ARG
    assert lib.recmv_cam_rays_backward(_p(x), None, None, _p(x), 1100, _p(c16), None, _p(part), nf, s) == ERR_ARG
    torch.cuda.synchronize()
    for t in (out, g7, g4, part):
        assert bool(torch.isnan(t).all()), "a refused call wrote"
    _guards_ok(out, g7, g4, part)
    assert lib.recmv_cam_partial_floats(0) == 7 and lib.recmv_cam_partial_floats(10 ** 9) == 7 * R.BWD_BLOCK_CAP


def test_camera_class_through_autograd():
    """project / transform_points_ndc / transform_points_screen ([N,P,3] input) / view_rays / view_rays_pix once each at P = 257:
    outputs and the gradients that reach the points, T, f and pp, against the same references."""
    from recmv.model import RectifiedPerspectiveCameras
    cam = R.make_camera("general")
    c = cam["cam16"]
    P = 257
    pts, g = R.make_points(cam, P)
    col, row, pix, gr = R.make_pixels(cam, P)
    ratios = {}

    def fresh():
        T, f, pp = (_dev(c[a:b].view(1, -1)).requires_grad_(True) for a, b in ((9, 12), (12, 14), (14, 16)))
        return RectifiedPerspectiveCameras(f, pp, _dev(c[:9].view(1, 3, 3)), T, image_size=[(cam["W"], cam["H"])]), T, f, pp

    for label, mode, shape in (("ndc", 0, (P, 3)), ("screen", 1, (1, P, 3)), ("project", 2, (P, 3))):
        camera, T, f, pp = fresh()
        ps = _dev(pts).view(shape).requires_grad_(True)
        out = {0: camera.transform_points_ndc, 1: camera.transform_points_screen, 2: camera.project}[mode](ps)
        gm = g[:, :2].contiguous() if mode == 2 else g
        assert out.shape == ((P, 2) if mode == 2 else shape)
        out.backward(_dev(gm).view(out.shape))
        ref = R.project_backward(c, pts, gm, cam["W"], cam["H"], mode)
        ratios[label] = _ratio(out, R.project(c, pts, cam["W"], cam["H"], mode))
        ratios[label + "_g_pts"] = _ratio(ps.grad, ref["g_pts"])
        ratios[label + "_sums"] = _ratio(torch.cat([T.grad.view(-1), f.grad.view(-1), pp.grad.view(-1)]), ref["sums"])
    for label in ("view_rays", "view_rays_pix"):
        camera, T, f, pp = fresh()
        if label == "view_rays":
            out = camera.view_rays(_dev(pix))
            x, y, w = pix[:, 0], pix[:, 1], pix[:, 2]
        else:
            out = camera.view_rays_pix(_dev(col), _dev(row))
            x, y, w = col.float(), row.float(), torch.ones(P)
        out.backward(_dev(gr))
        ratios[label] = _ratio(out, R.rays(c, x, y, w))
        ratios[label + "_sums"] = _ratio(torch.cat([f.grad.view(-1), pp.grad.view(-1)]), R.rays_backward(c, x, y, w, gr)["sums"])
    _report("camera class through autograd", **ratios)


# -------------------------------------------------------------------------------------------------------- vertex normals
def _normals(verts, faces, adjacency=None):
    """verts [N,V,3], faces [F,3] (host) -> normals [N,V,3] on the device; the adjacency is built on the host."""
    L, lib = _lib()
    N, V = verts.shape[:2]
    offsets, codes = adjacency if adjacency is not None else R.adjacency(faces, V)
    out = _out(N, V, 3)
    hold = [_dev(verts), _dev(faces), _dev(offsets), _dev(codes)]
    L.check(lib.recmv_verts_normals(_p(hold[0]), _p(hold[1]), _p(hold[2]), _p(hold[3]), N, V, faces.shape[0], _p(out), _stream()),
            "verts_normals")
    torch.cuda.synchronize()
    _guards_ok(out)
    return out


def _judge_normals(name, got, verts, faces):
    ref, norm, zero = R.verts_normals(verts, faces)
    assert bool((zero | (norm >= R.NORMAL_MIN)).all())
    got = got.cpu()
    assert _same_bits(got[zero], torch.zeros(int(zero.sum()), 3)), "%s: a vertex without a normal sum is not exactly +0" % name
    return _ratio(got, ref)


@pytest.mark.parametrize("N", (1, 3))
def test_verts_normals(N):
    """The perturbed 9 x 9 grid (also with a face whose index is out of range: skipped) and the soup (repeated indices, a
    zero-length edge, 50 unreferenced vertices); on the grid the bits are those of the float32 restatement in the header's order."""
    ratios = {}
    grids = [R.make_grid_mesh(9, k) for k in range(N)]
    faces = grids[0][1]
    verts = torch.stack([m[0] for m in grids])
    assert verts.shape[1:] == (81, 3) and faces.shape == (128, 3)
    got = _normals(verts, faces)
    ratios["grid"] = max(_judge_normals("grid", got[n], verts[n], faces) for n in range(N))
    adj = R.adjacency(faces, 81)
    for n in range(N):
        assert _same_bits(got[n].cpu(), R.verts_normals_float32(verts[n], faces, *adj)), "the corner order of the header (mesh %d)" % n
    bad = torch.cat([faces[:40], torch.tensor([[0, 1, 81 + 3], [-1, 5, 6]]), faces[40:]])
    got_bad = _normals(verts, bad)
    assert _same_bits(got_bad, got), "a face with an index out of range must be skipped"
    sv, sf, moved = R.make_soup()
    assert moved == 0, "the soup's seed must change"
    soup = torch.stack([sv] * N)
    got = _normals(soup, sf)
    ratios["soup"] = _judge_normals("soup", got[0], sv, sf)
    for n in range(1, N):
        assert _same_bits(got[n], got[0])
    _report("verts_normals N=%d" % N, **ratios)


def test_verts_normals_exact_integers():
    verts, faces = R.make_integer_mesh()
    got = _normals(verts[None], faces)[0].cpu()
    assert torch.equal(got, R.verts_normals(verts, faces)[0].v.float())


def test_verts_normals_grid_stride_wrap():
    """N = 2 copies of V = 262 144 + 150 vertices (3238 copies of the 81-vertex grid and 16 loose vertices): N V > 2048 * 256, so
    mesh 1 lies behind the wrap.  It must equal mesh 0 bit for bit, every tile of mesh 0 must equal the first, and the first tile
    is judged against float64."""
    tv, tf = R.make_grid_mesh(R.NORMALS_TILE_GRID)
    Vt = tv.shape[0]
    tiles, loose = divmod(R.NORMALS_WRAP_V, Vt)
    verts = torch.cat([tv.repeat(tiles, 1), torch.ones(loose, 3)])
    faces = (tf.unsqueeze(0) + (torch.arange(tiles) * Vt).view(-1, 1, 1)).reshape(-1, 3)
    assert 2 * verts.shape[0] > R.stream_grid(2 * verts.shape[0]) * 256
    got = _normals(torch.stack([verts, verts]), faces)
    assert _same_bits(got[1], got[0])
    body = got[0, :tiles * Vt].view(tiles, Vt, 3)
    assert _same_bits(body, body[:1].expand_as(body))
    assert _same_bits(got[0, tiles * Vt:], torch.zeros(loose, 3, device=DEV))
    _report("verts_normals across the wrap", first_tile=_judge_normals("tile", body[0], tv, tf))


# ----------------------------------------------------------------------------------------------------------------- phong
def _shade(case, normals, colors, prm, gt_mask=None, images=None):
    L, lib = _lib()
    N, V, F, H, W = case["N"], case["V"], case["F"], case["H"], case["W"]
    assert int(lib.recmv_hard_phong_params_floats()) == prm.numel()
    host = (C.c_float * prm.numel())(*prm.tolist())
    images = _out(N, H, W, 4) if images is None else images
    counts = _out(N, 2, dtype=torch.int64, fill=-5) if gt_mask is not None else None
    hold = [_dev(case["p2f"]), _dev(case["bary"]), _dev(case["verts"]), _dev(normals), _dev(colors), _dev(case["faces"]),
            _dev(case["cams"]), _dev(gt_mask)]
    rc = lib.recmv_hard_phong_shade(_p(hold[0]), _p(hold[1]), _p(hold[2]), _p(hold[3]), _p(hold[4]), colors.shape[0], _p(hold[5]),
                                    _p(hold[6]), N, V, F, H, W, host, _p(images), _p(hold[7]), _p(counts), _stream())
    torch.cuda.synchronize()
    return rc, images, counts


def _judge_phong(case, normals, colors, prm, images):
    ref = R.phong(case["p2f"], case["bary"], case["verts"], normals, colors, case["faces"], case["cams"], prm)
    fg, und = ref["fg"], ref["undecided"]
    assert int(und.sum()) * 100 <= int(fg.sum()), "more than 1 % of the foreground pixels are undecided: change the case"
    img = images.cpu()
    assert _same_bits(img[..., 3], torch.ones_like(img[..., 3])), "alpha must be 1"
    bg = prm[22:25].view(1, 1, 1, 3).expand_as(img[..., :3])
    assert _same_bits(img[..., :3][~fg], bg[~fg]), "a pixel without a valid face must be the background exactly"
    return R.phong_ratio(img[..., :3], ref), ref


@pytest.mark.parametrize("shininess", R.SHININESS)
@pytest.mark.parametrize("light", tuple(R.PHONG_LIGHTS))
def test_hard_phong(light, shininess):
    """24 x 40 host-built fragments on two grids, judged on the kernel's own normals: colours for one mesh and for N; a light in
    front and one behind (n.l < 0 on most pixels: no diffuse, and the specular term is pow(0, s): 0, but exactly 1 at shininess 0)."""
    case = R.make_phong_case()
    normals = _normals(case["verts"], case["faces"]).cpu()
    prm = R.phong_params(R.PHONG_LIGHTS[light], shininess)
    ratios = {}
    for label, colors in (("colors_N", case["colors"]), ("colors_1", case["colors"][:1].contiguous())):
        rc, images, _ = _shade(case, normals, colors, prm)
        assert rc == 0
        _guards_ok(images)
        ratios[label], _ = _judge_phong(case, normals, colors, prm, images)
    _report("hard_phong %s shininess %g" % (light, shininess), **ratios)


def test_hard_phong_frame_grid_cap_and_counts():
    """N = 64 frames of 96 x 96: ceil(2048 / 64) * 256 < 9216, so every frame's pixels wrap.  The frames are copies: they must
    agree bit for bit, frame 0 is judged against float64, and the silhouette counts are exact integers."""
    N, H, W = R.PHONG_WRAP
    case = R.make_phong_case(N, (H, W), copies=True)
    normals = _normals(case["verts"], case["faces"]).cpu()
    prm = R.phong_params(R.PHONG_LIGHTS["front"], 64.0)
    g = torch.Generator().manual_seed(5)
    gt = (torch.rand(1, H, W, generator=g) < 0.4).float().expand(N, H, W).contiguous()
    rc, images, counts = _shade(case, normals, case["colors"], prm, gt_mask=gt)
    assert rc == 0
    _guards_ok(images, counts)
    assert _same_bits(images, images[:1].expand_as(images))
    first = {k: (v[:1] if torch.is_tensor(v) and k != "faces" else v) for k, v in case.items()}
    first["N"] = 1
    r, ref = _judge_phong(first, normals[:1], case["colors"][:1], prm, images[:1])
    m = (case["p2f"] >= 0) & (case["p2f"] < N * case["F"])                     # the kernel's M: a face id inside the table
    want = torch.stack([(m & (gt != 0)).sum((1, 2)), (m | (gt != 0)).sum((1, 2))], 1)
    assert torch.equal(counts.cpu(), want)
    _report("hard_phong 64 frames of 96x96", frame0=r)


def test_hard_phong_refuses_a_misaligned_image():
    case = R.make_phong_case()
    normals = R.reference_normals(case)
    prm = R.phong_params(R.PHONG_LIGHTS["front"], 1.0)
    whole = _out(case["N"] * case["H"] * case["W"] * 4 + 4)
    rc, _, _ = _shade(case, normals, case["colors"], prm, images=whole[1:-3].view(case["N"], case["H"], case["W"], 4))
    assert rc == ERR_ARG
    assert bool(torch.isnan(whole).all())
    _guards_ok(whole)


def test_powf_accuracy():
    """powf in isolation: mat_spec = light_spec = 1, ambient = diffuse = 0, exact normals — the pixel is powf(alpha, s) of the
    kernel's alpha; alpha covers (0, 1] evenly on 2^16 pixels, s in {1, 10.5, 64}.  The argument is the float32 restatement of
    alpha (the s = 1 image must return it bit for bit); the error against float64 pow of it is printed in ulp, as is the smallest F
    for which every pixel is inside the reference's bound; both must stay inside the allowance POWF_ULP of render_reference."""
    case = R.make_sweep()
    c = {"p2f": case["p2f"], "bary": case["bary"], "verts": case["verts"], "faces": case["faces"], "cams": case["cam"], "N": 1, "V": 3,
         "F": 1, "H": case["p2f"].shape[1], "W": case["p2f"].shape[2]}
    alpha32 = R.sweep_alpha_float32(case)
    direct, need = {}, {}
    for s in R.SWEEP_SHININESS:
        prm = R.sweep_params(case, s)
        rc, images, _ = _shade(c, case["normals"], case["colors"], prm)
        assert rc == 0
        _guards_ok(images)
        ref = R.phong(case["p2f"], case["bary"], case["verts"], case["normals"], case["colors"], case["faces"], case["cam"], prm,
                      parts=True, powf_ulp=0.0)
        assert bool(((alpha32.double() - ref["alpha"].v[0]).abs() <= ref["alpha"].e[0]).all())
        img = images.cpu()
        assert _same_bits(img[..., 0], img[..., 1]) and _same_bits(img[..., 0], img[..., 2])
        got = img[0, :, :, 0]
        if s == 1.0:
            same = int((_bits(got) == _bits(alpha32)).sum())
            print("powf accuracy: powf(alpha, 1) returns the restated alpha bit for bit on %d of %d pixels" % (same, got.numel()))
        direct[s], n = R.powf_error_ulp(got, alpha32, s)
        need[s], _ = R.powf_needed_ulp(got, ref["alpha"][0], s)
        assert n >= 2 ** 13
        print("powf accuracy: shininess %g: %d pixels, error %.4f ulp, smallest F inside the bound %.4f" % (s, n, direct[s], need[s]))
    worst = max(max(direct.values()), max(need.values()))
    print("powf accuracy: measured maximum %.4f ulp" % worst)
    assert worst <= R.POWF_ULP


# ------------------------------------------------------------------------------------------------------------ compositor
def _composite(c, with_features=True):
    L, lib = _lib()
    N, H, W = c["shape"]
    K, Cn, P = c["K"], c["C"], c["P"]
    images, g_alphas = _out(N, Cn, H, W), _out(N, H, W, K)
    g_features = _out(Cn, P) if with_features else None
    hold = [_dev(c["idx"]), _dev(c["alphas"]), _dev(c["features"]), _dev(c["g_images"])]
    L.check(lib.recmv_alpha_composite_forward(_p(hold[0]), _p(hold[1]), _p(hold[2]), N, H, W, K, Cn, P, c["radius2"], _p(images),
                                              _stream()), "alpha_composite_forward")
    L.check(lib.recmv_alpha_composite_backward(_p(hold[0]), _p(hold[1]), _p(hold[2]), _p(hold[3]), N, H, W, K, Cn, P, c["radius2"],
                                               _p(g_alphas), _p(g_features), _stream()), "alpha_composite_backward")
    torch.cuda.synchronize()
    _guards_ok(images, g_alphas, g_features)
    return images, g_alphas, g_features


@pytest.mark.parametrize("case", R.COMPOSITE_CASES, ids=lambda c: "%dx%dx%d-K%d-C%d-%s" % (c[0] + (c[1], c[2], "dists" if c[3] else "alphas")))
def test_alpha_composite(case):
    """Host-built packed lists (empty and full pixels, NaN behind the lists; alphas 0, 1, 0.999 and within 1e-6 of 1), both
    opacity modes: the image, grad_alphas against the published double loop with its eps, grad_features; grad_alphas is the same
    bits with and without grad_features."""
    c = R.make_lists(*case)
    assert int(c["idx"].max()) < c["P"]
    images, g_alphas, g_features = _composite(c)
    _, g_alphas_alone, _ = _composite(c, with_features=False)
    assert _same_bits(g_alphas, g_alphas_alone), "grad_alphas depends on grad_features being asked for"
    bw = R.composite_backward(c)
    _report("alpha_composite %s" % (case,), images=_ratio(images, R.composite_forward(c)), g_alphas=_ratio(g_alphas, bw["g_alphas"]),
            g_features=_ratio(g_features, bw["g_features"]))


@pytest.mark.parametrize("K", (1, 3, 8))
def test_alpha_composite_exact_integers(K):
    c = R.make_lists((1, 16, 16), K, 2, False, integer=True)
    images, g_alphas, g_features = _composite(c)
    bw = R.composite_backward(c, integer=True)
    assert torch.equal(images.cpu(), R.composite_forward(c).v.float())
    assert torch.equal(g_alphas.cpu(), bw["g_alphas"].v.float())
    assert torch.equal(g_features.cpu(), bw["g_features"].v.float())


@pytest.mark.parametrize("fused", (False, True))
def test_alpha_composite_through_autograd(fused):
    """raster.alpha_composite / alpha_composite_dists once each on the K = 50 case."""
    from recmv import raster
    c = R.make_lists((2, 24, 24), 50, 2, fused)
    alphas = _dev(c["alphas"]).requires_grad_(True)
    feats = _dev(c["features"]).requires_grad_(True)
    if fused:
        radius = float(np.float32(0.05))
        assert float(np.float32(radius * radius)) == c["radius2"]
        out = raster.alpha_composite_dists(_dev(c["idx"]), alphas, radius, feats)
    else:
        out = raster.alpha_composite(_dev(c["idx"]), alphas, feats)
    out.backward(_dev(c["g_images"]))
    bw = R.composite_backward(c)
    _report("alpha_composite through autograd, %s" % ("dists" if fused else "alphas"), images=_ratio(out, R.composite_forward(c)),
            g_alphas=_ratio(alphas.grad, bw["g_alphas"]), g_features=_ratio(feats.grad, bw["g_features"]))
