"""The float64 references of tests/render_reference.py against float64 autograd of plain torch compositions, and every condition on
the test inputs that a bound of that module relies on.  No GPU."""
import re
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import render_reference as R  # noqa: E402

TOL = 1e-11
CSRC = Path(__file__).resolve().parent.parent / "rec-mv_amd" / "csrc"
NORMAL_FLOOR = 2.0 ** -100


def _close(a, b, tol=TOL):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= tol * (1.0 + (float(b.abs().max()) if b.numel() else 0.0)), err


# ----------------------------------------------------------------------------------------------- plain torch compositions
def _project_torch(ps, Rm, T, f, pp, W, H, mode):
    """model/CameraMine.py: project (2), transform_points_ndc (0), transform_points_screen (1) in float64."""
    v = (ps.unsqueeze(-1) * Rm.unsqueeze(0)).sum(-2) + T.view(1, 3)
    if mode == 2:
        return torch.stack([pp[0] - v[:, 0] * f[0] / v[:, 2], pp[1] - v[:, 1] * f[1] / v[:, 2]], 1)
    fx, fy = f[0] / (W / 2.0), f[1] / (H / 2.0)
    px = float(torch.tensor(1.0 - 1.0 / W, dtype=torch.float64).float()) - pp[0] / (W / 2.0)
    py = float(torch.tensor(1.0 - 1.0 / H, dtype=torch.float64).float()) - pp[1] / (H / 2.0)
    z = v[:, 2]
    ndc = torch.stack([(fx * v[:, 0] + px * z) / z, (fy * v[:, 1] + py * z) / z, z], 1)
    if mode == 0:
        return ndc
    return torch.stack([(W - 1.0) / 2.0 - W * ndc[:, 0] / 2.0, (H - 1.0) / 2.0 - H * ndc[:, 1] / 2.0, 1.0 / ndc[:, 2]], 1)


def _rays_torch(ps, Rm, f, pp):
    r0 = -ps[:, 0] / f[0] + ps[:, 2] * pp[0] / f[0]
    r1 = -ps[:, 1] / f[1] + ps[:, 2] * pp[1] / f[1]
    rays = torch.stack([r0, r1, ps[:, 2]], 1)
    rays = rays / torch.norm(rays, p=2, dim=1, keepdim=True)
    return (rays.unsqueeze(-1) * Rm.t().unsqueeze(0)).sum(-2)


def _leaves(cam16):
    c = cam16.double()
    return c[:9].view(3, 3), c[9:12].clone().requires_grad_(True), c[12:14].clone().requires_grad_(True), c[14:16].clone().requires_grad_(True)


# ---------------------------------------------------------------------------------------------------------------- camera
@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("name", R.CAM_NAMES + ("exact",))
def test_projection_and_its_gradients(name, mode):
    cam = R.make_camera(name)
    pts, g = R.make_points(cam, 257)
    g = g[:, :2] if mode == 2 else g
    Rm, T, f, pp = _leaves(cam["cam16"])
    ps = pts.double().requires_grad_(True)
    out = _project_torch(ps, Rm, T, f, pp, cam["W"], cam["H"], mode)
    grads = torch.autograd.grad((out * g.double()).sum(), (ps, T, f, pp))
    _close(R.project(cam["cam16"], pts, cam["W"], cam["H"], mode).v, out.detach())
    bw = R.project_backward(cam["cam16"], pts, g, cam["W"], cam["H"], mode)
    _close(bw["g_pts"].v, grads[0])
    _close(bw["sums"].v, torch.cat(grads[1:]), 1e-10)
    _close(bw["terms"].v.sum(0), bw["sums"].v)


@pytest.mark.parametrize("form", ("int", "float"))
@pytest.mark.parametrize("name", R.CAM_NAMES)
def test_rays_and_their_gradients(name, form):
    cam = R.make_camera(name)
    col, row, pix, g = R.make_pixels(cam, 257)
    if form == "int":
        pix = torch.stack([col.float(), row.float(), torch.ones(257)], 1)
    else:
        assert set(pix[:, 2].tolist()) == set(R.RAY_W)
    Rm, _, f, pp = _leaves(cam["cam16"])
    out = _rays_torch(pix.double(), Rm, f, pp)
    grads = torch.autograd.grad((out * g.double()).sum(), (f, pp))
    _close(R.rays(cam["cam16"], pix[:, 0], pix[:, 1], pix[:, 2]).v, out.detach())
    _close(R.rays_backward(cam["cam16"], pix[:, 0], pix[:, 1], pix[:, 2], g)["sums"].v, torch.cat(grads), 1e-10)


def test_camera_input_conditions():
    for name in R.CAM_NAMES + ("exact",):
        cam = R.make_camera(name)
        Rm = cam["cam16"][:9].view(3, 3).double()
        _close(Rm @ Rm.t(), torch.eye(3, dtype=torch.float64), 1e-6)
        for P in R.CAM_P:
            pts, g = R.make_points(cam, P)
            assert R.z_margin(cam["cam16"], pts) > 0
            if P == 0:
                continue
            live = [R.project(cam["cam16"], pts, cam["W"], cam["H"], m).v for m in (0, 1, 2)]
            live += [R.project_backward(cam["cam16"], pts, g[:, :2] if m == 2 else g, cam["W"], cam["H"], m)["terms"].v for m in (0, 1, 2)]
            col, row, pix, gr = R.make_pixels(cam, P)
            live += [R.rays_backward(cam["cam16"], pix[:, 0], pix[:, 1], pix[:, 2], gr)["terms"].v]
            assert R.smallest_nonzero(live) > NORMAL_FLOOR
    assert R.make_camera("general")["W"] != R.make_camera("general")["H"]
    z = R.to_view(R.make_camera("deep")["cam16"], R.make_points(R.make_camera("deep"), 4099)[0])[2].v
    assert float(z.min()) < 0.06 and float(z.max()) > 4.5 and float(z.min()) >= 0.05 - 1e-6


def test_exact_camera_is_exact_in_float32():
    """Every term is a multiple of 2^-8 and the absolute sums stay below 2^16: every partial sum of any order fits 24 bits."""
    cam = R.make_camera("exact")
    pts, g = R.make_points(cam, 257)
    assert torch.equal(pts, pts.round()) or torch.equal(pts * 2, (pts * 2).round())
    for mode in (0, 1, 2):
        out = R.project(cam["cam16"], pts, cam["W"], cam["H"], mode).v
        bw = R.project_backward(cam["cam16"], pts, g[:, :2] if mode == 2 else g, cam["W"], cam["H"], mode)
        for t in (out, bw["g_pts"].v, bw["terms"].v):
            assert torch.equal(t * 256, (t * 256).round()) and torch.equal(t.float().double(), t)
        assert float(bw["terms"].v.abs().sum(0).max()) < 2 ** 16


def test_grid_caps_restate_the_headers():
    common = (CSRC / "common.h").read_text()
    camera = (CSRC / "camera.hip").read_text()
    assert int(re.search(r"constexpr int kNumCU = (\d+);", common).group(1)) == R.NUM_CU
    assert int(re.search(r"constexpr int kWave = (\d+);", common).group(1)) == R.WAVE
    assert re.search(r"const int64_t cap = \(int64_t\)kNumCU \* 8;", common)
    assert int(re.search(r"constexpr int kBlk = (\d+);", camera).group(1)) == R.BLK
    assert re.search(r"ceil_div\(P, \(int64_t\)kBlk \* 4\)", camera)
    assert int(re.search(r"if \(g > (\d+)\) g = \1;", camera).group(1)) == R.BWD_BLOCK_CAP
    assert [R.bwd_blocks(P) for P in (0, 1, 1024, 1025, 10 ** 9)] == [1, 1, 1, 2, 1024]
    assert [R.stream_grid(P) for P in (0, 1, 256, 257, 10 ** 9)] == [1, 1, 1, 2, 2048]
    # the wrap sizes do wrap, by exactly WRAP_ROWS rows
    assert R.FWD_WRAP_P - R.stream_grid(R.FWD_WRAP_P) * R.BLK == R.WRAP_ROWS
    assert R.BWD_WRAP_P - R.bwd_blocks(R.BWD_WRAP_P) * R.BLK * 4 == R.WRAP_ROWS
    assert R.NORMALS_WRAP_V * 2 > R.stream_grid(R.NORMALS_WRAP_V * 2) * 256 and R.NORMALS_WRAP_V - 262144 == 150
    N, H, W = R.PHONG_WRAP
    assert R.ceil_div(R.NUM_CU * 8, N) * 256 < H * W


# --------------------------------------------------------------------------------------------------------------- normals
def _normals_torch(verts, faces):
    """tests/phong_reference.py: verts_normals_ref in float64 (faces with an index out of range dropped)."""
    verts = verts.double()
    faces = faces[((faces >= 0) & (faces < verts.shape[0])).all(1)]
    vf = verts[faces]
    n = torch.zeros_like(verts)
    n = n.index_add(0, faces[:, 1], torch.cross(vf[:, 2] - vf[:, 1], vf[:, 0] - vf[:, 1], dim=1))
    n = n.index_add(0, faces[:, 2], torch.cross(vf[:, 0] - vf[:, 2], vf[:, 1] - vf[:, 2], dim=1))
    n = n.index_add(0, faces[:, 0], torch.cross(vf[:, 1] - vf[:, 0], vf[:, 2] - vf[:, 0], dim=1))
    return F.normalize(n, eps=1e-6, dim=1)


def _meshes():
    soup = R.make_soup()
    assert soup[2] == 0, "the soup's seed must change: a vertex has a tiny nonzero normal sum"
    grid = R.make_grid_mesh()
    bad = torch.cat([grid[1], torch.tensor([[0, 1, grid[0].shape[0] + 3]])])
    return {"grid": grid, "grid_bad_face": (grid[0], bad), "soup": soup[:2], "integer": R.make_integer_mesh()}


@pytest.mark.parametrize("name", ("grid", "grid_bad_face", "soup", "integer"))
def test_vertex_normals(name):
    verts, faces = _meshes()[name]
    n, norm, zero = R.verts_normals(verts, faces)
    _close(n.v, _normals_torch(verts, faces))
    assert bool((zero | (norm >= R.NORMAL_MIN)).all())
    assert bool((n.v[zero] == 0).all()) and bool((n.e[zero] == 0).all())
    sums = norm[~zero]
    assert R.smallest_nonzero([sums]) > NORMAL_FLOOR
    if name == "grid":
        assert verts.shape[0] == 81 and faces.shape[0] == 128 and int(zero.sum()) == 0
    if name == "soup":
        assert verts.shape[0] == 700 and faces.shape[0] == 1500 and int(zero.sum()) >= 50
        assert bool((faces[:, 0] == faces[:, 1]).any()) and bool((verts[faces[3, 0]] == verts[faces[3, 1]]).all())
    if name == "integer":
        assert torch.equal(n.v, n.v.round()) and int(zero.sum()) == 1
        assert torch.equal(torch.log2(sums), torch.log2(sums).round())
    offsets, codes = R.adjacency(faces, verts.shape[0])
    assert int(offsets[-1]) <= codes.numel() == 3 * faces.shape[0]
    # the lists hold corner 1 of the faces in order, then corner 2, then corner 0
    for v in range(0, verts.shape[0], 37):
        mine = codes[int(offsets[v]):int(offsets[v + 1])].long()
        want = [3 * f + c for c in (1, 2, 0) for f in range(faces.shape[0]) if int(faces[f, c]) == v]
        assert mine.tolist() == want


# ----------------------------------------------------------------------------------------------------------------- phong
def _phong_torch(p2f, bary, verts, faces, normals, colors, cams, prm):
    """tests/phong_reference.py: hard_phong_ref in float64; p2f < 0 is the background."""
    N, V = verts.shape[:2]
    verts, normals, colors, bary, prm = verts.double(), normals.double(), colors.double().expand(N, -1, -1), bary.double(), prm.double()
    packed = (faces[None] + (torch.arange(N) * V).view(N, 1, 1)).reshape(-1, 3)
    idx = p2f.clamp(min=0)

    def interp(vals):
        return (bary[..., None] * vals.reshape(-1, 3)[packed][idx]).sum(-2)

    pts, nrm, tex = interp(verts), interp(normals), interp(colors)
    n_ = F.normalize(nrm, p=2, dim=-1, eps=1e-6)
    d_ = F.normalize(prm[0:3].view(1, 1, 1, 3) - pts, p=2, dim=-1, eps=1e-6)
    cos = (n_ * d_).sum(-1)
    view = F.normalize(cams.double().view(N, 1, 1, 3) - pts, p=2, dim=-1, eps=1e-6)
    reflect = -d_ + 2 * (cos[..., None] * n_)
    alpha = F.relu((view * reflect).sum(-1)) * (cos > 0).double()
    spec = prm[9:12] * torch.pow(alpha, float(prm[21]))[..., None]
    rgb = (prm[12:15] * prm[3:6] + prm[15:18] * (prm[6:9] * F.relu(cos)[..., None])) * tex + prm[18:21] * spec
    rgb[p2f < 0] = prm[22:25]
    return rgb


def _phong_cases():
    for light in R.PHONG_LIGHTS:
        for s in R.SHININESS:
            yield R.make_phong_case(), light, s
    yield R.make_phong_case(*R.PHONG_WRAP[:1], R.PHONG_WRAP[1:], copies=True), "front", 64.0


def test_phong_matches_torch_and_its_input_conditions():
    for case, light, s in _phong_cases():
        if case["N"] == R.PHONG_WRAP[0]:                                    # copies: frame 0 is the case
            case = {k: (v[:1] if torch.is_tensor(v) and k != "faces" else v) for k, v in case.items()}
            case["N"] = 1
        prm = R.phong_params(R.PHONG_LIGHTS[light], s)
        normals = R.reference_normals(case)
        for colors in (case["colors"], case["colors"][:1]):
            ref = R.phong(case["p2f"], case["bary"], case["verts"], normals, colors, case["faces"], case["cams"], prm)
            fg, und = ref["fg"], ref["undecided"]
            assert int(und.sum()) * 100 <= int(fg.sum()), "more than 1 % of the foreground pixels are undecided: change the case"
            p2f = torch.where(fg, case["p2f"] % case["F"] + (case["p2f"] // case["F"]) * case["F"], torch.full_like(case["p2f"], -1))
            want = _phong_torch(p2f, case["bary"], case["verts"], case["faces"].clamp(max=case["V"] - 1), normals, colors, case["cams"], prm)
            got = torch.where(ref["decided_on"].unsqueeze(-1), ref["rgb_on"].v, ref["rgb_off"].v)
            keep = ~und
            _close(got[keep], want[keep])
            # the cases reach what they are for
            assert int(fg.sum()) > 0.6 * fg.numel() and int((~fg).sum()) > 0.1 * fg.numel()
            lit = int(ref["decided_on"].sum())
            assert (lit > 0.9 * int(fg.sum())) if light == "front" else (lit < 0.1 * int(fg.sum()))
            assert bool((case["bary"] == torch.tensor([1.0, 0.0, 0.0])).all(-1).any())


def test_sweep_covers_the_unit_interval():
    case = R.make_sweep()
    for s in R.SWEEP_SHININESS:
        ref = R.phong(case["p2f"], case["bary"], case["verts"], case["normals"], case["colors"], case["faces"], case["cam"],
                      R.sweep_params(case, s), parts=True, powf_ulp=0.0)
        a = ref["alpha"].v.reshape(-1)
        assert int(ref["undecided"].sum()) == 0 and bool(ref["fg"].all())
        assert int((a > 0).sum()) >= 2 ** 16 * 0.9 and float(a.max()) > 1 - 1e-6
        hist = torch.histc(a[a > 0], bins=16, min=0.0, max=1.0)
        assert int(hist.min()) >= 256, hist


# ------------------------------------------------------------------------------------------------------------ compositor
def _composite_torch(idx, a, feats):
    """The published forward, pixel by pixel: a [npix,K] float64 (requires grad), idx [npix,K], feats [C,P]."""
    out = []
    for i in range(idx.shape[0]):
        cum, res = 1.0, torch.zeros(feats.shape[0], dtype=torch.float64)
        for k in range(idx.shape[1]):
            if idx[i, k] < 0:
                break
            res = res + cum * a[i, k] * feats[:, idx[i, k]]
            cum = cum * (1 - a[i, k])
        out.append(res)
    return torch.stack(out)


def _published_backward_loops(idx, a, feats, g):
    """pytorch3d's alpha_composite backward, loop by loop (float64, eps = float32(1e-9))."""
    ga = torch.zeros_like(a)
    for i in range(idx.shape[0]):
        cum = 1.0
        for k in range(idx.shape[1]):
            if idx[i, k] < 0:
                break
            for ch in range(feats.shape[0]):
                ga[i, k] += g[i, ch] * cum * feats[ch, idx[i, k]]
                for t in range(k):
                    ga[i, t] -= g[i, ch] * feats[ch, idx[i, k]] * cum * a[i, k] / (1 - a[i, t] + R.ALPHA_EPS)
            cum = cum * (1 - a[i, k])
    return ga


@pytest.mark.parametrize("case", R.COMPOSITE_CASES, ids=lambda c: "%dx%dx%d-K%d-C%d-%s" % (c[0] + (c[1], c[2], "dists" if c[3] else "alphas")))
def test_compositor(case):
    c = R.make_lists(*case)
    N, H, W = c["shape"]
    K, C = c["K"], c["C"]
    idx = c["idx"].reshape(-1, K).long()
    live = idx >= 0
    assert int(idx.max()) < c["P"], "an index >= total_points never occurs"
    lengths = live.sum(1)
    assert bool((lengths == 0).any()) and bool((lengths == K).any()) and bool((live.long().diff(dim=1) <= 0).all())
    raw = torch.where(live, c["alphas"].reshape(-1, K).double(), torch.zeros(live.shape, dtype=torch.float64))
    assert bool(torch.isnan(c["alphas"].reshape(-1, K)[~live]).all())
    a0 = (1 - raw / c["radius2"]) if c["radius2"] else raw
    if not c["radius2"] and K >= 3:
        vals = c["alphas"].reshape(-1, K)[live]
        assert bool((vals == 0).any()) and bool((vals == 1).any()) and bool((vals == torch.tensor(0.999)).any())
        assert bool(((vals < 1) & (vals > 1 - 1e-6)).any())
    a = a0.clone().requires_grad_(True)
    feats = c["features"].double().requires_grad_(True)
    g = c["g_images"].double().permute(0, 2, 3, 1).reshape(-1, C)
    small = slice(0, 64)
    out = _composite_torch(idx[small], a[small], feats)
    fw = R.composite_forward(c).v.permute(0, 2, 3, 1).reshape(-1, C)
    _close(fw[small], out.detach())
    trace = []
    bw = R.composite_backward(c, trace)
    R.composite_forward(c, trace)
    assert R.smallest_nonzero(trace) > NORMAL_FLOOR
    ga = bw["g_alphas"].v.reshape(-1, K)
    chain = (-1.0 / c["radius2"]) if c["radius2"] else 1.0
    _close(ga[small], _published_backward_loops(idx[small], a0[small], c["features"].double(), g[small]) * chain * live[small], 1e-10)
    # the recurrence the bound follows is the same number as the published double loop
    _close(bw["recurrence"], bw["g_alphas"].v, 1e-9)
    # autograd knows no eps: it agrees where 1 - a >> eps, and for the features everywhere (checked on the first pixels' lists)
    g_a, = torch.autograd.grad((out * g[small]).sum(), a, retain_graph=True)
    far = live[small] & ((1 - a0[small]).abs() > 0.01)
    _close((ga[small] / chain)[far], g_a[small][far], 1e-6)
    full = _composite_torch(idx, a0, feats) if idx.shape[0] <= 300 and K <= 3 else None
    if full is not None:
        g_f, = torch.autograd.grad((full * g).sum(), feats)
        _close(bw["g_features"].v, g_f)


def test_integer_compositor_is_exact_in_float32():
    for K in (1, 3, 8):
        c = R.make_lists((1, 16, 16), K, 2, False, integer=True)
        fw, bw = R.composite_forward(c), R.composite_backward(c, integer=True)
        for t in (fw.v, bw["g_alphas"].v, bw["g_features"].v):
            assert torch.equal(t * 2 ** 12, (t * 2 ** 12).round()) and float(t.abs().max()) < 2 ** 10
        vals = c["alphas"][c["idx"] >= 0]
        assert set(vals.tolist()) <= {0.0, 0.5, 1.0}
