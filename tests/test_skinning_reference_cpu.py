"""The float64 references of tests/skinning_reference.py against float64 autograd of plain torch compositions, and every
condition on the test inputs that a bound of that module relies on.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import skinning_reference as R  # noqa: E402

TOL = 1e-11


def _close(a, b, tol=TOL):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= tol * (1.0 + float(b.abs().max()) if b.numel() else 1.0), err


# ----------------------------------------------------------------------------------------------- plain torch compositions
def _sample(p, grid):
    """[P,24] through F.grid_sample, border padding, align_corners=False."""
    vol = grid["vol"].double().permute(3, 0, 1, 2).unsqueeze(0)
    g = ((p - grid["center"].double()) * grid["scale"].double()).view(1, 1, 1, -1, 3)
    return F.grid_sample(vol, g, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0, 0, :].t()


def _sample_twice_differentiable(p, grid):
    """The same trilinear sample from gathers and products (grid_sample has no double backward)."""
    vol = grid["vol"].double()
    D, H, W = vol.shape[:3]
    size = torch.tensor([W, H, D], dtype=torch.float64)
    ix = (((p - grid["center"].double()) * grid["scale"].double() + 1) * size - 1) / 2
    ix = torch.minimum(torch.maximum(ix, torch.zeros(3, dtype=torch.float64)), size - 1)
    x0 = torch.minimum(torch.floor(ix.detach()), size - 2)
    f1 = ix - x0
    f0 = 1 - f1
    x0 = x0.long()
    out = 0
    for k in range(8):
        bx, by, bz = k & 1, (k >> 1) & 1, k >> 2
        wk = (f1 if bx else f0)[:, 0] * (f1 if by else f0)[:, 1] * (f1 if bz else f0)[:, 2]
        out = out + wk.unsqueeze(1) * vol[x0[:, 2] + bz, x0[:, 1] + by, x0[:, 0] + bx]
    return out


def _skin(p, frame, A, trans, grid, sample=_sample):
    w = sample(p, grid)
    T = (w[:, :, None, None] * A[frame]).sum(1)
    ph = torch.cat([p, torch.ones(p.shape[0], 1, dtype=torch.float64)], 1)
    return (T[:, :3, :] * ph.unsqueeze(1)).sum(-1) + trans[frame]


def _jacobian(p, frame, A, trans, grid, sample, create_graph):
    d = _skin(p, frame, A, trans, grid, sample)
    rows = [torch.autograd.grad(d[:, i].sum(), p, create_graph=create_graph, retain_graph=True)[0] for i in range(3)]
    return d, torch.stack(rows, 1)                                       # J[p, i, k] = d v_i / d p_k


def _case(shape, P=96, B=3, seed=0, only=(R.FAM_IN, R.FAM_CLIP)):
    grid = R.make_volume(shape, seed)
    p, fam = R.make_points(grid, P, seed)
    keep = torch.zeros(P, dtype=torch.bool)
    for f in only:
        keep |= fam == f
    p = p[keep]
    frame, A, trans = R.make_frames(p.shape[0], B, seed)
    return grid, p, frame, A, trans


# -------------------------------------------------------------------------------------------------------------- skinning
@pytest.mark.parametrize("shape", R.VOLUMES)
def test_weights_and_their_derivatives(shape):
    grid, p, *_ = _case(shape)
    s = R.lbs_weights(p, grid)
    pd = p.double().requires_grad_(True)
    _close(s["w"].v, _sample(pd, grid).detach())
    w2 = _sample_twice_differentiable(pd, grid)
    _close(s["w"].v, w2.detach())
    for j in (0, 7, 23):
        g1, = torch.autograd.grad(_sample(pd, grid)[:, j].sum(), pd)
        _close(s["D"].v[:, :, j], g1)
        ga, = torch.autograd.grad(w2[:, j].sum(), pd, create_graph=True)
        _close(s["D"].v[:, :, j], ga.detach())
        hx, = torch.autograd.grad(ga[:, 0].sum(), pd, retain_graph=True)
        hy, = torch.autograd.grad(ga[:, 1].sum(), pd, retain_graph=True)
        _close(s["H"].v[:, 0, j], hx[:, 1])
        _close(s["H"].v[:, 1, j], hx[:, 2])
        _close(s["H"].v[:, 2, j], hy[:, 2])
        assert float(hx[:, 0].abs().max()) == 0.0                        # linear in each coordinate


def test_clipped_axes_have_zero_derivatives_and_nan_points_zero_weights():
    grid = R.make_volume((3, 5, 4))
    P = 26 * 3
    p, fam = R.make_points(grid, P, 1, torch.full((P,), R.FAM_CLIP))
    s = R.lbs_weights(p, grid)
    ix, size = R.coords(p, grid)
    out = (ix.v <= 0) | (ix.v >= size - 1)
    assert bool(out.any(1).all()) and bool((out.sum(1) == 3).any()) and bool((out.sum(1) == 1).any())
    assert bool(((ix.v <= 0).any(0)).all()) and bool(((ix.v >= size - 1).any(0)).all())      # either side on every axis
    assert bool((s["D"].v.abs().amax(2)[out] == 0).all())
    frame, A, trans = R.make_frames(P, 2)
    jet = R.lbs_jet_forward(p, frame, A, trans, grid)
    fw = R.lbs_forward(p, frame, A, trans, grid)
    T = (fw["w"].v[:, :, None, None] * A.double()[frame][:, :, :3, :3]).sum(1)
    all3 = out.all(1)
    _close(jet["J"].v[all3], T[all3])
    pn, _ = R.make_points(grid, 64, 2, torch.full((64,), R.FAM_NAN))
    sn = R.lbs_weights(pn, grid)
    assert not bool(sn["valid"].any()) and float(sn["w"].v.abs().max()) == 0.0 and float(sn["w"].e.max()) == 0.0


@pytest.mark.parametrize("shape", R.VOLUMES)
def test_forward_vjp_stage_and_jet_against_autograd(shape):
    grid, p, frame, A, trans = _case(shape)
    P, B = p.shape[0], A.shape[0]
    g = torch.Generator().manual_seed(5)
    g_d = torch.randn(P, 3, generator=g)
    gv, gJ = torch.randn(P, 3, generator=g), torch.randn(P, 9, generator=g)
    pd = p.double().requires_grad_(True)
    Ad = A.double().requires_grad_(True)
    td = trans.double().requires_grad_(True)
    d = _skin(pd, frame, Ad, td, grid)
    fw = R.lbs_forward(p, frame, A, trans, grid)
    _close(fw["d"].v, d.detach())
    gp, gA, gt = torch.autograd.grad(d, [pd, Ad, td], g_d.double())
    _close(R.lbs_vjp_input(p, frame, A, grid, g_d)["g_p"].v, gp)
    st = R.lbs_params_stage(p, frame, B, grid, g_d)
    _close((st["W"].v.t() @ st["Q"].v).reshape(24, B, 3, 4).permute(1, 0, 2, 3), gA[:, :, :3, :])
    _close(st["Gs"].v.sum(0).reshape(B, 3), gt)
    # the jet and its reverse
    v, J = _jacobian(pd, frame, Ad, td, grid, _sample_twice_differentiable, True)
    jet = R.lbs_jet_forward(p, frame, A, trans, grid)
    _close(jet["v"].v, v.detach())
    _close(jet["J"].v, J.detach())
    _, J1 = _jacobian(pd, frame, Ad, td, grid, _sample, False)
    _close(jet["J"].v, J1)
    for use_v, use_j in ((True, True), (True, False), (False, True)):
        loss = 0
        if use_v:
            loss = loss + (v * gv.double()).sum()
        if use_j:
            loss = loss + (J * gJ.double().reshape(P, 3, 3)).sum()
        gp, gA, gt = torch.autograd.grad(loss, [pd, Ad, td], retain_graph=True, allow_unused=True)
        bw = R.lbs_jet_backward(p, frame, A, B, grid, gv if use_v else None, gJ if use_j else None)
        _close(bw["g_p"].v, gp)
        _close((bw["W4"].v.t() @ bw["Q4"].v).reshape(24, B, 3, 4).permute(1, 0, 2, 3), gA[:, :, :3, :])
        _close(bw["Gs"].v.sum(0).reshape(B, 3), gt if gt is not None else torch.zeros(B, 3, dtype=torch.float64))
        _close(bw["W4"].v[0::4], st["W"].v)


def test_ray_energy_against_autograd_and_its_preconditions():
    g = torch.Generator().manual_seed(2)
    P = 4099
    d = torch.randn(P, 3, generator=g)
    cam = torch.tensor([0.3, -2.5, 0.4])
    for lo in (1e-6, 1e-3):
        rays = R.make_rays(d, cam, lo)
        dd = d.double().requires_grad_(True)
        e = dd - cam.double()
        un = torch.linalg.cross(e, rays.double().expand_as(e)).norm(dim=1)
        loss2 = un / e.norm(dim=1)
        gd, = torch.autograd.grad(loss2.sum(), dd)
        ref = R.ray_energy(d, cam, rays)
        _close(ref["loss2"].v, loss2.detach())
        _close(ref["angle"].v, torch.rad2deg(torch.asin(loss2.detach())) * (R.RAD2DEG / (180 / np.pi)), 1e-9)
        _close(ref["g_d"].v, gd, 1e-8)
        # the ratio stays at or below 0.99 (asin's conditioning) and covers the range down to lo
        r = ref["loss2"]
        assert float((r.v + r.e).max()) <= R.RATIO_MAX and float(r.v.min()) < lo * 1.5
        assert bool(torch.isfinite(ref["angle"].e).all()) and bool(torch.isfinite(ref["g_d"].e).all())
        # the cancellation: the bound of g_d is of order u / (un dn) per unit |e| |v|, not relative to g_d
        assert float((ref["g_d"].e.amax(1) * ref["loss2"].v).max()) < 1e-4


@pytest.mark.parametrize("shape", R.VOLUMES)
def test_every_in_voxel_point_is_inside_its_cell(shape):
    grid = R.make_volume(shape)
    for P in R.LBS_P:
        p, fam = R.make_points(grid, P)
        ix, size = R.coords(p, grid)
        inv = fam == R.FAM_IN
        c = ix.v[inv]
        assert bool(((c - torch.round(c)).abs() >= 1.0 / 32).all())
        assert bool((c >= 1.0 / 32).all()) and bool((c <= size - 1 - 1.0 / 32).all())
        assert c.numel() == 0 or float(ix.e[inv].max()) < 1.0 / 64
        cl = ix.v[fam == R.FAM_CLIP]
        outside = (cl <= -0.4) | (cl >= size - 1 + 0.4)
        inside = ((cl - torch.round(cl)).abs() >= 1.0 / 32) & (cl >= 1.0 / 32) & (cl <= size - 1 - 1.0 / 32)
        assert bool((outside | inside).all()) and bool(outside.any(1).all())
        lat = ix.v[fam == R.FAM_LATTICE]
        assert bool(((lat - torch.round(lat)).abs() < 1e-4).all())
        if P >= 257:
            assert set(fam.tolist()) == {R.FAM_IN, R.FAM_CLIP, R.FAM_LATTICE, R.FAM_NAN}
        assert bool(torch.isnan(p[fam == R.FAM_NAN]).any(1).all()) and bool(torch.isfinite(p[fam != R.FAM_NAN]).all())
    assert float(grid["vol"].min()) >= 0 and float(grid["vol"].max()) <= 1


def test_integer_family_is_exact_in_float32():
    # |Q4 entry| <= |gv| |p| + |gJ| <= 3 * 2 + 3, far below 2^24; every value an integer
    P, B = 257, 3
    g = torch.Generator().manual_seed(1)
    grid = R.make_volume((3, 5, 4))
    p = torch.randint(-2, 3, (P, 3), generator=g).float()
    gv = torch.randint(-3, 4, (P, 3), generator=g).float()
    gJ = torch.randint(-3, 4, (P, 9), generator=g).float()
    frame, A, _ = R.make_frames(P, B)
    bw = R.lbs_jet_backward(p, frame, A, B, grid, gv, gJ)
    st = R.lbs_params_stage(p, frame, B, grid, gv)
    for t in (bw["Q4"], bw["Gs"], st["Q"], st["Gs"]):
        assert float(t.v.abs().max()) < 2 ** 24 and bool((t.v == torch.round(t.v)).all())
        assert bool((t.v.float().double() == t.v).all())
    own = torch.zeros(P, B * 12, dtype=torch.bool)
    own.scatter_(1, frame.unsqueeze(1) * 12 + torch.arange(12).unsqueeze(0), True)
    assert float(st["Q"].v[~own].abs().max()) == 0.0 and float(st["Q"].e[~own].max()) == 0.0


# ----------------------------------------------------------------------------------------------------------- root finder
@pytest.mark.parametrize("family", R.ROOT_FAMILIES)
def test_rootfind_update_against_a_plain_loop(family):
    P = 257
    c = R.make_rootfind(P, family)
    for do_update in (0, 1):
        ref = R.rootfind_update(c["p"], c["f"], c["gf"], c["loss2"], c["angle"], c["gd"], c["unfinished"], 5, R.ROOT_DTHR,
                                R.ROOT_ATHR, R.ROOT_W1, R.ROOT_W2, do_update)
        assert ref["margin"] > 0                                          # |grad|^2 minus its error: never a division by ~0
        n = 5
        for i in range(P):
            f, a = np.float32(c["f"][i].item()), np.float32(c["angle"][i].item())
            done = bool(abs(f) < np.float32(R.ROOT_DTHR)) and bool(a < np.float32(R.ROOT_ATHR))
            un = bool(c["unfinished"][i]) and not done
            assert int(ref["unfinished"][i]) == int(un)
            n += un
            want = c["p"][i].double()
            if un and do_update:
                loss = R.ROOT_W1 * abs(float(f)) + R.ROOT_W2 * float(c["loss2"][i])
                grad = R.ROOT_W1 * float(np.sign(f)) * c["gf"][i].double() + R.ROOT_W2 * c["gd"][i].double()
                want = want - loss * grad / float((grad * grad).sum())
            else:
                assert float(ref["p"].e[i].max()) == 0.0
            _close(ref["p"].v[i], want)
        assert ref["count"] == n
    if family == "finished":
        assert int(ref["unfinished"].sum()) == 0
    if family == "none":
        assert torch.equal(ref["unfinished"], c["unfinished"])
    if family == "mixed":
        i = torch.arange(P) % 8
        keep = c["unfinished"] != 0
        for k in (0, 1, 2, 3):                                           # sign 0, NaN angle, the two exact thresholds: unfinished
            assert bool((ref["unfinished"][(i == k) & keep] == 1).all())
        assert bool((ref["unfinished"][i == 4] == 0).all())
        assert bool((c["f"][i == 2].abs() == np.float32(R.ROOT_DTHR)).all()) and bool((c["angle"][i == 3] == np.float32(R.ROOT_ATHR)).all())


# -------------------------------------------------------------------------------------------------------- kinematic chain
def _rodrigues_torch(theta):
    angle = torch.norm(theta + R.EPS_RODRIGUES, dim=1, keepdim=True)
    n = theta / angle
    half = angle * 0.5
    q = torch.cat([torch.cos(half), torch.sin(half) * n], 1)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                        2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                        2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], 1).view(-1, 3, 3)


def _chain_torch(poses, Js, parents, init_pose):
    B = poses.shape[0]
    Rm = _rodrigues_torch(poses.reshape(-1, 3)).view(B, 24, 3, 3)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(B, 1, 4)

    def mat(Rj, t):
        return torch.cat([torch.cat([Rj, t.expand(B, 3).unsqueeze(-1)], 2), bottom], 1)
    out = [mat(Rm[:, 0], Js[0])]
    for j in range(1, 24):                                               # the 23-step loop
        out.append(out[parents[j]] @ mat(Rm[:, j], Js[j] - Js[parents[j]]))
    G = torch.stack(out, 1)
    return G, G @ init_pose.unsqueeze(0)


@pytest.mark.parametrize("table", sorted(R.parent_tables()))
def test_chain_against_autograd_through_the_loop(table):
    parents = R.parent_tables()[table]
    B = 5
    poses, Js = R.make_poses(B), R.make_joints()
    ip = R.make_init_pose(0, general_last_row=True)
    g = torch.Generator().manual_seed(4)
    gG, gA = torch.randn(B, 24, 4, 4, generator=g), torch.randn(B, 24, 4, 4, generator=g)
    pd = poses.double().requires_grad_(True)
    G, A = _chain_torch(pd, Js.double(), parents, ip.double())
    fw = R.chain_forward(poses, Js, parents, ip)
    _close(fw["G"].v, G.detach())
    _close(fw["A"].v, A.detach())
    for use_g, use_a in ((True, True), (True, False), (False, True)):
        loss = ((G * gG.double()).sum() if use_g else 0) + ((A * gA.double()).sum() if use_a else 0)
        want, = torch.autograd.grad(loss, pd, retain_graph=True)
        got = R.chain_backward(poses, Js, parents, ip, gG if use_g else None, gA if use_a else None)["gposes"]
        _close(got.v, want, 1e-7)                                        # the zero pose differentiates through 1 / 1.7e-8
        assert bool(torch.isfinite(got.e).all()) and bool(torch.isfinite(fw["G"].e).all())
    # the poses the issue names are there, the documented singularity is not
    n = poses.norm(dim=2)
    assert bool((n == 0).any()) and bool(((n - 3.14).abs() < 1e-3).any()) and bool(((n - 6.28).abs() < 1e-3).any())
    assert bool(((n > 5e-7) & (n < 5e-6)).any()) and bool(((n > 5e-4) & (n < 5e-3)).any())
    assert float((poses.double() + R.EPS_RODRIGUES).norm(dim=2).min()) > 1e-8


# --------------------------------------------------------------------------------------------------- positional encoding
def _posenc_torch(x, L, w, out_scale):
    cols = [x]
    for b in range(L):
        cols += [w[2 * b] * torch.sin(x * 2.0 ** b), w[2 * b + 1] * torch.cos(x * 2.0 ** b)]
    return torch.cat(cols, 1) * out_scale


@pytest.mark.parametrize("L", R.PE_L)
def test_posenc_against_autograd(L):
    P = 33
    x = R.make_pe_x(P)
    g = torch.Generator().manual_seed(L)
    gm = torch.randn(P, 3 + 6 * L, generator=g)
    t = torch.randn(P, 3, generator=g)
    for name, w in R.pe_weight_sets(L).items():
        wd = torch.ones(2 * L, dtype=torch.float64) if w is None else w.double()
        xd = x.double().requires_grad_(True)
        out = _posenc_torch(xd, L, wd, 1.0)
        _close(R.posenc(x, L, w, 2 ** -0.5).v, out.detach() * float(np.float32(2 ** -0.5)))
        vjp, = torch.autograd.grad(out, xd, gm.double(), create_graph=True)
        _close(R.posenc_vjp(x, gm, L, w).v, vjp.detach(), 1e-10)
        if L:
            second, = torch.autograd.grad((vjp * t.double()).sum(), xd)
            _close(R.posenc_vjp(x, gm, L, w, t).v, second, 1e-10)
            _close(R.posenc_vjp(x, gm, L, w, t[:1]).v, second / t.double() * t[:1].double(), 1e-9)
        else:
            assert float(R.posenc_vjp(x, gm, L, w, t).v.abs().max()) == 0.0
        _, jvp = torch.autograd.functional.jvp(lambda z: _posenc_torch(z, L, wd, 1.0), x.double(), t.double())
        _close(R.posenc_jvp(x, t, L, w).v, jvp, 1e-10)
    if L:
        assert bool((R.pe_weight_sets(L)["anneal"] == 0).any()) and bool((R.pe_weight_sets(L)["negative"] < 0).any())


def test_error_rules_hold_for_float32_evaluation_on_the_host():
    """The E rules against actual float32 arithmetic of numpy: a dot product in two orders, a quotient, a square root."""
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(1000, 37, generator=g), torch.randn(1000, 37, generator=g)
    ref = R.esum(R.E(R.f64(a)) * R.E(R.f64(b)), -1)
    for order in (slice(None), slice(None, None, -1)):
        acc = np.zeros(1000, dtype=np.float32)
        for k in range(37)[order]:
            acc = acc + a[:, k].numpy() * b[:, k].numpy()
        assert R.ratio((torch.from_numpy(acc).double() - ref.v).abs(), ref.e) <= 1.0
    q = R.esqrt(ref * ref) / (R.E(R.f64(a[:, 0])) + 8.0)
    acc64 = torch.from_numpy(acc)
    got = torch.sqrt(acc64 * acc64) / (a[:, 0] + 8.0)
    assert R.ratio((got.double() - q.v).abs(), q.e) <= 1.0
