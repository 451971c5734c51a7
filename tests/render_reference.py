"""Plain float64 references, test inputs and error bounds for the render side of the loop: the camera (csrc/camera.hip), the vertex
normals and the hard Phong shader (csrc/shade_meshes.hip) and the point-splat compositor (csrc/rasterize_points.hip:
recmv_alpha_composite_forward / _backward).

Everything here runs on the host in float64 from float32 inputs and shares no code with recmv.  The (v, e) pairs, u = 2^-24 (1 +
2^-10) and the running-error rules (+, -, *, /, sqrt, sum) are those of tests/skinning_reference.py, whose docstring states them;
tests/test_render_reference_cpu.py checks the references against float64 autograd of plain torch compositions and checks every
condition on the inputs that a bound relies on; tests/test_gpu_render.py judges the kernels.

Camera.  The three projection modes and the rays are restated operation by operation as the kernels (and the torch expressions of
model/CameraMine.py they keep the order of) write them, so the rules give e.  1 / z and 1 / z^2 are carried by the division rule:
|z| - e_z > 0 is asserted for every point.  cx = float32(1 - 1 / W) is formed on the host in double and is an exact input.  The
seven (four) camera gradients are sums over the points with a DOCUMENTED FIXED shape: a thread adds its ceil(P / (blocks 256))
terms serially, a 64-lane tree (6 levels) follows, then the 4 waves in order, then a double-precision pass over the blocks and one
cast.  A term passes through at most d = ceil(P / (blocks 256)) + 6 + 4 float additions, so [Higham, 4.2]
    e_sum = sum e_i + gamma_d sum (|v_i| + e_i) + blocks 2^-53 sum (|v_i| + e_i),    then one rounding: e = e_sum + u (|v| + e_sum).
bwd_blocks (min(ceil(P / 1024), 1024), at least 1) and stream_grid (cap 8 kNumCU = 2048 blocks) are restated here; the GPU test
asserts blocks == recmv_cam_partial_floats(P) / 7 and the CPU test reads the constants back from the headers.

Vertex normals.  Per face the three corner cross products (corner 1: (v2-v1)x(v0-v1), corner 2: (v0-v2)x(v1-v2), corner 0:
(v1-v0)x(v2-v0)), summed per vertex (sum rule with the vertex's number of terms), divided by max(norm, 1e-6).  The inputs are
chosen so that a vertex either has a sum that is EXACTLY zero (no face, or only faces with a repeated index: every product has an
exact zero factor) — compared bit for bit with +0 — or a float64 norm >= 1e-3 (asserted), where the max() is not in play.

Phong.  Interpolation w0 a + w1 b + w2 c left to right, the two normalize(eps=1e-6) (norm - e > 1e-6 asserted), relu(n.l), the
reflection -l + 2 ((n.l) n), alpha = relu(v.r) [n.l > 0], pow(alpha, shininess), colour (amb + dif) tex + spec in the kernel's grouping.
The shader is judged on the kernel's own float32 normals as exact inputs.  relu is 1-Lipschitz: it keeps e, and is exact 0 where
v < -e.  The switch [n.l > 0] is discontinuous: a pixel with |n.l| <= e_(n.l) ("undecided") is judged against both branches and
passes inside the bound of either; at most 1 % of a case's foreground pixels may be undecided (asserted from the reference alone).
pow is carried through its conditioning: p = s (alpha + e_alpha)^(s-1) e_alpha (s >= 1; 0 for s = 0; exact 0 at an exact
alpha = 0, s > 0), e = p + 2 F u (|v| + p) + 2^-120, F = powf's error in ulp.  The last term covers the underflow of alpha^64 and of
its two products with the colours (|colour| <= 2): the only place of the render side where a test input leaves the normal range.
powf.  The ROCm tree carries no accuracy table, so F is measured: test_powf_accuracy (tests/test_gpu_render.py) shades one flat
triangle with mat_spec = light_spec = 1 and ambient = diffuse = 0 — the pixel is powf(alpha, s), every other step exact — on 2^16
pixels whose alpha covers (0, 1], s in {1, 10.5, 64}, against float64.  The conditioning s e_alpha / alpha of the bound is hundreds
of ulp at s = 64 and would hide powf's own error, so powf's exact argument is restated in float32 operation by operation
(sweep_alpha_float32; at s = 1 the image must return it bit for bit, which checks the restatement) and the error is taken against
float64 pow of that argument.  The test prints that error, prints the smallest F for which every pixel is inside its bound and
asserts the allowance: the measured maximum rounded up to a whole ulp plus one ulp because the sweep is finite.
Measured on an MI355X (gfx950, ROCm 7.0), one ulp counted as 2 u |v| as in skinning_reference: powf 0.995 ulp at s = 1 (it returns
its argument bit for bit on 63 409 of the 65 536 pixels), 1.068 ulp at s = 10.5, 1.047 ulp at s = 64; inside the reference's own
bound the smallest F is 0 for all three (the conditioning covers it).  Rounded up: 2 ulp; allowance POWF_ULP = 3 ulp.

Compositor.  Forward res += (cum a) f, cum = cum (1 - a), a = alphas or 1 - d / r^2.  The backward VALUE is the published double
loop in float64 with its eps = float32(1e-9):  g_a[t] = sum_c g_c (cum_t f_tc - sum_(k>t) f_kc cum_k a_k / (1 - a_t + eps)); the
BOUND follows the recurrence the kernel runs (F_t = sum_c g_c f_tc, R_(t-1) = F_t a_t + (1 - a_t) R_t, cum, and
g_a[t] = cum_t (F_t - R_t ((1 - a_t) / ((1 - a_t) + eps)))), whose exact value is the same number (checked on the CPU).  An exact a = 1
gives an exact 1 - a = 0 and exact zeros behind it.  grad_features is a sum of float atomics: any-order sum rule.  The test lists
keep every nonzero intermediate above 2^-100 (asserted), so no underflow term is needed.

Exact-integer inputs are compared with torch.equal: a camera with a signed permutation R, integer T and pp, power-of-two f, W / 2,
H / 2 and z_view; alphas in {0, 0.5, 1} with small-integer features; small-integer meshes whose summed normals are axis aligned
with a power-of-two length.
"""
import math

import numpy as np
import torch

from skinning_reference import E, U, ecat, esqrt, estack, esum, f64, gamma, ratio  # noqa: F401

# measured by test_powf_accuracy on an MI355X (gfx950, ROCm 7.0): 1.068 ulp; allowance = rounded up to a whole ulp (2) + 1
POWF_ULP = 3.0
TINY = 2.0 ** -120
NUM_CU = 256
BLK = 256
WAVE = 64
BWD_BLOCK_CAP = 1024
NORM_EPS = float(np.float32(1e-6))
ALPHA_EPS = float(np.float32(1e-9))
NORMAL_MIN = 1e-3

CAM_P = (0, 1, 255, 256, 257, 1023, 1025, 4099)
CAM_NAMES = ("loop", "general", "deep")
FWD_WRAP_P = 524288 + 300
BWD_WRAP_P = 1048576 + 300
WRAP_ROWS = 300
WRAP_TILE = 4096
NORMALS_TILE_GRID = 9
RAY_W = (1.0, 0.5, 2.0, -1.0)
NORMALS_WRAP_V = 262144 + 150
SHININESS = (0.0, 1.0, 64.0)
SWEEP_SHININESS = (1.0, 10.5, 64.0)
# (N, H, W), K, C, fused opacity
COMPOSITE_CASES = (((1, 15, 17), 1, 1, False), ((1, 16, 16), 3, 2, False), ((1, 1, 257), 50, 4, False), ((2, 24, 24), 50, 2, False),
                   ((1, 15, 17), 3, 4, True), ((1, 16, 16), 50, 1, True), ((1, 1, 257), 1, 2, True), ((2, 24, 24), 3, 1, True))


def ceil_div(a, b):
    return (a + b - 1) // b


def stream_grid(n, block=BLK):
    return max(1, min(ceil_div(n, block), NUM_CU * 8))


def bwd_blocks(P):
    return max(1, min(ceil_div(P, BLK * 4), BWD_BLOCK_CAP))


def esel(mask, a, b):
    a, b = E.lift(a), E.lift(b)
    return E(torch.where(mask, a.v, b.v), torch.where(mask, a.e, b.e))


def erelu(x):
    return E(x.v.clamp_min(0), torch.where(x.v < -x.e, torch.zeros_like(x.e), x.e))


def edot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# --------------------------------------------------------------------------------------------------------------- camera
def make_camera(name):
    """cam16 = (R row major, T, f, pp) float32 and the image size (W, H)."""
    g = torch.Generator().manual_seed({"loop": 11, "general": 12, "deep": 13, "exact": 14}[name])
    if name == "exact":
        R = torch.tensor([[0., -1., 0.], [0., 0., 1.], [-1., 0., 0.]])
        return {"name": name, "cam16": torch.cat([R.reshape(-1), torch.tensor([2., -3., 1., 64., 128., 40., 20.])]), "W": 128.0, "H": 64.0}
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    if name == "loop":
        small, _ = torch.linalg.qr(torch.eye(3, dtype=torch.float64) + 0.02 * torch.randn(3, 3, generator=g, dtype=torch.float64))
        R = torch.diag(torch.tensor([-1., -1., 1.], dtype=torch.float64)) @ (small * torch.sign(torch.diagonal(small)))
        rest, W, H = [0.02, 0.1, 3.0, 1000.3, 999.1, 256.4, 191.2], 512.0, 384.0
    elif name == "general":
        R, rest, W, H = q, [0.3, -0.2, 0.4, 80.5, 77.25, 70.3, 11.8], 97.0, 61.0
    else:
        small, _ = torch.linalg.qr(torch.eye(3, dtype=torch.float64) + 0.2 * torch.randn(3, 3, generator=g, dtype=torch.float64))
        R, rest, W, H = small, [0.1, 0.05, 0.2, 300.0, 310.5, 150.2, 130.9], 320.0, 240.0
    return {"name": name, "cam16": torch.cat([R.reshape(-1), torch.tensor(rest, dtype=torch.float64)]).float(), "W": W, "H": H}


def make_points(cam, P, seed=0):
    """World points [P,3] float32 built from view-space positions, and a cotangent [P,3] with a nonzero mean (so that the reduced
    gradients do not cancel to nothing against sum |v_i|)."""
    g = torch.Generator().manual_seed(1000 + 7 * P + seed)
    c = cam["cam16"].double()
    R, T = c[:9].view(3, 3), c[9:12]
    r = torch.rand(P, 3, generator=g, dtype=torch.float64)
    if cam["name"] == "exact":
        v = torch.stack([torch.floor(r[:, 0] * 9) - 4, torch.floor(r[:, 1] * 9) - 4, 2.0 ** torch.floor(r[:, 2] * 3)], 1)
        gout = torch.floor(torch.rand(P, 3, generator=g) * 3) - 1
    else:
        if cam["name"] == "loop":
            v = torch.stack([r[:, 0] * 1.2 - 0.6, r[:, 1] * 1.6 - 0.8, 2.6 + 0.8 * r[:, 2]], 1)
        elif cam["name"] == "general":
            v = torch.stack([0.2 + 0.8 * r[:, 0], 0.1 + 0.7 * r[:, 1], 1.5 + 1.5 * r[:, 2]], 1)
        else:
            z = 0.05 * 100.0 ** r[:, 2]
            v = torch.stack([(r[:, 0] - 0.3) * 0.6 * z, (r[:, 1] - 0.4) * 0.5 * z, z], 1)
        gout = torch.randn(P, 3, generator=g) + 0.7
    pts = ((v - T) @ R.t()).float()                                          # v = p R + T
    return pts, gout.float()


def make_pixels(cam, P, seed=0):
    """(col, row) int64 and the float form [P,3] with w cycling through RAY_W, and a cotangent [P,3]."""
    g = torch.Generator().manual_seed(2000 + 7 * P + seed)
    W, H = int(cam["W"]), int(cam["H"])
    col = torch.randint(0, W, (P,), generator=g)
    row = torch.randint(0, H, (P,), generator=g)
    w = torch.tensor(RAY_W)[torch.arange(P) % len(RAY_W)]
    pix = torch.stack([torch.rand(P, generator=g) * W, torch.rand(P, generator=g) * H, w], 1).float()
    return col, row, pix, (torch.randn(P, 3, generator=g) + 0.5).float()


def _cam(cam16):
    c = f64(cam16)
    return E(c[:9].view(3, 3)), E(c[9:12]), E(c[12:14]), E(c[14:16])


def to_view(cam16, pts):
    R, T, _, _ = _cam(cam16)
    p = E(f64(pts))
    return [((p[:, 0] * R[0, j] + p[:, 1] * R[1, j]) + p[:, 2] * R[2, j]) + T[j] for j in range(3)]


def z_margin(cam16, pts):
    """min over the points of |z| - e_z (must be > 0)."""
    z = to_view(cam16, pts)[2]
    return float((z.v.abs() - z.e).min()) if z.v.numel() else float("inf")


def _ndc_consts(cam16, W, H):
    _, _, f, pp = _cam(cam16)
    hw, hh = E(torch.tensor(W / 2.0)), E(torch.tensor(H / 2.0))
    cx = E(torch.tensor(float(np.float32(1.0 - 1.0 / W))))
    cy = E(torch.tensor(float(np.float32(1.0 - 1.0 / H))))
    return f[0] / hw, f[1] / hh, cx - pp[0] / hw, cy - pp[1] / hh, hw, hh


def project(cam16, pts, W, H, mode):
    """[P,3] (modes 0, 1) or [P,2] (mode 2) as an E."""
    _, _, f, pp = _cam(cam16)
    v = to_view(cam16, pts)
    z = v[2]
    assert bool((z.v.abs() - z.e > 0).all()), "a point whose z_view is not separated from 0"
    if mode == 2:
        return estack([pp[0] - v[0] * f[0] / z, pp[1] - v[1] * f[1] / z], 1)
    fx, fy, px, py, _, _ = _ndc_consts(cam16, W, H)
    xn, yn = (fx * v[0] + px * z) / z, (fy * v[1] + py * z) / z
    if mode == 0:
        return estack([xn, yn, z], 1)
    return estack([E(torch.tensor((W - 1.0) / 2.0)) - (xn * W).scaled(0.5), E(torch.tensor((H - 1.0) / 2.0)) - (yn * H).scaled(0.5),
                   1.0 / z], 1)


def reduce_fixed(terms, P, counts=None):
    """The kernel's two-stage fixed-order sum over the P points of terms [P,nv] (module docstring).  counts [rows]: the rows are
    a tile and row i stands for counts[i] of the P points."""
    nv = terms.v.shape[1]
    if P == 0:
        return E(torch.zeros(nv, dtype=torch.float64))
    w = torch.ones(terms.v.shape[0], 1, dtype=torch.float64) if counts is None else counts.double().view(-1, 1)
    assert int(w.sum()) == P
    nb = bwd_blocks(P)
    d = ceil_div(P, nb * BLK) + 6 + BLK // WAVE
    mag = ((terms.v.abs() + terms.e) * w).sum(0)
    v = (terms.v * w).sum(0)
    p = (terms.e * w).sum(0) + gamma(d) * mag + nb * 2.0 ** -53 * mag
    return E.rounded(v, p)


def project_backward(cam16, pts, g_out, W, H, mode, counts=None):
    """g_pts [P,3], the per-point terms [P,7] of (gT[3], gf[2], gpp[2]) and their reduced sums [7], each an E.  counts: see
    reduce_fixed."""
    R, _, f, _ = _cam(cam16)
    P = pts.shape[0]
    v = to_view(cam16, pts)
    z = v[2]
    assert bool((z.v.abs() - z.e > 0).all())
    iz = 1.0 / z
    g = E(f64(g_out))
    if mode == 2:
        g0, g1 = g[:, 0], g[:, 1]
        gv = [(-g0) * f[0] * iz, (-g1) * f[1] * iz, (g0 * v[0] * f[0] + g1 * v[1] * f[1]) * iz * iz]
        t = [(-g0) * v[0] * iz, (-g1) * v[1] * iz, g0, g1]
    else:
        fx, fy, _, _, hw, hh = _ndc_consts(cam16, W, H)
        g0, g1, g2 = g[:, 0], g[:, 1], g[:, 2]
        if mode == 1:
            g0, g1, g2 = g0 * (-0.5 * W), g1 * (-0.5 * H), (-g2) * iz * iz
        gv = [g0 * fx * iz, g1 * fy * iz, g2 - (g0 * fx * v[0] + g1 * fy * v[1]) * iz * iz]
        t = [g0 * v[0] * iz / hw, g1 * v[1] * iz / hh, (-g0) / hw, (-g1) / hh]
    terms = estack(gv + t, 1) if P else E(torch.zeros(0, 7, dtype=torch.float64))
    g_pts = estack([(R[r, 0] * gv[0] + R[r, 1] * gv[1]) + R[r, 2] * gv[2] for r in range(3)], 1)
    return {"g_pts": g_pts, "terms": terms, "sums": reduce_fixed(terms, P if counts is None else int(counts.sum()), counts)}


def _ray_parts(cam16, x, y, w):
    _, _, f, pp = _cam(cam16)
    x, y, w = E(f64(x)), E(f64(y)), E(f64(w))
    r0 = (-x) / f[0] + w * pp[0] / f[0]
    r1 = (-y) / f[1] + w * pp[1] / f[1]
    n = esqrt((r0 * r0 + r1 * r1) + w * w)
    return r0, r1, w, n, [r0 / n, r1 / n, w / n]


def rays(cam16, x, y, w):
    """Unit world rays [P,3] (E) of the pixels (x, y, w): float32 tensors (the int64 form passes col, row and ones)."""
    R = _cam(cam16)[0]
    u = _ray_parts(cam16, x, y, w)[4]
    return estack([(u[0] * R[j, 0] + u[1] * R[j, 1]) + u[2] * R[j, 2] for j in range(3)], 1)


def rays_backward(cam16, x, y, w, g_out, counts=None):
    """Per-point terms [P,4] of (gf[2], gpp[2]) and their reduced sums [4].  counts: see reduce_fixed."""
    R, _, f, _ = _cam(cam16)
    P = g_out.shape[0]
    r0, r1, w, n, u = _ray_parts(cam16, x, y, w)
    g = E(f64(g_out))
    gu = [(g[:, 0] * R[0, c] + g[:, 1] * R[1, c]) + g[:, 2] * R[2, c] for c in range(3)]
    dot = u[0] * gu[0] + u[1] * gu[1] + u[2] * gu[2]
    gr0, gr1 = (gu[0] - u[0] * dot) / n, (gu[1] - u[1] * dot) / n
    terms = estack([gr0 * ((-r0) / f[0]), gr1 * ((-r1) / f[1]), gr0 * w / f[0], gr1 * w / f[1]], 1)
    return {"terms": terms, "sums": reduce_fixed(terms, P if counts is None else int(counts.sum()), counts)}


# -------------------------------------------------------------------------------------------------------- vertex normals
def adjacency(faces, V):
    """Vertex -> (face, corner) lists in the summation order of the three passes (corner 1, corner 2, corner 0, each in face
    order): (offsets int32 [V+1], codes int32 [3F], code = face * 3 + corner).  A corner whose vertex index is out of range has no
    list to go to; its slot of `codes` is filled with the face's own code at the end of no list (unused padding)."""
    faces = faces.long()
    F = faces.shape[0]
    order = [1, 2, 0]
    vid = faces[:, order].t().reshape(-1)
    codes = (torch.arange(F).view(1, F) * 3 + torch.tensor(order).view(3, 1)).reshape(-1)
    ok = (vid >= 0) & (vid < V)
    vid_ok, codes_ok = vid[ok], codes[ok]
    _, perm = torch.sort(vid_ok, stable=True)
    counts = torch.bincount(vid_ok, minlength=V)
    offsets = torch.zeros(V + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets.to(torch.int32), torch.cat([codes_ok[perm], codes[~ok]]).to(torch.int32)


def _ecross(a, b):
    return estack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def verts_normals_float32(verts, faces, offsets, codes):
    """The normals kernel operation by operation in float32 (numpy scalars round every operation; the kernel is built without
    contraction and with correctly rounded division and sqrt): the bits it must produce, for small meshes."""
    f32 = np.float32
    v = verts.numpy().astype(f32)
    fc, V = faces.numpy(), verts.shape[0]
    out = np.zeros((V, 3), f32)

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    for i in range(V):
        acc = [f32(0), f32(0), f32(0)]
        for e in range(int(offsets[i]), int(offsets[i + 1])):
            f, corner = int(codes[e]) // 3, int(codes[e]) % 3
            i0, i1, i2 = (int(x) for x in fc[f])
            if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= V:
                continue
            p0, p1, p2 = v[i0], v[i1], v[i2]
            c = cross(p2 - p1, p0 - p1) if corner == 1 else cross(p0 - p2, p1 - p2) if corner == 2 else cross(p1 - p0, p2 - p0)
            acc = [acc[k] + c[k] for k in range(3)]
        n = max(np.sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]), f32(NORM_EPS))
        out[i] = [acc[k] / n for k in range(3)]
    return torch.from_numpy(out)


def verts_normals(verts, faces):
    """verts [V,3] float32, faces [F,3] int64 (a face with an index outside [0, V) is skipped).  Returns the unit normals [V,3]
    (E), the float64 norm of the sums [V], and the mask of the vertices whose sum is exactly zero."""
    V = verts.shape[0]
    faces = faces.long()
    fs = faces[((faces >= 0) & (faces < V)).all(1)]
    p = E(f64(verts))
    p0, p1, p2 = p[fs[:, 0]], p[fs[:, 1]], p[fs[:, 2]]
    c = ecat([_ecross(p2 - p1, p0 - p1), _ecross(p0 - p2, p1 - p2), _ecross(p1 - p0, p2 - p0)], 0)
    vid = torch.cat([fs[:, 1], fs[:, 2], fs[:, 0]])
    z = torch.zeros(V, 3, dtype=torch.float64)
    cnt = torch.bincount(vid, minlength=V).double()
    g = (cnt - 1).clamp_min(0) * U
    g = (g / (1.0 - g)).unsqueeze(1)
    s = E(z.index_add(0, vid, c.v), z.index_add(0, vid, c.e) + g * z.index_add(0, vid, c.v.abs() + c.e))
    zero = ((s.v == 0) & (s.e == 0)).all(1)
    n = esqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    den = esel(zero, E(torch.ones(V, dtype=torch.float64)), n)
    assert bool((den.v - den.e > NORM_EPS).all())
    out = estack([s[:, k] / den for k in range(3)], 1)
    return esel(zero.unsqueeze(1), E(torch.zeros(V, 3, dtype=torch.float64)), out), n.v, zero


def make_grid_mesh(n=9, seed=0, amp=0.25):
    """A perturbed n x n grid in the plane z = 0, faces wound so that the normals point to +z: V = n^2, F = 2 (n-1)^2."""
    g = torch.Generator().manual_seed(300 + seed)
    ax = torch.linspace(-1, 1, n)
    Y, X = torch.meshgrid(ax, ax, indexing="ij")
    verts = torch.stack([X, Y, torch.zeros_like(X)], -1).reshape(-1, 3)
    verts = verts + (torch.rand(n * n, 3, generator=g) - 0.5) * torch.tensor([0.1, 0.1, 2 * amp])
    i = (torch.arange(n - 1).view(-1, 1) * n + torch.arange(n - 1).view(1, -1)).reshape(-1)
    faces = torch.cat([torch.stack([i, i + 1, i + n], 1), torch.stack([i + 1, i + n + 1, i + n], 1)])
    return verts.float(), faces.long()


def make_soup(V=700, F=1500, seed=0, loose=50):
    """A random triangle soup: repeated-index faces, a zero-length edge (two vertices at one position) and `loose` unreferenced
    vertices.  Returns verts, faces and the number of vertices the norm filter had to move (must be 0, or the seed changes)."""
    g = torch.Generator().manual_seed(400 + seed)
    verts = torch.randn(V, 3, generator=g)
    faces = torch.randint(0, V - loose, (F, 3), generator=g)
    faces[::97, 1] = faces[::97, 0]                                          # repeated indices
    faces[5::131, 2] = faces[5::131, 2 - 1]
    verts[faces[3, 1]] = verts[faces[3, 0]]                                  # a zero-length edge between distinct indices
    verts = verts.float()
    _, norm, zero = verts_normals(verts, faces)
    bad = ~zero & (norm < NORMAL_MIN)
    return verts, faces.long(), int(bad.sum())


def make_integer_mesh():
    """Small-integer coordinates; every vertex's summed normal is axis aligned with a power-of-two length (or zero)."""
    verts = torch.tensor([[0., 0., 0.], [2., 0., 0.], [0., 2., 0.], [2., 2., 0.],        # a square in z = 0: sums (0, 0, 4 k)
                          [0., 0., 1.], [0., 4., 1.], [0., 0., 5.], [7., 7., 7.],        # a triangle in x = 0: (16, 0, 0); 7: loose
                          [5., 1., 0.], [5., 1., 2.], [7., 1., 0.]])                    # a triangle in y = 1: (0, 4, 0)
    faces = torch.tensor([[0, 1, 2], [1, 3, 2], [4, 5, 6], [8, 9, 10], [0, 0, 3]])
    return verts, faces


# ----------------------------------------------------------------------------------------------------------------- phong
def phong_params(light_loc, shininess, light_amb=(0.4, 0.5, 0.3), light_diff=(0.3, 0.6, 0.5), light_spec=(0.2, 0.7, 0.4),
                 mat_amb=(1.0, 0.8, 0.9), mat_diff=(0.9, 1.0, 0.7), mat_spec=(0.6, 1.0, 0.8), background=(0.25, 0.5, 1.0)):
    """The 26 floats of the kernel's parameter block, in its order."""
    vals = list(light_loc) + list(light_amb) + list(light_diff) + list(light_spec) + list(mat_amb) + list(mat_diff) + list(mat_spec) \
        + [shininess] + list(background)
    return torch.tensor(vals, dtype=torch.float32)


def _enormalize(a, where):
    n = esqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
    assert bool(((n.v - n.e)[where] > NORM_EPS).all()), "a direction whose norm is not separated from eps"
    n = esel(where, n, E(torch.ones_like(n.v)))
    return estack([a[..., k] / n for k in range(3)], -1)


def epow(a, s, ulp=None):
    """pow(alpha, s) for alpha >= 0 and s = 0 or s >= 1 (module docstring)."""
    ulp = POWF_ULP if ulp is None else ulp
    assert s == 0.0 or s >= 1.0
    v = torch.pow(a.v, s)
    p = torch.zeros_like(v) if s == 0.0 else s * torch.pow(a.v + a.e, s - 1.0) * a.e
    e = p + 2.0 * ulp * U * (v.abs() + p) + TINY
    exact0 = (a.v == 0) & (a.e == 0)
    return E(v, torch.where(exact0, torch.zeros_like(e), e))


def phong(p2f, bary, verts, normals, colors, faces, cam_centers, params, parts=False, powf_ulp=None):
    """p2f [N,H,W] int64 packed (mesh * F + face), bary [N,H,W,3], verts / normals [N,V,3], colors [1 or N,V,3], faces [F,3],
    cam_centers [N,3], params [26] — all float32 inputs taken as exact.  Returns fg [N,H,W] (the pixels that are shaded: face in
    [0, N F) with all three indices inside [0, V)), rgb_on / rgb_off [N,H,W,3] (E: the colour with the switch [n.l > 0] on / off;
    the background where not fg), decided_on / undecided [N,H,W], and with parts=True also alpha (E, the switch on)."""
    N, V = verts.shape[:2]
    F = faces.shape[0]
    faces = faces.long()
    prm = f64(params)
    lloc, lamb, ldif, lspec = E(prm[0:3]), E(prm[3:6]), E(prm[6:9]), E(prm[9:12])
    mamb, mdif, mspec, s, bg = E(prm[12:15]), E(prm[15:18]), E(prm[18:21]), float(prm[21]), prm[22:25]
    face = p2f.long()
    fg = (face >= 0) & (face < N * F)
    fc = torch.where(fg, face, torch.zeros_like(face))
    m, f = fc // F, fc % F
    tri = faces[f]                                                           # [N,H,W,3]
    fg = fg & ((tri >= 0) & (tri < V)).all(-1)
    tri = torch.where(fg.unsqueeze(-1), tri, torch.zeros_like(tri))
    m = torch.where(fg, m, torch.zeros_like(m))
    w = E(f64(bary))
    cm = m if colors.shape[0] != 1 else torch.zeros_like(m)

    def interp(table, mesh):
        t = f64(table)
        a, b, c = (E(t[mesh, tri[..., k]]) for k in range(3))
        return (a * w[..., 0:1] + b * w[..., 1:2]) + c * w[..., 2:3]

    pt, nrm_raw, tex = interp(verts, m), interp(normals, m), interp(colors, cm)
    nrm = _enormalize(nrm_raw, fg)
    ldir = _enormalize(lloc - pt, fg)
    cosang = edot3(nrm, ldir)
    angle = erelu(cosang)
    cam = E(f64(cam_centers)[:, None, None, :])
    view = _enormalize(cam - pt, fg)
    refl = estack([(-ldir[..., k]) + (cosang * nrm[..., k]).scaled(2.0) for k in range(3)], -1)
    alpha_on = erelu(edot3(view, refl))
    alpha_off = E(torch.zeros_like(alpha_on.v))
    undecided = fg & (cosang.v.abs() <= cosang.e)
    decided_on = fg & ~undecided & (cosang.v > 0)
    bgE = E(bg.expand(fg.shape + (3,)))

    def colour(alpha):
        spec = epow(alpha, s, powf_ulp).map(lambda t: t.unsqueeze(-1))
        amb = mamb * lamb
        dif = mdif * (ldif * angle.map(lambda t: t.unsqueeze(-1)))
        spc = mspec * (lspec * spec)
        return esel(fg.unsqueeze(-1), (amb + dif) * tex + spc, bgE)

    out = {"fg": fg, "rgb_on": colour(alpha_on), "rgb_off": colour(alpha_off), "decided_on": decided_on, "undecided": undecided}
    if parts:
        out["alpha"] = alpha_on
        out["cosang"] = cosang
    return out


def phong_ratio(got_rgb, ref):
    """Largest error / bound over the image [N,H,W,3]: decided pixels against their branch, undecided ones against the nearer."""
    got = got_rgb.detach().cpu().double()
    r_on = (got - ref["rgb_on"].v).abs() / ref["rgb_on"].e.clamp_min(1e-300)
    r_on = torch.where((ref["rgb_on"].e == 0) & (got == ref["rgb_on"].v), torch.zeros_like(r_on), r_on)
    r_off = (got - ref["rgb_off"].v).abs() / ref["rgb_off"].e.clamp_min(1e-300)
    r_off = torch.where((ref["rgb_off"].e == 0) & (got == ref["rgb_off"].v), torch.zeros_like(r_off), r_off)
    on, und = ref["decided_on"].unsqueeze(-1), ref["undecided"]
    r = torch.where(on, r_on, r_off)
    both = torch.minimum(r_on.amax(-1), r_off.amax(-1)).unsqueeze(-1).expand_as(r)
    r = torch.where(und.unsqueeze(-1), both, r)
    r = torch.where(torch.isnan(got), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def make_fragments(N, H, W, F_valid, F_total, seed=0):
    """Host-built fragments: p2f [N,H,W] (frame n draws faces of mesh n; every 11th pixel is -1, every 13th is >= N F_total, every
    17th is the face F_total - 1, which the caller makes the one with a vertex index out of range) and barycentrics on the simplex
    with exact corners (1, 0, 0) mixed in."""
    g = torch.Generator().manual_seed(500 + seed)
    p2f = torch.randint(0, F_valid, (N, H, W), generator=g) + (torch.arange(N) * F_total).view(N, 1, 1)
    lin = torch.arange(N * H * W).view(N, H, W)
    p2f[lin % 17 == 4] = F_total - 1
    p2f[lin % 13 == 3] = N * F_total + 5
    p2f[lin % 11 == 2] = -1
    b = torch.rand(N, H, W, 3, generator=g) + 0.05
    b = b / b.sum(-1, keepdim=True)
    b[lin % 7 == 1] = torch.tensor([1.0, 0.0, 0.0])
    return p2f, b.float()


def make_sweep(side=256, seed=0):
    """One flat triangle in z = 0 with exact normals (0, 0, 1), light at (-1, 0, 1), camera at (1, 0, 1): alpha = v.r runs from 1 at
    the corner (0, 0, 0) down to 0 near x = sqrt 2.  side^2 pixels whose barycentrics spread alpha evenly over (0, 1]."""
    g = torch.Generator().manual_seed(600 + seed)
    verts = torch.tensor([[[0., 0., 0.], [1.4, 0.6, 0.], [1.4, -0.6, 0.]]])
    # on the line y = 0, alpha(x) = (2 - x^2) / sqrt(x^4 + 4): x^2 = 2 (1 - sqrt(1 - c^2)) / c with c = 1 - alpha^2 spreads alpha evenly
    target = 0.001 + 0.999 * torch.rand(side * side, generator=g, dtype=torch.float64)
    c = 1.0 - target * target
    t = torch.sqrt(2.0 * (1.0 - torch.sqrt(1.0 - c * c)) / c.clamp_min(1e-300)) / 1.4
    d = 0.6 * torch.rand(side * side, generator=g, dtype=torch.float64) - 0.3
    b = torch.stack([1.0 - t, t * (0.5 + d), t * (0.5 - d)], 1).view(1, side, side, 3).float()
    b[0, 0, 0] = torch.tensor([1.0, 0.0, 0.0])
    return {"verts": verts, "normals": torch.tensor([[[0., 0., 1.]] * 3]), "colors": torch.ones(1, 3, 3),
            "faces": torch.tensor([[0, 1, 2]]), "p2f": torch.zeros(1, side, side, dtype=torch.int64), "bary": b,
            "cam": torch.tensor([[1., 0., 1.]]), "light": (-1.0, 0.0, 1.0)}


def sweep_params(case, s):
    zero, one = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    return phong_params(case["light"], s, light_amb=zero, light_diff=zero, light_spec=one, mat_amb=zero, mat_diff=zero, mat_spec=one)


def sweep_alpha_float32(case):
    """The shader's alpha of the sweep, operation by operation in float32 (numpy arrays round every operation; the kernel is built
    without contraction and with correctly rounded division and sqrt): powf's exact argument, [side, side] float32."""
    f32 = np.float32
    w = case["bary"][0].numpy().astype(f32)
    w0, w1, w2 = w[..., 0], w[..., 1], w[..., 2]
    two, eps = f32(2), f32(NORM_EPS)

    def interp(t):
        a, b, c = (t[0, k].numpy().astype(f32) for k in range(3))
        return [(w0 * a[k] + w1 * b[k]) + w2 * c[k] for k in range(3)]

    def normalize(a):
        n = np.maximum(np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]), eps)
        return [a[k] / n for k in range(3)]

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    pt = interp(case["verts"])
    nrm = normalize(interp(case["normals"]))
    ldir = normalize([f32(case["light"][k]) - pt[k] for k in range(3)])
    cos = dot(nrm, ldir)
    view = normalize([case["cam"][0, k].numpy().astype(f32) - pt[k] for k in range(3)])
    refl = [-ldir[k] + two * (cos * nrm[k]) for k in range(3)]
    alpha = np.maximum(dot(view, refl), f32(0)) * (cos > 0).astype(f32)
    assert alpha.dtype == np.float32
    return torch.from_numpy(alpha)


def powf_error_ulp(got, alpha32, s):
    """The largest |got - alpha32^s| in units of 2 u |alpha32^s| (the F of the bound) over the pixels whose power is in the normal
    range, and their number."""
    v = torch.pow(alpha32.double(), s)
    live = (alpha32 > 0) & (v > 2.0 ** -100)
    err = (got.detach().cpu().double() - v).abs() / (2.0 * U * v).clamp_min(1e-300)
    return float(err[live].max()), int(live.sum())


def powf_needed_ulp(got, alpha, s):
    """The smallest F for which every pixel of the sweep (got [..] = powf(alpha_kernel, s)) is inside p + 2 F u (|v| + p) + TINY."""
    v = torch.pow(alpha.v, s)
    p = s * torch.pow(alpha.v + alpha.e, s - 1.0) * alpha.e
    err = (got.detach().cpu().double() - v).abs()
    need = ((err - p - TINY) / (2.0 * U * (v.abs() + p)).clamp_min(1e-300)).clamp_min(0)
    live = (alpha.v > 0) & (v > 2.0 ** -100)
    return float(need[live].max()), int(live.sum())


# ------------------------------------------------------------------------------------------------------------ compositor
def make_lists(shape, K, C, fused, seed=0, integer=False):
    """Packed, -1 terminated splat lists: idx int32 [N,H,W,K], alphas (or squared distances) float32 with NaN behind the lists,
    features [C,P], g_images [N,C,H,W], radius2 (0 when the alphas are given)."""
    N, H, W = shape
    npix = N * H * W
    g = torch.Generator().manual_seed(700 + 13 * npix + K + 100 * C + int(fused) + seed)
    P = max(3 * npix // 4, 7)
    length = torch.randint(0, K + 1, (npix,), generator=g)
    length[::5] = K
    length[1::7] = 0
    slot = torch.arange(K).view(1, K)
    live = slot < length.view(-1, 1)
    idx = torch.where(live, torch.randint(0, P, (npix, K), generator=g), torch.full((npix, K), -1)).to(torch.int32)
    radius2 = 0.0
    if integer:
        a = torch.randint(0, 3, (npix, K), generator=g).float() * 0.5
        feats = torch.randint(-3, 4, (C, P), generator=g).float()
        gim = torch.randint(-2, 3, (N, C, H, W), generator=g).float()
    else:
        a = 0.02 + 0.48 * torch.rand(npix, K, generator=g)
        if fused:
            radius2 = float(np.float32(0.05) * np.float32(0.05))
            a = 0.02 + 0.96 * torch.rand(npix, K, generator=g)                       # d / r^2
            a[torch.rand(npix, K, generator=g) < 0.05] = 0.0                         # a point on the pixel centre: a = 1 exactly
            a = (a * radius2).float()
        else:
            # at most one of each special value per list, so that cum stays far above the subnormal range
            special = torch.tensor([0.0, 0.999, 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -24, 1.0])
            for j in range(len(special)):
                pos = torch.randint(0, K, (npix,), generator=g)
                use = torch.rand(npix, generator=g) < (0.15 if j == 4 else 0.3)
                a[torch.arange(npix)[use], pos[use]] = special[j]
        feats = torch.randn(C, P, generator=g)
        gim = torch.randn(N, C, H, W, generator=g)
    alphas = torch.where(live, a.float(), torch.full((npix, K), float("nan")))
    assert int(idx.max()) < P
    return {"idx": idx.view(N, H, W, K), "alphas": alphas.view(N, H, W, K), "features": feats.float(), "g_images": gim.float(),
            "radius2": radius2, "P": P, "shape": shape, "K": K, "C": C}


def _alpha_E(c):
    """a [npix,K] (E) and the live mask; a = 0 exactly behind a list."""
    K = c["K"]
    live = c["idx"].reshape(-1, K) >= 0
    raw = torch.where(live, f64(c["alphas"]).reshape(-1, K), torch.zeros(live.shape, dtype=torch.float64))
    a = E(raw)
    if c["radius2"] != 0.0:
        # d = 0 gives 0 / r^2 = 0 and 1 - 0 = 1 without a rounding
        a = esel(raw == 0, E(torch.ones_like(raw)), 1.0 - a / E(torch.tensor(c["radius2"], dtype=torch.float64)))
    return esel(live, a, E(torch.zeros_like(raw))), live


def _gathered(c):
    """features of every slot [npix,K,C] and g_images per pixel [npix,C] in float64."""
    N, H, W = c["shape"]
    K, C = c["K"], c["C"]
    idx = c["idx"].reshape(-1, K).long().clamp_min(0)
    f = f64(c["features"]).t()[idx]                                          # [npix,K,C]
    g = f64(c["g_images"]).permute(0, 2, 3, 1).reshape(-1, C)
    return f, g


def composite_forward(c, trace=None):
    """images [N,C,H,W] (E)."""
    N, H, W = c["shape"]
    K, C = c["K"], c["C"]
    a, live = _alpha_E(c)
    f, _ = _gathered(c)
    npix = a.v.shape[0]
    cum, res = E(torch.ones(npix, 1, dtype=torch.float64)), E(torch.zeros(npix, C, dtype=torch.float64))
    for k in range(K):
        on = live[:, k:k + 1]
        ak = a[:, k:k + 1]
        res = esel(on, res + cum * ak * E(f[:, k]), res)
        cum = esel(on, cum * (1.0 - ak), cum)
        if trace is not None:
            trace.append(cum.v[on.expand_as(cum.v)])
    return res.map(lambda t: t.view(N, H, W, C).permute(0, 3, 1, 2))


def composite_backward_published(c):
    """The published double loop in float64, eps included: g_alphas [N,H,W,K] (d image / d a; for the fused mode times
    d a / d dist = -1 / r^2) — zero behind the lists."""
    N, H, W = c["shape"]
    K = c["K"]
    a, live = _alpha_E(c)
    a = a.v
    f, g = _gathered(c)
    Fk = (f * g.unsqueeze(1)).sum(-1) * live                                 # [npix,K]
    cum = torch.cat([torch.ones(a.shape[0], 1, dtype=torch.float64), torch.cumprod(1.0 - a, 1)[:, :-1]], 1)
    ga = cum * Fk
    for t in range(K):
        for k in range(t + 1, K):
            ga[:, t] -= Fk[:, k] * cum[:, k] * a[:, k] / (1.0 - a[:, t] + ALPHA_EPS)
    ga = ga * live
    if c["radius2"] != 0.0:
        ga = -ga / c["radius2"]
    return ga.view(N, H, W, K)


def composite_backward(c, trace=None, integer=False):
    """g_alphas [N,H,W,K] and g_features [C,P] as E: the published value with the bound of the kernel's recurrence.  The
    recurrence's own float64 value is returned as 'recurrence' for the CPU check that both are the same number.
    integer: the exact-integer case (alphas in {0, 0.5, 1}), where float32 rounds (1 - a) + eps to 1 - a, so that the quotient is
    exactly 1 (or 0 at a = 1) and every other step is exact: the value is the recurrence with that quotient."""
    N, H, W = c["shape"]
    K, C, P = c["K"], c["C"], c["P"]
    a, live = _alpha_E(c)
    f, g = _gathered(c)
    npix = a.v.shape[0]
    gE = E(g)
    Fs = []
    for k in range(K):
        prod = E(f[:, k]) * gE
        Fk = prod[:, 0]
        for ch in range(1, C):
            Fk = Fk + prod[:, ch]
        Fs.append(Fk)
    zero = E(torch.zeros(npix, dtype=torch.float64))
    Rs, R = [None] * K, zero
    for t in range(K - 1, -1, -1):
        on = live[:, t]
        Rs[t] = esel(on, R, zero)
        R = esel(on, Fs[t] * a[:, t] + (1.0 - a[:, t]) * R, R)
        if trace is not None:
            trace.append(R.v[on])
    cum, out = E(torch.ones(npix, dtype=torch.float64)), []
    gf_v, gf_e, gf_m = (torch.zeros(C, P, dtype=torch.float64) for _ in range(3))
    cnt = torch.zeros(P, dtype=torch.float64)
    idx = c["idx"].reshape(-1, K).long()
    for t in range(K):
        on = live[:, t]
        one_m = 1.0 - a[:, t]
        q = E((one_m.v > 0).double()) if integer else one_m / (one_m + ALPHA_EPS)
        ga = cum * (Fs[t] - Rs[t] * q)
        if c["radius2"] != 0.0:
            ga = (-ga) / E(torch.tensor(c["radius2"], dtype=torch.float64))
        out.append(esel(on, ga, zero))
        term = (cum * a[:, t]).map(lambda x: x.unsqueeze(1)) * gE              # [npix,C]
        rows = idx[on, t]
        gf_v.index_add_(1, rows, term.v[on].t())
        gf_e.index_add_(1, rows, term.e[on].t())
        gf_m.index_add_(1, rows, (term.v.abs() + term.e)[on].t())
        cnt.index_add_(0, rows, torch.ones(rows.shape[0], dtype=torch.float64))
        cum = esel(on, cum * one_m, cum)
    rec = estack(out, 1)
    pub = rec.v.view(N, H, W, K) if integer else composite_backward_published(c)
    gk = (cnt - 1).clamp_min(0) * U
    gk = gk / (1.0 - gk)
    return {"g_alphas": E(pub, rec.e.view(N, H, W, K)), "recurrence": rec.v.view(N, H, W, K), "g_features": E(gf_v, gf_e + gk * gf_m)}


def smallest_nonzero(tensors):
    vals = [t.abs()[t != 0].min() for t in tensors if bool((t != 0).any())]
    return float(min(vals)) if vals else math.inf


PHONG_LIGHTS = {"front": (0.5, 1.0, 2.5), "behind": (0.3, -0.5, -2.0)}
PHONG_IMAGE = (24, 40)
PHONG_WRAP = (64, 96, 96)


def make_phong_case(N=2, image=PHONG_IMAGE, copies=False, seed=0):
    """N perturbed 9 x 9 grids (copies: N times the same one) sharing one face table whose last face has a vertex index out of
    range, host-built fragments, per-vertex colours for one mesh and for N, one camera centre per frame."""
    H, W = image
    meshes = [make_grid_mesh(9, 0 if copies else k) for k in range(N)]
    verts = torch.stack([m[0] for m in meshes])
    V = verts.shape[1]
    faces = torch.cat([meshes[0][1], torch.tensor([[0, 1, V + 3]])])
    F = faces.shape[0]
    g = torch.Generator().manual_seed(800 + seed)
    colors = 0.2 + 0.8 * torch.rand(N, V, 3, generator=g)
    cams = torch.tensor([[0.2, -0.3, 3.0], [-0.5, 0.4, 2.5]])[torch.arange(N) % 2]
    if copies:
        base, bary = make_fragments(1, H, W, F - 1, F, seed)
        inside = (base >= 0) & (base < F)
        beyond = torch.where(base < 0, torch.full_like(base, -1), torch.full_like(base, N * F + 5)).expand(N, H, W)
        p2f = torch.where(inside.expand(N, H, W), base + (torch.arange(N) * F).view(N, 1, 1), beyond)
        bary, colors, cams = bary.expand(N, H, W, 3).contiguous(), colors[:1].expand(N, V, 3).contiguous(), cams[:1].expand(N, 3).contiguous()
    else:
        p2f, bary = make_fragments(N, H, W, F - 1, F, seed)
    return {"verts": verts, "faces": faces, "colors": colors, "cams": cams, "p2f": p2f, "bary": bary, "N": N, "V": V, "F": F,
            "H": H, "W": W}


def reference_normals(case):
    """float32 stand-ins for the kernel's normals (the CPU test has no kernel): the reference's own, rounded."""
    return torch.stack([verts_normals(v, case["faces"])[0].v for v in case["verts"]]).float()
