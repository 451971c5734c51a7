"""recmv_closest_point_grid (recmv.metrics.MeshGrid) on the GPU.

Primary judge: recmv_closest_point, bit for bit in face, point and dist2 — both kernels run closest_tri.h on (a, b - a,
c - a) as load_tri forms it and take an order-independent minimum on (distance, face id), so equality is required, not a
tolerance.  Every launch shape (1, 8 and 64 lanes per query, queries sorted by cell or not) must give those bits.

Second judge: the float64 search of tests/collide_reference.py with the bound tests/test_gpu_animation.py derives for this
point-triangle routine, BOUND_D2 = 16 eps32 (d + Lmax)^2 (d the distance, Lmax the longest edge).
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import collide_reference as CR  # noqa: E402
import mesh_metrics_reference as MR  # noqa: E402
from test_gpu_animation import _bound_d2, _irregular_body, _longest_edge  # noqa: E402
from test_nricp_cpu import icosphere  # noqa: E402

DEV = "cuda:0"
SHAPES = ((1, False), (1, True), (8, True), (64, False), (64, True))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _check(p, v, f, shapes=SHAPES, **grid):
    """The grid query of every launch shape against the brute force on the same arrays; returns (grid, brute result)."""
    from recmv import metrics
    from recmv.iso_remesh import closest_point
    p, v, f = p.to(DEV), v.to(DEV), f.to(DEV)
    brute = closest_point(p, v, f)
    g = metrics.MeshGrid(v, f, **grid)
    for lanes, sort in shapes:
        got = g.closest_point(p, lanes=lanes, sort=sort)
        assert got[0].dtype == torch.int64 and got[1].shape == (p.shape[0], 3) and got[2].dtype == torch.float32
        bad = (got[0] != brute[0]) | (_bits(got[2]) != _bits(brute[2])) | (_bits(got[1]) != _bits(brute[1])).any(1)
        assert not bool(bad.any()), (lanes, sort, g.dims, int(bad.sum()), p[bad][:3].tolist(), got[0][bad][:3].tolist(),
                                     brute[0][bad][:3].tolist())
    return g, brute


def _level3_queries(v, f, origin, h, dims):
    """About 4 000 queries around the irregular level-3 icosphere: inside, near the surface and outside; far outside the
    box; exactly on vertices and edge midpoints; exactly on cell boundaries and on the grid's corners."""
    g = torch.Generator().manual_seed(5)
    lo, hi = v.amin(0), v.amax(0)
    diag = float((hi - lo).norm())
    centre = 0.5 * (lo + hi)
    parts = [torch.randn(1200, 3, generator=g) * 0.3,                                       # inside and outside
             v[torch.randint(0, v.shape[0], (1200,), generator=g)] * (1 + 0.04 * torch.randn(1200, 1, generator=g))]
    axes = torch.cat([torch.eye(3), -torch.eye(3)])
    corners = torch.tensor([[x, y, z] for x in (-1., 1.) for y in (-1., 1.) for z in (-1., 1.)]) / 3 ** 0.5
    parts.append(centre + 10 * diag * torch.cat([axes, corners]))                           # 10 diagonals away
    parts.append(centre + 1.5 * diag * torch.cat([axes, corners]))
    parts.append(v)                                                                          # on the vertices (642)
    e = torch.cat([f[:300, [0, 1]], f[300:600, [1, 2]]])
    parts.append(0.5 * (v[e[:, 0]] + v[e[:, 1]]))                                            # edge midpoints (600)
    o = torch.tensor(origin, dtype=torch.float32)
    n = torch.tensor(dims, dtype=torch.float32)
    lattice = torch.stack([torch.randint(0, d + 1, (300,), generator=g) for d in dims], 1).float()
    parts.append(o + lattice * h)                                                            # cell corners
    half = lattice.clone()
    half[:, 0] += 0.37                                                                       # on cell faces, off the corners
    parts.append(o + half * h)
    parts.append(o + torch.tensor([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)]) * n * h)
    return torch.cat(parts).float().contiguous()


@pytest.fixture(scope="module")
def level3():
    from recmv import metrics
    v, f = _irregular_body(level=3)
    g = metrics.MeshGrid(v.to(DEV), f.to(DEV))
    p = _level3_queries(v, f, list(g.origin), g.cell_size, g.dims)
    return v, f, p


def test_grid_equals_brute_force_on_an_irregular_icosphere(level3):
    v, f, p = level3
    assert f.shape[0] == 1280 and 3900 <= p.shape[0] <= 4300
    g, brute = _check(p, v, f)
    assert min(g.dims) > 1 and g.n_entries >= f.shape[0]
    # on a vertex the distance is an exact zero and the face is the lowest of those around it
    on = slice(2428, 2428 + v.shape[0])
    assert torch.equal(p[on], v)
    assert bool((brute[2][on] == 0).all())
    lowest = torch.full((v.shape[0],), f.shape[0], dtype=torch.int64).scatter_reduce(
        0, f.reshape(-1), torch.arange(f.shape[0]).repeat_interleave(3), "amin")
    assert torch.equal(brute[0][on].cpu(), lowest)


def test_grid_against_the_float64_search(level3):
    from recmv import metrics
    v, f, p = level3
    face, _, d2 = metrics.MeshGrid(v.to(DEV), f.to(DEV)).closest_point(p.to(DEV))
    face, d2 = face.cpu().numpy(), d2.cpu().double().numpy()
    ref_face, ref_d2 = MR.nearest(p.numpy(), v.numpy(), f.numpy())
    bound = _bound_d2(ref_d2, _longest_edge(v, f))
    err = np.abs(d2 - ref_d2)
    print("largest |d2 error| / bound %.3g" % float((err / bound).max()))
    assert (err <= bound).all(), (float(err.max()), float(bound[err.argmax()]))
    vv, tri = v.double().numpy(), f.numpy()[face]
    d_named, _ = CR.closest_on_triangle(p.double().numpy(), vv[tri[:, 0]], vv[tri[:, 1]], vv[tri[:, 2]])
    assert (d_named <= ref_d2 + bound).all()               # the face named is a valid argmin


def test_one_huge_triangle_among_many_tiny_ones():
    """The huge triangle's box is the whole grid: it sits in every cell (spread over a wave by the build), and a query is
    answered by it or by a tiny face several rings away."""
    sv, sf = icosphere(2)
    v = torch.cat([torch.tensor([[-1., -1., -1.], [1., -1., 1.], [-1., 1., 1.]]), 0.15 * sv + torch.tensor([0.7, 0.7, -0.6])])
    f = torch.cat([torch.tensor([[0, 1, 2]]), sf + 3, torch.tensor([[0, 1, 2]])]).contiguous()
    g = torch.Generator().manual_seed(1)
    p = torch.cat([(torch.rand(700, 3, generator=g) * 3 - 1.5), v[3:] * 1.02, v[:3]]).contiguous()
    grid, brute = _check(p, v.contiguous(), f)
    assert bool((grid.counts >= 2).all())                  # both copies of the huge face in every cell
    grid, _ = _check(p, v.contiguous(), f, shapes=((1, True), (64, False)), dims=(12, 12, 12))   # 1 728 cells: the wave path
    assert bool((grid.counts >= 2).all()) and int(grid.counts.sum()) == grid.n_entries
    assert int(brute[0].max()) < f.shape[0] - 1            # the copy never wins over face 0


def test_a_planar_mesh_has_one_cell_along_its_normal():
    v64, f = MR.square(0.25, n=12)
    g = torch.Generator().manual_seed(2)
    v = torch.from_numpy(v64).float()
    v[:, :2] += 0.02 * (torch.rand(v.shape[0], 2, generator=g) - 0.5)
    p = torch.cat([torch.rand(500, 3, generator=g) * 2 - 0.5, v, torch.cat([torch.rand(200, 2, generator=g),
                                                                            torch.full((200, 1), 0.25)], 1)]).contiguous()
    grid, _ = _check(p, v.contiguous(), torch.from_numpy(f))
    assert grid.dims[2] == 1 and grid.dims[0] > 1 and grid.dims[1] > 1


@pytest.mark.parametrize("faces", [[[0, 1, 2]], [[0, 1, 2], [2, 1, 3]]])
def test_tiny_meshes(faces):
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.2], [0., 1., 0.], [1., 1., 1.]])
    g = torch.Generator().manual_seed(3)
    p = torch.cat([torch.randn(300, 3, generator=g), v]).contiguous()
    _check(p, v, torch.tensor(faces))


@pytest.mark.parametrize("dims", [(1, 1, 1), (40, 40, 40), (1, 57, 3)])
def test_forced_grids(dims):
    """One cell for everything; a grid so fine that most cells are empty (the rings run far before they meet a face); an
    uneven one."""
    v, f = _irregular_body(level=2)
    if dims == (40, 40, 40):
        f = f[:2]                                          # two faces in 64 000 cells
    g = torch.Generator().manual_seed(4)
    p = torch.cat([torch.randn(250, 3, generator=g) * 0.4, v[:50]]).contiguous()
    grid, _ = _check(p, v, f.contiguous(), shapes=((1, True), (64, False)), dims=dims)
    assert grid.dims == dims


def test_duplicate_degenerate_and_invalid_faces():
    """Duplicated faces (the lower id wins), faces without area, and faces with an index outside the mesh (skipped) mixed in:
    the result equals the brute force on the same arrays."""
    v, f = _irregular_body(level=2)
    V, F = v.shape[0], f.shape[0]
    dup = f[[3, 50, 200, 319]]
    flat = torch.tensor([[5, 5, 9], [7, 11, 11], [4, 4, 4]])
    a, b = v[20], v[21]
    v = torch.cat([v, (0.5 * (a + b))[None]])                                        # a vertex on an edge: a collinear face
    flat = torch.cat([flat, torch.tensor([[20, 21, V]])])
    bad = torch.tensor([[0, 1, V + 1], [-1, 2, 3], [V + 7, V + 8, V + 9]])
    faces = torch.cat([f[:100], bad[:1], dup[:2], f[100:], flat, bad[1:], dup[2:]]).contiguous()
    g = torch.Generator().manual_seed(6)
    p = torch.cat([torch.randn(600, 3, generator=g) * 0.4, v]).contiguous()
    grid, brute = _check(p, v.contiguous(), faces)
    face = brute[0].cpu()
    assert int(face.min()) >= 0
    named = faces[face]
    assert bool(((named >= 0) & (named < v.shape[0])).all())                            # an invalid face is never named
    first = {tuple(t): i for i, t in reversed(list(enumerate(faces.tolist())))}          # the first copy of every triple
    assert all(first[tuple(t)] == i for i, t in zip(face.tolist(), named.tolist()))


def test_no_query_and_one_query(level3):
    from recmv import metrics
    from recmv.iso_remesh import closest_point
    v, f, p = level3
    g = metrics.MeshGrid(v.to(DEV), f.to(DEV))
    face, point, d2 = g.closest_point(torch.zeros(0, 3, device=DEV))
    assert face.shape == (0,) and point.shape == (0, 3) and d2.shape == (0,)
    for lanes in (1, 8, 64):
        one = p[7:8].to(DEV)
        assert _same(g.closest_point(one, lanes=lanes), closest_point(one, v.to(DEV), f.to(DEV)))
    with pytest.raises(ValueError):
        metrics.MeshGrid(v.to(DEV), f[:0].to(DEV))


def test_the_query_is_reproducible_whatever_the_entry_order(level3):
    """The order of a cell's entries follows an integer cursor and may change from build to build; the result may not."""
    from recmv import metrics
    v, f, p = level3
    v, f, p = v.to(DEV), f.to(DEV), p.to(DEV)
    g1 = metrics.MeshGrid(v, f)
    a = g1.closest_point(p)
    assert _same(a, g1.closest_point(p))
    g2 = metrics.MeshGrid(v, f)
    assert _same(a, g2.closest_point(p))
    assert torch.equal(g1.offsets, g2.offsets) and g1.n_entries == g2.n_entries == int(g1.offsets[-1])
    # both builds hold the same faces in every cell
    cell = torch.repeat_interleave(torch.arange(g1.offsets.shape[0] - 1, device=DEV), g1.counts.long())
    key1 = torch.sort(cell * f.shape[0] + g1.entries[:g1.n_entries].long())[0]
    key2 = torch.sort(cell * f.shape[0] + g2.entries[:g2.n_entries].long())[0]
    assert torch.equal(key1, key2) and bool((key1[1:] > key1[:-1]).all())


def test_poisoned_workspaces_are_written_before_they_are_read(monkeypatch):
    """RECMV_POISON=1 reaches L.workspace (0xff bytes, NaN for float64), and a grid build and query on the smallest mesh that has
    a grid give the same tensors with it as without: every buffer they allocate is written before it is read."""
    import mesh_topology_cases as TC
    from recmv import _lib as L
    from recmv import metrics
    v, f = (torch.from_numpy(x).to(DEV) for x in TC.tetrahedron())
    p = torch.tensor([[0.1, 0.2, 0.3], [2., -1., 0.5], [0.25, 0.25, 0.25], [-3., -3., -3.]], device=DEV)

    def run():
        g = metrics.MeshGrid(v, f)
        return (g.offsets, g.tris, g.counts) + tuple(g.closest_point(p))
    monkeypatch.delenv("RECMV_POISON", raising=False)
    plain = run()
    monkeypatch.setenv("RECMV_POISON", "1")
    dev = torch.device(DEV)
    assert bool((L.workspace(64, dev, "t") == 0xff).all()) and L.workspace(64, dev, "t").shape == (64,)
    ws = L.workspace(64, dev, "t", dtype=torch.float64)
    assert ws.shape == (8,) and bool(torch.isnan(ws).all())
    poisoned = run()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(plain, poisoned))
    assert not bool(torch.isnan(poisoned[4]).any()) and not bool(torch.isnan(poisoned[5]).any())
