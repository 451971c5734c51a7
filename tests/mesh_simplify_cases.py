"""The meshes of the simplification tests and the invariants both drivers must keep (tests/test_mesh_simplify_cpu.py runs the
float64 torch path on CPU tensors, tests/test_gpu_mesh_simplify.py the kernel path).  numpy; float32 vertices, int64 faces."""
import numpy as np

import mesh_topology_cases as TC


def bumpy_sphere():
    """1 280 faces, closed, genus 0, every vertex pushed in or out."""
    from test_gpu_animation import _irregular_body
    v, f = _irregular_body(level=3)
    return v.numpy().astype(np.float32), f.numpy().astype(np.int64)


def torus():
    return TC.torus(24, 12)                                # 24 x 12 quads, 576 faces


def tube():
    return TC.tube(16, 9)                                  # 16 x 8 quads, 256 faces, two boundary loops of 16 edges


def flat_grid(n=9):
    """(n - 1)^2 quads in the plane z = 0 with integer coordinates (n = 9: 128 faces)."""
    v = np.array([[i, j, 0] for j in range(n) for i in range(n)], np.float32)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            f += [[a, a + 1, a + n + 1], [a, a + n + 1, a + n]]
    return v, np.array(f, np.int64)


def fan(n=200, seed=3):
    """n triangles round hub 0 (closed: the hub is interior), the rim on a bumpy circle."""
    g = np.random.default_rng(seed)
    t = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(t), np.sin(t), 0.1 * g.standard_normal(n)], 1)
    v = np.concatenate([[[0, 0, 0.3]], rim]).astype(np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int64)
    return v, f


def area(v, f):
    v = v.astype(np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum()


def border_edges(f):
    use = {}
    for row in f:
        for i in range(3):
            a, b = int(row[i]), int(row[(i + 1) % 3])
            use[(min(a, b), max(a, b))] = use.get((min(a, b), max(a, b)), 0) + 1
    return np.array([e for e, n in sorted(use.items()) if n == 1], np.int64).reshape(-1, 2)


def distance_to_polyline(p, v, segments):
    """The distance of every point p [N,3] to the nearest of the segments [S,2] of v, float64."""
    p = p.astype(np.float64)[:, None]
    a, b = v[segments[:, 0]].astype(np.float64)[None], v[segments[:, 1]].astype(np.float64)[None]
    ab = b - a
    t = np.clip(((p - a) * ab).sum(-1) / (ab * ab).sum(-1), 0., 1.)
    return np.linalg.norm(a + t[..., None] * ab - p, axis=-1).min(1)


def check_sphere(v, f, info, report):
    r = report(v, f)
    assert len(f) in (320, 321) and info['faces_after'] == len(f) and info['stopped'] == 'target', info
    assert r['components_vertex'] == 1 and r['watertight'] and r['euler_characteristic'] == 2 and r['nonmanifold_edges'] == 0, r
    assert info['faces_before'] == 1280 and info['vertices_before'] == 642 and info['vertices_after'] == len(v)
    assert info['collapses'] == 642 - len(v) and info['rounds'] >= 1 and 0 < info['max_error'] and 0 < info['max_cost']


def check_torus(v, f, info, report):
    r = report(v, f)
    assert len(f) in (144, 145) and info['stopped'] == 'target', info
    assert r['components'][0]['genus'] == 1 and r['watertight'] and r['euler_characteristic'] == 0 and r['nonmanifold_edges'] == 0, r


def check_tube(v, f, info, report, v_in, f_in, target):
    r = report(v, f)
    assert len(f) in (target, target + 1) and info['stopped'] == 'target', info
    assert r['boundary_loops'] == 2 and r['components_vertex'] == 1 and r['nonmanifold_edges'] == 0, r
    assert r['boundary_pinch_vertices'] == 0 and r['components'][0]['genus'] == 0
    be = border_edges(f)
    assert len(be) >= 6                                     # two loops of at least 3 edges each ...
    from recmv.connectivity import boundary_loops
    for loop in boundary_loops(f):
        assert len(loop) >= 3
    on = np.unique(be)
    d = distance_to_polyline(v[on], v_in, border_edges(f_in))
    assert d.max() <= 1e-12, d.max()                       # ... whose vertices never left the input's boundary polyline


def check_flat_grid(v, f, info, report, v_in, f_in):
    r = report(v, f)
    assert len(f) in (16, 17) and info['stopped'] == 'target', info
    assert (v[:, 2] == 0).all()
    assert abs(area(v, f) - area(v_in, f_in)) <= 1e-6 * area(v_in, f_in)
    have = {tuple(p) for p in v.tolist()}
    for corner in ((0., 0., 0.), (8., 0., 0.), (0., 8., 0.), (8., 8., 0.)):
        assert corner in have, (corner, sorted(have))
    assert r['components_vertex'] == 1 and r['boundary_loops'] == 1 and r['nonmanifold_edges'] == 0 and r['zero_area_faces'] == 0


def quality_figures(device, samples=20000, seed=0):
    """The quality comparison of tests/test_gpu_mesh_simplify.py, also recorded by tools/mesh_simplify_timing.py: on the bumpy
    sphere, metrics.surface_distance (fixed samples and seed) of the result against the input for recmv.simplify at 320 faces
    (kernel path) and for the serial greedy reference at 160 faces — one halving of the face budget is what choosing
    collapses in independent sets rather than in strict cost order may cost."""
    import torch
    import mesh_simplify_reference as SR
    from recmv import metrics, simplify
    v, f = bumpy_sphere()
    tv, tf = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
    pv, pf, info = simplify.simplify(tv, tf, target_faces=320)
    gv, gf, _ = SR.greedy_simplify(v, f, 160, simplify.BOUNDARY_WEIGHT, simplify.REACH)
    parallel = metrics.surface_distance(pv, pf, tv, tf, samples=samples, seed=seed)
    serial = metrics.surface_distance(torch.from_numpy(gv).to(device), torch.from_numpy(gf).to(device), tv, tf, samples=samples,
                                      seed=seed)
    return {'mesh': 'bumpy sphere, 1280 faces', 'samples': samples, 'seed': seed,
            'parallel_faces': int(pf.shape[0]), 'parallel_chamfer_l1': parallel['chamfer_l1'], 'parallel_rounds': info['rounds'],
            'serial_greedy_faces': int(gf.shape[0]), 'serial_greedy_chamfer_l1': serial['chamfer_l1']}
