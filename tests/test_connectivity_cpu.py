"""recmv.connectivity without a GPU: the edge table, the boundary walks and the compaction on hand-sized meshes, read off by
hand or checked against the independent restatements the callers' tests already use (tests/icp_reference.py,
tests/mesh_topology_reference.py, the numpy edge count of test_lap_align_cpu.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE.parent / "rec-mv_amd")]

from recmv import align, connectivity as CN, curves  # noqa: E402
import icp_reference as IR  # noqa: E402
import mesh_topology_cases as TC  # noqa: E402
import mesh_topology_reference as TR  # noqa: E402
from test_lap_align_cpu import cut_sphere  # noqa: E402

TRIANGLE = [[0, 1, 2]]
SQUARE = [[0, 1, 2], [1, 3, 2]]                                         # two faces sharing the edge (1, 2)
STRIP = [[0, 2, 1], [2, 3, 1], [2, 4, 3], [4, 5, 3]]                    # six vertices, 0 2 4 below 1 3 5
FAN = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]]                      # vertex 0 is interior
FIN = [[0, 1, 2], [1, 0, 3], [0, 1, 4]]                                 # three faces on the edge (0, 1)
BOWTIE = [[0, 1, 2], [2, 3, 4]]                                         # two triangles that share vertex 2 only
BOTH_WAYS = [[0, 1, 2], [0, 1, 3], [1, 0, 4], [4, 0, 5]]                # (0, 1) twice forward and once back; (0, 4) both ways


def _meshes():
    """{name: (faces int64 [F,3] tensor, V)}: the meshes of every test here and of test_gpu_connectivity.py."""
    out = {name: (np.array(f, np.int64), int(np.max(f)) + 1) for name, f in (
        ("triangle", TRIANGLE), ("square", SQUARE), ("strip", STRIP), ("tetrahedron", TC.TETRA_F), ("fan", FAN), ("fin", FIN),
        ("bow-tie", BOWTIE), ("both ways", BOTH_WAYS))}
    out["tube"] = (TC.tube()[1], len(TC.tube()[0]))
    two = TC.merge(TC.tube(), TC.tube(n=7, m=3))
    out["two tubes"] = (two[1], len(two[0]) + 2)                        # and two vertices that no face uses
    v, f = cut_sphere(2, caps=('neck',))
    out["cut icosphere"] = (f.numpy(), v.shape[0])
    out["no faces"] = (np.zeros((0, 3), np.int64), 5)
    return {k: (torch.from_numpy(np.ascontiguousarray(f)), V) for k, (f, V) in out.items()}


MESHES = _meshes()
NAMES = sorted(MESHES)


def _verts(V):
    return np.random.default_rng(V).random((V, 3)).astype(np.float32)


def _numpy_border(f, V):
    """(border edges as a set of (lo, hi), bool [V] border vertices) by numpy's row count, as test_lap_align_cpu.py counts."""
    f = f.numpy()
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    uniq, cnt = np.unique(edges, axis=0, return_counts=True)
    border = uniq[cnt == 1]
    mask = np.zeros(V, bool)
    mask[border.reshape(-1)] = True
    return {tuple(e) for e in border.tolist()}, mask


def test_tables_read_off_by_hand():
    t = CN.EdgeTable(torch.tensor(TRIANGLE), 3)
    assert t.edges.tolist() == [[0, 1], [0, 2], [1, 2]] and t.face_to_edge.tolist() == [[2, 1, 0]]
    assert t.count.tolist() == [1, 1, 1] and t.boundary_edge.all() and t.boundary_vertex.all() and not t.nonmanifold_edge.any()
    assert t.forward.tolist() == [[True, False, True]]                  # 1 -> 2, 2 -> 0, 0 -> 1
    t = CN.EdgeTable(torch.tensor(SQUARE), 5)                           # vertex 4: no face uses it
    assert t.edges.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]] and t.count.tolist() == [1, 1, 2, 1, 1]
    assert t.face_to_edge.tolist() == [[2, 1, 0], [4, 2, 3]]
    assert t.boundary_edge.tolist() == [True, True, False, True, True] and t.boundary_vertex.tolist() == [True] * 4 + [False]
    t = CN.EdgeTable(torch.tensor(TC.TETRA_F), 4)
    assert t.E == 6 and (t.count == 2).all() and not t.boundary_vertex.any()
    t = CN.EdgeTable(torch.tensor(FAN), 5)
    assert t.boundary_vertex.tolist() == [False, True, True, True, True] and int(t.boundary_edge.sum()) == 4
    t = CN.EdgeTable(torch.tensor(FIN), 5)
    assert t.edges[0].tolist() == [0, 1] and t.count.tolist() == [3, 1, 1, 1, 1, 1, 1]
    assert t.nonmanifold_edge.tolist() == [True] + [False] * 6 and t.boundary_edge.tolist() == [False] + [True] * 6
    t = CN.EdgeTable(torch.tensor(BOTH_WAYS), 6)
    ahead = torch.zeros(t.E, dtype=torch.int64).index_add_(0, t.face_to_edge.reshape(-1), t.forward.reshape(-1).long())
    use = {tuple(e): (int(c), int(a)) for e, c, a in zip(t.edges.tolist(), t.count, ahead)}
    assert use[(0, 1)] == (3, 2) and use[(0, 4)] == (2, 1)              # (faces, of them lower -> higher)
    for name, V in (("no faces", 5), ("no faces", 0)):
        t = CN.EdgeTable(MESHES[name][0], V)
        assert t.edges.shape == (0, 2) and t.face_to_edge.shape == (0, 3) and t.forward.shape == (0, 3)
        assert t.count.shape == t.boundary_edge.shape == t.nonmanifold_edge.shape == (0,) and t.boundary_vertex.tolist() == [False] * V


@pytest.mark.parametrize("name", NAMES)
def test_edge_table_equals_the_restatements(name):
    f, V = MESHES[name]
    t = CN.EdgeTable(f, V)
    e, f2e = CN.edges_packed(f, V)
    assert torch.equal(t.edges, e) and torch.equal(t.face_to_edge, f2e) and (e[:, 0] <= e[:, 1]).all()
    for k in range(3):                                                  # column k: the edge opposite corner k, and its direction
        a, b = f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        assert torch.equal(e[f2e[:, k]], torch.stack([torch.minimum(a, b), torch.maximum(a, b)], 1))
        assert torch.equal(t.forward[:, k], a < b)
    border, mask = _numpy_border(f, V)
    assert {tuple(x) for x in e[t.boundary_edge].tolist()} == border
    assert np.array_equal(t.boundary_vertex.numpy(), mask)
    assert torch.equal(t.boundary_edge, t.count == 1) and torch.equal(t.nonmanifold_edge, t.count > 2)
    want = TR.report(_verts(V), f.numpy())
    ahead = torch.zeros(t.E, dtype=torch.int64).index_add_(0, f2e.reshape(-1), t.forward.reshape(-1).long())
    got = (t.E, int(t.boundary_edge.sum()), int(t.nonmanifold_edge.sum()), int(((t.count == 2) & (ahead != 1)).sum()))
    assert got == (want['edges'], want['boundary_edges'], want['nonmanifold_edges'], want['orientation_conflicts'])
    assert np.array_equal(align.border_flags(f, V).numpy(), IR.border_flags(f.numpy(), V))


@pytest.mark.parametrize("name", NAMES)
def test_compact_equals_the_reference_map(name):
    f, V = MESHES[name]
    v = torch.from_numpy(_verts(V + 1))                                 # the last vertex: never used
    for faces in (f, f[1::2]):                                          # and with every other face gone
        want_v, want_f, _, want_map, _, _ = TR.keep_components(v.numpy(), faces.numpy())
        got_v, got_f, got_map = CN.compact(v, faces)
        assert got_map.dtype == torch.int64 and np.array_equal(got_map.numpy(), want_map) and got_map[-1] == -1
        assert np.array_equal(got_v.numpy().view(np.uint32), want_v.view(np.uint32)) and np.array_equal(got_f.numpy(), want_f)


def test_boundary_loops_walk_order():
    BL = CN.boundary_loops
    assert BL(torch.tensor(TRIANGLE)) == [[0, 1, 2]] and BL(torch.tensor(SQUARE)) == [[0, 1, 3, 2]]
    assert BL(np.array(STRIP)) == [[0, 1, 3, 5, 4, 2]] and BL(FAN, 5) == [[1, 2, 3, 4]]
    assert BL(torch.tensor(TC.TETRA_F)) == [] and BL(torch.zeros(0, 3, dtype=torch.int64)) == []
    assert BL(torch.tensor(BOWTIE)) == [[0, 1, 2], [2, 3, 4]]           # the touching vertex is in both
    # a pinch that is not a start: the walk takes its lowest unwalked neighbour and passes it twice
    assert BL(torch.tensor([[0, 1, 9], [0, 9, 5], [9, 3, 4]])) == [[0, 1, 9, 3, 4, 9, 5]]
    for name in NAMES:
        f, V = MESHES[name]
        loops = BL(f, V)
        border, mask = _numpy_border(f, V)
        walked = [(min(a, b), max(a, b)) for loop in loops for a, b in zip(loop, loop[1:] + loop[:1])]
        if not CN.EdgeTable(f, V).nonmanifold_edge.any():               # (else a vertex has three border edges and walks end open)
            assert sorted(walked) == sorted(border)
        assert sorted({i for loop in loops for i in loop}) == np.nonzero(mask)[0].tolist()
        assert [loop[0] for loop in loops] == sorted(loop[0] for loop in loops)
        assert all(loop[0] == min(loop) for loop in loops)
    assert len(BL(*MESHES["tube"])) == 2 and len(BL(*MESHES["two tubes"])) == 4 and len(BL(*MESHES["cut icosphere"])) == 1


def test_longest_boundary_loop_is_the_longer_walk():
    v, f = cut_sphere(2, caps=('neck', 'upper_bottom'), h=0.6)
    f = f[(f != int(v[:, 1].abs().argmin())).all(1)]                    # and a hole around a vertex of the equator: three loops
    assert len(CN.boundary_loops(f)) == 3
    with pytest.raises(AssertionError, match="has two boundary loops, found 3"):
        curves.longest_boundary_loop(f)
    with pytest.raises(AssertionError, match="every boundary vertex has two boundary edges"):
        curves.longest_boundary_loop(torch.tensor(BOWTIE))
    with pytest.raises(AssertionError, match="has two boundary loops, found 0"):
        curves.longest_boundary_loop(torch.tensor(TC.TETRA_F))
    tube = MESHES["tube"][0]
    assert curves.longest_boundary_loop(tube) == CN.boundary_loops(tube)[1]        # equal lengths: the second
    notched = torch.from_numpy(TC.tube(n=9, m=3)[1])[1:]                # without a face of one rim: that rim has 10 edges now
    loops = CN.boundary_loops(notched)
    assert sorted(len(l) for l in loops) == [9, 10]
    assert curves.longest_boundary_loop(notched) == max(loops, key=len)


def test_range_and_dtype_errors():
    with pytest.raises(ValueError, match=r"a face index lies outside \[0, 3\)"):
        CN.EdgeTable(torch.tensor([[0, 1, 7]]), 3)
    with pytest.raises(ValueError, match=r"a face index lies outside \[0, 3\)"):
        CN.EdgeTable(torch.tensor([[0, -1, 2]]), 3)
    with pytest.raises(ValueError, match="faces must be int64"):
        CN.EdgeTable(torch.tensor([[0, 1, 2]], dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="faces must be int64"):
        CN.EdgeTable(torch.tensor([0, 1, 2]), 3)
    with pytest.raises(ValueError, match="outside"):
        CN.boundary_loops(torch.tensor(SQUARE), 3)
