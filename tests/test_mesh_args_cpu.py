"""The shared argument checks of the mesh toolkit (recmv.mesh_args), connectivity.filed_slots_csr and L.workspace's refusal,
without a GPU.
"""
import json
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import mesh_topology_cases as TC  # noqa: E402


def _tetra():
    return tuple(torch.from_numpy(x) for x in TC.tetrahedron())


# ---- check_mesh -------------------------------------------------------------------------------------------------------------------
def test_check_mesh_returns_the_contiguous_pair():
    from recmv.mesh_args import check_mesh
    v, f = _tetra()
    assert v.shape == (4, 3) and f.shape == (4, 3)
    cv, cf = check_mesh(v, f, cuda=False)
    assert cv is v and cf is f                                                     # contiguous already: nothing is copied
    vv = v[:, [2, 1, 0]].t().contiguous().t()                                      # the columns swapped, strides (1, 4)
    wide = torch.cat([f, f], 1).t().contiguous().t()                               # [4,6] with strides (1, 4)
    ff = wide[:, :3]                                                               # transposed, then sliced
    assert not vv.is_contiguous() and not ff.is_contiguous()
    cv, cf = check_mesh(vv, ff, cuda=False)
    assert cv.is_contiguous() and cf.is_contiguous()
    assert torch.equal(cv, v[:, [2, 1, 0]]) and torch.equal(cf, f)


def test_check_mesh_wants_cuda_tensors_by_default():
    from recmv.mesh_args import check_mesh
    v, f = _tetra()
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        check_mesh(v, f)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        check_mesh(v, f, cuda=True)


def test_check_mesh_names_every_single_fault():
    from recmv.mesh_args import check_mesh
    v, f = _tetra()
    for bad_v, bad_f, text in ((v.numpy(), f, "verts and faces must be tensors"),
                               (v.double(), f, r"verts must be float32 of shape \[V,3\]"),
                               (v[:, :2], f, r"verts must be float32 of shape \[V,3\]"),
                               (v, f.int(), r"faces must be int64 of shape \[F,3\]"),
                               (v, torch.cat([f, f[:, :1]], 1), r"faces must be int64 of shape \[F,3\]")):
        with pytest.raises(ValueError, match=text):
            check_mesh(bad_v, bad_f, cuda=False)
    for bad_v, bad_f in ((v, f[:0]), (v[:0], f)):
        with pytest.raises(ValueError, match="the surface is empty"):
            check_mesh(bad_v, bad_f, cuda=False, allow_empty=False)
        assert check_mesh(bad_v, bad_f, cuda=False)[1].shape == bad_f.shape        # allowed by default
    with pytest.raises(ValueError, match="must be on one device"):
        check_mesh(v, f.to("meta"), cuda=False)


def test_check_mesh_float_verts_and_names():
    from recmv.mesh_args import check_mesh
    v, f = _tetra()
    cv, _ = check_mesh(v.double(), f, cuda=False, float_verts=True)
    assert cv.dtype == torch.float64
    with pytest.raises(ValueError, match=r"verts must be floating point of shape \[V,3\]"):
        check_mesh(v.long(), f, cuda=False, float_verts=True)
    with pytest.raises(ValueError, match=r"src_faces must be int64 of shape \[F,3\]"):
        check_mesh(v, f.int(), cuda=False, names=("src_verts", "src_faces"))


def test_check_mesh_shapes_come_before_the_device():
    """The one order: a host tensor that also has a wrong dtype is a ValueError, whatever `cuda` says."""
    from recmv.mesh_args import check_mesh
    v, f = _tetra()
    with pytest.raises(ValueError, match=r"faces must be int64 of shape \[F,3\]"):
        check_mesh(v, f.int(), cuda=True)


def test_check_mesh_cap31_without_allocating():
    from recmv.mesh_args import check_mesh
    huge_v = torch.empty((1 << 31, 3), device="meta")
    huge_f = torch.empty((1 << 31, 3), dtype=torch.int64, device="meta")
    small_v, small_f = huge_v[:4], huge_f[:4]
    for v, f in ((huge_v, small_f), (small_v, huge_f)):
        with pytest.raises(ValueError, match=r"at most 2\^31 - 1 vertices and faces"):
            check_mesh(v, f, cuda=False, cap31=True)
        check_mesh(v, f, cuda=False)                                               # not asked for: not tested
    check_mesh(huge_v[:(1 << 31) - 1], small_f, cuda=False, cap31=True)


# ---- check_points, check_csr, info_json -------------------------------------------------------------------------------------------
def test_check_points():
    from recmv.mesh_args import check_points
    v, _ = _tetra()
    p = check_points(v[:, [2, 1, 0]], "p", cuda=False)
    assert p.is_contiguous() and torch.equal(p, v[:, [2, 1, 0]])
    for bad in (v.double(), v[:, :2], v.reshape(-1), v.numpy()):
        with pytest.raises(ValueError, match=r"p must be float32 of shape \[P,3\]"):
            check_points(bad, "p", cuda=False, shape="[P,3]")
    with pytest.raises(RuntimeError, match="q must be a CUDA tensor"):
        check_points(v, "q")


def test_check_csr():
    from recmv.mesh_args import check_csr
    off, idx = torch.tensor([0, 2, 3], dtype=torch.int32), torch.tensor([1, 0, 0], dtype=torch.int32)
    got = check_csr((off, idx), 2, torch.int32, "nbr_csr")
    assert torch.equal(got[0], off) and torch.equal(got[1], idx) and got[0].is_contiguous()
    for bad, rows, dtype in (((off, idx), 3, torch.int32), ((off.long(), idx), 2, torch.int32), ((off, idx), 2, torch.int64),
                             ((off[None], idx), 2, torch.int32)):
        with pytest.raises(ValueError, match=r"nbr_csr must be \(offsets \[%d\], entries\)" % (rows + 1)):
            check_csr(bad, rows, dtype, "nbr_csr")


def test_info_json_is_one_rule_for_both_modules():
    from recmv import holes, mesh_args, repair
    assert repair.info_json is mesh_args.info_json and holes.info_json is mesh_args.info_json
    nested = {'weld': {'pairs': 3, 'vertex_map': torch.arange(3), 'cluster_radius_max': 0.5}, 'kept_faces': torch.arange(2),
              'dims': (1, 2, 3)}
    assert mesh_args.info_json(nested) == {'weld': {'pairs': 3, 'cluster_radius_max': 0.5}, 'dims': [1, 2, 3]}
    fill = {'loops': 2, 'status': ['filled', 'max_edges'], 'patch_area': [0.5, None], 'face_start': (4, -1), 'refine_capped': False,
            'mixed': [1, torch.zeros(1)], 'tensor': torch.zeros(2), 'none': None}
    want = {'loops': 2, 'status': ['filled', 'max_edges'], 'patch_area': [0.5, None], 'face_start': [4, -1], 'refine_capped': False,
            'none': None}
    assert mesh_args.info_json(fill) == want and json.loads(json.dumps(mesh_args.info_json(fill))) == want


# ---- connectivity.filed_slots_csr -------------------------------------------------------------------------------------------------
def _filed_as_geodesic_did(faces, V):
    """The block geodesic._Mesh and param._Mesh both held before it moved to connectivity.filed_slots_csr."""
    from recmv import connectivity
    if faces.shape[0]:
        filed = torch.where((faces >= 0) & (faces < V), faces, V)
        off, slots = connectivity.vertex_slots_csr(filed, V + 1)
        return off[:V + 1].contiguous(), slots.contiguous()
    return torch.zeros(V + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)


def test_filed_slots_csr_files_bad_corners_under_no_vertex():
    from recmv import connectivity
    V = 4
    faces = torch.tensor([[0, 1, -1], [2, V, 1]], dtype=torch.int64)
    off, slots = connectivity.filed_slots_csr(faces, V)
    assert off.shape == (V + 1,) and off.dtype == torch.int64 and slots.shape == (6,) and slots.dtype == torch.int64
    assert off.tolist() == [0, 1, 3, 4, 4]
    reachable = slots[:int(off[V])].tolist()
    assert sorted(reachable) == [0, 1, 3, 5] and 2 not in reachable and 4 not in reachable   # slots 2 (-1) and 4 (== V)
    for vtx in range(V):
        row = slots[int(off[vtx]):int(off[vtx + 1])]
        assert bool((faces.reshape(-1)[row] == vtx).all()) and row.tolist() == sorted(row.tolist())
    want = _filed_as_geodesic_did(faces, V)
    assert torch.equal(off, want[0]) and torch.equal(slots, want[1])
    v, f = _tetra()
    got, want = connectivity.filed_slots_csr(f, 4), _filed_as_geodesic_did(f, 4)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_filed_slots_csr_of_no_faces():
    from recmv import connectivity
    off, slots = connectivity.filed_slots_csr(torch.zeros((0, 3), dtype=torch.int64), 5)
    assert off.tolist() == [0] * 6 and off.dtype == torch.int64 and slots.shape == (0,) and slots.dtype == torch.int64


# ---- L.workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_refuses_a_negative_size_by_name(monkeypatch):
    from recmv import _lib as L

    def no_allocation(*a, **k):
        raise AssertionError("workspace allocated for a negative size")
    monkeypatch.setattr(L, "scratch", no_allocation)
    with pytest.raises(RuntimeError, match="some_workspace_bytes"):
        L.workspace(-1, torch.device("cpu"), "some_workspace_bytes")
    monkeypatch.undo()
    ws = L.workspace(3, torch.device("cpu"), "t")                                  # the floor: never an empty block
    assert ws.shape == (8,) and ws.dtype == torch.uint8
    assert L.workspace(100, torch.device("cpu"), "t", dtype=torch.float64).shape == (12,)
    assert L.workspace(0, torch.device("cpu"), "t", floor=256).shape == (256,)
