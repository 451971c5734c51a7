"""recmv.connectivity on the GPU: the same integer tables as on the CPU for the meshes of test_connectivity_cpu.py and for a cut
level-3 icosphere with its vertex ids shuffled, and the 'edge' pieces of a fin, whose rows no longer depend on an unstable sort."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE.parent / "rec-mv_amd")]

from recmv import align, connectivity as CN  # noqa: E402
from test_connectivity_cpu import FIN, MESHES, _verts  # noqa: E402
from test_lap_align_cpu import cut_sphere  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _shuffled_cut_icosphere():
    v, f = cut_sphere(3, caps=('neck',))                                # cut from the 642 vertices of level 3
    perm = torch.randperm(v.shape[0], generator=torch.Generator().manual_seed(7))
    return perm[f].contiguous(), v.shape[0]


CASES = dict(MESHES, **{"cut icosphere 3, shuffled": _shuffled_cut_icosphere()})


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_equal_the_cpus(name):
    f, V = CASES[name]
    want, got = CN.EdgeTable(f, V), CN.EdgeTable(f.to(DEV), V)
    for k in ("edges", "face_to_edge", "count", "boundary_edge", "nonmanifold_edge", "boundary_vertex", "forward"):
        g, w = getattr(got, k), getattr(want, k)
        assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w), k
    assert (got.V, got.F, got.E) == (want.V, want.F, want.E)
    assert torch.equal(align.border_flags(f.to(DEV), V).cpu(), align.border_flags(f, V))
    v = torch.from_numpy(_verts(V + 1))
    for faces in (f, f[1::2]):
        for g, w in zip(CN.compact(v.to(DEV), faces.to(DEV)), CN.compact(v, faces)):
            assert g.is_cuda and g.dtype == w.dtype and np.array_equal(g.cpu().numpy().view(np.uint8), w.numpy().view(np.uint8))


def test_edge_pieces_of_a_fin():
    from recmv import topology
    v, f = torch.from_numpy(_verts(5)).to(DEV), torch.tensor(FIN, device=DEV)
    first, second = topology.components(v, f, 'edge'), topology.components(v, f, 'edge')
    assert first['count'] == second['count'] == 1 and first['face_component'].tolist() == [0, 0, 0]
    assert first['rounds'] == second['rounds']
