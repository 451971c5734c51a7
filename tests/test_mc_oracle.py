"""Marching-cubes oracle: table pin + invariants (the reference has no MC test or golden mesh, so parity
with its binary is UNPINNED; these are the invariants SURVEY.md §4 lists)."""
import hashlib
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
TABLE_SHA = "d76fca19e486f1d5a41e349985c93caca53fea9e8062379af3e9c25f7752391e"  # tools/gen_mc_tables.py


def _table_words(path):
    return [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", path.read_text())]


@pytest.mark.parametrize("rel", ["oracle/mc_tables.inc", "rec-mv_amd/csrc/mc_tables.inc"])
def test_table_matches_reference_digest(rel):
    words = _table_words(REPO / rel)
    assert len(words) == 256
    assert hashlib.sha256(b"".join(w.to_bytes(8, "little") for w in words)).hexdigest() == TABLE_SHA


def test_table_against_the_stored_reference_table():
    # the reference's triangle table, stored by tests/golden/make_golden_mc_table.py
    tri = json.loads((REPO / "tests/golden/mc_triangle_table.json").read_text())
    assert len(tri) == 256 and all(len(row) == 16 for row in tri)
    words = _table_words(REPO / "oracle/mc_tables.inc")
    for case in range(256):
        for i in range(16):
            v = (words[case] >> (4 * i)) & 0xF
            assert (-1 if v == 0xF else v) == tri[case][i]


def sphere_volume(n, r=0.6, center=(0.03, -0.02, 0.01)):
    ax = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (torch.sqrt((X - center[0]) ** 2 + (Y - center[1]) ** 2 + (Z - center[2]) ** 2) - r).float().contiguous()


def mesh_invariants(verts, faces):
    V, F = verts.shape[0], faces.shape[0]
    assert faces.min() >= 0 and faces.max() < V
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)
    und = torch.sort(e, dim=1)[0]
    uniq, cnt = torch.unique(und, dim=0, return_counts=True)
    assert (cnt == 2).all(), "every edge of a closed 2-manifold is shared by exactly two triangles"
    # consistent orientation: each directed edge appears once
    assert torch.unique(e, dim=0).shape[0] == e.shape[0]
    return V - uniq.shape[0] + F


def test_sphere_is_closed_manifold_with_euler_2(oracle):
    n = 33
    vol = sphere_volume(n)
    step = 2.0 / (n - 1)
    verts, faces = oracle.mc(vol, step, step, step, -1.0, -1.0, -1.0, 0.0)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int64
    assert mesh_invariants(verts, faces) == 2
    r = torch.sqrt(((verts - torch.tensor([0.03, -0.02, 0.01])) ** 2).sum(1))
    assert (r - 0.6).abs().max() < 2e-3      # linear interpolation of a smooth field
    # every vertex used, canonical vertex order = edge-key order => x-major lexicographic on the lattice cell
    assert torch.unique(faces).numel() == verts.shape[0]
    cell = torch.floor((verts + 1.0) / step + 1e-4)
    key = (cell[:, 0] * n + cell[:, 1]) * n + cell[:, 2]
    assert (key[1:] >= key[:-1]).all()


def test_surface_touching_the_box_gives_minus_one(oracle):
    """Edges on the +x/+y/+z boundary have no owner voxel -> index -1, like the reference (CudaKernels.cu:324)."""
    vol = sphere_volume(9, r=1.2)
    _, faces = oracle.mc(vol)
    assert (faces == -1).any()


def test_degenerate_inputs(oracle):
    v, f = oracle.mc(torch.ones(5, 6, 7))             # no sign change
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = oracle.mc(torch.ones(1, 1, 1))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    vol = torch.ones(3, 3, 3)
    vol[1, 1, 1] = -1.0                                 # a single inside lattice point -> octahedron
    v, f = oracle.mc(vol)
    assert v.shape == (6, 3) and f.shape == (8, 3) and mesh_invariants(v, f) == 2
    vol[1, 1, 1] = 0.0                                  # equal to iso is NOT inside (strict <)
    v, f = oracle.mc(vol)
    assert v.shape[0] == 0
