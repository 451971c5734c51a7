"""Mesh voxelisation without a GPU: the new C entry points (declared, exported, argument errors before any HIP call), the lattice
arithmetic and the ValueErrors of recmv.voxelize, the refusal of CPU tensors, the commands' new flags, the float64 restatement
(tests/voxelize_reference.py) on hand cases and on the two sign meshes of the GPU test, the decidability of that test's node
samples, and the host build of the kernels under the sanitizers.

The cases of tests/test_gpu_voxelize.py are defined here so that both files see the same meshes, lattices and samples.
"""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import host_check  # noqa: E402
import mesh_topology_cases as TC  # noqa: E402
import voxelize_reference as VR  # noqa: E402

BODY_STEP, BODY_DIMS = 0.06, (23, 25, 27)
TORUS_STEP, TORUS_PAD = 0.05, 3
SAMPLE, SAMPLE_SEED = 1500, 7
UNDECIDED_CAP = 0.03


def body():
    from test_gpu_animation import _irregular_body
    return _irregular_body(level=3)                        # 1280 faces, radius 0.5 +- 9 %


def body_lattice(v, dims=BODY_DIMS):
    """Step 0.06, origin = the box's minimum less 3 steps."""
    from recmv import voxelize
    step = np.float32(BODY_STEP)
    return voxelize.Lattice((v.amin(0).numpy() - np.float32(3) * step).tolist(), BODY_STEP, dims)


def torus():
    v, f = TC.torus(n=24, m=16, R=0.5, r=0.18)
    return torch.from_numpy(v), torch.from_numpy(f)


def torus_lattice(v):
    from recmv import voxelize
    return voxelize.lattice_from_box(v.amin(0).tolist(), v.amax(0).tolist(), step=TORUS_STEP, pad_steps=TORUS_PAD)


def sign_cases():
    bv, bf = body()
    tv, tf = torus()
    return {'body': (bv, bf, body_lattice(bv)), 'torus': (tv, tf, torus_lattice(tv))}


def sample_nodes(lattice):
    """SAMPLE flat node indices, drawn without replacement with a fixed seed."""
    g = torch.Generator().manual_seed(SAMPLE_SEED)
    return torch.randperm(lattice.n_nodes, generator=g)[:SAMPLE]


def sample_reference(v, f, lattice):
    """(index [SAMPLE], inside, decided) of the float64 reference on the drawn nodes."""
    from recmv import metrics
    idx = sample_nodes(lattice)
    pts = VR.nodes(lattice.origin, lattice.step, lattice.dims)[idx.numpy()]
    inside, decided = VR.inside(pts, v.numpy(), f.numpy(), metrics.INSIDE_DIRECTIONS)
    return idx, inside, decided


# ---------------------------------------------------------------------------------------------------------- the C ABI
ONE = C.c_void_p(16)                                       # a non-NULL pointer that is never followed


def _lat(origin=(0., 0., 0.), step=0.5, dims=(4, 5, 6)):
    from recmv import _lib
    d = _lib.Lattice()
    d.origin[:] = origin
    d.step = step
    d.nx, d.ny, d.nz = dims
    return d


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in ("recmv_voxel_band_workspace_bytes", "recmv_voxel_band_distance", "recmv_voxel_sign_fill"):
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION == 11
    assert C.sizeof(_lib.Lattice) == 28
    hdr = (REPO / "include" / "recmv_hip.h").read_text()
    assert "recmv_voxel_band_distance, recmv_voxel_sign_fill" in hdr[:hdr.index("int recmv_abi_version")]   # the "added since" note


def test_argument_errors_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    err = lib.recmv_last_error
    assert lib.recmv_voxel_band_workspace_bytes(C.byref(_lat())) == 4 * 5 * 6 * 8
    assert lib.recmv_voxel_band_workspace_bytes(C.byref(_lat(dims=(4, 0, 6)))) == 0
    assert lib.recmv_voxel_band_workspace_bytes(None) == -1 and b"NULL lattice" in err()
    assert lib.recmv_voxel_band_workspace_bytes(C.byref(_lat(dims=(1024, 1024, 257)))) == -1 and b"2^28" in err()
    assert lib.recmv_voxel_band_workspace_bytes(C.byref(_lat(dims=(1024, 1024, 256)))) == (1 << 28) * 8

    def band(*, mesh=(ONE, 3, ONE, 1), lat=None, null=False, band=0.2, out=(ONE, ONE), ws=(ONE, 4 * 5 * 6 * 8)):
        l = None if null else C.byref(lat if lat is not None else _lat())
        return lib.recmv_voxel_band_distance(*mesh, l, band, *out, *ws, None)
    assert band(mesh=(ONE, -3, ONE, 1)) == -1 and b"V=-3" in err()
    assert band(mesh=(ONE, 3, ONE, -2)) == -1 and b"F=-2" in err()
    assert band(mesh=(ONE, 3, ONE, 1 << 31)) == -1 and b"faces" in err()
    assert band(band=-0.1) == -1 and b"band=-0.1" in err()
    assert band(band=float("nan")) == -1 and b"band" in err()
    assert band(band=float("inf")) == -1 and b"band" in err()
    assert band(null=True) == -1 and b"NULL lattice" in err()
    for s in (0., -1., float("nan"), float("inf")):
        assert band(lat=_lat(step=s)) == -1 and b"step" in err()
    assert band(lat=_lat(origin=(0., float("nan"), 0.))) == -1 and b"origin" in err()
    assert band(lat=_lat(dims=(4, -1, 6))) == -1 and b"dims=(4,-1,6)" in err()
    assert band(lat=_lat(dims=(1 << 10, 1 << 10, 257))) == -1 and b"2^28 nodes" in err()
    assert band(lat=_lat(dims=(1 << 30, 1 << 30, 1 << 30))) == -1 and b"2^28 nodes" in err()
    assert band(out=(None, ONE)) == -1 and b"NULL output" in err()
    assert band(out=(ONE, None)) == -1 and b"NULL output" in err()
    assert band(mesh=(None, 3, ONE, 1)) == -1 and b"NULL pointer of the mesh" in err()
    assert band(mesh=(ONE, 3, None, 1)) == -1 and b"NULL pointer of the mesh" in err()
    assert band(ws=(None, 960)) == -1 and b"NULL workspace" in err()
    assert band(ws=(ONE, 959)) == -1 and b"workspace of 959 bytes, 960 needed" in err()
    assert band(ws=(C.c_void_p(20), 960)) == -1 and b"aligned" in err()
    assert band(lat=_lat(dims=(4, 0, 6)), out=(None, None), ws=(None, 0)) == 0      # a dimension of 0: a no-op

    def fill(*, d2=ONE, flags=ONE, lat=None, null=False, band=0.2, signed=1, out=(ONE, ONE, ONE)):
        l = None if null else C.byref(lat if lat is not None else _lat())
        return lib.recmv_voxel_sign_fill(d2, flags, l, band, signed, *out, None)
    assert fill(band=-1.) == -1 and b"band=-1" in err()
    assert fill(band=float("nan")) == -1 and b"band" in err()
    assert fill(signed=2) == -1 and b"signed=2" in err()
    assert fill(null=True) == -1 and b"NULL lattice" in err()
    assert fill(lat=_lat(step=0.)) == -1 and b"step" in err()
    assert fill(lat=_lat(dims=(1 << 10, 1 << 10, 257))) == -1 and b"2^28 nodes" in err()
    assert fill(out=(ONE, ONE, None)) == -1 and b"NULL open_columns" in err()
    assert fill(d2=None) == -1 and b"NULL pointer" in err()
    assert fill(out=(None, ONE, ONE)) == -1 and b"NULL pointer" in err()
    assert fill(out=(ONE, None, ONE)) == -1 and b"NULL pointer" in err()
    assert fill(flags=None) == -1 and b"signed=1 needs inside_band" in err()


# ------------------------------------------------------------------------------------------------------ recmv.voxelize
def test_lattice_arithmetic_and_value_errors():
    from recmv import voxelize as VX
    lo, hi = [-0.5, -0.25, 0.], [0.5, 0.25, 0.1]
    lat = VX.lattice_from_box(lo, hi, step=0.1, pad_steps=4)
    step = float(np.float32(0.1))
    assert lat.step == step and lat.origin == tuple(float(np.float32(a - 4 * step)) for a in lo)
    assert lat.dims == (19, 14, 10)                        # extent / step + 1 nodes and 4 more on each side
    for a in range(3):                                     # the box and the padding lie inside the lattice
        last = np.float32(lat.origin[a]) + np.float32(lat.dims[a] - 1) * np.float32(lat.step)
        assert lat.origin[a] <= lo[a] - 3.999 * step and last >= hi[a] + 3.999 * step
    lat = VX.lattice_from_box(lo, hi, resolution=33, pad_steps=4)
    assert lat.dims[0] == 33 and abs(lat.step - 1. / 24) < 1e-7 and lat.dims[1] == 12 + 1 + 8 and lat.dims[2] == 3 + 1 + 8
    lat = VX.lattice_from_box(lo, hi, resolution=33, pad_steps=lambda s: int(math.ceil(0.2 / s)) + 1)
    assert lat.dims[0] == 33 and lat.origin[0] <= lo[0] - 0.2 - lat.step * 0.999
    assert VX.Lattice((0, 0, 0), 0.1, (2, 3, 4)).n_nodes == 24
    assert VX.Lattice((0, 0, 0), 0.1, (2, 3, 4)).json() == {'origin': [0., 0., 0.], 'step': step, 'dims': [2, 3, 4]}
    pts = VX.Lattice((0.3, -1., 2.), 0.07, (3, 4, 5)).nodes('cpu')
    want = VR.nodes((0.3, -1., 2.), 0.07, (3, 4, 5))
    assert pts.shape == (3, 4, 5, 3) and np.array_equal(pts.reshape(-1, 3).numpy().view(np.int32), want.view(np.int32))
    idx = torch.tensor([0, 7, 59, 33])
    assert torch.equal(VX.Lattice((0.3, -1., 2.), 0.07, (3, 4, 5)).points(idx), pts.reshape(-1, 3)[idx])
    with pytest.raises(ValueError):
        VX.lattice_from_box(lo, hi)                        # neither
    with pytest.raises(ValueError):
        VX.lattice_from_box(lo, hi, step=0.1, resolution=9)
    with pytest.raises(ValueError):
        VX.lattice_from_box(lo, [float("inf"), 0., 0.], step=0.1)
    with pytest.raises(ValueError):
        VX.lattice_from_box([float("nan"), 0., 0.], hi, step=0.1)
    with pytest.raises(ValueError):
        VX.lattice_from_box(lo, hi, step=0.0005)           # 2009 x 1009 x 209 nodes: beyond 2^28
    with pytest.raises(ValueError):
        VX.lattice_from_box(lo, hi, step=0.)
    with pytest.raises(ValueError):
        VX.lattice_from_box(lo, hi, resolution=9, pad_steps=4)                     # no cell left
    with pytest.raises(ValueError):
        VX.Lattice((0, 0, 0), 0.1, (1024, 1024, 257))
    with pytest.raises(ValueError):
        VX.Lattice((0, 0, 0), float("nan"), (2, 2, 2))


def test_band_and_thickness_value_errors_and_cpu_tensors_are_refused():
    from recmv import voxelize as VX
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])
    f = torch.tensor([[0, 1, 2]])
    lat = VX.Lattice((0, 0, 0), 0.1, (4, 4, 4))
    with pytest.raises(ValueError, match="below 2 steps"):
        VX.distance_field(v, f, lat, band=0.19)
    with pytest.raises(ValueError, match="below 2 steps"):
        VX.distance_field(v, f, lat, band=float("nan"))
    with pytest.raises(ValueError, match="below 3 steps"):
        VX.solidify(v, f, 0.1, step=0.04)
    with pytest.raises(ValueError):
        VX.solidify(v, f, 0., step=0.04)
    with pytest.raises(ValueError):
        VX.distance_field(v, f, lat, method='fast')
    for call in (lambda: VX.lattice_for(v, step=0.1), lambda: VX.distance_field(v, f, lat), lambda: VX.distance_field(v, f, lat, signed=False),
                 lambda: VX.signed_distance(v, v, f), lambda: VX.remesh(v, f, step=0.1), lambda: VX.solidify(v, f, 0.5, step=0.1),
                 lambda: VX.occupancy(v, f, lat), lambda: VX.volume(v, f, lat), lambda: VX.volume_iou(v, f, v, f, step=0.1),
                 lambda: VX.extract(torch.zeros(4, 4, 4), lat)):
        with pytest.raises(RuntimeError):
            call()
    assert VX.DEFAULT_BAND_STEPS == 3. and VX.DEFAULT_PAD_STEPS >= VX.DEFAULT_BAND_STEPS + 1
    for word in ("winding-number", "union of overlapping", "cavity", "GridSamplerMine", "MCGpu, metrics"):
        assert word in VX.__doc__                          # what is out of scope is stated


def test_the_commands_carry_the_new_flags_and_they_default_to_off():
    import clean_fl
    import eval_fl
    me = str(HERE / "voxelize_reference.py")               # any existing file: the usage errors come before it is read
    a = clean_fl.build_parser().parse_args(["--in", "x"])
    assert a.voxel_remesh is None and a.voxel_resolution is None and a.voxel_force is False and a.solidify is None
    a = clean_fl.build_parser().parse_args(["--in", "x", "--voxel-remesh", "0.04", "--voxel-force", "--solidify", "0.2"])
    assert a.voxel_remesh == 0.04 and a.voxel_force and a.solidify == 0.2
    assert clean_fl.build_parser().parse_args(["--in", "x", "--voxel-resolution", "65"]).voxel_resolution == 65
    for bad in (["--voxel-remesh", "0.04", "--voxel-resolution", "65"], ["--solidify", "0.2"], ["--voxel-force"],
                ["--voxel-remesh", "0"], ["--voxel-remesh", "0.04", "--report-only"], ["--voxel-resolution", "1"],
                ["--voxel-remesh", "0.04", "--solidify", "-1"]):
        with pytest.raises(SystemExit):                    # before any device work
            clean_fl.main(["--in", me, "--out", "unused"] + bad)
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g"])
    assert a.volume is False and a.volume_step is None
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g", "--volume", "--volume-step", "0.04"])
    assert a.volume and a.volume_step == 0.04
    with pytest.raises(SystemExit):
        eval_fl.main(["--pred", me, "--gt", me, "--volume-step", "0.04"])
    with pytest.raises(SystemExit):
        eval_fl.main(["--pred", me, "--gt", me, "--volume", "--volume-step", "0"])


# ------------------------------------------------------------------------------------------------------ the reference
def test_reference_on_hand_cases():
    tri_v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float64)
    tri_f = np.array([[0, 1, 2]])
    pts = np.array([[0.5, 0.5, 0.75], [0.5, 0.5, -0.25], [3., 0., 0.], [-1., -1., 1.]])
    d2, face, in_band = VR.band_distance(pts, tri_v, tri_f, 0.8)
    assert np.allclose(d2, [0.75 ** 2, 0.25 ** 2, 1., 3.], rtol=0, atol=1e-15)     # plane, plane, vertex b, vertex a
    assert face.tolist() == [0, 0, 0, 0] and in_band.tolist() == [True, True, False, False]
    d2, face, _ = VR.band_distance(pts, np.concatenate([tri_v, [[np.nan, 0, 0]]]), np.array([[0, 1, 3], [0, 1, 9], [0, 1, 2]]), 1.)
    assert face.tolist() == [2, 2, 2, 2]                   # the faces with a NaN corner or an index out of range never win
    n = VR.nodes((0.5, -1., 0.25), 0.1, (2, 3, 4))
    assert n.dtype == np.float32 and n.shape == (24, 3)
    assert n[1].tolist() == [0.5, -1., float(np.float32(0.25) + np.float32(1) * np.float32(0.1))]           # z fastest
    assert n[4 * 3].tolist()[0] == float(np.float32(0.5) + np.float32(0.1))
    # the column rule on a hand-made column of 8 nodes along x:   band   . B B . . B . B      flags  x 1 0 x x 1 x 0
    in_band = np.array([0, 1, 1, 0, 0, 1, 0, 1], bool)
    flags = np.array([1, 1, 0, 1, 1, 1, 0, 0], bool)       # the flags at the nodes outside the band are not read
    inside, open_columns = VR.column_fill(in_band, flags, (8, 1, 1))
    assert inside.reshape(-1).tolist() == [False, True, False, False, False, True, True, False] and open_columns == 0
    inside, open_columns = VR.column_fill(in_band[:7], flags[:7], (7, 1, 1))
    assert inside.reshape(-1).tolist() == [False, True, False, False, False, True, True] and open_columns == 1
    inside, open_columns = VR.column_fill(np.tile(in_band[:7], (2, 1)).T.reshape(-1), np.tile(flags[:7], (2, 1)).T.reshape(-1), (7, 1, 2))
    assert open_columns == 2 and inside[:, 0, 1].tolist() == inside[:, 0, 0].tolist()
    assert VR.volume(np.array([1, 0, 1, 1], bool), 0.5) == 3 * 0.125
    # two columns side by side whose flags differ at x = 3, 4 and 6, all three outside the band: three edges between the columns;
    # along x every change of flag has a band node at one end
    a = np.array([0, 1, 0, 0, 0, 1, 1, 0], bool)
    b = np.array([0, 1, 0, 1, 1, 1, 0, 0], bool)
    band2 = np.stack([in_band, in_band], 1).reshape(-1)
    assert VR.sign_conflicts(np.stack([a, b], 1).reshape(-1), band2, (8, 1, 2)) == 3
    assert VR.sign_conflicts(np.stack([a, a], 1).reshape(-1), band2, (8, 1, 2)) == 0


@pytest.mark.parametrize("name", ["body", "torus"])
def test_reference_propagation_equals_the_per_node_inside_test(name):
    """On the GPU test's two sign meshes and lattices, in float64: at bands of 1, 2 and 3 steps the column rule applied to the
    band nodes' flags gives the inside flag of EVERY node, and no column ends inside."""
    from recmv import metrics
    v, f, lat = sign_cases()[name]
    pts = VR.nodes(lat.origin, lat.step, lat.dims)
    d2, _, _ = VR.band_distance(pts, v.numpy(), f.numpy(), 1.)
    inside, decided = VR.inside(pts, v.numpy(), f.numpy(), metrics.INSIDE_DIRECTIONS)
    print("%s: %d nodes, %d inside, %.2f %% undecided" % (name, len(pts), inside.sum(), 100. * (~decided).mean()))
    assert inside.sum() >= 2000 and (~decided).mean() <= UNDECIDED_CAP
    for steps in (1, 2, 3):
        in_band = d2 <= (steps * lat.step) ** 2
        filled, open_columns = VR.column_fill(in_band, inside, lat.dims)
        print("band of %d steps: %d band nodes, %d mismatches, %d open columns" % (steps, in_band.sum(),
                                                                                  (filled.reshape(-1) != inside).sum(), open_columns))
        assert open_columns == 0 and np.array_equal(filled.reshape(-1), inside)
        assert VR.sign_conflicts(filled, in_band, lat.dims) == 0


@pytest.mark.parametrize("name", ["body", "torus"])
def test_the_gpu_tests_node_samples_are_decidable(name):
    v, f, lat = sign_cases()[name]
    idx, inside, decided = sample_reference(v, f, lat)
    print("%s: %d nodes drawn, %d inside, %.2f %% undecided" % (name, len(idx), inside.sum(), 100. * (~decided).mean()))
    assert len(idx) == SAMPLE and len(set(idx.tolist())) == SAMPLE
    assert (~decided).mean() <= UNDECIDED_CAP and inside.sum() >= 100


def test_host_build_of_the_kernels_equals_the_brute_loop(tmp_path):
    """tools/voxelize_host_check: csrc/mesh_voxelize.hip's kernels compiled for the CPU under the address and undefined-behaviour
    sanitizers; the scatter over the faces' dilated boxes gives the keys of a loop over every (node, face) pair on nine lattices
    and meshes (clipping, single-node axes, faces larger than the lattice, broken faces), and the column walk its restatement."""
    r = host_check.run("voxelize", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(" 0 mismatches") == 9, r.stdout + r.stderr
    for name in ("covers half of it", "faces larger than the lattice", "single-node axes 1x9x70", "broken faces"):
        assert name in r.stdout
