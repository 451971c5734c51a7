"""Mesh topology without a GPU: the numpy / scipy restatement (tests/mesh_topology_reference.py) on hand cases with known
answers, its boundary loops against lap_align.boundary_loops, the new C entry points (declared, exported, argument errors before
any HIP call), the refusal of CPU tensors and wrong dtypes or shapes, the commands' new flags, and the host build of the kernels
under the sanitizers (tools/mesh_topology_host_check)."""
import ctypes as C
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
import mesh_topology_reference as TR  # noqa: E402


def body():
    from test_gpu_animation import _irregular_body
    v, f = _irregular_body(level=3)                        # 1280 faces, closed
    return v.numpy(), f.numpy()


def test_reference_on_closed_and_open_surfaces():
    r = TR.report(*TC.tetrahedron())
    assert r['euler_characteristic'] == 2 and r['watertight'] and r['components'][0]['genus'] == 0
    assert (r['vertices'], r['faces'], r['edges'], r['boundary_edges'], r['boundary_loops']) == (4, 4, 6, 0, 0)
    assert r['components_vertex'] == r['components_edge'] == 1 and r['orientation_conflicts'] == 0
    assert abs(r['area'] - (1.5 + 0.5 * 3 ** 0.5)) < 1e-12
    r = TR.report(*TC.tube())
    assert r['boundary_loops'] == 2 and r['euler_characteristic'] == 0 and r['components'][0]['genus'] == 0
    assert not r['watertight'] and r['boundary_edges'] == 24 and r['boundary_pinch_vertices'] == 0
    assert r['components'][0]['boundary_loops'] == 2 and r['components'][0]['euler_characteristic'] == 0
    r = TR.report(*TC.torus())
    assert r['euler_characteristic'] == 0 and r['watertight'] and r['components'][0]['genus'] == 1 and r['boundary_loops'] == 0
    r = TR.report(*body())
    assert r['euler_characteristic'] == 2 and r['watertight'] and r['components'][0]['genus'] == 0 and r['faces'] == 1280
    assert 0 < r['min_angle_deg']['min'] <= r['min_angle_deg']['mean'] <= 60 and r['min_angle_deg']['below_10_deg'] == 0
    assert r['edge_length']['min'] <= r['edge_length']['mean'] <= r['edge_length']['max']


def test_reference_on_pinched_hinged_and_flipped_meshes():
    v, f = TC.pinched_tetrahedra()
    r = TR.report(v, f)
    assert r['components_vertex'] == 1 and r['components_edge'] == 2 and r['nonmanifold_edges'] == 0
    assert r['euler_characteristic'] == 3 and r['boundary_loops'] == 0     # 7 - 12 + 8: no closed orientable surface has an odd
    assert r['components'][0]['genus'] is None                             # characteristic, so no genus is given
    assert TR.components(v, f, 'edge')['face_component'].tolist() == [0] * 4 + [1] * 4
    assert TR.components(v, f, 'vertex')['vertex_component'].tolist() == [0] * 7
    v, f = TC.hinged_tetrahedra()
    r = TR.report(v, f)
    assert r['nonmanifold_edges'] == 1 and r['components_edge'] == 1 and not r['watertight'] and r['components'][0]['genus'] is None
    r = TR.report(*TC.flipped(TC.tetrahedron()))
    assert r['orientation_conflicts'] == 3 and r['boundary_edges'] == 0 and not r['watertight']
    assert r['components'][0]['genus'] is None


def test_reference_on_duplicates_unreferenced_vertices_and_invalid_faces():
    v, f = TC.tetrahedron()
    r = TR.report(v, np.concatenate([f, f[1:2, [1, 2, 0]]]))                       # face 1 again, rotated
    assert r['duplicate_faces'] == 1 and r['nonmanifold_edges'] == 3 and r['edges'] == 6
    r = TR.report(np.concatenate([v, [[5, 5, 5]]]).astype(np.float32), f)
    assert r['unreferenced_vertices'] == 1 and r['vertices'] == 5 and r['euler_characteristic'] == 2 and r['watertight']
    c = TR.components(np.concatenate([v, [[5, 5, 5]]]).astype(np.float32), f)
    assert c['vertex_component'].tolist() == [0, 0, 0, 0, -1]
    f2 = np.concatenate([f, [[0, 1, 4]], [[2, 2, 3]], [[-1, 0, 1]]])               # an index >= V, a face (a, a, b), a negative one
    r = TR.report(v, f2)
    assert r['invalid_faces'] == 3 and not r['watertight'] and r['euler_characteristic'] == 2 and r['edges'] == 6
    c = TR.components(v, f2)
    assert c['face_component'].tolist() == [0, 0, 0, 0, -1, -1, -1] and c['count'] == 1
    area, ang, ratio, nonfinite = TR.face_stats(v, f2)
    assert area[4:].tolist() == [0, 0, 0] and np.isnan(ang[4:]).all() and np.isnan(ratio[4:]).all() and nonfinite == 0
    vz = v.copy()
    vz[3] = vz[0]                                          # the two faces with both corners lose their area, none its validity
    r = TR.report(vz, f)
    assert r['zero_area_faces'] == 2 and r['invalid_faces'] == 0 and not r['watertight']
    assert np.isinf(TR.face_stats(vz, f)[2][1])
    vn = v.copy()
    vn[3, 0] = np.nan
    r = TR.report(vn, f)
    assert r['nonfinite_faces'] == 3 and r['zero_area_faces'] == 0 and abs(r['area'] - 0.5) < 1e-15


def test_reference_graph_components_and_keep_components():
    links = np.array([[4, 5], [1, 2], [7, 7], [2, 9], [5, 3], [0, 10], [-1, 2]])
    label, invalid = TR.graph_components(10, links)
    assert label.tolist() == [0, 1, 1, 3, 3, 3, 6, 7, 8, 1] and invalid == 3
    label, invalid = TR.graph_components(6, np.array([[5, 4, 3], [0, 0, 1], [3, 1, 2]]))
    assert label.tolist() == [0, 1, 1, 1, 1, 1] and invalid == 1
    bv, bf = body()
    fv, ff = TC.floaters(3)
    v, f = TC.merge((bv, bf), (fv, ff))
    kv, kf, kept, vmap, dropped, dropped_faces = TR.keep_components(v, f, min_area_frac=0.01)
    assert np.array_equal(kv, bv) and np.array_equal(kf, bf) and dropped == 3 and dropped_faces == 12
    assert kept.tolist() == list(range(len(bf))) and vmap[len(bv):].tolist() == [-1] * 12
    assert len(TR.keep_components(v, f, largest=2)[1]) == len(bf) + 4
    assert TR.keep_components(v, f, largest=2)[2][-4:].tolist() == list(range(len(f) - 4, len(f)))   # the last floater is the largest
    assert len(TR.keep_components(v, f, min_faces=5)[1]) == len(bf)
    assert len(TR.keep_components(v, f, largest=3, min_faces=5)[1]) == len(bf)
    assert len(TR.keep_components(v, f)[1]) == len(f)
    c = TR.components(v, f)
    assert c['by_area'].tolist() == [0, 3, 2, 1] and c['faces_per_component'].tolist() == [1280, 4, 4, 4]


@pytest.mark.parametrize("mesh", ["tube", "body", "two tubes", "body with a hole"])
def test_boundary_loops_equal_lap_aligns_walks(mesh):
    """On meshes without pinch vertices the number of boundary-graph components is the number of lap_align's ordered walks."""
    from recmv import lap_align
    if mesh == "tube":
        v, f = TC.tube()
    elif mesh == "body":
        v, f = body()
    elif mesh == "two tubes":
        v, f = TC.merge(TC.tube(), TC.tube(7, 3))
    else:
        v, f = body()
        beside = [k for k in range(len(f)) if len(set(f[k]) & set(f[400])) == 2][0]
        f = np.delete(f, [5, 400, beside], 0)              # one face, and two that share an edge
    r = TR.report(v, f)
    assert r['boundary_pinch_vertices'] == 0
    assert r['boundary_loops'] == len(lap_align.boundary_loops(torch.from_numpy(f)))
    assert r['boundary_loops'] == {"tube": 2, "body": 0, "two tubes": 4, "body with a hole": 2}[mesh]


NEW_SYMBOLS = ("recmv_graph_components", "recmv_mesh_face_stats", "recmv_segment_sums", "recmv_segment_sums_chunk",
               "recmv_segment_sums_workspace_bytes")


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in declared and hasattr(lib, n)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION == 11


def test_argument_errors_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    one = C.c_void_p(16)                                   # a non-NULL pointer that is never followed
    err = lib.recmv_last_error

    def comp(n=5, M=3, K=2, done=0, rounds=4, links=one, out=(one, one, one)):
        return lib.recmv_graph_components(n, links, M, K, done, rounds, *out, None)
    assert comp(K=4) == -1 and b"K=4" in err()
    assert comp(K=1) == -1 and b"K=1" in err()
    assert comp(n=-1) == -1 and b"n=-1" in err()
    assert comp(M=-2) == -1 and b"M=-2" in err()
    assert comp(n=1 << 31) == -1 and b"2^31" in err()
    assert comp(rounds=65) == -1 and b"rounds=65" in err()
    assert comp(done=-1) == -1 and b"rounds_done=-1" in err()
    assert comp(links=None) == -1 and b"NULL" in err()
    assert comp(out=(one, None, one)) == -1 and b"NULL" in err()
    assert comp(M=0, links=None, out=(None, None, None)) == 0                      # M = 0: a no-op
    assert comp(n=0, M=0, links=None, out=(None, None, None)) == 0

    def stats(V=3, F=1, mesh=(one, one), out=(one, one, one, one)):
        return lib.recmv_mesh_face_stats(mesh[0], V, mesh[1], F, *out, None)
    assert stats(V=-3) == -1 and b"V=-3" in err()
    assert stats(F=-1) == -1 and b"F=-1" in err()
    assert stats(F=1 << 31) == -1 and b"faces" in err()
    assert stats(mesh=(one, None)) == -1 and b"NULL mesh" in err()
    assert stats(out=(one, one, None, one)) == -1 and b"NULL output" in err()
    assert stats(F=0, mesh=(None, None), out=(None, None, None, None)) == 0

    def sums(N=10, Cn=1, S=2, ptrs=(one, one, one), out=(one, one, one), ws=(one, 1 << 20)):
        return lib.recmv_segment_sums(ptrs[0], N, Cn, ptrs[1], S, ptrs[2], *out, *ws, None)
    assert sums(N=-1) == -1 and b"N=-1" in err()
    assert sums(S=-1) == -1 and b"S=-1" in err()
    assert sums(Cn=0) == -1 and b"C=0" in err()
    assert sums(Cn=9) == -1 and b"C=9" in err()
    assert sums(ptrs=(one, None, one)) == -1 and b"NULL" in err()
    assert sums(out=(one, one, None)) == -1 and b"NULL" in err()
    assert sums(ws=(one, 8)) == -1 and b"workspace" in err()
    assert sums(ws=(C.c_void_p(20), 1 << 20)) == -1 and b"aligned" in err()
    assert sums(S=0, ptrs=(None, None, None), out=(None, None, None), ws=(None, 0)) == 0
    chunk = lib.recmv_segment_sums_chunk()
    assert chunk >= 64 and lib.recmv_segment_sums_workspace_bytes(10 * chunk + 1, 3, 2) == (3 + 10) * 2 * 3 * 8
    assert lib.recmv_segment_sums_workspace_bytes(5, 0, 1) == 0


def test_the_python_entry_points_refuse_cpu_tensors_and_bad_arguments():
    from recmv import topology
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])
    f = torch.tensor([[0, 1, 2]])
    for call in (lambda: topology.graph_components(3, f), lambda: topology.components(v, f), lambda: topology.report(v, f),
                 lambda: topology.keep_components(v, f), lambda: topology.components(v, f, 'edge'),
                 lambda: topology.segment_sums(v.double(), torch.tensor([0, 3]))):
        with pytest.raises(RuntimeError):
            call()
    meta = torch.device('meta')                            # (is_cuda is False: refused like a host tensor, before any dtype check)
    with pytest.raises(RuntimeError):
        topology.graph_components(3, f.to(meta))
    assert topology.round_cap(1) == 2 and topology.round_cap(2) == 4 and topology.round_cap(4098) == 28
    assert topology.round_cap(200000) == 38 and topology.round_cap((1 << 31) - 1) == 64
    assert topology.ROUNDS_PER_READBACK >= 1

    class Cuda(torch.Tensor):                              # a tensor that claims to be on the device: the checks behind require_cuda
        is_cuda = True

    def fake(t):
        return t.as_subclass(Cuda)
    with pytest.raises(ValueError):
        topology.graph_components(3, fake(f.int()))                                # dtype
    with pytest.raises(ValueError):
        topology.graph_components(3, fake(torch.zeros(2, 4, dtype=torch.int64)))   # K = 4
    with pytest.raises(ValueError):
        topology.graph_components(3, fake(torch.zeros(6, dtype=torch.int64)))      # not [M,K]
    with pytest.raises(ValueError):
        topology.graph_components(-1, fake(f))
    with pytest.raises(ValueError):
        topology.graph_components(3, fake(f), rounds_per_readback=0)
    with pytest.raises(ValueError):
        topology.components(fake(v.double()), fake(f))
    with pytest.raises(ValueError):
        topology.components(fake(v), fake(f.int()))
    with pytest.raises(ValueError):
        topology.components(fake(v), fake(f), connectivity='face')
    with pytest.raises(ValueError):
        topology.keep_components(fake(v), fake(f), min_area_frac=1.5)
    with pytest.raises(ValueError):
        topology.keep_components(fake(v), fake(f), largest=-1)
    with pytest.raises(ValueError):
        topology.segment_sums(fake(v), fake(torch.tensor([0, 3])))                 # float32 values


def test_the_commands_carry_the_new_flags_and_they_default_to_off(tmp_path, capsys):
    import clean_fl
    import eval_fl
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g"])
    assert a.topology is False and a.drop_floaters is None
    a = eval_fl.build_parser().parse_args(["--pred", "p", "--gt", "g", "--topology", "--drop-floaters", "0.01"])
    assert a.topology is True and a.drop_floaters == 0.01
    me = str(HERE / "mesh_topology_reference.py")          # any existing file: the usage errors come before it is read
    for bad in ("-0.1", "1.5"):
        with pytest.raises(SystemExit):
            eval_fl.main(["--pred", me, "--gt", me, "--drop-floaters", bad])
    a = clean_fl.build_parser().parse_args(["--in", "x", "--out", "y"])
    assert (a.largest, a.min_area_frac, a.min_faces, a.connectivity, a.report_only, a.gpu_ids) == (None, None, None, 'vertex',
                                                                                                   False, [0])
    a = clean_fl.build_parser().parse_args(["--in", "x", "--out", "y", "--largest", "2", "--min-area-frac", "0.05", "--min-faces",
                                            "10", "--connectivity", "edge", "--report-only", "--gpu-ids", "3"])
    assert (a.largest, a.min_area_frac, a.min_faces, a.connectivity, a.report_only, a.gpu_ids) == (2, 0.05, 10, 'edge', True, [3])
    for bad in ("-0.5", "1.01"):
        with pytest.raises(SystemExit):                    # before any device work
            clean_fl.main(["--in", me, "--out", str(tmp_path), "--min-area-frac", bad])
    with pytest.raises(SystemExit):
        clean_fl.main(["--in", me])                        # neither --out nor --report-only
    with pytest.raises(SystemExit):
        clean_fl.main(["--in", str(tmp_path / "absent"), "--report-only"])
    with pytest.raises(SystemExit):
        clean_fl.main(["--in", str(tmp_path), "--report-only"])                    # a directory without meshes
    with pytest.raises(SystemExit):
        clean_fl.build_parser().parse_args(["--in", "x", "--connectivity", "face"])
    capsys.readouterr()


def test_host_build_of_the_kernels_equals_union_find(tmp_path):
    """tools/mesh_topology_host_check: csrc/mesh_topology.hip's kernels compiled for the CPU under the address and
    undefined-behaviour sanitizers, a stand-alone program.  The rounds run serially; the labels equal a plain union-find's, the
    round counts a plain restatement of the synchronous algorithm and stay within 2 ceil(log2 n) + 2, on the link sets of the
    GPU test, on paths numbered ascending, descending and randomly, and on empty input; the face figures and the segment sums
    equal plain loops, and tables that are not what the header describes stay inside the arrays."""
    r = host_check.run("mesh_topology", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(" 0 mismatches") == 33
    for name in ("strip 4097 random", "hub of 5000 triangles", "body and 3000 isolated triangles", "first rows of the strip",
                 "strip with invalid rows", "path 4098 descending", "path 200000 random", "empty", "face figures", "segment sums"):
        assert name in r.stdout
    rounds = {line.split(":")[0]: int(line.split(" rounds")[0].split()[-1]) for line in r.stdout.splitlines() if " rounds" in line}
    assert rounds["path 4098 ascending"] == 2 and rounds["path 200000 descending"] == 2
    assert rounds["path 4098 random"] <= 28 and rounds["path 200000 random"] <= 38
