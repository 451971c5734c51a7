"""Animation on novel poses without a GPU: the motion reader against the reference's own `load_motion` and hand-computed
cases, the snug dataset on a capture directory, the float64 restatement of the collision repair (tests/collide_reference.py)
pinned on hand-computed cases, the command line of infer_fl_animation.py and the argument checks of the new C entry points."""
import ctypes as C
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import capture_fixture as cf  # noqa: E402
import collide_reference as CR  # noqa: E402

CONDS = {'deformer': 16, 'render': 8}
# float32 round-off of values of magnitude <= pi: the reference rounds its float64 results to float32 once (half an ulp of a
# value below 4 = 2^-23 * 4 / 2), and the restatement's float64 arithmetic differs from scipy's by a few 1e-16; velocities are
# 30 x differences of translations (magnitude <= 4 assumed for both), so the same absolute bound holds after the rounding.
F32_TOL = float(np.finfo(np.float32).eps) * 4. / 2.


# ------------------------------------------------------------------------------------------------- motion reader
def _write_motion(path, poses, trans, rate):
    np.savez(path, poses=poses, trans=trans, mocap_framerate=np.float64(rate))
    return str(path)


def test_load_motion_matches_the_reference_function():
    from recmv.dataset import load_motion
    want = np.load(HERE / "golden" / "motion_out.npz")
    pose, trans, vel = load_motion(str(HERE / "golden" / "motion_in.npz"))
    for got, key in ((pose, 'pose'), (trans, 'trans'), (vel, 'trans_vel')):
        assert got.dtype == np.float32 and got.shape == want[key].shape, key
        assert np.abs(want[key]).max() <= 4.
        assert np.abs(got - want[key]).max() <= F32_TOL, (key, np.abs(got - want[key]).max())
    assert pose.shape == (12, 72) and trans.shape == (12, 3)


def test_load_motion_hand_computed_cases(tmp_path):
    from recmv.dataset import load_motion
    T = 9
    poses = np.zeros((T, 156))
    poses[:, 22 * 3:22 * 3 + 3] = [0.5, -0.2, 0.1]                       # hands: scaled by 0.1
    poses[:, 23 * 3:23 * 3 + 3] = [-0.3, 0.4, 0.2]
    poses[:, 5 * 3:5 * 3 + 3] = [0.1, 0.2, 0.3]                          # any other joint: untouched
    poses[:, 72:] = 7.                                                   # columns past 72 are not read
    trans = np.arange(T)[:, None] * np.array([[0.12, 0.24, -0.36]]) + np.array([[1., 2., 3.]])
    pose, tr, vel = load_motion(_write_motion(tmp_path / "identity.npz", poses, trans, 120.))
    # 120 fps -> 30 fps: frames 0, 4, 8
    assert pose.shape == (3, 72) and tr.shape == (3, 3) and vel.shape == (3, 3)
    # identity root: the root becomes the swap itself, R = Rx(270 deg) Rz(-90 deg) = [[0,1,0],[0,0,1],[1,0,0]], a rotation by
    # 120 deg about -(1,1,1)/sqrt(3)
    want_root = -(2 * np.pi / 3) / np.sqrt(3.) * np.ones(3)
    assert np.abs(pose[:, :3] - want_root).max() <= F32_TOL
    # shoulders: identity composed with -/+ 20 degrees about z
    assert np.abs(pose[:, 17 * 3:17 * 3 + 3] - [0, 0, -np.deg2rad(20)]).max() <= F32_TOL
    assert np.abs(pose[:, 16 * 3:16 * 3 + 3] - [0, 0, np.deg2rad(20)]).max() <= F32_TOL
    assert np.abs(pose[:, 22 * 3:22 * 3 + 3] - [0.05, -0.02, 0.01]).max() <= F32_TOL
    assert np.abs(pose[:, 23 * 3:23 * 3 + 3] - [-0.03, 0.04, 0.02]).max() <= F32_TOL
    assert np.abs(pose[:, 5 * 3:5 * 3 + 3] - [0.1, 0.2, 0.3]).max() <= F32_TOL
    # translation: R (x, y, z) = (y, z, x), centred on the first frame; frames 4 apart
    step = 4 * np.array([0.24, -0.36, 0.12])
    assert np.abs(tr - np.arange(3)[:, None] * step[None]).max() <= F32_TOL
    assert np.abs(vel[0]).max() == 0 and np.abs(vel[1:] - step * 30.).max() <= 30 * F32_TOL
    # a pure z rotation of the root by 0.7 rad: R Rz(0.7), still about an axis computed by hand from the matrix
    poses2 = np.zeros((4, 72))
    poses2[:, 2] = 0.7
    pose2, _, _ = load_motion(_write_motion(tmp_path / "zrot.npz", poses2, np.zeros((4, 3)), 30.))
    assert pose2.shape == (4, 72)                                        # 30 fps: every frame kept
    c, s = np.cos(0.7), np.sin(0.7)
    M = np.array([[0., 1., 0.], [0., 0., 1.], [1., 0., 0.]]) @ np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]])
    angle = np.arccos((np.trace(M) - 1.) / 2.)
    axis = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / (2. * np.sin(angle))
    assert np.abs(pose2[:, :3] - angle * axis).max() <= F32_TOL
    # 60 fps -> every second frame; 100 fps -> int(100 // 30) = 3
    assert load_motion(_write_motion(tmp_path / "r60.npz", np.zeros((10, 72)), np.zeros((10, 3)), 60.))[0].shape[0] == 5
    assert load_motion(_write_motion(tmp_path / "r100.npz", np.zeros((10, 72)), np.zeros((10, 3)), 100.))[0].shape[0] == 4


# ------------------------------------------------------------------------------------------------- snug dataset
@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    return cf.write_capture(str(tmp_path_factory.mktemp("capture")))


def test_snug_dataset_on_a_capture_directory(capture):
    from recmv.dataset import SceneDataset, Snug_SceneDataset, getDatasetAndLoader, load_motion
    motion = str(HERE / "golden" / "motion_in.npz")
    anim = load_motion(motion)[0]
    torch.manual_seed(4)
    ds = Snug_SceneDataset(capture, dict(CONDS), cf.GARMENT_TYPE, fl_sampling=30, motion=motion)
    torch.manual_seed(4)
    base = SceneDataset(capture, dict(CONDS), cf.GARMENT_TYPE, fl_sampling=30)
    assert len(ds) == anim.shape[0] == 12 and ds.origin_size() == cf.FRAMES and ds.frame_num == cf.FRAMES
    idx, item = ds[5]
    assert idx == 5 and set(item) == {'poses_y'} and item['poses_y'].shape == (72,) and item['poses_y'].dtype == torch.float32
    assert np.array_equal(item['poses_y'].numpy(), anim[5])
    ids = torch.tensor([2, 7])
    poses, trans, c0, c1 = ds.get_grad_parameters(ids, 'cpu')
    bposes, btrans, b0, b1 = base.get_grad_parameters(ids, 'cpu')
    assert torch.equal(poses, bposes) and torch.equal(c0, b0) and torch.equal(c1, b1)
    assert torch.equal(trans[:, :2], btrans[:, :2]) and torch.equal(trans[:, 2], -btrans[:, 2])
    assert torch.equal(ds.trans, base.trans)                             # the stored translations keep their sign
    cam, bcam = ds.get_camera_parameters(2, 'cpu'), base.get_camera_parameters(2, 'cpu')
    assert torch.equal(cam[0], bcam[0]) and torch.equal(cam[1], bcam[1]) and torch.equal(cam[3], bcam[3]) and cam[4:] == bcam[4:]
    assert cam[2].shape == (2, 3, 3) and torch.equal(cam[2], bcam[2] @ torch.diag(torch.tensor([1., -1., -1.])))
    # a motion of another length, given as arrays; the capture's per-line weights do not depend on it
    short = Snug_SceneDataset(capture, dict(CONDS), cf.GARMENT_TYPE, fl_sampling=30, motion=anim[:4])
    assert len(short) == 4 and short.origin_size() == cf.FRAMES
    long_ = Snug_SceneDataset(capture, dict(CONDS), cf.GARMENT_TYPE, fl_sampling=30, motion=np.zeros((40, 24, 3)))
    assert len(long_) == 40 and long_.fl_weights == base.fl_weights
    with pytest.raises(ValueError):
        Snug_SceneDataset(capture, dict(CONDS), cf.GARMENT_TYPE, motion=np.zeros((4, 60)))
    # the factory: raises without a motion, builds with one; the loader walks the motion's frames in order
    with pytest.raises(NotImplementedError):
        getDatasetAndLoader(capture, dict(CONDS), 1, False, 0, True, True, False, cf.GARMENT_TYPE, data_type='snug')
    ds2, loader = getDatasetAndLoader(capture, dict(CONDS), 1, False, 0, True, True, False, cf.GARMENT_TYPE, data_type='snug',
                                      motion=motion)
    assert isinstance(ds2, Snug_SceneDataset) and len(loader) == 12 and ds2.poses.requires_grad
    got = [(int(i), o['poses_y']) for i, o in loader]
    assert [i for i, _ in got] == list(range(12)) and got[3][1].shape == (1, 72)
    assert np.array_equal(got[3][1][0].numpy(), anim[3])


# ------------------------------------------------------------------------------------------------- the float64 restatement
TRI_V = np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])             # one triangle in the plane z = 0


def test_restatement_closest_point_regions():
    # over the face interior: foot of the perpendicular, barycentric weights of (0.25, 0.25)
    d, w = CR.closest_on_triangle(np.array([0.25, 0.25, 2.]), *TRI_V)
    assert d == pytest.approx(4., abs=1e-15) and np.allclose(w, [0.5, 0.25, 0.25], atol=1e-15)
    # over the edge bc (the hypotenuse): (1, 1, 1) projects to (0.5, 0.5, 0); distance^2 = 0.5 + 1
    d, w = CR.closest_on_triangle(np.array([1., 1., 1.]), *TRI_V)
    assert d == pytest.approx(1.5, abs=1e-15) and np.allclose(w, [0., 0.5, 0.5], atol=1e-15)
    # over the edge ab from outside: (0.3, -2, 0) -> (0.3, 0, 0)
    d, w = CR.closest_on_triangle(np.array([0.3, -2., 0.]), *TRI_V)
    assert d == pytest.approx(4., abs=1e-15) and np.allclose(w, [0.7, 0.3, 0.], atol=1e-15)
    # over the edge ac
    d, w = CR.closest_on_triangle(np.array([-1., 0.6, 0.]), *TRI_V)
    assert d == pytest.approx(1., abs=1e-15) and np.allclose(w, [0.4, 0., 0.6], atol=1e-15)
    # the three corners
    for p, want_w, want_d in (([-1., -1., 1.], [1., 0., 0.], 3.), ([3., -0.5, 0.], [0., 1., 0.], 4.25),
                              ([-0.5, 3., 0.], [0., 0., 1.], 4.25)):
        d, w = CR.closest_on_triangle(np.array(p), *TRI_V)
        assert d == pytest.approx(want_d, abs=1e-15) and np.allclose(w, want_w, atol=1e-15)
    # a degenerate (zero-area) triangle is its longest segment
    d, w = CR.closest_on_triangle(np.array([0.5, 1., 0.]), np.zeros(3), np.array([1., 0., 0.]), np.array([2., 0., 0.]))
    assert d == pytest.approx(1., abs=1e-15)


def test_restatement_nearest_signed_distance_and_push():
    # the unit octahedron: face 0 lies in the plane x + y + z = 1 with the outward normal (1,1,1)/sqrt(3)
    V = np.array([[1., 0., 0.], [-1., 0., 0.], [0., 1., 0.], [0., -1., 0.], [0., 0., 1.], [0., 0., -1.]])
    F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    vn = CR.vertex_normals(V, F)
    assert np.allclose(vn, V, atol=1e-15)                                 # by symmetry the vertex normals are the vertices
    c = np.array([1., 1., 1.]) / 3.                                       # centroid of face 0, its plane x + y + z = 1
    n0 = np.array([1., 1., 1.]) / np.sqrt(3.)
    eps, md = 0.05, 0.2
    pts = np.stack([c + 0.5 * n0,                                         # outside over the face interior: s = 0.5
                    c - 0.1 * n0,                                         # inside by 0.1: s = -0.1 -> pushed to s = eps
                    c - 0.25 * n0,                                        # deeper than max_depth: unresolved, unmoved
                    c + 0.01 * n0,                                        # outside but closer than eps: pushed
                    np.array([0.5, 0.5, 0.]) + 0.3 * np.array([1., 1., 0.]) / np.sqrt(2.),      # over the edge 0-2
                    np.array([0., 0., 1.7])])                             # over the corner 4
    face, d1, d2, w = CR.nearest(pts, V, F)
    assert face.tolist()[:4] == [0, 0, 0, 0] and np.allclose(d1[:4], [0.25, 0.01, 0.0625, 1e-4], atol=1e-15)
    assert np.allclose(w[:4], 1. / 3., atol=1e-15)
    # the point over the edge 0-2 is exactly between the faces 0 and 4: the lowest index wins, the runner-up is as near
    assert face[4] == 0 and d1[4] == pytest.approx(0.09, abs=1e-15) and d2[4] == pytest.approx(d1[4], abs=1e-15)
    assert np.allclose(w[4], [0.5, 0.5, 0.], atol=1e-15)
    # over the corner: four faces tie, face 0 wins, weight 1 on vertex 4
    assert face[5] == 0 and d1[5] == pytest.approx(0.49, abs=1e-15) and np.allclose(w[5], [0., 0., 1.], atol=1e-15)
    s, n, _ = CR.signed_distance(pts, V, F)
    assert np.allclose(s, [0.5, -0.1, -0.25, 0.01, 0.3, 0.7], atol=1e-14)
    assert np.allclose(n[:4], n0, atol=1e-15) and np.allclose(n[5], [0., 0., 1.], atol=1e-15)
    out, moved, unresolved, s2 = CR.push(pts, V, F, eps, md)
    assert moved.tolist() == [False, True, False, True, False, False]
    assert unresolved.tolist() == [False, False, True, False, False, False]
    assert np.array_equal(out[[0, 2, 4, 5]], pts[[0, 2, 4, 5]])           # copied exactly
    assert np.allclose(out[1], c + eps * n0, atol=1e-15) and np.allclose(out[3], c + eps * n0, atol=1e-15)
    res, ever, unres, passes = CR.resolve(pts, V, F, eps, md, iters=3)
    assert ever.tolist() == moved.tolist() and unres.tolist() == unresolved.tolist()
    assert CR.signed_distance(res, V, F)[0][[1, 3]] == pytest.approx(eps, abs=1e-14)
    assert passes <= 3


def test_restatement_agrees_with_the_torch_restatement_of_the_kernel():
    """Two independent formulations (perpendicular foot / segments here, Ericson's regions in recmv.iso_remesh) on random
    points round an icosphere, float64 both."""
    from recmv.iso_remesh import closest_point_torch
    from test_nricp_cpu import icosphere
    v, f = icosphere(2)
    g = torch.Generator().manual_seed(8)
    p = (torch.randn(300, 3, generator=g) * 0.8).double()
    face, d1, d2, _ = CR.nearest(p.numpy(), v.double().numpy(), f.numpy())
    tf, _, td = closest_point_torch(p, v.double(), f)
    assert np.abs(td.numpy() - d1).max() <= 1e-13
    clear = (d2 - d1) > 1e-12
    assert clear.mean() > 0.3 and np.array_equal(tf.numpy()[clear], face[clear])


# ------------------------------------------------------------------------------------------------- command line, C ABI
def _animation_module():
    spec = importlib.util.spec_from_file_location("infer_fl_animation", REPO / "rec-mv_amd" / "infer_fl_animation.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_parses_the_reference_flags_and_the_new_ones():
    mod = _animation_module()
    p = mod.build_parser()
    a = p.parse_args(['--gpu-ids', '0', '1', '--batch-size', '2', '--rec-root', '/x/run', '--frames', '7', '--data-type', 'snug',
                      '--nV', '--C', '--nColor', '--motion', 'm.npz', '--fix-collisions', '--collision-eps', '0.004',
                      '--collision-iters', '5'])
    assert a.gpu_ids == [0, 1] and a.batch_size == 2 and a.rec_root == '/x/run' and a.frames == 7 and a.data_type == 'snug'
    assert a.nV and a.C and a.nColor and not a.nI and a.motion == 'm.npz' and a.fix_collisions
    assert a.collision_eps == 0.004 and a.collision_iters == 5 and a.a_pose is False and a.conf is None
    d = p.parse_args(['--data-type', 'snug', '--nI'])
    assert d.batch_size == 1 and d.frames == -1 and d.nI and not d.fix_collisions and d.motion is None
    assert d.collision_eps is None and d.collision_iters is None
    with pytest.raises(SystemExit):
        p.parse_args([])                                                  # --data-type is required, as in the reference
    with pytest.raises(SystemExit):
        mod.main(['--data-type', 'snug', '--rec-root', '/x/run'])         # snug without a motion
    with pytest.raises(SystemExit):
        mod.main(['--data-type', 'scene', '--rec-root', '/x/run', '--motion', 'm.npz'])


def test_temporal_smoothness_is_the_mean_second_difference():
    mod = _animation_module()
    t = np.arange(5, dtype=np.float64)
    # vertex 0 moves uniformly (second difference 0), vertex 1 accelerates along x: x = t^2 -> second difference 2
    seq = np.zeros((5, 2, 3))
    seq[:, 0, 1] = 3. * t
    seq[:, 1, 0] = t ** 2
    assert mod.temporal_smoothness(seq) == pytest.approx(1.0, abs=1e-15)  # mean over the two vertices of (0, 2)
    assert mod.temporal_smoothness(seq[:2]) is None


def test_collision_entry_points_check_their_arguments_without_a_gpu():
    from recmv import _lib, collide
    lib = _lib.lib()
    assert lib.recmv_abi_version() == 11 and _lib.ABI_VERSION == 11
    assert {"recmv_point_mesh_nearest", "recmv_point_mesh_nearest_workspace_bytes",
            "recmv_collision_push"} <= set(_lib.exported_symbols())
    n, p = None, C.c_void_p(16)
    near, push = lib.recmv_point_mesh_nearest, lib.recmv_collision_push
    assert lib.recmv_point_mesh_nearest_workspace_bytes(2, 10) == 160
    assert lib.recmv_point_mesh_nearest_workspace_bytes(0, 10) == 0 and lib.recmv_point_mesh_nearest_workspace_bytes(3, 0) == 0
    assert near(n, n, n, 1, 4, 3, 0, n, n, n, 0, n) == -1                 # F = 0
    assert b"must not be empty" in lib.recmv_last_error()
    assert near(n, n, n, 1, 4, 0, 1, n, n, n, 0, n) == -1                 # V = 0
    assert near(n, n, n, -1, 4, 3, 1, n, n, n, 0, n) == -1
    assert near(n, n, n, 1, -4, 3, 1, n, n, n, 0, n) == -1
    assert near(n, n, n, 70000, 4, 3, 1, n, n, n, 0, n) == -1             # more frames than a grid axis holds
    assert near(n, n, n, 0, 4, 3, 1, n, n, n, 0, n) == 0                  # B = 0: no-op
    assert near(n, n, n, 2, 0, 3, 1, n, n, n, 0, n) == 0                  # N = 0: no-op
    assert near(n, n, n, 1, 4, 3, 1, n, n, n, 0, n) == -1                 # NULL pointers
    assert b"NULL" in lib.recmv_last_error()
    assert near(p, p, p, 2, 16, 3, 1, p, p, p, 8, n) == -1                # workspace too small
    assert b"workspace" in lib.recmv_last_error()
    assert near(p, p, p, 2, 16, 3, 1, p, p, C.c_void_p(12), 256, n) == -1  # misaligned workspace
    assert push(n, n, n, n, n, 1, 4, 3, 0, 0.002, 0.03, n, n, n, n) == -1  # F = 0
    assert push(n, n, n, n, n, -1, 4, 3, 1, 0.002, 0.03, n, n, n, n) == -1
    assert push(n, n, n, n, n, 1, 4, 3, 1, -0.002, 0.03, n, n, n, n) == -1
    assert b"eps" in lib.recmv_last_error()
    assert push(n, n, n, n, n, 1, 4, 3, 1, 0.002, float("nan"), n, n, n, n) == -1
    assert push(n, n, n, n, n, 0, 4, 3, 1, 0.002, 0.03, n, n, n, n) == 0   # B = 0: no-op
    assert push(n, n, n, n, n, 1, 4, 3, 1, 0.002, 0.03, n, n, n, n) == -1  # NULL count pointers
    assert push(n, n, n, n, n, 1, 4, 3, 1, 0.002, 0.03, n, p, p, n) == -1  # NULL mesh pointers
    # the python layer refuses CPU tensors like every other op
    v, f = torch.zeros(1, 4, 3), torch.zeros(2, 3, dtype=torch.int64)
    for call in (lambda: collide.point_mesh_nearest(v, v, f), lambda: collide.resolve(v, v, f),
                 lambda: collide.collision_push(v, v, v, f, torch.zeros(1, 4, dtype=torch.int64))):
        with pytest.raises(RuntimeError):
            call()
    assert collide.COLLISION_EPS == 2e-3 and collide.COLLISION_MAX_DEPTH == 3e-2 and collide.COLLISION_ITERS == 3
