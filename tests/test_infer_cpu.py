"""Inference without a GPU: the CLI's flags, the HOCON writer, the mesh / image writers, the Phong restatement the GPU tests
compare against (on a hand-computed triangle), and the argument checks of the new C entry points."""
import glob
import math
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "rec-mv_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
REFERENCE = Path("/root/reference")


def _infer_fl():
    import importlib.util
    spec = importlib.util.spec_from_file_location("infer_fl", REPO / "rec-mv_amd" / "infer_fl.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_accepts_every_reference_flag():
    p = _infer_fl().build_parser()
    a = p.parse_args(['--gpu-ids', '0', '1', '--batch-size', '2', '--rec-root', 'cap/run', '--frames', '5', '--nV',
                      '--data-type', 'scene', '--nI', '--C', '--nColor', '--a_pose', '--conf', 'x.conf'])
    assert a.gpu_ids == [0, 1] and a.batch_size == 2 and a.rec_root == 'cap/run' and a.frames == 5
    assert a.nV and a.nI and a.C and a.nColor and a.a_pose and a.data_type == 'scene' and a.conf == 'x.conf'
    d = p.parse_args([])
    assert d.batch_size == 1 and d.frames == -1 and d.data_type == 'synthe' and d.conf is None
    assert not (d.nV or d.nI or d.C or d.nColor or d.a_pose)
    with pytest.raises(SystemExit):
        p.parse_args(['--frames'])                       # takes one value
    with pytest.raises(SystemExit):
        p.parse_args(['--nColor', 'yes'])                # a switch takes none


def _roundtrip(path):
    from recmv.hocon import ConfigFactory, HOCONConverter
    conf = ConfigFactory.parse_file(path)
    text = HOCONConverter.convert(conf, 'hocon')
    back = ConfigFactory.parse_string(text)
    assert back == conf, path
    assert HOCONConverter.convert(back, 'hocon') == text


def test_hocon_writer_round_trips_the_synthetic_configs():
    paths = sorted(glob.glob(str(REPO / "configs" / "synthetic" / "*.conf")))
    assert paths
    for p in paths:
        _roundtrip(p)


def test_hocon_writer_round_trips_odd_values():
    from recmv.hocon import ConfigFactory, ConfigTree, HOCONConverter
    conf = ConfigFactory.parse_string('a { b = "1.", c = [1, 2.5, "x y"], d = true, e = null, "f g" = 3 }\nh = -0.001\n'
                                      'i = "quote \\" and back\\\\slash"\nj {}')
    conf.put('k.l', 1e-7)
    back = ConfigFactory.parse_string(HOCONConverter.convert(conf))
    assert back == conf and isinstance(back.get_config('j'), ConfigTree)
    assert back.get_string('a.b') == '1.' and back.get_float('k.l') == 1e-7 and back['a']['f g'] == 3


def test_hocon_writer_round_trips_the_reference_configs():
    paths = sorted(glob.glob(str(REFERENCE / "configs" / "**" / "*.conf"), recursive=True))
    if not paths:
        pytest.skip("reference tree not available")
    assert len(paths) == 21
    for p in paths:
        _roundtrip(p)


def test_obj_ply_png_writers_round_trip(tmp_path):
    from recmv.dataset import read_image_bgr, write_image_bgr
    from recmv.utils import read_obj, read_ply, write_obj, write_ply
    rng = np.random.RandomState(0)
    v = torch.from_numpy(rng.randn(50, 3).astype(np.float32))
    f = torch.from_numpy(rng.randint(0, 50, (80, 3)).astype(np.int64))
    write_obj(str(tmp_path / "m.obj"), v, f)
    lines = (tmp_path / "m.obj").read_text().splitlines()
    assert lines[0] == "v %f %f %f" % tuple(v[0].tolist()) and lines[50] == "f %d %d %d" % tuple((f[0] + 1).tolist())
    v2, f2 = read_obj(str(tmp_path / "m.obj"))
    assert torch.equal(f2, f) and (v2 - v).abs().max() <= 5e-7
    write_ply(str(tmp_path / "m.ply"), v, f)
    v3, f3 = read_ply(str(tmp_path / "m.ply"))
    assert torch.equal(v3, v) and torch.equal(f3, f)
    for shape in ((7, 9, 3), (7, 9)):
        img = rng.randint(0, 256, shape).astype(np.uint8)
        write_image_bgr(str(tmp_path / "i.png"), img)
        back = read_image_bgr(str(tmp_path / "i.png"))
        assert np.array_equal(back, img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2))
    # the channel order on disk is cv2's: B,G,R in memory -> an RGB file
    from PIL import Image
    img = np.zeros((2, 2, 3), np.uint8)
    img[..., 0] = 200                                       # blue
    write_image_bgr(str(tmp_path / "b.png"), img)
    assert tuple(np.asarray(Image.open(tmp_path / "b.png"))[0, 0]) == (0, 0, 200)


def _triangle_case(flip=False, cam=(0., 2., 0.), texel=(0.5, 0.25, 1.0)):
    from phong_reference import hard_phong_ref, verts_normals_ref
    verts = torch.tensor([[[-1., 0., -1.], [0., 0., 1.], [1., 0., -1.]]])
    faces = torch.tensor([[0, 2, 1]] if flip else [[0, 1, 2]])
    normals = verts_normals_ref(verts[0], faces)[None]
    p2f = torch.tensor([0, -1]).view(1, 1, 2, 1)
    bary = torch.tensor([[0.25, 0.5, 0.25], [0., 0., 0.]]).view(1, 1, 2, 1, 3)
    if flip:
        bary = bary[..., [0, 2, 1]]
    colors = torch.tensor([texel] * 3).view(1, 3, 3)
    return normals, hard_phong_ref(p2f, bary, verts, faces, normals, colors, torch.tensor([cam]))


def test_phong_restatement_on_a_hand_computed_triangle():
    """Light straight above the shaded point (0,0,0) of a triangle in the plane y = 0: n.l = 1, so ambient 0.5 +
    diffuse 0.3; the reflection is +y, so a camera above sees specular 0.2 and one at 45 degrees 0.2 cos(45)^64."""
    texel = torch.tensor([0.5, 0.25, 1.0])
    normals, img = _triangle_case()
    assert torch.equal(normals[0], torch.tensor([[0., 1., 0.]] * 3))
    assert torch.allclose(img[0, 0, 0, :3], 0.8 * texel + 0.2, atol=1e-6, rtol=0)
    assert torch.equal(img[0, 0, 1], torch.tensor([1., 1., 1., 1.]))            # background + alpha 1
    assert img[0, 0, 0, 3] == 1.
    _, img = _triangle_case(cam=(0., 1., 1.))
    assert torch.allclose(img[0, 0, 0, :3], 0.8 * texel + 0.2 * math.sqrt(0.5) ** 64, atol=1e-7, rtol=0)
    # the other winding: the normal points down, away from the light -> ambient only
    normals, img = _triangle_case(flip=True)
    assert torch.equal(normals[0], torch.tensor([[0., -1., 0.]] * 3))
    assert torch.allclose(img[0, 0, 0, :3], 0.5 * texel, atol=1e-7, rtol=0)


def test_vertex_normal_restatement_sums_in_corner_order():
    """Area weighting and the corner order: a vertex shared by two faces gets the sum of both faces' cross products; a
    degenerate face adds nothing and an unreferenced vertex normalises to 0."""
    from phong_reference import verts_normals_ref
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., 2.], [5., 5., 5.], [1., 0., 0.]])
    f = torch.tensor([[0, 1, 2], [0, 3, 1], [1, 5, 1]])
    n = verts_normals_ref(v, f)
    expect0 = torch.tensor([0., 0., 1.]) + torch.tensor([0., 2., 0.])
    assert torch.allclose(n[0], expect0 / expect0.norm(), atol=1e-7)
    assert torch.equal(n[4], torch.zeros(3))


def test_new_abi_functions_check_arguments_without_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    assert lib.recmv_abi_version() == 11 == _lib.ABI_VERSION
    assert lib.recmv_verts_normals(None, None, None, None, 1, -1, 4, None, None) == _lib.C.c_int(-1).value
    assert b"verts_normals: bad sizes" in lib.recmv_last_error()
    assert lib.recmv_verts_normals(None, None, None, None, 0, 10, 4, None, None) == 0          # empty batch: no-op
    assert lib.recmv_verts_normals(None, None, None, None, 2, 10, 4, None, None) == -1
    assert b"NULL" in lib.recmv_last_error()
    nf = lib.recmv_hard_phong_params_floats()
    assert nf == 25
    params = (_lib.C.c_float * nf)()
    assert lib.recmv_hard_phong_shade(None, None, None, None, None, 1, None, None, 1, 3, 1, 0, 8, params, None, None, None,
                                      None) == -1                                                 # H = 0
    assert b"hard_phong_shade: bad sizes" in lib.recmv_last_error()
    assert lib.recmv_hard_phong_shade(None, None, None, None, None, 2, None, None, 3, 3, 1, 8, 8, params, None, None, None,
                                      None) == -1
    assert b"colors_batch" in lib.recmv_last_error()
    assert lib.recmv_hard_phong_shade(None, None, None, None, None, 1, None, None, 1, 3, 1, 8, 8, None, None, None, None,
                                      None) == -1
    assert b"params_host" in lib.recmv_last_error()
    assert lib.recmv_hard_phong_shade(None, None, None, None, None, 1, None, None, 1, 3, 1, 8, 8, params, None, None,
                                      _lib.C.c_void_p(16), None) == -1
    assert b"together" in lib.recmv_last_error()


def test_shading_refuses_host_tensors():
    from recmv import raster, shading
    v = torch.zeros(1, 3, 3)
    f = torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError):
        shading.verts_normals(v, f)
    with pytest.raises(RuntimeError):
        shading.vertex_face_adjacency(f, 3)
    frags = raster.Fragments(torch.zeros(1, 2, 2, 1, dtype=torch.int64), None, torch.zeros(1, 2, 2, 1, 3), None)
    with pytest.raises(RuntimeError):
        shading.hard_phong_shade(frags, v, f, v, v, torch.zeros(1, 3))


def test_pytorch3d_defaults():
    from recmv import shading
    lights, mat, blend = shading.PointLights(), shading.Materials(), shading.BlendParams()
    f32 = lambda x: [float(np.float32(x))] * 3                                  # noqa: E731  (float32 like pytorch3d's tensors)
    assert lights.ambient_color == f32(0.5) and lights.diffuse_color == f32(0.3) and lights.specular_color == f32(0.2)
    assert lights.location == [0., 1., 0.]
    assert mat.ambient_color == mat.diffuse_color == mat.specular_color == [1.] * 3 and mat.shininess == 64.
    assert blend.background_color == (1.0, 1.0, 1.0) and blend.sigma == 1e-4 and blend.gamma == 1e-4
