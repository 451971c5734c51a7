"""Texture baking without a GPU: the numpy restatement (tests/bake_reference.py) against exact arithmetic and on the hand cases of
tests/bake_cases.py; the gutter's order; tangent frames; fit_uv; the OBJ / MTL files and the PNG quantisation; flatten_fl.py's
parser; every ValueError of recmv.bake and its refusal of CPU tensors; the C entry points (declared, exported, argument errors
and empty no-ops before any HIP call); and the host build of the kernels under the sanitizers.
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE), str(REPO / "rec-mv_amd")]
import bake_cases as BC  # noqa: E402
import bake_reference as BR  # noqa: E402
import host_check  # noqa: E402
import param_cases as PC  # noqa: E402

NAMES = ["recmv_bake_raster", "recmv_bake_gutter", "recmv_bake_pad", "recmv_bake_interpolate", "recmv_bake_transfer",
         "recmv_bake_vertex_tangents", "recmv_bake_encode_normal"]
# (covered texels, texels with count 2, texels with count above 2) where the float64 rule equals exact arithmetic
TABLE = {"grid16": (256, 64, 0), "grid8": (64, 32, 0), "grid6x2": (12, 8, 4), "planar97x61": (3249, 0, 0)}


@functools.lru_cache(maxsize=None)
def raster(name):
    make, size, _ = BC.RASTER[name]
    uv, f = make()
    out = (uv, f, size) + BR.rasterize(uv, f, size)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", BC.EXACT)
def test_the_float64_rule_equals_exact_arithmetic_and_leaves_no_crack(name):
    uv, f, size, face, bary, count = raster(name)
    owner, exact_count = BR.rasterize_exact(uv, f, size)
    got = (int((face >= 0).sum()), int((count == 2).sum()), int((count > 2).sum()))
    print(name, size, "covered, count 2, count > 2:", got, "owner differs at", int((owner != face).sum()), "count at",
          int((exact_count != count).sum()))
    assert np.array_equal(face, owner) and np.array_equal(count, exact_count)
    assert got == TABLE[name]
    assert (face[exact_count > 0] >= 0).all()              # crack-freedom: what the geometry covers has an owner
    assert ((count > 0) == (face >= 0)).all()
    inside = bary[face >= 0].astype(np.float64)
    assert (inside >= 0).all() and np.abs(inside.sum(1) - 1).max() <= 3 * 2. ** -24


def test_where_the_rule_and_exact_arithmetic_part():
    """planar_irregular(9, seed 3) fitted with margin 1.5 at 33 x 29: the chart's border and many interior edges pass within a
    rounding error of texel centres, and the float64 formula decides 2 owners (3 counts) differently from exact arithmetic on
    the same inputs.  The formula is the definition; the geometry is not.  A case of the restatement only."""
    uv, f, size, face, _, count = raster("planar33x29")
    owner, exact_count = BR.rasterize_exact(uv, f, size)
    print("owner differs at", int((owner != face).sum()), "count at", int((exact_count != count).sum()))
    assert not np.array_equal(face, owner) and int((owner != face).sum()) == 2 and int((exact_count != count).sum()) == 3
    assert int((face >= 0).sum()) == 729 == int((owner >= 0).sum())


def test_hand_cases():
    for name, (_, _, reason) in BC.RASTER.items():
        assert reason and reason.strip(), name
    _, f, _, base, base_bary, base_count = raster("grid16")
    _, _, _, face, bary, count = raster("flipped")
    assert np.array_equal(face, base) and np.array_equal(count, base_count)
    mine = face == 3                                       # corners 1 and 2 swapped: so are their weights, bit for bit
    assert mine.sum() > 0 and np.array_equal(bary[mine][:, [0, 2, 1]], base_bary[mine])
    assert np.array_equal(bary[~mine], base_bary[~mine])
    _, _, _, face, bary, count = raster("zero_area")
    assert not (face == 0).any() and np.array_equal(face, base + 1) and np.array_equal(count, base_count)
    assert np.array_equal(bary, base_bary)
    _, _, _, face, bary, count = raster("overlap")
    assert np.array_equal(face, base) and np.array_equal(count, 2 * base_count) and face.max() < f.shape[0]
    uv, ft, size, face, bary, count = raster("outside")
    owner, exact_count = BR.rasterize_exact(uv, ft, size)
    assert np.array_equal(face, owner) and np.array_equal(count, exact_count)
    assert 0 < (face >= 0).sum() < face.size                                     # clipped on all four sides of the image
    assert (face[:, 0] >= 0).any() and (face[:, -1] >= 0).any() and (face[0] >= 0).any() and (face[-1] >= 0).any()
    _, _, _, face, bary, count = raster("one_texel")
    assert face.shape == (1, 1) and face[0, 0] == 10 and count[0, 0] == 8    # the centre is vertex 12: its eight faces, the lowest owns
    assert sorted(bary[0, 0].tolist()) == [0., 0., 1.]
    _, _, size, face, bary, count = raster("empty")
    assert face.shape == size and (face == -1).all() and (count == 0).all() and (bary == 0).all()
    uv, _, _, face, bary, count = raster("nan")
    bad = ~np.isfinite(uv[f]).all((1, 2))
    assert bad.sum() == 8 + 2 and not np.isin(face, np.nonzero(bad)[0]).any()
    kept = np.isin(base, np.nonzero(~bad)[0])
    assert (face[~kept] != base[~kept]).all() and not np.isnan(bary).any()
    assert np.array_equal(face[kept], base[kept]) and np.array_equal(bary[kept], base_bary[kept])
    _, fi, _, face, bary, count = raster("invalid")
    assert not np.isin(face, [0, 5, 9]).any() and (face >= 0).sum() == 238
    _, _, _, face, _, count = raster("big")
    assert (face >= 0).sum() == 3599 and count.max() == 1


def test_the_gutter_order():
    face = BC.island()
    H, W = face.shape
    own = np.arange(H * W, dtype=np.int32).reshape(H, W)
    s0 = BR.gutter(face, 0)
    assert np.array_equal(s0, np.where(face >= 0, own, -1))
    s1 = BR.gutter(face, 1)
    assert s1[4, 5] == own[4, 4]                           # W (4, 4) and E (4, 6) are both filled: W is tried first
    assert s1[3, 5] == own[3, 4] and s1[2, 3] == own[3, 3]     # W; S (N and the diagonals are empty or come later)
    assert s1[2, 1] == own[3, 2] and s1[5, 5] == own[4, 4]     # SE only; NW before NE (4, 6)
    assert s1[5, 6] == own[4, 6] and s1[5, 7] == own[4, 6] and s1[H - 2, W - 2] == own[H - 1, W - 1]
    assert (s1 >= 0).sum() == 6 + 14 + 6 + 3 + 1           # the block and its ring, the lone texel's part of a ring, the corner's
    assert s1[0, 0] == -1 and s1[4, 8] == -1
    s3 = BR.gutter(face, 3)
    assert np.array_equal(s3[s1 >= 0], s1[s1 >= 0]) and (s3 >= 0).sum() > (s1 >= 0).sum() and s3[0, W - 1] == -1
    assert s3[4, 8] == own[4, 6] and s3[1, 3] == s1[2, 3]      # pass 2 copies what pass 1 filled
    assert np.isin(s3[s3 >= 0], own[face >= 0]).all()
    full = np.zeros((5, 7), np.int32)
    for n in (0, 1, 3):
        assert np.array_equal(BR.gutter(full, n), np.arange(35, dtype=np.int32).reshape(5, 7))
    image = np.random.RandomState(0).rand(H, W, 3).astype(np.float32)
    padded = BR.pad(image, s3)
    assert np.array_equal(padded[face >= 0], image[face >= 0]) and (padded[s3 < 0] == 0).all()
    assert np.array_equal(padded[4, 8], image[4, 6])


def cap_chart(n=9):
    """cap(n) with the planar uv of its grid, fitted: (verts, faces, unit uv, unit vertex normals)."""
    v, f = PC.cap(n)
    uv = BR.fit_uv(v[:, :2].astype(np.float64), (48, 64), 2.)
    nrm = (v / np.linalg.norm(v.astype(np.float64), axis=1)[:, None]).astype(np.float32)        # a sphere's normals
    return v, f, uv, nrm


def test_tangent_frames():
    v, f, uv, nrm = cap_chart()
    tan = BR.vertex_tangents(v, f, uv, nrm)
    t, n = tan[:, :3].astype(np.float64), nrm.astype(np.float64)
    assert np.abs((t * t).sum(1) - 1).max() < 1e-6 and np.abs((t * n).sum(1)).max() < 1e-6
    assert (tan[:, 3] == 1).all()                          # uv = xy: cross(n, t) is the direction of growing v
    assert (t[:, 0] > 0.3).all() and (t[40] == [1., 0., 0.]).all()     # and t that of growing u = x (the pole has it exactly)
    mirrored = uv.copy()
    mirrored[:, 0] = 1. - uv[:, 0]
    flipped = BR.vertex_tangents(v, f, mirrored, nrm)
    assert (flipped[:, 3] == -1).all() and np.abs(flipped[:, :3] + tan[:, :3]).max() < 1e-6
    lonely = np.concatenate([v, np.array([[5., 5., 5.]], np.float32)], 0)      # a vertex without a face, a face without uv area
    uv2 = np.concatenate([uv, [[0.5, 0.5]]], 0)
    uv2[[0, 1, 10]] = uv2[0]
    out = BR.vertex_tangents(lonely, f, uv2, np.concatenate([nrm, [[0, 0, 1]]], 0).astype(np.float32))
    assert out[-1].tolist() == [0., 0., 0., 1.] and np.isfinite(out).all()
    enc = BR.encode_normal(np.array([0, -1], np.int32), nrm[[3, 3]], nrm[[3, 3]], tan[[3, 3]])
    assert np.abs(enc[0] - [0.5, 0.5, 1.]).max() < 1e-6 and (enc[1] == 0).all()       # the frame's own normal is (0, 0, 1)


def test_fit_uv_margins_and_aspect():
    from recmv import bake
    rng = np.random.RandomState(2)
    uv = rng.rand(40, 2) * [30., 7.] + [100., -50.]
    for size, margin in (((64, 64), 4.), ((48, 96), 2.5), ((200, 30), 0.)):
        H, W = size
        got = bake.fit_uv(torch.from_numpy(uv), size, margin)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), BR.fit_uv(uv, size, margin))
        tex = got.numpy() * [W, H]
        assert tex.min(0)[0] >= margin - 1e-9 and tex.min(0)[1] >= margin - 1e-9
        assert tex.max(0)[0] <= W - margin + 1e-9 and tex.max(0)[1] <= H - margin + 1e-9
        ext, want = np.ptp(tex, 0), np.ptp(uv, 0)
        assert abs(ext[0] / ext[1] - want[0] / want[1]) < 1e-9             # one scale in texels: the chart keeps its shape
        assert min(abs(ext[0] - (W - 2 * margin)), abs(ext[1] - (H - 2 * margin))) < 1e-9      # and touches one pair of margins
        assert np.abs((tex.min(0) + tex.max(0)) / 2 - [W / 2, H / 2]).max() < 1e-9           # centred
    assert np.array_equal(bake.fit_uv(torch.from_numpy(uv), 32, 1.).numpy(), BR.fit_uv(uv, (32, 32), 1.))
    for bad in (lambda: bake.fit_uv(torch.from_numpy(uv), (8, 8), 4.), lambda: bake.fit_uv(torch.from_numpy(uv[:1]), (8, 8), 1.),
                lambda: bake.fit_uv(torch.from_numpy(uv).float(), (8, 8), 1.), lambda: bake.fit_uv(torch.from_numpy(uv), (8, 8), -1.),
                lambda: bake.fit_uv(torch.full((3, 2), float("nan"), dtype=torch.float64), (8, 8), 1.)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------------- files
def test_obj_mtl_round_trip_and_png_quantisation(tmp_path):
    from PIL import Image
    from recmv import bake
    from recmv.dataset.dataset import write_image_bgr
    from recmv.utils.utils import read_obj, read_obj_uv, write_obj_uv_mtl
    v, f = (torch.from_numpy(x) for x in PC.grid(3))
    uv = v[:, :2].double() / 2.
    colors = torch.linspace(0, 1, 27).reshape(9, 3)
    maps = {"position": "a_position.npy", "normal": "a_normal.png", "tangent_normal": "a_tangent_normal.png", "color": "a_color.png"}
    write_obj_uv_mtl(str(tmp_path / "a.obj"), v, uv, f, maps, colors=colors)
    lines = (tmp_path / "a.obj").read_text().splitlines()
    assert lines[:2] == ["mtllib a.mtl", "usemtl baked"]
    assert [l.split()[0] for l in lines[2:]] == ["v"] * 9 + ["vt"] * 9 + ["f"] * 8
    assert lines[2 + 9 + 4] == "vt 0.50000000 0.50000000" and lines[2 + 18] == "f 1/1 4/4 5/5" and len(lines[2].split()) == 7
    r = read_obj_uv(str(tmp_path / "a.obj"))
    assert torch.equal(r["verts"], v) and torch.equal(r["faces"], f) and torch.equal(r["faces_uv"], f) and torch.equal(r["uv"], uv)
    assert torch.allclose(r["colors"], colors, atol=1e-6) and r["mtllib"] == "a.mtl" and r["usemtl"] == "baked"
    rv, rf = read_obj(str(tmp_path / "a.obj"))             # read_obj still reads what it read
    assert torch.equal(rv, v) and torch.equal(rf, f)
    mtl = (tmp_path / "a.mtl").read_text().splitlines()
    assert mtl[0] == "newmtl baked" and "map_Kd a_color.png" in mtl and "norm a_tangent_normal.png" in mtl
    assert "# normal a_normal.png" in mtl and "# position a_position.npy" in mtl
    write_obj_uv_mtl(str(tmp_path / "b.obj"), v, uv, f, {})
    r = read_obj_uv(str(tmp_path / "b.obj"))
    assert r["colors"] is None and torch.equal(r["uv"], uv)
    (tmp_path / "c.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    r = read_obj_uv(str(tmp_path / "c.obj"))
    assert r["uv"] is None and r["faces_uv"] is None and r["colors"] is None and r["mtllib"] is None
    x = torch.tensor([[[-0.2, 0., 0.004], [0.006, 0.0098, 0.999], [1., 7., float("nan")], [0.25, 0.5, 0.75]]])
    q = bake.quantise(x)
    assert q.dtype == np.uint8 and np.array_equal(q, BR.quantise(x.numpy()))
    assert q.tolist() == [[[0, 0, 1], [2, 2, 255], [255, 255, 0], [64, 128, 191]]]     # 127.5 goes to the even value
    write_image_bgr(str(tmp_path / "x.png"), q[:, :, ::-1])
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "x.png"))), q)        # red first in the file


def test_flatten_fl_parser_with_bake(capsys, tmp_path):
    import flatten_fl
    help_text = flatten_fl.build_parser().format_help()
    for option in ("--bake SIZE", "--bake-source", "--bake-maps", "--bake-gutter", "--bake-projection", "--bake-lanes"):
        assert option in help_text and option.split()[0] in flatten_fl.__doc__
    a = flatten_fl.build_parser().parse_args(["--in", ".", "--out", "x"])
    assert a.bake is None and a.bake_gutter == 4 and a.bake_projection == "closest" and a.bake_lanes is None
    assert a.bake_maps == "position,normal,tangent_normal,color"
    base = ["--in", str(tmp_path), "--out", str(tmp_path / "o")]
    for extra in (["--bake", "0"], ["--bake", "x"], ["--bake", "32", "--bake-gutter", "-1"], ["--bake", "8", "--bake-gutter", "4"],
                  ["--bake", "32", "--bake-maps", "normal,albedo"], ["--bake", "32", "--bake-maps", ""],
                  ["--bake", "32", "--bake-projection", "ray"], ["--bake", "32", "--bake-lanes", "16"],
                  ["--bake", "32", "--bake-source", str(tmp_path / "none.obj")]):
        with pytest.raises(SystemExit):                    # a parser.error, before any mesh is read
            flatten_fl.main(base + extra)
        assert "usage:" in capsys.readouterr().err
    (tmp_path / "s.obj").write_text("v 0 0 0\n")
    assert flatten_fl._bake_source(None, "a.obj") is None and flatten_fl._bake_source(str(tmp_path), "a.obj") is None
    assert flatten_fl._bake_source(str(tmp_path), "s.obj") == str(tmp_path / "s.obj")
    assert flatten_fl._bake_source(str(tmp_path / "s.obj"), "a.obj") == str(tmp_path / "s.obj")


# ---------------------------------------------------------------------------------------------- recmv.bake's arguments
def test_argument_errors_and_cpu_tensors():
    from recmv import bake
    assert bake.LANES == (8, 64) and bake.MAPS == ("position", "normal", "tangent_normal", "color") and bake.MAX_CHANNELS == 16
    v, f = (torch.from_numpy(x) for x in PC.grid(5))
    uv = v[:, :2].double() / 4.
    face, bary = torch.zeros(8, 8, dtype=torch.int32), torch.zeros(8, 8, 3)
    n = torch.zeros(25, 3)
    hit, point = torch.zeros(4, dtype=torch.int64), torch.zeros(4, 3)
    bad = [lambda: bake.rasterize_uv(uv.float(), f, 8), lambda: bake.rasterize_uv(uv, f.int(), 8), lambda: bake.rasterize_uv(uv, f, -1),
           lambda: bake.rasterize_uv(uv, f, (1 << 16, 1 << 15)), lambda: bake.rasterize_uv(uv, f, 8, lanes=16),
           lambda: bake.rasterize_uv(uv[:, :1], f, 8), lambda: bake.rasterize_uv(uv, f[:, :2], 8),
           lambda: bake.gutter(face.long()), lambda: bake.gutter(face, -1), lambda: bake.gutter(face[0]),
           lambda: bake.pad(bary, face[:4]), lambda: bake.pad(bary.double(), face), lambda: bake.pad(bary, face.long()),
           lambda: bake.interpolate(face, bary[:4], f, v), lambda: bake.interpolate(face, bary, f, v.double()),
           lambda: bake.interpolate(face, bary, f, torch.zeros(25, 17)), lambda: bake.interpolate(face, bary, f, v[:, :2], normalise=True),
           lambda: bake.interpolate(face.long(), bary, f, v), lambda: bake.interpolate(face, bary, f.int(), v),
           lambda: bake.vertex_tangents(v, f, uv[:24], n), lambda: bake.vertex_tangents(v, f, uv, n[:24]),
           lambda: bake.vertex_tangents(v.double(), f, uv, n), lambda: bake.vertex_tangents(v, f, uv.float(), n),
           lambda: bake.encode_normal(face, bary, bary, bary), lambda: bake.encode_normal(face.long(), bary, bary, torch.zeros(8, 8, 4)),
           lambda: bake.project(point, point, v, f, projection='ray'), lambda: bake.project(point, point[:3], v, f),
           lambda: bake.project(point, point, v, f, max_distance=0.), lambda: bake.project(point.double(), point, v, f),
           lambda: bake.transfer(hit.int(), point, v, f, n), lambda: bake.transfer(hit, point[:3], v, f, n),
           lambda: bake.transfer(hit, point, v, f, n[:24]), lambda: bake.transfer(hit, point, v, f, torch.zeros(25, 17)),
           lambda: bake.transfer(hit, point, v, f, n[:, :2].contiguous(), normalise=True),
           lambda: bake.scatter(torch.zeros(3, 2, 2), face), lambda: bake.scatter(torch.zeros(3), face, size=9),
           lambda: bake.bake(v, f, uv, 16, maps=('albedo',)), lambda: bake.bake(v, f, uv, 16, projection='ray'),
           lambda: bake.bake(v, f, uv, 16, gutter=-1), lambda: bake.bake(v, f, uv[:24], 16), lambda: bake.bake(v.double(), f, uv, 16),
           lambda: bake.bake(v, f, uv, 16, colors=n[:24]), lambda: bake.bake(v, f, uv, 16, source=(v,)),
           lambda: bake.bake(v, f, uv, 16, source=(v, f, n[:24])), lambda: bake.bake(v, f, uv, -16)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d raised nothing" % k)
    for call in (lambda: bake.rasterize_uv(uv, f, 8), lambda: bake.gutter(face), lambda: bake.pad(bary, face),
                 lambda: bake.interpolate(face, bary, f, v), lambda: bake.vertex_tangents(v, f, uv, n),
                 lambda: bake.encode_normal(face, bary, bary, torch.zeros(8, 8, 4)), lambda: bake.project(point, point, v, f),
                 lambda: bake.transfer(hit, point, v, f, n), lambda: bake.texels(face, bary, f, v),
                 lambda: bake.scatter(torch.zeros(64, 3), face), lambda: bake.bake(v, f, uv, 16)):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            call()
    fwd, bwd = bake.choose_hits(np.array([1, 1, 1, 0, 0], bool), np.array([.2, .3, .2, np.nan, np.nan]),
                                np.array([1, 1, 0, 1, 0], bool), np.array([.2, .1, np.nan, .4, np.nan]))
    assert fwd.tolist() == [True, False, True, False, False] and bwd.tolist() == [False, True, False, True, False]


# ------------------------------------------------------------------------------------------------------------ the C ABI
ONE = C.c_void_p(256)                                      # a pointer nobody reads: the errors come first


def test_symbols_are_declared_and_exported():
    from recmv import _lib
    declared = _lib.exported_symbols()
    lib = _lib.lib()
    for n in NAMES:
        assert n in declared and hasattr(lib, n)
    assert sorted(n for n in declared if n.startswith("recmv_bake_")) == sorted(NAMES)
    assert lib.recmv_abi_version() == _lib.ABI_VERSION
    hdr = (REPO / "include" / "recmv_hip.h").read_text()
    note = hdr[:hdr.index("int recmv_abi_version")]
    for n in NAMES:
        assert n in note
    assert "(texture baking: pure additions, still v%d)" % _lib.ABI_VERSION in note
    assert "(mesh parameterisation: pure additions, still v11)" in note           # the earlier phrases stand


def test_a_library_without_the_symbols_is_rejected():
    from recmv import _lib

    class Partial:
        def __init__(self, missing):
            self.missing = missing

        def __getattr__(self, name):
            if name == self.missing:
                raise AttributeError(name)
            return getattr(_lib.lib(), name)
    for n in NAMES:
        with pytest.raises(AttributeError, match=n):
            _lib._declare(Partial(n))


def test_c_argument_errors_and_empty_inputs_do_not_need_a_gpu():
    from recmv import _lib
    lib = _lib.lib()
    err = lib.recmv_last_error

    def raster_(*, uv=ONE, V=9, faces=ONE, F=8, H=4, W=4, lanes=8, out=(ONE, ONE, ONE)):
        return lib.recmv_bake_raster(uv, V, faces, F, H, W, lanes, *out, None)
    assert raster_(V=-9) == -1 and b"V=-9" in err() and b"bake_raster:" in err()
    assert raster_(F=-8) == -1 and b"F=-8" in err()
    assert raster_(V=1 << 31) == -1 and b"2^31" in err() and raster_(F=1 << 31) == -1 and b"2^31" in err()
    assert raster_(H=-4) == -1 and b"H=-4" in err() and raster_(W=-4) == -1 and b"W=-4" in err()
    assert raster_(H=1 << 16, W=1 << 15) == -1 and b"2^31 - 1" in err()
    for lanes in (0, 1, 16, 63, -8):
        assert raster_(lanes=lanes) == -1 and b"lanes=%d must be 8 or 64" % lanes in err()
    for k in range(3):
        out = [ONE, ONE, ONE]
        out[k] = None
        assert raster_(out=tuple(out)) == -1 and b"NULL image" in err()
    assert raster_(uv=None) == -1 and b"NULL pointer of the mesh" in err()
    assert raster_(faces=None) == -1 and b"NULL pointer of the mesh" in err()
    assert raster_(H=0, out=(None, None, None)) == 0 and raster_(W=0, uv=None, faces=None, out=(None, None, None)) == 0

    def gutter_(*, face=ONE, H=4, W=4, passes=2, src=ONE, scratch=ONE):
        return lib.recmv_bake_gutter(face, H, W, passes, src, scratch, None)
    assert gutter_(H=-1) == -1 and b"H=-1" in err() and gutter_(passes=-2) == -1 and b"passes=-2" in err()
    assert gutter_(H=1 << 16, W=1 << 15) == -1 and b"2^31 - 1" in err()
    assert gutter_(face=None) == -1 and b"NULL image" in err() and gutter_(src=None) == -1 and b"NULL image" in err()
    assert gutter_(scratch=None) == -1 and b"NULL scratch" in err()
    assert gutter_(H=0, face=None, src=None, scratch=None) == 0

    pad_ = lib.recmv_bake_pad
    assert pad_(ONE, ONE, -1, 3, ONE, None) == -1 and b"T=-1" in err() and pad_(ONE, ONE, 4, -3, ONE, None) == -1 and b"C=-3" in err()
    assert pad_(ONE, ONE, 1 << 31, 3, ONE, None) == -1 and b"2^31" in err()
    assert pad_(None, ONE, 4, 3, ONE, None) == -1 and b"NULL pointer" in err()
    assert pad_(ONE, ONE, 4, 3, ONE, None) == -1 and b"must not be the image" in err()
    assert pad_(None, None, 0, 3, None, None) == 0 and pad_(None, None, 4, 0, None, None) == 0

    def mix_(*, face=ONE, bary=ONE, T=16, faces=ONE, F=8, attr=ONE, V=9, Cn=3, normalise=0, out=ONE):
        return lib.recmv_bake_interpolate(face, bary, T, faces, F, attr, V, Cn, normalise, out, None)
    assert mix_(T=-16) == -1 and b"T=-16" in err() and mix_(V=-9) == -1 and b"V=-9" in err() and mix_(F=-8) == -1 and b"F=-8" in err()
    assert mix_(T=1 << 31) == -1 and b"2^31" in err()
    for c in (0, 17, -1):
        assert mix_(Cn=c) == -1 and (b"C=%d must be 1 .. 16" % c in err() or b"C=-1" in err())
    assert mix_(Cn=2, normalise=1) == -1 and b"normalise needs C >= 3" in err()
    for k in ("face", "bary", "out"):
        assert mix_(**{k: None}) == -1 and b"NULL image" in err()
    assert mix_(faces=None) == -1 and b"NULL pointer of the mesh" in err() and mix_(attr=None) == -1 and b"of the mesh" in err()
    assert mix_(T=0, face=None, bary=None, out=None) == 0

    def transfer_(*, hit=ONE, point=ONE, T=16, verts=ONE, V=9, faces=ONE, F=8, attr=ONE, Cn=3, normalise=0, bary=ONE, out=ONE):
        return lib.recmv_bake_transfer(hit, point, T, verts, V, faces, F, attr, Cn, normalise, bary, out, None)
    assert transfer_(T=-16) == -1 and b"T=-16" in err() and b"bake_transfer:" in err()
    assert transfer_(V=1 << 31) == -1 and b"2^31" in err() and transfer_(Cn=17) == -1 and b"C=17" in err()
    assert transfer_(Cn=1, normalise=1) == -1 and b"normalise needs C >= 3" in err()
    for k in ("hit", "point", "bary", "out"):
        assert transfer_(**{k: None}) == -1 and b"NULL pointer of the hits" in err()
    for k in ("verts", "faces", "attr"):
        assert transfer_(**{k: None}) == -1 and b"NULL pointer of the source" in err()
    assert transfer_(T=0, hit=None, point=None, bary=None, out=None) == 0

    def tangents_(*, verts=ONE, uv=ONE, normals=ONE, V=9, faces=ONE, F=8, off=ONE, codes=ONE, out=ONE):
        return lib.recmv_bake_vertex_tangents(verts, uv, normals, V, faces, F, off, codes, out, None)
    assert tangents_(V=-9) == -1 and b"V=-9" in err() and tangents_(F=(1 << 31) // 3 + 1) == -1 and b"(2^31 - 1) / 3" in err()
    for k in ("verts", "uv", "normals", "off", "out"):
        assert tangents_(**{k: None}) == -1 and b"NULL pointer of the vertices" in err()
    for k in ("faces", "codes"):
        assert tangents_(**{k: None}) == -1 and b"NULL pointer of the faces" in err()
    assert tangents_(V=0, verts=None, uv=None, normals=None, off=None, out=None) == 0

    enc = lib.recmv_bake_encode_normal
    assert enc(ONE, ONE, ONE, ONE, -4, ONE, None) == -1 and b"T=-4" in err()
    assert enc(ONE, ONE, ONE, ONE, 1 << 31, ONE, None) == -1 and b"2^31" in err()
    for k in (0, 1, 2, 3, 5):
        a = [ONE, ONE, ONE, ONE, 4, ONE]
        a[k] = None
        assert enc(*a, None) == -1 and b"NULL pointer" in err()
    assert enc(None, None, None, None, 0, None, None) == 0


# ------------------------------------------------------------------------------------------------------ the host build
def test_host_build_of_the_kernels_equals_the_plain_loops(tmp_path, monkeypatch):
    """tools/texture_bake_host_check: csrc/texture_bake.hip's kernels compiled for the CPU under the address and
    undefined-behaviour sanitizers as a stand-alone program — the rasteriser with 8 and 64 lanes, the gutter, the padding, the
    interpolation, the transfer, the tangents and the encoding against plain loops, bit for bit, on five inputs."""
    monkeypatch.setitem(host_check.CHECKS, "texture_bake", ((("texture_bake.hip", "bake.inc"),), ()))
    r = host_check.run("texture_bake", tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count("-> 0 mismatches") == 5, r.stdout + r.stderr
    for name in ("a jittered 7 x 9 grid with flawed faces and coordinates: 63 vertices, 97 faces, 37 x 29 texels, 688 covered",
                 "the grid partly outside the unit square: 63 vertices, 96 faces, 16 x 24 texels, 384 covered",
                 "one triangle over 96 x 80 texels: 4 vertices, 1 faces, 96 x 80 texels, 3496 covered",
                 "a 1 x 1 image: 9 vertices, 8 faces, 1 x 1 texels, 1 covered, 1 shared",
                 "a mesh without faces: 9 vertices, 0 faces, 5 x 4 texels, 0 covered"):
        assert name in r.stdout
