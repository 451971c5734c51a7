"""The inputs of the texture-baking tests, each with its reason: (uv [V,2] float64 in unit coordinates, faces [F,3] int64, (H, W)).
The meshes are those of param_cases."""
import numpy as np

import bake_reference as BR
import param_cases as PC


def grid_uv(n=5):
    """grid(n) with uv = xy / (n - 1): the unit square, every coordinate a multiple of 1 / 4 for n = 5."""
    v, f = PC.grid(n)
    return v[:, :2].astype(np.float64) / (n - 1), f


def planar(n, seed, margin, size):
    """planar_irregular's isometric uv fitted into the image."""
    _, f, xy = PC.planar_irregular(n, seed)
    return BR.fit_uv(xy, size, margin), f


def flipped():
    """grid(5) with face 3 turned round (two corners swapped): A < 0, the three E negated, the same texels covered."""
    uv, f = grid_uv()
    f = f.copy()
    f[3] = f[3, [0, 2, 1]]
    return uv, f


def zero_area():
    """grid(5) and a face over three vertices of one grid line (A == 0) at the lowest id: it covers nothing and owns nothing."""
    uv, f = grid_uv()
    return uv, np.concatenate([np.array([[0, 5, 10]], np.int64), f], 0)


def overlap():
    """Two copies of grid(5) on top of each other: the lowest id wins, count is 2 inside the faces (4 on the shared edges)."""
    uv, f = grid_uv()
    return np.concatenate([uv, uv], 0), np.concatenate([f, f + uv.shape[0]], 0)


def outside():
    """A triangle partly outside [0,1]^2 on three sides: the box is clipped to the image."""
    return np.array([[-0.3, 0.2], [1.4, -0.2], [0.45, 1.3]]), np.array([[0, 1, 2]], np.int64)


def empty():
    """F = 0: nothing is covered."""
    return np.zeros((3, 2)), np.zeros((0, 3), np.int64)


def nan_uv():
    """grid(5) with one vertex at NaN and one at infinity: their faces cover nothing, the others what they did."""
    uv, f = grid_uv()
    uv = uv.copy()
    uv[12, 0] = np.nan
    uv[3, 1] = np.inf
    return uv, f


def invalid_rows():
    """grid(5) with an index outside [0, V), a negative index and a repeated corner: those rows cover nothing."""
    uv, f = grid_uv()
    f = f.copy()
    f[0, 1], f[5, 2], f[9, 1] = 25, -1, f[9, 0]
    return uv, f


def big_triangle():
    """One triangle over a 96 x 80 image: its box (7680 texels) exceeds one pass of 64 lanes 120 times."""
    return np.array([[0.01, 0.02], [0.99, 0.03], [0.4, 0.98]]), np.array([[0, 1, 2]], np.int64)


# name -> (builder of (uv, faces), (H, W), reason)
RASTER = {
    "grid16": (grid_uv, (16, 16), "edges between the centres: every texel covered once, the diagonals' centres twice"),
    "grid8": (grid_uv, (8, 8), "centres on the diagonals"),
    "grid6x2": (grid_uv, (2, 6), "6 columns, 2 rows: centres on vertices (columns 1 and 4)"),
    "planar97x61": (lambda: planar(17, 5, 2., (61, 97)), (61, 97), "irregular, non-square, more than one workgroup of texels"),
    "planar33x29": (lambda: planar(9, 3, 1.5, (29, 33)), (29, 33), "the float64 rule and exact arithmetic part at 2 texels"),
    "flipped": (flipped, (16, 16), flipped.__doc__),
    "zero_area": (zero_area, (16, 16), zero_area.__doc__),
    "overlap": (overlap, (16, 16), overlap.__doc__),
    "outside": (outside, (13, 11), outside.__doc__),
    "one_texel": (grid_uv, (1, 1), "a 1 x 1 image: the centre (0.5, 0.5) is a vertex of the grid"),
    "empty": (empty, (7, 5), empty.__doc__),
    "nan": (nan_uv, (16, 16), nan_uv.__doc__),
    "invalid": (invalid_rows, (16, 16), invalid_rows.__doc__),
    "big": (big_triangle, (96, 80), big_triangle.__doc__),
}
EXACT = ("grid16", "grid8", "grid6x2", "planar97x61")      # the float64 rule equals exact arithmetic on these


def island(H=9, W=11):
    """A face image with one covered 2 x 3 block, one lone texel two columns from it (the texel between them has a W and an E
    candidate: W wins) and one in a corner."""
    face = np.full((H, W), -1, np.int32)
    face[3:5, 2:5] = 7
    face[4, 6] = 9
    face[H - 1, W - 1] = 1
    return face
