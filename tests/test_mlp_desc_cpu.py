"""The recmv_mlp descriptor's validation (csrc/mlp_desc.h) and the workspace layouts of the three MLP families, without a GPU.

Every call here returns before it reaches a HIP call: the descriptors carry dummy non-NULL pointers, and a VALID descriptor is only
ever handed to the host-side byte-count functions and recmv_mlp_rows_supported, never to an entry point that launches.
"""
import ctypes as C
import json
from pathlib import Path

import pytest

import mlp_reference as M

GOLDEN = Path(__file__).resolve().parent / "golden" / "mlp_workspace_bytes.json"
LAYOUT_NETS = ("sdf", "offset", "two")
LAYOUT_P = (1, 33, 257, 4096)
ERR_ARG = -1


def _lib():
    from recmv import _lib as L
    return L, L.lib()


def dummy_desc(m):
    """The descriptor of a net of mlp_reference with made-up, distinct, 256-byte aligned non-NULL pointers."""
    L, _ = _lib()
    d = L.Mlp()
    d.n_layers, d.multires, d.cond_dim, d.skip_layer = m["n"], m["L"], m["cond_dim"], m["skip"]
    d.hidden_act, d.residual, d.act_param = m["act"], int(m["residual"]), m["p"]
    for i, v in enumerate(m["dims"]):
        d.dims[i] = v
    for i in range(32):
        d.pe_weights[i] = 1.0
    ptr = iter(range(0x10000, 0x100000, 0x100))
    for l in range(m["n"]):
        d.rows[l] = m["rows"][l]
        d.W[l], d.Wt[l] = next(ptr), next(ptr)
        d.bias[l] = next(ptr) if m["b"][l] is not None else None
        if m["W2"] is not None:
            d.W2[l], d.Wt2[l] = next(ptr), next(ptr)
            d.bias2[l] = next(ptr) if m["b2"][l] is not None else None
    d.split_row = m["split"]
    return d


def byte_counts(lib, d, P):
    """The four byte-count functions of the MLP families for one descriptor and row count."""
    r = C.byref(d) if d is not None else None
    return {"mlp_keep0": lib.recmv_mlp_workspace_bytes(r, P, 0), "mlp_keep1": lib.recmv_mlp_workspace_bytes(r, P, 1),
            "jet": lib.recmv_mlp_jet_workspace_bytes(r, P), "rows": lib.recmv_mlp_rows_workspace_bytes(r, P),
            "pack": lib.recmv_mlp_pack_bytes(r)}


def layout_table(lib):
    return {name: {str(P): byte_counts(lib, dummy_desc(M.net(name)), P) for P in LAYOUT_P} for name in LAYOUT_NETS}


# ------------------------------------------------------------------------------------------------------------ entry points
_P = 4
_X, _OUT, _GX, _WS, _PK, _EYE, _TANG = (C.c_void_p(0x200000 + 0x1000 * i) for i in range(7))
_NB = 1 << 30
_PN = (C.c_void_p * M.MAX_LAYERS)()


def _entries(lib):
    """name -> call(descriptor reference) for the seven entry points that take a descriptor and may launch."""
    return {
        "mlp_forward": lambda r: lib.recmv_mlp_forward(r, _X, None, 0, None, _P, 1, _OUT, 1, _WS, _NB, 1, None),
        "mlp_vjp_input": lambda r: lib.recmv_mlp_vjp_input(r, _X, _P, 1, None, 0, _GX, _WS, _NB, None),
        "mlp_jet_forward": lambda r: lib.recmv_mlp_jet_forward(r, _X, None, 0, None, _EYE, _P, 1, _OUT, 8, _TANG, _WS, _NB, None),
        "mlp_jet_backward": lambda r: lib.recmv_mlp_jet_backward(r, _X, _EYE, _P, 1, None, 0, None, C.cast(_PN, C.c_void_p),
                                                                 C.cast(_PN, C.c_void_p), None, _GX, _WS, _NB, None),
        "mlp_rows_forward": lambda r: lib.recmv_mlp_rows_forward(r, _PK, _X, None, 0, None, _P, 1, _OUT, 1, _WS, _NB, 1, None),
        "mlp_rows_vjp_input": lambda r: lib.recmv_mlp_rows_vjp_input(r, _PK, _X, _P, 1, None, 0, _GX, _WS, _NB, None),
        "mlp_pack": lambda r: lib.recmv_mlp_pack(r, _PK, _NB, None),
    }


def _set(**fields):
    def change(d):
        for k, v in fields.items():
            setattr(d, k, v)
    return change


def _item(field, index, value):
    def change(d):
        getattr(d, field)[index] = value
    return change


# the SDF net: 4 layers, 6 bands (gamma is 39 wide), skip in front of layer 2: dims 39, 40, 25 + 39, 48, 7; rows 40, 25, 48, 7
MALFORMED = {
    "null": ("sdf", None),
    "n_layers_0": ("sdf", _set(n_layers=0)),
    "n_layers_13": ("sdf", _set(n_layers=13)),
    "multires_-1": ("sdf", _set(multires=-1)),
    "multires_17": ("sdf", _set(multires=17)),
    "cond_dim_-1": ("sdf", _set(cond_dim=-1)),
    "dims0_off_by_one": ("sdf", _item("dims", 0, 40)),
    "W_null": ("sdf", _item("W", 2, None)),
    "dims_l_zero": ("sdf", _item("dims", 3, 0)),
    "rows_plain_layer": ("sdf", _item("rows", 0, 41)),
    "rows_before_skip": ("sdf", _item("rows", 1, 64)),              # dims[2] without gamma's 39 columns taken off
    "skip_is_n_layers": ("sdf", _set(skip_layer=4)),
    "split_row_100": ("two", _set(split_row=100)),
    "bias2_missing": ("two", _item("bias2", 1, None)),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_descriptor_is_refused_by_every_entry_point(case):
    _, lib = _lib()
    name, change = MALFORMED[case]
    d = None
    if change is not None:
        d = dummy_desc(M.net(name))
        change(d)
    r = C.byref(d) if d is not None else None
    for entry, call in _entries(lib).items():
        assert call(r) == ERR_ARG, entry
        msg = lib.recmv_last_error().decode()
        assert msg.startswith(entry + ": "), (entry, msg)
    assert all(v == 0 for v in byte_counts(lib, d, 33).values())
    assert lib.recmv_mlp_rows_supported(r) == 0


def test_jet_refuses_a_second_weight_set():
    """A well-formed two-net descriptor: the chain's (its byte counts are in the layout table below), but not the jet's."""
    _, lib = _lib()
    d = dummy_desc(M.net("two"))
    for entry in ("mlp_jet_forward", "mlp_jet_backward"):
        assert _entries(lib)[entry](C.byref(d)) == ERR_ARG, entry
        assert lib.recmv_last_error().decode().startswith(entry + ": "), entry


def test_does_not_fit_leaves_the_last_error_alone():
    """A valid net with a 513-wide layer: the only reason for rows_supported == 0 is "too wide", which is an answer, not an error."""
    _, lib = _lib()
    d = dummy_desc(M.make_net("w513", 3, 1, [513, 8, 1], M.ACT_RELU))
    assert d.dims[1] == 513
    assert lib.recmv_mlp_pack(None, _PK, _NB, None) == ERR_ARG
    before = lib.recmv_last_error()
    assert before.startswith(b"mlp_pack: ")
    assert lib.recmv_mlp_rows_supported(C.byref(d)) == 0
    assert lib.recmv_last_error() == before
    assert lib.recmv_mlp_workspace_bytes(C.byref(d), 33, 1) > 0 and lib.recmv_mlp_jet_workspace_bytes(C.byref(d), 33) > 0
    d.dims[1], d.rows[0] = 512, 512
    assert lib.recmv_mlp_rows_supported(C.byref(d)) == 1


def test_workspace_layouts_are_those_of_the_recorded_library():
    """The byte counts of the chain, jet and row-tile workspaces and of the packed weights, recorded from the library before the
    layouts' offset carving was shared (tests/golden/make_golden_mlp_workspace_bytes.py)."""
    _, lib = _lib()
    want = json.loads(GOLDEN.read_text())["bytes"]
    got = layout_table(lib)
    assert got == want
    assert all(v > 0 for P in LAYOUT_P for k, v in got["sdf"][str(P)].items())
    assert all(got["two"][str(P)][k] == 0 for P in LAYOUT_P for k in ("rows", "pack"))          # one net only
