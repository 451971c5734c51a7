"""The argument checks of the mesh toolkit, once: what a mesh, a point set and a CSR table are, and which part of an info dict
is JSON.  Shapes and dtypes first (ValueError), then the device (RuntimeError): the argument errors do not need a GPU.
"""
import torch

from . import _lib as L

_PLAIN = (bool, int, float, str, type(None))


def check_mesh(verts, faces, *, cuda=True, allow_empty=True, float_verts=False, cap31=False, names=("verts", "faces")):
    """verts [V,3] float32 (any floating type with `float_verts`) and faces [F,3] int64 on one device -> the contiguous pair.
    `cap31`: fewer than 2^31 vertices and faces; `allow_empty=False`: at least one of each; `cuda`: both on the GPU."""
    vn, fn = names
    if not (isinstance(verts, torch.Tensor) and isinstance(faces, torch.Tensor)):
        raise ValueError("%s and %s must be tensors" % (vn, fn))
    if verts.dim() != 2 or verts.shape[1] != 3 or not (verts.dtype.is_floating_point if float_verts else verts.dtype == torch.float32):
        raise ValueError("%s must be %s of shape [V,3]" % (vn, "floating point" if float_verts else "float32"))
    if faces.dtype != torch.int64 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("%s must be int64 of shape [F,3]" % fn)
    if verts.device != faces.device:
        raise ValueError("%s and %s must be on one device" % (vn, fn))
    if cap31 and (verts.shape[0] >= 1 << 31 or faces.shape[0] >= 1 << 31):
        raise ValueError("at most 2^31 - 1 vertices and faces")
    if not allow_empty and (faces.shape[0] == 0 or verts.shape[0] == 0):
        raise ValueError("the surface is empty")
    if cuda:
        L.require_cuda(verts, vn)
        L.require_cuda(faces, fn)
    return verts.contiguous(), faces.contiguous()


def check_points(p, name, *, cuda=True, shape="[N,3]"):
    """p [N,3] float32 -> p.contiguous(); `shape` is how the message writes the shape."""
    if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != 3:
        raise ValueError("%s must be float32 of shape %s" % (name, shape))
    if cuda:
        L.require_cuda(p, name)
    return p.contiguous()


def check_csr(csr, rows, dtype, name):
    """(offsets [rows + 1], entries) of `dtype` -> the contiguous pair."""
    off, idx = csr
    if off.dtype != dtype or idx.dtype != dtype or off.dim() != 1 or idx.dim() != 1 or off.numel() != rows + 1:
        raise ValueError("%s must be (offsets [%d], entries) of %s" % (name, rows + 1, dtype))
    return off.contiguous(), idx.contiguous()


def info_json(info):
    """The JSON-able part of an info dict: numbers, strings and None, lists and tuples of them (as lists), and nested dicts
    likewise; tensors and everything else are left out."""
    out = {}
    for k, x in info.items():
        if isinstance(x, dict):
            out[k] = info_json(x)
        elif isinstance(x, _PLAIN):
            out[k] = x
        elif isinstance(x, (tuple, list)) and all(isinstance(y, _PLAIN) for y in x):
            out[k] = list(x)
    return out
