"""Cast shadows: which lights each face's centre can see, and that visibility painted into images (brdf_amd/csrc/light_visibility.hip).

light_visibility / apply_visibility run on the device; light_visibility_host / apply_visibility_host are their NumPy twins -- the
definitions of include/brdf_levmar.h as code, operation for operation, so the device results have the twins' bytes.  A face's
visibility is one 64-bit word, bit l for light l; it travels as an int64 tensor or array holding the bit pattern (bit 63 is the sign
bit).  lit_matrix unpacks it."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from ._lib import D
from .fit import _STREAM, _call, _out_tensor, _require
from .raster import INT_MAX, _corners, _mesh

STAT_NAMES = ("faces_valid", "faces_invalid", "pairs_facing_away", "pairs_lit", "pairs_shadowed")
MAX_L = 64


class LightVisibility(NamedTuple):
    face_lit: object   # [nf] int64 (CUDA tensor, or ndarray from the twin): bit l set iff light l is visible from the face's centre
    stats: np.ndarray  # [5] int64, in the order of STAT_NAMES


class AppliedVisibility(NamedTuple):
    images: object    # [L, H, W, 3] uint8: the input's bytes, `level` where the pixel's face does not see the image's light
    shadowed: object  # [L] int64: the painted pixels per light


def _rig(leds, t_min):
    la = np.ascontiguousarray(np.asarray(leds, dtype=np.float64)).reshape(-1, 3)
    _require(1 <= la.shape[0] <= MAX_L, f"bad argument: L = {la.shape[0]}: need 1 <= L <= {MAX_L}")
    _require(bool(np.all(np.isfinite(la))), "bad argument: need finite light positions")
    t_min = float(t_min)
    _require(0.0 <= t_min < 0.5, f"bad argument: t_min = {t_min}: need 0 <= t_min < 0.5")
    return la, t_min


# ---- the device entries ---------------------------------------------------------------------------------------------------------------
def light_visibility(vertices, faces, leds, *, normals=None, t_min: float = 1e-9, validate: bool = True) -> LightVisibility:
    """Per-light face visibility on the device (brdf_hip_light_visibility_dev): vertices [nv,3] float64, faces [nf,3] int32, normals
    [nf,3] float64 or None: CUDA tensors; leds [L,3], 1 <= L <= 64: host.  Bit l of face_lit[f] is set iff no valid face other than f
    lies between f's centre and light l (and, with normals, f does not face away from it).  Brute force over all pairs of faces: meant
    to run once per capture session.  The result has the bytes of light_visibility_host.  validate=False: a face with a vertex index
    outside [0, nv) is invalid (lit = 0, occludes nothing) instead of a ValueError."""
    import torch
    vertices, faces = _mesh(vertices, faces, validate)
    la, t_min = _rig(leds, t_min)
    nf, dev = int(faces.shape[0]), vertices.device
    if normals is not None:
        normals = normals.contiguous()
        _require(normals.is_cuda and normals.device == dev and normals.dtype == torch.float64 and tuple(normals.shape) == (nf, 3),
                 "bad argument: normals: CUDA float64 [nf,3] on the mesh's device")
    lit = torch.empty((nf,), dtype=torch.int64, device=dev)
    stats = np.zeros(5, dtype=np.int64)
    _call("brdf_hip_light_visibility_dev", dev, vertices.data_ptr(), int(vertices.shape[0]), faces.data_ptr(), nf,
          None if normals is None else normals.data_ptr(), la.ctypes.data_as(D), int(la.shape[0]), t_min, lit.data_ptr(),
          stats.ctypes.data_as(C.POINTER(C.c_longlong)), _STREAM)
    return LightVisibility(lit, stats)


def apply_visibility(images, pixel_map, face_lit, *, level: int = 0, out=None) -> AppliedVisibility:
    """Paint a visibility word into images (brdf_hip_capture_apply_visibility_dev): images [L,H,W,3] uint8, pixel_map [H,W] int32,
    face_lit [nf] int64: CUDA tensors.  Where map pixel (y, x) carries a face that does not see light l, the three bytes of image l at
    row H-1-y, column x become `level`; every other byte is the input's.  out: None (a new tensor), `images` itself (in place) or
    another tensor of its shape.  With level=0 and v_min >= 1 every capture entry leaves the shadowed samples out.  The result has the
    bytes of apply_visibility_host."""
    import torch
    _require(torch.is_tensor(images) and images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[3] == 3 and images.is_contiguous(),
             "bad argument: images: contiguous CUDA uint8 [L,H,W,3]")
    L, H, W = (int(n) for n in images.shape[:3])
    dev = images.device
    _require(1 <= L <= MAX_L, f"bad argument: L = {L}: need 1 <= L <= {MAX_L}")
    _require(torch.is_tensor(pixel_map) and pixel_map.is_cuda and pixel_map.device == dev and pixel_map.dtype == torch.int32 and tuple(pixel_map.shape) == (H, W)
             and pixel_map.is_contiguous(), "bad argument: pixel_map: contiguous CUDA int32 [H,W] on the images' device")
    _require(torch.is_tensor(face_lit) and face_lit.is_cuda and face_lit.device == dev and face_lit.dtype == torch.int64 and face_lit.dim() == 1
             and face_lit.is_contiguous() and face_lit.shape[0] >= 1, "bad argument: face_lit: contiguous CUDA int64 [nf] on the images' device")
    _require(0 <= int(level) <= 255, f"bad argument: level = {level}: need 0 ... 255")
    if out is None:
        out = torch.empty_like(images)
    elif out is not images:
        out = _out_tensor(out, (L, H, W, 3), torch.uint8, dev, "out", torch)
    shadowed = torch.empty((L,), dtype=torch.int64, device=dev)
    _call("brdf_hip_capture_apply_visibility_dev", dev, images.data_ptr(), L, H, W, pixel_map.data_ptr(), face_lit.data_ptr(), int(face_lit.shape[0]),
          int(level), out.data_ptr(), shadowed.data_ptr(), _STREAM)
    return AppliedVisibility(out, shadowed)


def lit_matrix(face_lit, L: int):
    """face_lit [nf] int64 (tensor or array) -> bool [nf, L]: entry (f, l) is bit l of face f's word"""
    _require(1 <= int(L) <= MAX_L, f"bad argument: L = {L}: need 1 <= L <= {MAX_L}")
    try:
        import torch
        if torch.is_tensor(face_lit):
            _require(face_lit.dtype == torch.int64 and face_lit.dim() == 1, "bad argument: face_lit: int64 [nf]")
            return ((face_lit[:, None] >> torch.arange(int(L), device=face_lit.device)[None, :]) & 1).bool()  # (an arithmetic shift: bit l all the same)
    except ImportError:  # pragma: no cover - torch is part of this image
        pass
    words = np.ascontiguousarray(face_lit, dtype=np.int64).reshape(-1).view(np.uint64)
    return ((words[:, None] >> np.arange(int(L), dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


# ---- the twins --------------------------------------------------------------------------------------------------------------------------
def _dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross3(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def light_visibility_host(vertices, faces, leds, *, normals=None, t_min: float = 1e-9, rows: int = 128) -> LightVisibility:
    """brdf_hip_light_visibility_dev's definition in NumPy (include/brdf_levmar.h), every operation in the entry's order: the same
    bytes.  All nf occluders against `rows` origins at a time: memory grows with rows * nf, time with nf^2 L."""
    la, t_min = _rig(leds, t_min)
    a, b, c, good = _corners(vertices, faces)
    nf, L = a.shape[0], la.shape[0]
    _require(1 <= nf <= INT_MAX, "bad argument: need 1 <= nf <= INT_MAX")
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
        _require(normals.shape[0] == nf, "bad argument: normals [nf,3]")
    lit = np.zeros(nf, dtype=np.uint64)
    stats = np.zeros(5, dtype=np.int64)
    with np.errstate(all="ignore"):
        valid = good & np.all(np.isfinite(a), axis=1) & np.all(np.isfinite(b), axis=1) & np.all(np.isfinite(c), axis=1)
        o = ((a + b) + c) / 3.0
        v0, e1, e2 = a[None], (b - a)[None], (c - a)[None]  # [1,nf,3]: the occluders
        for f0 in range(0, nf, rows):
            f1 = min(f0 + rows, nf)
            own = np.arange(f0, f1)
            s = o[f0:f1, None, :] - v0       # [m,nf,3]
            q = _cross3(s, e1)
            T = _dot3(e2, q)
            blocks = np.broadcast_to(valid[None, :], T.shape).copy()  # an invalid face occludes nothing,
            blocks[own - f0, own] = False                              # and no face shadows itself
            for l in range(L):
                d = la[l] - o[f0:f1]         # [m,3]
                toward = valid[f0:f1] & (np.ones(f1 - f0, dtype=bool) if normals is None else _dot3(normals[f0:f1], d) > 0.0)
                dd = d[:, None, :]
                h = _cross3(dd, e2)
                aa = _dot3(e1, h)
                U, V = _dot3(s, h), _dot3(dd, q)
                neg = aa < 0.0
                A, Un, Vn, Tn = np.abs(aa), np.where(neg, -U, U), np.where(neg, -V, V), np.where(neg, -T, T)
                hit = (A > 0.0) & (Un >= 0.0) & (Vn >= 0.0) & (Un + Vn <= A) & (Tn > t_min * A) & (Tn < (1.0 - t_min) * A)
                dark = np.any(hit & blocks, axis=1)
                lit[f0:f1] |= (toward & ~dark).astype(np.uint64) << np.uint64(l)
                stats[2] += int((valid[f0:f1] & ~toward).sum())
                stats[3] += int((toward & ~dark).sum())
                stats[4] += int((toward & dark).sum())
    stats[0], stats[1] = int(valid.sum()), int((~valid).sum())
    return LightVisibility(lit.view(np.int64), stats)


def apply_visibility_host(images, pixel_map, face_lit, *, level: int = 0, out=None) -> AppliedVisibility:
    """brdf_hip_capture_apply_visibility_dev's definition in NumPy: images [L,H,W,3] uint8, pixel_map [H,W], face_lit [nf] int64.
    out: None (a new array), `images` itself (in place) or another uint8 array of its shape."""
    images, pixel_map = np.asarray(images), np.asarray(pixel_map)
    _require(images.ndim == 4 and images.shape[3] == 3 and images.dtype == np.uint8 and pixel_map.shape == images.shape[1:3],
             "bad argument: images [L,H,W,3] uint8, pixel_map [H,W]")
    L = images.shape[0]
    _require(1 <= L <= MAX_L, f"bad argument: L = {L}: need 1 <= L <= {MAX_L}")
    _require(0 <= int(level) <= 255, f"bad argument: level = {level}: need 0 ... 255")
    words = np.ascontiguousarray(face_lit, dtype=np.int64).reshape(-1)
    nf = words.shape[0]
    _require(nf >= 1, "bad argument: face_lit [nf], nf >= 1")
    if out is None:
        out = images.copy()
    elif out is not images:
        _require(isinstance(out, np.ndarray) and out.shape == images.shape and out.dtype == np.uint8, "bad argument: out: uint8 [L,H,W,3]")
        out[...] = images
    flipped = pixel_map[::-1]  # image row r is map row H - 1 - r
    carried = (flipped > -1) & (flipped < nf)
    lit = np.zeros(flipped.shape + (L,), dtype=bool)
    lit[carried] = lit_matrix(words, L)[flipped[carried]]
    dark = (carried[:, :, None] & ~lit).transpose(2, 0, 1)  # [L,H,W]
    out[dark] = int(level)
    return AppliedVisibility(out, dark.reshape(L, -1).sum(axis=1).astype(np.int64))
