"""Mesh + camera -> the capture entries' two inputs: face normals and the pixel-to-face map (brdf_amd/csrc/pixel_map.hip).

face_normals / pixel_map run on the device; face_normals_host / pixel_map_host are their NumPy twins -- the definitions of
include/brdf_levmar.h as code, operation for operation, so the device results have the twins' bytes.  The helpers below them build
the three arrays an application would read with glGetDoublev / glGetIntegerv, without a GL context: gl_frustum, gl_look_at, the
reference's MakeFrustum, and the calibrated pinhole of a Tsai .cal file."""
from __future__ import annotations

import ctypes as C
import math
import re
from typing import NamedTuple

import numpy as np

from ._lib import D
from .fit import _STREAM, _call, _check_indices, _f64, _require

STAT_NAMES = ("faces_rasterised", "faces_unprojectable", "faces_degenerate", "faces_culled", "faces_outside", "candidates", "pixels_owned",
              "writes_refused")
INT_MAX = 2 ** 31 - 1


class PixelMap(NamedTuple):
    pixel_map: object    # [H, W] int32: face index or -1, row y = window row y (bottom-up)
    depth: object        # [H, W] float64 or None: the owner's window z, 2.0 where no face owns the pixel
    face_pixels: object  # [nf] int32 or None: the pixels each face owns
    stats: np.ndarray    # [8] int64, in the order of STAT_NAMES


# ---- the device entries ---------------------------------------------------------------------------------------------------------------
def _mesh(vertices, faces, validate):
    import torch
    vertices, faces = vertices.contiguous(), faces.contiguous()
    _require(vertices.is_cuda and faces.is_cuda, "bad argument: vertices.is_cuda and faces.is_cuda")
    _require(vertices.dtype == torch.float64 and faces.dtype == torch.int32, "bad argument: vertices.dtype == torch.float64 and faces.dtype == torch.int32")
    _require(vertices.dim() == 2 and faces.dim() == 2 and vertices.shape[1] == 3 and faces.shape[1] == 3, "bad argument: vertices [nv,3], faces [nf,3]")
    if validate:
        _check_indices(faces, vertices.shape[0], "face index outside the vertex array")
    return vertices, faces


def face_normals(vertices, faces, *, validate: bool = True):
    """CalcFaceNormals (brdfdata.cpp:314-330) on the device (brdf_hip_face_normals_dev): vertices [nv,3] float64, faces [nf,3] int32,
    CUDA tensors -> CUDA float64 [nf,3] with the bytes of face_normals_host.  validate=False: a face with a vertex index outside
    [0, nv) gets a NaN normal instead of a ValueError."""
    import torch
    vertices, faces = _mesh(vertices, faces, validate)
    out = torch.empty((faces.shape[0], 3), dtype=torch.float64, device=vertices.device)
    _call("brdf_hip_face_normals_dev", vertices.device, vertices.data_ptr(), int(vertices.shape[0]), faces.data_ptr(), int(faces.shape[0]),
          out.data_ptr(), _STREAM)
    return out


def pixel_map(vertices, faces, model_view, projection, viewport, H: int, W: int, *, mode: int = 1, cull: int = 0, want_depth: bool = False,
              want_face_pixels: bool = True, validate: bool = True) -> PixelMap:
    """The pixel map of a mesh under a camera on the device (brdf_hip_pixel_map_dev).  model_view, projection: 16 values each,
    column-major as glGetDoublev returns them; viewport: (x, y, width, height); mode 1: rasterised and z-buffered, mode 0: the
    reference's one-pixel-per-centroid map; cull=1 drops the faces of negative window-space area.  The result has the bytes of
    pixel_map_host.  validate=False: a face with a vertex index outside [0, nv) is dropped as unprojectable instead of a ValueError."""
    import torch
    vertices, faces = _mesh(vertices, faces, validate)
    mv, pr, vp = _f64(model_view, 16), _f64(projection, 16), _f64(viewport, 4)
    _require(1 <= int(H) and 1 <= int(W) and int(H) * int(W) <= INT_MAX, f"bad argument: H = {H}, W = {W}: need H, W >= 1 and H W <= INT_MAX")
    dev = vertices.device
    pm = torch.empty((int(H), int(W)), dtype=torch.int32, device=dev)
    depth = torch.empty((int(H), int(W)), dtype=torch.float64, device=dev) if want_depth else None
    fp = torch.empty((faces.shape[0],), dtype=torch.int32, device=dev) if want_face_pixels else None
    stats = np.zeros(8, dtype=np.int64)
    _call("brdf_hip_pixel_map_dev", dev, vertices.data_ptr(), int(vertices.shape[0]), faces.data_ptr(), int(faces.shape[0]), mv.ctypes.data_as(D),
          pr.ctypes.data_as(D), vp.ctypes.data_as(D), int(H), int(W), int(mode), int(cull), pm.data_ptr(), depth.data_ptr() if want_depth else None,
          fp.data_ptr() if want_face_pixels else None, stats.ctypes.data_as(C.POINTER(C.c_longlong)), _STREAM)
    return PixelMap(pm, depth, fp, stats)


# ---- the twins --------------------------------------------------------------------------------------------------------------------------
def _corners(vertices, faces):
    """([nf,3] per corner, [nf] bool: all three indices inside [0, nv)); faces with a bad index read vertex 0"""
    vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    good = np.all((faces >= 0) & (faces < vertices.shape[0]), axis=1)
    idx = np.where(good[:, None], faces, 0)
    return vertices[idx[:, 0]], vertices[idx[:, 1]], vertices[idx[:, 2]], good


def face_normals_host(vertices, faces) -> np.ndarray:
    """CalcFaceNormals: n = (v2 - v1) x (v3 - v1), then Eigen's normalize(): divided by sqrt((n0^2 + n1^2) + n2^2) where that sum is
    > 0, left as it is otherwise.  A face with a vertex index outside [0, nv): NaN."""
    a, b, c, good = _corners(vertices, faces)
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        z = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        s = np.sqrt(np.where(z > 0.0, z, 1.0))
        n = np.where((z > 0.0)[:, None], n / s[:, None], n)
    n[~good] = np.nan
    return n


def project_host(points, model_view, projection, viewport):
    """gluProject's arithmetic on [n,3] points: (win [n,3], clip w [n], ok [n] bool: w != 0 and everything finite)"""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    m, q, vp = _f64(model_view, 16), _f64(projection, 16), _f64(viewport, 4)
    with np.errstate(all="ignore"):
        e = [((p[:, 0] * m[i] + p[:, 1] * m[4 + i]) + p[:, 2] * m[8 + i]) + m[12 + i] for i in range(4)]
        c = [((e[0] * q[i] + e[1] * q[4 + i]) + e[2] * q[8 + i]) + e[3] * q[12 + i] for i in range(4)]
        ok = (c[3] != 0.0) & np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & np.isfinite(c[3])
        d = np.where(ok, c[3], 1.0)
        win = np.stack([(c[0] / d * 0.5 + 0.5) * vp[2] + vp[0], (c[1] / d * 0.5 + 0.5) * vp[3] + vp[1], c[2] / d * 0.5 + 0.5], axis=1)
        ok &= np.all(np.isfinite(win), axis=1)
    return win, c[3], ok


def _check_camera(model_view, projection, viewport, H, W, mode, cull):
    _require(int(H) >= 1 and int(W) >= 1 and int(H) * int(W) <= INT_MAX, f"bad argument: H = {H}, W = {W}: need H, W >= 1 and H W <= INT_MAX")
    _require(mode in (0, 1) and cull in (0, 1), f"bad argument: mode = {mode}, cull = {cull}: need 0 or 1 each")
    mv, pr, vp = _f64(model_view, 16), _f64(projection, 16), _f64(viewport, 4)
    _require(bool(np.all(np.isfinite(mv)) and np.all(np.isfinite(pr)) and np.all(np.isfinite(vp))), "bad argument: need finite matrices and viewport")
    _require(vp[2] > 0.0 and vp[3] > 0.0, "bad argument: need a viewport of positive width and height")
    return mv, pr, vp


def pixel_map_host(vertices, faces, model_view, projection, viewport, H: int, W: int, *, mode: int = 1, cull: int = 0) -> PixelMap:
    """brdf_hip_pixel_map_dev's definition in NumPy (include/brdf_levmar.h), every operation in the entry's order: the same bytes.
    Vectorised over all candidates (face, box pixel) at once: memory grows with their number."""
    H, W = int(H), int(W)
    mv, pr, vp = _check_camera(model_view, projection, viewport, H, W, mode, cull)
    a, b, c, good = _corners(vertices, faces)
    nf = a.shape[0]
    _require(1 <= nf <= INT_MAX, "bad argument: need 1 <= nf <= INT_MAX")
    stats = np.zeros(8, dtype=np.int64)
    pm = np.full(H * W, -1, dtype=np.int32)
    depth = np.full(H * W, 2.0)
    if mode == 0:
        with np.errstate(all="ignore"):
            win, _, ok = project_host(((a + b) + c) / 3.0, mv, pr, vp)
        ok &= good
        inside = ok & (win[:, 1] >= 0.0) & (win[:, 0] >= 0.0)
        refused = inside & ((win[:, 0] >= W) | (win[:, 1] >= H))
        written = inside & ~refused
        f = np.nonzero(written)[0]  # ascending: the last write of a pixel is the highest index
        pix = win[f, 1].astype(np.int64) * W + win[f, 0].astype(np.int64)
        pm[pix] = f
        owned = pm >= 0
        depth[owned] = win[pm[owned], 2]
        stats[[0, 1, 4, 7]] = written.sum(), (~ok).sum(), (ok & ~inside).sum(), refused.sum()
    else:
        wa, qa, oka = project_host(a, mv, pr, vp)
        wb, qb, okb = project_host(b, mv, pr, vp)
        wc, qc, okc = project_host(c, mv, pr, vp)
        with np.errstate(all="ignore"):
            ok = good & oka & okb & okc & (qa > 0.0) & (qb > 0.0) & (qc > 0.0)
            A = (wb[:, 0] - wa[:, 0]) * (wc[:, 1] - wa[:, 1]) - (wb[:, 1] - wa[:, 1]) * (wc[:, 0] - wa[:, 0])
            degenerate = ok & ((A == 0.0) | ~np.isfinite(A))
            culled = ok & ~degenerate & (A < 0.0) & bool(cull)
            minx, maxx = np.minimum(np.minimum(wa[:, 0], wb[:, 0]), wc[:, 0]), np.maximum(np.maximum(wa[:, 0], wb[:, 0]), wc[:, 0])
            miny, maxy = np.minimum(np.minimum(wa[:, 1], wb[:, 1]), wc[:, 1]), np.maximum(np.maximum(wa[:, 1], wb[:, 1]), wc[:, 1])
            live = ok & ~degenerate & ~culled
            outside = live & ((maxx < 0.0) | (minx > W) | (maxy < 0.0) | (miny > H))
            raster = live & ~outside
            x0, x1 = np.maximum(np.ceil(minx - 0.5), 0.0), np.minimum(np.floor(maxx - 0.5), W - 1.0)
            y0, y1 = np.maximum(np.ceil(miny - 0.5), 0.0), np.minimum(np.floor(maxy - 0.5), H - 1.0)
            boxed = raster & (x0 <= x1) & (y0 <= y1)
        fs = np.nonzero(boxed)[0]
        bx0, by0 = x0[fs].astype(np.int64), y0[fs].astype(np.int64)
        bw = x1[fs].astype(np.int64) - bx0 + 1
        count = bw * (y1[fs].astype(np.int64) - by0 + 1)
        first = np.concatenate([[0], np.cumsum(count)])
        T = int(first[-1])
        k = np.repeat(np.arange(fs.size), count)  # candidate -> its place among the boxed faces
        r = np.arange(T, dtype=np.int64) - first[k]
        row, col = by0[k] + r // bw[k], bx0[k] + r % bw[k]
        f = fs[k]
        px, py = col + 0.5, row + 0.5
        ax, ay, az, bx, by, bz, cx, cy, cz = wa[f, 0], wa[f, 1], wa[f, 2], wb[f, 0], wb[f, 1], wb[f, 2], wc[f, 0], wc[f, 1], wc[f, 2]
        with np.errstate(all="ignore"):
            E0 = (bx - px) * (cy - py) - (by - py) * (cx - px)
            E1 = (cx - px) * (ay - py) - (cy - py) * (ax - px)
            E2 = (ax - px) * (by - py) - (ay - py) * (bx - px)
            s = np.where(A[f] > 0.0, 1.0, -1.0)
            z = ((E0 * az + E1 * bz) + E2 * cz) / A[f]
            covered = (s * E0 >= 0.0) & (s * E1 >= 0.0) & (s * E2 >= 0.0) & (z >= 0.0) & (z <= 1.0)
        z = np.where(z == 0.0, 0.0, z)[covered]
        pix, f = (row * W + col)[covered], f[covered]
        order = np.lexsort((f, z, pix))  # by pixel, then depth (non-negative doubles order as their bits), then face index
        pix, f, z = pix[order], f[order], z[order]
        lead = np.ones(pix.size, dtype=bool)
        lead[1:] = pix[1:] != pix[:-1]
        pm[pix[lead]] = f[lead]
        depth[pix[lead]] = z[lead]
        stats[:6] = raster.sum(), (~ok).sum(), degenerate.sum(), culled.sum(), outside.sum(), T
    stats[6] = (pm >= 0).sum()
    face_pixels = np.bincount(pm[pm >= 0], minlength=nf).astype(np.int32)
    return PixelMap(pm.reshape(H, W), depth.reshape(H, W), face_pixels, stats)


# ---- matrices without a GL context ---------------------------------------------------------------------------------------------------------
def gl_frustum(l, r, b, t, n, f) -> np.ndarray:
    """glFrustum's matrix, column-major [16]"""
    m = np.zeros(16)
    m[0], m[5] = 2.0 * n / (r - l), 2.0 * n / (t - b)
    m[8], m[9], m[10], m[11] = (r + l) / (r - l), (t + b) / (t - b), -(f + n) / (f - n), -1.0
    m[14] = -2.0 * f * n / (f - n)
    return m


def gl_look_at(eye, centre, up) -> np.ndarray:
    """gluLookAt's matrix, column-major [16]: f = normalize(centre - eye), s = normalize(f x up), u = s x f; rows s, u, -f; then the
    translation by -eye"""
    eye, centre, up = _f64(eye, 3), _f64(centre, 3), _f64(up, 3)
    f = centre - eye
    f = f / np.sqrt(f @ f)
    s = np.cross(f, up)
    s = s / np.sqrt(s @ s)
    u = np.cross(s, f)
    m = np.zeros(16)
    m[0:12:4], m[1:12:4], m[2:12:4] = s, u, -f
    m[12], m[13], m[14], m[15] = -(s @ eye), -(u @ eye), f @ eye, 1.0
    return m


def make_frustum(fovy_deg, aspect, near, far, cx, cy, H, W) -> np.ndarray:
    """The reference's MakeFrustum (glutcallbacks.cpp:626-642): an asymmetric glFrustum from (fovy, aspect, near, far), shifted by the
    principal point (cx, cy) of an H x W image -- with its DEG2RAD = 3.14159265 / 180 and its offsets as written there."""
    deg2rad = 3.14159265 / 180
    tangent = math.tan(fovy_deg / 2 * deg2rad)
    height = near * tangent
    width = height * aspect
    offset_y = 2.0 * (H / 2.0 - cy) / H
    offset_x = 2.0 * (W / 2.0 - cx) / W
    return gl_frustum(-width + offset_x, width + offset_x, -height - offset_y, height - offset_y, near, far)


CAL_TAGS = ("cx", "cy", "f", "sx", "kappa1", "nx", "ny", "nz", "ox", "oy", "oz", "ax", "ay", "az", "px", "py", "pz")


def parse_cal(text: str) -> dict:
    """The flat <tag>value</tag> lines of a Tsai .cal file -> {"camera_model": str, every tag of CAL_TAGS: float}.
    An unknown tag, a tag given twice, a missing one or a closing tag that does not match raises ValueError."""
    out = {}
    for line in text.splitlines():
        line = line.strip()
        if not line:
            continue
        m = re.fullmatch(r"<(\w+)>(.*)</(\w+)>", line)
        _require(m is not None and m.group(1) == m.group(3), f"parse_cal: not a <tag>value</tag> line: {line!r}")
        tag, value = m.group(1), m.group(2).strip()
        _require(tag == "camera_model" or tag in CAL_TAGS, f"parse_cal: unknown tag <{tag}>")
        _require(tag not in out, f"parse_cal: <{tag}> given twice")
        out[tag] = value if tag == "camera_model" else float(value)
    missing = [t for t in ("camera_model",) + CAL_TAGS if t not in out]
    _require(not missing, f"parse_cal: missing tags {missing}")
    return out


def tsai_camera(cal: dict, H: int, W: int, near: float, far: float):
    """(model_view [16], projection [16], viewport (0, 0, W, H)) of the calibrated pinhole of a parsed .cal, for pixel_map:
        Xc = (n . (X - p), o . (X - p), a . (X - p)),  u = cx + sx f Xc.x / Xc.z,  v = cy + f Xc.y / Xc.z
    and a world point lands at winX = u, winY = H - v (image row v counted from the top, window rows from the bottom), with depth
    increasing along a from `near` to `far`.  kappa1, the radial distortion, is IGNORED.  The convention is this project's own: the
    reference never uses n, o, a, f, sx for its map (it looks from (0, 0, 50))."""
    n, o, a, p = (np.array([cal[k + "x"], cal[k + "y"], cal[k + "z"]]) for k in "noap")
    mv = np.zeros(16)  # eye space looks down -z with y up: rows n, -o, -a
    mv[0:12:4], mv[1:12:4], mv[2:12:4] = n, -o, -a
    mv[12], mv[13], mv[14], mv[15] = -(n @ p), o @ p, a @ p, 1.0
    pr = np.zeros(16)
    pr[0], pr[5] = 2.0 * cal["sx"] * cal["f"] / W, 2.0 * cal["f"] / H
    pr[8], pr[9] = 1.0 - 2.0 * cal["cx"] / W, 2.0 * cal["cy"] / H - 1.0
    pr[10], pr[11], pr[14] = -(far + near) / (far - near), -1.0, -2.0 * far * near / (far - near)
    return mv, pr, np.array([0.0, 0.0, float(W), float(H)])
