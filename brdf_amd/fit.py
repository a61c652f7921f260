"""Python host API over the C ABI: torch CUDA(=HIP) tensors provide the device memory and stream."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from ._lib import D, I, ExtraData, last_error, lib

MODEL_PHONG, MODEL_BLINN_PHONG, MODEL_WARD = 0, 1, 2
METHOD_DIF, METHOD_BC_DIF, METHOD_BC_DER, METHOD_DER = 0, 1, 2, 3  # 2 / 3: dlevmar_bc_der / dlevmar_der with the analytic Jacobian


@dataclass
class FitResult:
    ret: int  # number of iterations, or -1 (LM_ERROR)
    p: np.ndarray  # fitted parameters [3]
    info: np.ndarray  # levmar info[10]
    covar: np.ndarray | None = None


def _require(cond: bool, what: str) -> None:
    """Argument check that survives `python -O` (an `assert` would not): a bad shape, dtype or index must never reach a kernel."""
    if not cond:
        raise ValueError(what)


def _dptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(D)


def _iptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(I)


def _f64(v, size):
    if v is None:
        return None
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    _require(a.size == size, f"expected {size} values, got {a.size}")
    return a


def _stream_handle(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_STREAM = object()  # among _call's arguments: the current stream of the call's device


def _call(name: str, device, *args) -> None:
    """lib.<name>(*args) with `device` current (None: a host-pointer entry, no device scope); a non-zero return raises RuntimeError
    with the library's error text."""
    if device is None:
        rc = getattr(lib, name)(*args)
    else:
        import torch
        with torch.cuda.device(device):
            stream = _stream_handle(torch)
            rc = getattr(lib, name)(*(stream if a is _STREAM else a for a in args))
    if rc != 0:
        raise RuntimeError(f"{name} failed: {last_error()}")


# brdf_hip_fit_dev once more, with plain addresses for its pointer arguments: ndarray.ctypes.data_as() costs ~3 us per pointer and a
# single-fit call passes seven of them -- more host time than the launch itself.  One scratch array per call, one base address.
_FIT_DEV = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(("brdf_hip_fit_dev", lib))
_OFF_P, _OFF_LB, _OFF_UB, _OFF_DS, _OFF_OPTS, _OFF_INFO, _OFF_COVAR, _SCRATCH = 0, 3, 6, 9, 12, 17, 27, 36


def fit_single(method: int, model: int, angles, x, p0, *, lb=None, ub=None, dscl=None, itmax=100, opts=None,
               want_covar=False) -> FitResult:
    """One fit over device-resident samples.  angles: CUDA float64 tensor [3,n] (or [3n]), x: [n].

    Mirrors a dlevmar_dif / dlevmar_bc_dif call (levmar.h:112-127) with the samples already in HBM.
    """
    import torch
    _require(angles.is_cuda and x.is_cuda and angles.dtype == torch.float64 and x.dtype == torch.float64, "angles, x: CUDA float64 tensors")
    if not angles.is_contiguous():
        angles = angles.contiguous()
    if not x.is_contiguous():
        x = x.contiguous()
    n = x.numel()
    _require(angles.numel() == 3 * n, "angles must hold 3 planes of x.numel() doubles")
    buf = np.zeros(_SCRATCH)  # p | lb | ub | dscl | opts | info | covar: the call's host arguments and results
    base = buf.ctypes.data

    def put(off, v, size):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float64).reshape(-1)
        _require(a.size == size, f"expected {size} values, got {a.size}")
        buf[off:off + size] = a
        return base + 8 * off

    p_ptr = put(_OFF_P, p0, 3)
    _require(p_ptr is not None, "p0 is required")
    args = (method, model, angles.data_ptr(), x.data_ptr(), n, p_ptr, put(_OFF_LB, lb, 3), put(_OFF_UB, ub, 3), put(_OFF_DS, dscl, 3), itmax,
            put(_OFF_OPTS, opts, 5), base + 8 * _OFF_INFO, (base + 8 * _OFF_COVAR) if want_covar else None)
    dev = x.device
    if torch.cuda.current_device() == (dev.index if dev.index is not None else torch.cuda.current_device()):
        ret = _FIT_DEV(*args, torch.cuda.current_stream().cuda_stream)
    else:
        with torch.cuda.device(dev):
            ret = _FIT_DEV(*args, torch.cuda.current_stream().cuda_stream)
    return FitResult(ret, buf[_OFF_P:_OFF_P + 3].copy(), buf[_OFF_INFO:_OFF_INFO + 10].copy(),
                     buf[_OFF_COVAR:_OFF_COVAR + 9].reshape(3, 3).copy() if want_covar else None)


def fit_channels(method: int, model: int, angles, x, p0, *, lb=None, ub=None, dscl=None, itmax=100, opts=None, want_covar=False,
                 x_stride=None):
    """K fits over ONE set of planes (brdf_hip_fit_channels_dev): the three colour channels of a capture, as the reference's
    callers fit them (brdfdata.cpp:1159-1181).  angles: CUDA float64 [3,n]; x: CUDA float64 [K,n]; p0: [K,3] (or [3]: the same
    start for every channel).  x_stride (optional): x is [K,x_stride] and channel c's n = angles.numel() / 3 measurements are the
    first n of its row (the ABI's x_stride > n; what lies behind them is never read).
    Returns a list of K FitResult; `last_channels_stats()` tells whether they shared one launch."""
    import torch
    _require(angles.is_cuda and x.is_cuda and angles.dtype == torch.float64 and x.dtype == torch.float64, "angles, x: CUDA float64 tensors")
    angles, x = angles.contiguous(), x.contiguous()
    if x_stride is None:
        _require(x.dim() == 2 and angles.numel() == 3 * x.shape[1], "angles [3,n], x [K,n]")
        x_stride = int(x.shape[1])
    _require(x.dim() == 2 and angles.numel() % 3 == 0 and int(x.shape[1]) == int(x_stride) >= angles.numel() // 3 > 0,
             "angles [3,n], x [K,x_stride] with x_stride >= n")
    K, n = int(x.shape[0]), angles.numel() // 3
    p = np.ascontiguousarray(np.broadcast_to(np.asarray(p0, dtype=np.float64).reshape(-1, 3), (K, 3))).copy()
    info = np.zeros((K, 10))
    covar = np.zeros((K, 9)) if want_covar else None
    lba, uba, dsa = _f64(lb, 3), _f64(ub, 3), _f64(dscl, 3)
    oa = _f64(opts, 5) if opts is not None else None
    with torch.cuda.device(angles.device):
        rc = lib.brdf_hip_fit_channels_dev(method, model, angles.data_ptr(), x.data_ptr(), int(x_stride), n, K, _dptr(p), _dptr(lba), _dptr(uba),
                                           _dptr(dsa), itmax, _dptr(oa), _dptr(info), _dptr(covar), _stream_handle(torch))
    out = []
    for c in range(K):
        failed = info[c, 6] in (4, 7) or (rc != 0 and info[c, 6] == 0)  # levmar's LM_ERROR cases (lm_core.c:841); the ABI returns the worst channel
        out.append(FitResult(-1 if failed else int(info[c, 5]), p[c].copy(), info[c].copy(), None if covar is None else covar[c].reshape(3, 3).copy()))
    return out


def last_channels_stats(channels: int = 3):
    """per channel of the last fit_channels(): passes, jac_passes, device_us; and whether the channels shared one launch"""
    shared = C.c_int(0)
    per = []
    for c in range(channels):
        passes, jac, us = C.c_longlong(0), C.c_longlong(0), C.c_double(0.0)
        lib.brdf_hip_last_channels_stats(c, C.byref(shared), C.byref(passes), C.byref(jac), C.byref(us))
        per.append({"passes": passes.value, "jac_passes": jac.value, "device_us": us.value})
    return {"shared_launch": bool(shared.value), "channels": per, "kernel_us": lib.brdf_hip_last_channels_kernel_us()}


def compact_samples(angles, x, valid):
    """Stable front-compaction of the valid samples of S fits: angles [S,3,n], x [S,n], valid [S,n] (bool) -> (angles, x, counts)
    of the same shapes and kind (torch tensors on the inputs' device, or numpy arrays), counts [S] int32.  Fit s's valid samples,
    in their order, are its samples [0, counts[s]); the entries behind them are NaN (a ragged fit never uses them).  What
    fit_capture_masked does on the device, for callers that build their own batches: fit_batch(..., counts=counts)."""
    if isinstance(x, np.ndarray):
        valid = np.asarray(valid, dtype=bool)
        _require(x.ndim == 2 and angles.shape == (x.shape[0], 3, x.shape[1]) and valid.shape == x.shape, "angles [S,3,n], x [S,n], valid [S,n]")
        order = np.argsort(~valid, axis=1, kind="stable")  # valid samples first, each group in its own order
        counts = valid.sum(axis=1).astype(np.int32)
        keep = np.arange(x.shape[1])[None, :] < counts[:, None]
        xo = np.where(keep, np.take_along_axis(x, order, axis=1), np.nan)
        ao = np.where(keep[:, None, :], np.take_along_axis(angles, np.broadcast_to(order[:, None, :], angles.shape), axis=2), np.nan)
        return ao, xo, counts
    import torch
    valid = valid.to(torch.bool)
    _require(x.dim() == 2 and tuple(angles.shape) == (x.shape[0], 3, x.shape[1]) and valid.shape == x.shape, "angles [S,3,n], x [S,n], valid [S,n]")
    order = torch.sort((~valid).to(torch.int8), dim=1, stable=True).indices
    counts = valid.sum(dim=1).to(torch.int32)
    keep = torch.arange(x.shape[1], device=x.device)[None, :] < counts[:, None]
    nan = torch.full((), float("nan"), dtype=x.dtype, device=x.device)
    xo = torch.where(keep, torch.gather(x, 1, order), nan)
    ao = torch.where(keep[:, None, :], torch.gather(angles, 2, order[:, None, :].expand(angles.shape)), nan)
    return ao, xo, counts


def _counts_arg(counts, S, device, torch):
    _require(counts.is_cuda and counts.device == device and counts.dtype == torch.int32 and tuple(counts.shape) == (S,),
             "counts: CUDA int32 [S] on the device of x")
    return counts.contiguous()


def fit_batch(method: int, model: int, angles, x, p0, *, lb=None, ub=None, itmax=100, opts=None, counts=None):
    """S independent fits.  angles: CUDA float64 [S,3,n], x: [S,n], p0: CUDA float64 [S,3] (updated in place).
    counts (CUDA int32 [S], optional): a ragged batch -- fit s uses samples [0, counts[s]) of its rows, n is the row stride
    (brdf_hip_fit_batch_ragged_dev: a count below 3 gives ret -1, zero info, p as it came; bucket very unequal counts by size class).

    Returns (p [S,3], info [S,10], ret [S] int32) as CUDA tensors; asynchronous on the current stream.
    """
    import torch
    _require(angles.is_cuda and x.is_cuda and p0.is_cuda and angles.device == x.device == p0.device, "bad argument: " 'angles.is_cuda and x.is_cuda and p0.is_cuda and angles.device == x.device == p0.device')
    _require(angles.dtype == torch.float64 and x.dtype == torch.float64 and p0.dtype == torch.float64, "bad argument: " 'angles.dtype == torch.float64 and x.dtype == torch.float64 and p0.dtype == torch.float64')  # the kernels read raw doubles
    S, n = x.shape
    _require(tuple(angles.shape) == (S, 3, n) and tuple(p0.shape) == (S, 3), "bad argument: " 'tuple(angles.shape) == (S, 3, n) and tuple(p0.shape) == (S, 3)')
    angles = angles.contiguous()
    x = x.contiguous()
    p = p0.contiguous()
    info = torch.zeros((S, 10), dtype=torch.float64, device=x.device)
    ret = torch.zeros((S,), dtype=torch.int32, device=x.device)
    lb_a, ub_a, op_a = _f64(lb, 3), _f64(ub, 3), _f64(opts, 5)
    if counts is not None:
        counts = _counts_arg(counts, S, x.device, torch)
    # (null counts: the uniform call, include/brdf_levmar.h)
    _call("brdf_hip_fit_batch_ragged_dev", x.device, method, model, angles.data_ptr(), x.data_ptr(), None if counts is None else counts.data_ptr(),
          S, n, p.data_ptr(), _dptr(lb_a), _dptr(ub_a), itmax, _dptr(op_a), info.data_ptr(), ret.data_ptr(), _STREAM)
    return p, info, ret


@dataclass
class FitStats:
    """Per-fit statistics at a fitted point (brdf_hip_fit_stats_batch_dev): torch CUDA tensors, or numpy for numpy inputs."""
    covar: object  # [S,3,3]  sumsq/(n-3) * inverse(J^T J), J at p
    stats: object  # [S,8]    sumsq, R2, sd[0..2], rho01, rho02, rho12
    rank: object   # [S] int32: 3, or 0 where the covariance could not be formed (covar and its six derived values are 0)


def _zero_stats(lead: tuple, device=None) -> FitStats:
    """zeroed covar [*lead,3,3], stats [*lead,8] and rank [*lead]: CUDA tensors on `device`, or numpy arrays (None)"""
    if device is None:
        return FitStats(np.zeros(lead + (3, 3)), np.zeros(lead + (8,)), np.zeros(lead, dtype=np.int32))
    import torch
    return FitStats(torch.zeros(lead + (3, 3), dtype=torch.float64, device=device), torch.zeros(lead + (8,), dtype=torch.float64, device=device),
                    torch.zeros(lead, dtype=torch.int32, device=device))


def fit_stats_batch(method: int, model: int, angles, x, p, *, opts=None, counts=None) -> FitStats:
    """Covariance, standard errors, correlations and R^2 of S fits at their fitted points p: one evaluation pass, whoever
    fitted p.  angles [S,3,n], x [S,n], p [S,3]: CUDA float64 tensors (asynchronous on the current stream), or numpy arrays
    (host-pointer entry: uploads, runs, downloads).  `method` selects how the Jacobian row is formed (finite differences
    with opts[4]'s step, or the analytic row); for METHOD_DIF it is the Jacobian at p, not levmar's secant one.
    counts ([S] int32, of the inputs' kind; optional): per-fit sample counts of a ragged batch (degrees of freedom counts[s] - 3;
    below 3: rank 0)."""
    op_a = _f64(opts, 5)
    if isinstance(x, np.ndarray):
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64)
        _require(x.ndim == 2, "x must be [S, n]")
        S, n = x.shape
        _require(angles.shape == (S, 3, n) and p.shape == (S, 3), "angles must be [S, 3, n], p [S, 3]")
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            _require(counts.shape == (S,), "counts must be [S]")
        st = _zero_stats((S,))
        _call("brdf_hip_fit_stats_batch_ragged", None, method, model, _dptr(angles), _dptr(x), _iptr(counts), S, n, _dptr(p), _dptr(op_a),
              _dptr(st.covar), _dptr(st.stats), _iptr(st.rank))
        return st
    import torch
    _require(angles.is_cuda and x.is_cuda and p.is_cuda and angles.device == x.device == p.device, "angles, x, p: CUDA tensors on one device")
    _require(angles.dtype == torch.float64 and x.dtype == torch.float64 and p.dtype == torch.float64, "angles, x, p: float64")  # the kernels read raw doubles
    _require(x.dim() == 2, "x must be [S, n]")
    S, n = x.shape
    _require(tuple(angles.shape) == (S, 3, n) and tuple(p.shape) == (S, 3), "angles must be [S, 3, n], p [S, 3]")
    angles, x, p = angles.contiguous(), x.contiguous(), p.contiguous()
    if counts is not None:
        counts = _counts_arg(counts, S, x.device, torch)
    st = _zero_stats((S,), x.device)
    _call("brdf_hip_fit_stats_batch_ragged_dev", x.device, method, model, angles.data_ptr(), x.data_ptr(), None if counts is None else counts.data_ptr(),
          S, n, p.data_ptr(), _dptr(op_a), st.covar.data_ptr(), st.stats.data_ptr(), st.rank.data_ptr(), _STREAM)
    return st


def _weights_arg(w, x, torch):
    _require(w.is_cuda and w.device == x.device and w.dtype == torch.float64 and tuple(w.shape) == tuple(x.shape),
             "w: CUDA float64 [S,n] on the device of x")
    return w.contiguous()


def fit_batch_weighted(method: int, model: int, angles, x, w, p0, *, lb=None, ub=None, itmax=100, opts=None, counts=None):
    """fit_batch with a weight per sample (brdf_hip_fit_batch_weighted_dev): fit s is levmar on sqrt(w) f against sqrt(w) x over its
    first counts[s] samples.  n <= 16, METHOD_BC_DIF / METHOD_BC_DER only.  w: CUDA float64 [S,n]; the rest as fit_batch.  A weight
    of 0 leaves a sample out of the sums (it still counts in n); a negative or non-finite counted weight refuses the fit (ret -1, zero
    info, p as it came).  With w = 1 the result has the bytes of fit_batch(..., counts=counts).

    Returns (p [S,3], info [S,10], ret [S] int32) as CUDA tensors; asynchronous on the current stream."""
    import torch
    _require(angles.is_cuda and x.is_cuda and p0.is_cuda and angles.device == x.device == p0.device, "angles, x, p0: CUDA tensors on one device")
    _require(angles.dtype == torch.float64 and x.dtype == torch.float64 and p0.dtype == torch.float64, "angles, x, p0: float64")  # the kernels read raw doubles
    _require(x.dim() == 2, "x must be [S, n]")
    S, n = x.shape
    _require(tuple(angles.shape) == (S, 3, n) and tuple(p0.shape) == (S, 3), "angles must be [S, 3, n], p0 [S, 3]")
    w = _weights_arg(w, x, torch)
    angles, x, p = angles.contiguous(), x.contiguous(), p0.contiguous()
    info = torch.zeros((S, 10), dtype=torch.float64, device=x.device)
    ret = torch.zeros((S,), dtype=torch.int32, device=x.device)
    lb_a, ub_a, op_a = _f64(lb, 3), _f64(ub, 3), _f64(opts, 5)
    if counts is not None:
        counts = _counts_arg(counts, S, x.device, torch)
    _call("brdf_hip_fit_batch_weighted_dev", x.device, method, model, angles.data_ptr(), x.data_ptr(), w.data_ptr(),
          None if counts is None else counts.data_ptr(), S, n, p.data_ptr(), _dptr(lb_a), _dptr(ub_a), itmax, _dptr(op_a), info.data_ptr(),
          ret.data_ptr(), _STREAM)
    return p, info, ret


def fit_stats_batch_weighted(method: int, model: int, angles, x, w, p, *, opts=None, counts=None, extra_ss=None, nobs=None) -> FitStats:
    """fit_stats_batch for the weighted problem (brdf_hip_fit_stats_batch_weighted_dev; n <= 16, METHOD_BC_DIF / METHOD_BC_DER):
    sumsq = sum w e^2, covar = sumsq / (nobs - 3) * inverse(J^T W J), R2 against sum w (x - weighted mean)^2.  extra_ss ([S] float64,
    optional) is added to sumsq and to SStot; nobs ([S] int32, optional; default: the fit's count) is the observation count of the
    degrees of freedom.  CUDA tensors (asynchronous on the current stream), or numpy arrays (host-pointer entry)."""
    op_a = _f64(opts, 5)
    if isinstance(x, np.ndarray):
        angles, x, w, p = (np.ascontiguousarray(v, dtype=np.float64) for v in (angles, x, w, p))
        _require(x.ndim == 2, "x must be [S, n]")
        S, n = x.shape
        _require(angles.shape == (S, 3, n) and p.shape == (S, 3) and w.shape == (S, n), "angles must be [S, 3, n], p [S, 3], w [S, n]")
        counts, nobs = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (counts, nobs))
        extra_ss = None if extra_ss is None else np.ascontiguousarray(extra_ss, dtype=np.float64)
        _require(all(v is None or v.shape == (S,) for v in (counts, nobs, extra_ss)), "counts, nobs, extra_ss must be [S]")
        st = _zero_stats((S,))
        _call("brdf_hip_fit_stats_batch_weighted", None, method, model, _dptr(angles), _dptr(x), _dptr(w), _iptr(counts), S, n, _dptr(p),
              _dptr(op_a), _dptr(extra_ss), _iptr(nobs), _dptr(st.covar), _dptr(st.stats), _iptr(st.rank))
        return st
    import torch
    _require(angles.is_cuda and x.is_cuda and p.is_cuda and angles.device == x.device == p.device, "angles, x, p: CUDA tensors on one device")
    _require(angles.dtype == torch.float64 and x.dtype == torch.float64 and p.dtype == torch.float64, "angles, x, p: float64")  # the kernels read raw doubles
    _require(x.dim() == 2, "x must be [S, n]")
    S, n = x.shape
    _require(tuple(angles.shape) == (S, 3, n) and tuple(p.shape) == (S, 3), "angles must be [S, 3, n], p [S, 3]")
    w = _weights_arg(w, x, torch)
    angles, x, p = angles.contiguous(), x.contiguous(), p.contiguous()
    if counts is not None:
        counts = _counts_arg(counts, S, x.device, torch)
    if nobs is not None:
        _require(nobs.is_cuda and nobs.device == x.device and nobs.dtype == torch.int32 and tuple(nobs.shape) == (S,), "nobs: CUDA int32 [S] on the device of x")
        nobs = nobs.contiguous()
    if extra_ss is not None:
        _require(extra_ss.is_cuda and extra_ss.device == x.device and extra_ss.dtype == torch.float64 and tuple(extra_ss.shape) == (S,),
                 "extra_ss: CUDA float64 [S] on the device of x")
        extra_ss = extra_ss.contiguous()
    st = _zero_stats((S,), x.device)
    _call("brdf_hip_fit_stats_batch_weighted_dev", x.device, method, model, angles.data_ptr(), x.data_ptr(), w.data_ptr(),
          None if counts is None else counts.data_ptr(), S, n, p.data_ptr(), _dptr(op_a), None if extra_ss is None else extra_ss.data_ptr(),
          None if nobs is None else nobs.data_ptr(), st.covar.data_ptr(), st.stats.data_ptr(), st.rank.data_ptr(), _STREAM)
    return st


def pack_samples(angles, x, counts):
    """Padded rows -> a packed batch: angles [S,3,n], x [S,n], counts [S] (integers; torch tensors on one device, or numpy arrays)
    -> (angles [3 * total] float64, x [total], offsets [S+1] int64) of the same kind, total = sum(counts).  Fit s's first counts[s]
    samples are laid back to back: its three planes at angles[3 * offsets[s]:], counts[s] values each, its measurements at
    x[offsets[s]:] -- the layout fit_batch_packed reads, and the inverse of what its gather does.  Entries at and behind a count
    (NaN padding included) do not travel; a count outside [0, n] is clipped.  compact_samples -> pack_samples -> fit_batch_packed is
    a pipeline."""
    if isinstance(x, np.ndarray):
        _require(x.ndim == 2 and angles.shape == (x.shape[0], 3, x.shape[1]) and np.shape(counts) == (x.shape[0],), "angles [S,3,n], x [S,n], counts [S]")
        k = np.clip(np.asarray(counts).astype(np.int64), 0, x.shape[1])
        keep = np.arange(x.shape[1])[None, :] < k[:, None]
        offsets = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(k)])
        return (np.ascontiguousarray(angles[np.broadcast_to(keep[:, None, :], angles.shape)], dtype=np.float64),
                np.ascontiguousarray(x[keep], dtype=np.float64), offsets)
    import torch
    _require(x.dim() == 2 and tuple(angles.shape) == (x.shape[0], 3, x.shape[1]) and tuple(counts.shape) == (x.shape[0],), "angles [S,3,n], x [S,n], counts [S]")
    k = counts.to(torch.int64).clamp(0, x.shape[1])
    keep = torch.arange(x.shape[1], device=x.device)[None, :] < k[:, None]
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=x.device), torch.cumsum(k, 0)])
    return angles[keep[:, None, :].expand(angles.shape)].to(torch.float64), x[keep].to(torch.float64), offsets


def _packed_args(angles, x, offsets, p, validate, torch):
    _require(angles.is_cuda and x.is_cuda and offsets.is_cuda and p.is_cuda and angles.device == x.device == offsets.device == p.device,
             "angles, x, offsets, p: CUDA tensors on one device")
    _require(angles.dtype == torch.float64 and x.dtype == torch.float64 and p.dtype == torch.float64 and offsets.dtype == torch.int64,
             "angles, x, p: float64; offsets: int64")  # the kernels read raw doubles and long longs
    _require(offsets.dim() == 1 and offsets.numel() >= 2 and p.dim() == 2 and tuple(p.shape) == (offsets.numel() - 1, 3),
             "offsets [S+1], p [S,3]")
    _require(angles.dim() == 1 and x.dim() == 1 and angles.numel() >= 3 * x.numel(), "angles [3 * total], x [total]: flat, packed")
    if validate:  # (synchronises: the packed calls wait for the stream anyway)
        lo, hi = int(offsets[0]), int(offsets[-1])
        _require(0 <= lo <= hi <= x.numel(), f"offsets cover [{lo}, {hi}), x holds {x.numel()} samples")
        _require(bool((offsets[1:] >= offsets[:-1]).all()), "offsets must not decrease")
    return angles.contiguous(), x.contiguous(), offsets.contiguous(), p.contiguous()


def fit_batch_packed(method: int, model: int, angles, x, offsets, p0, *, lb=None, ub=None, itmax=100, opts=None, workspace_bytes: int = 0,
                     validate: bool = True):
    """S fits of ANY size in one call (brdf_hip_fit_batch_packed_dev): a packed batch, bucketed by size class inside the library.
    angles: CUDA float64 [3 * total], x: [total], offsets: CUDA int64 [S+1] (pack_samples builds all three), p0: CUDA float64 [S,3]
    (updated in place).  Fit s has k = offsets[s+1] - offsets[s] samples: planes [3][k] at angles[3 * offsets[s]:], measurements at
    x[offsets[s]:].  A fit of k >= 3 samples gets the bytes fit_batch gives it alone at n = k; k < 3: ret -1, zero info, p as it came.
    workspace_bytes bounds the padded rows of one chunk (0: 1 GiB).  validate=False skips the range check of the offsets (callers that
    vouch for them).  Returns (p [S,3], info [S,10], ret [S] int32) as CUDA tensors; the call waits for the stream once."""
    import torch
    angles, x, offsets, p = _packed_args(angles, x, offsets, p0, validate, torch)
    S = offsets.numel() - 1
    info = torch.zeros((S, 10), dtype=torch.float64, device=x.device)
    ret = torch.zeros((S,), dtype=torch.int32, device=x.device)
    lb_a, ub_a, op_a = _f64(lb, 3), _f64(ub, 3), _f64(opts, 5)
    _call("brdf_hip_fit_batch_packed_dev", x.device, method, model, angles.data_ptr(), x.data_ptr(), offsets.data_ptr(), S, p.data_ptr(), _dptr(lb_a),
          _dptr(ub_a), itmax, _dptr(op_a), info.data_ptr(), ret.data_ptr(), int(workspace_bytes), _STREAM)
    return p, info, ret


def fit_stats_batch_packed(method: int, model: int, angles, x, offsets, p, *, opts=None, workspace_bytes: int = 0, validate: bool = True) -> FitStats:
    """fit_stats_batch for a packed batch (brdf_hip_fit_stats_batch_packed_dev): arguments as fit_batch_packed, p [S,3] read only.
    Every fit's covar / stats / rank are the bytes fit_stats_batch gives it alone at n = its count; a count below 3: rank 0."""
    import torch
    angles, x, offsets, p = _packed_args(angles, x, offsets, p, validate, torch)
    S = offsets.numel() - 1
    st = _zero_stats((S,), x.device)
    _call("brdf_hip_fit_stats_batch_packed_dev", x.device, method, model, angles.data_ptr(), x.data_ptr(), offsets.data_ptr(), S, p.data_ptr(),
          _dptr(_f64(opts, 5)), st.covar.data_ptr(), st.stats.data_ptr(), st.rank.data_ptr(), int(workspace_bytes), _STREAM)
    return st


class ClippedFit(NamedTuple):
    """What fit_batch_packed_clipped returns (CUDA tensors)."""
    p: object            # [S,3] float64
    info: object         # [S,10] float64
    ret: object          # [S] int32
    stats: FitStats      # covar [S,3,3], stats [S,8], rank [S]: at p over the returned sample set
    kept: object         # [S] int32: the samples of the fit's returned set
    rounds_used: object  # [S] int32: the last clip round that refitted the fit (0: none)
    mask: object         # [offsets[S] - offsets[0]] uint8: 1 = in the returned set, by the caller's sample position


SIGMA_MIN_8BIT = 1.0 / (255.0 * 12.0 ** 0.5)  # the standard deviation of an 8-bit capture's quantisation: the recommended sigma_min


def fit_batch_packed_clipped(method: int, model: int, angles, x, offsets, p0, *, kappa: float, sigma_min: float, rounds: int, lb=None, ub=None,
                             itmax=100, opts=None, workspace_bytes: int = 0, validate: bool = True) -> ClippedFit:
    """fit_batch_packed with sigma clipping (brdf_hip_fit_batch_packed_clipped_dev): fit, drop the samples further than kappa * sigma
    from the fit, fit the survivors again from the current p, at most `rounds` times or until nothing more is dropped.  Arguments as
    fit_batch_packed.  sigma = max(sqrt(sumsq / (k - 3)), sigma_min) with the statistics pass's sumsq over the fit's current k samples
    (k == 3: sigma_min; SIGMA_MIN_8BIT is recommended for 8-bit captures); a fit that is refused, ends with ret < 0, drops nothing or
    would keep fewer than 3 samples is settled and keeps its samples.  Every returned fit is a fit of its returned sample set: p,
    info and ret have fit_batch_packed's bytes on that set from the previous round's p, `stats` fit_stats_batch_packed's at p.
    rounds = 0 or kappa = inf return the two packed calls' bytes.  With rounds > 0 the offsets must not descend (refused on the device, also
    with validate=False).  clip_samples is one clip round of this definition as NumPy code."""
    import torch
    angles, x, offsets, p = _packed_args(angles, x, offsets, p0, validate, torch)
    S = offsets.numel() - 1
    dev = x.device
    total = int(offsets[-1]) - int(offsets[0])
    _require(total >= 0, "offsets[S] < offsets[0]")
    info = torch.zeros((S, 10), dtype=torch.float64, device=dev)
    ret, kept, used = (torch.zeros((S,), dtype=torch.int32, device=dev) for _ in range(3))
    mask = torch.zeros((total,), dtype=torch.uint8, device=dev)
    st = _zero_stats((S,), dev)
    lb_a, ub_a, op_a = _f64(lb, 3), _f64(ub, 3), _f64(opts, 5)
    _call("brdf_hip_fit_batch_packed_clipped_dev", dev, method, model, angles.data_ptr(), x.data_ptr(), offsets.data_ptr(), S, p.data_ptr(), _dptr(lb_a),
          _dptr(ub_a), itmax, _dptr(op_a), float(kappa), float(sigma_min), int(rounds), info.data_ptr(), ret.data_ptr(), st.covar.data_ptr(),
          st.stats.data_ptr(), st.rank.data_ptr(), kept.data_ptr(), used.data_ptr(), mask.data_ptr(), int(workspace_bytes), _STREAM)
    return ClippedFit(p, info, ret, st, kept, used, mask)


def last_clip_stats() -> list:
    """per clip round of this thread's last clipped call: the fits that were clipped and refitted, and the samples dropped"""
    out = []
    active, clipped = C.c_longlong(0), C.c_longlong(0)
    while lib.brdf_hip_last_clip_stats(len(out) + 1, C.byref(active), C.byref(clipped)) == 0:
        out.append({"active": active.value, "clipped": clipped.value})
    return out


def clip_samples(model: int, angles, x, offsets, p, sumsq, ret, *, kappa: float, sigma_min: float):
    """ONE clip round of fit_batch_packed_clipped's definition, as NumPy code on the host (no device): the packed batch angles
    [3 * total], x [total], offsets [S+1] holds the fits' CURRENT sample sets, p [S,3] their current parameters, sumsq [S] the
    statistics pass's stats[:, 0] at p over those sets, ret [S] the fits' ret.  Returns (keep [offsets[S] - offsets[0]] bool, by sample
    position, and settled [S] bool).  For a fit with ret < 0, fewer than 3 samples or a sumsq that is not finite: settled, all kept.
    Otherwise sigma = max(sqrt(sumsq / (k - 3)), sigma_min) (k == 3: sigma_min) and sample i survives iff |x_i - f_i(p)| <= kappa *
    sigma (a NaN residual does not); nothing dropped, or fewer than 3 survivors: settled, all kept.  The caller marks settled fits and
    never passes them as unsettled again: here every fit given is looked at."""
    from . import synth
    angles, x = np.asarray(angles, dtype=np.float64), np.asarray(x, dtype=np.float64)
    offsets = np.asarray(offsets, dtype=np.int64)
    p, sumsq, ret = np.asarray(p, dtype=np.float64), np.asarray(sumsq, dtype=np.float64), np.asarray(ret)
    S = offsets.size - 1
    _require(p.shape == (S, 3) and sumsq.shape == (S,) and ret.shape == (S,), "p [S,3], sumsq [S], ret [S]")
    o0 = int(offsets[0])
    keep = np.ones(int(offsets[-1]) - o0, dtype=bool)
    settled = np.ones(S, dtype=bool)
    for s in range(S):
        o, k = int(offsets[s]), int(offsets[s + 1] - offsets[s])
        if ret[s] < 0 or k < 3 or not np.isfinite(sumsq[s]):
            continue
        a = angles[3 * o:3 * o + 3 * k].reshape(3, k)
        with np.errstate(all="ignore"):
            sigma = max(float(np.sqrt(sumsq[s] / (k - 3))), float(sigma_min)) if k > 3 else float(sigma_min)
            e = x[o:o + k] - synth.model_value(model, p[s], a[0], a[1], a[2])
            ok = np.abs(e) <= np.float64(kappa) * np.float64(sigma)  # (False for a NaN)
        if ok.all() or int(ok.sum()) < 3:
            continue
        keep[o - o0:o - o0 + k] = ok
        settled[s] = False
    return keep, settled


def last_packed_stats() -> list:
    """per size class 0..5 (<= 16, 64, 256, 1024, 4096 samples, above) of this thread's last packed call: fits, the row stride of its
    launches (0: empty class; class 5: the largest count) and chunks (class 5: one run per fit)"""
    out = []
    fits, stride, chunks = C.c_longlong(0), C.c_int(0), C.c_int(0)
    while lib.brdf_hip_last_packed_stats(len(out), C.byref(fits), C.byref(stride), C.byref(chunks)) == 0:
        out.append({"fits": fits.value, "stride": stride.value, "chunks": chunks.value})
    return out


BATCH_KERNELS = ("lane", "rows", "wave", "workgroup", "eight-wave", "512x8", "weighted lane")  # brdf_hip_last_batch_launch's codes


def last_batch_launch() -> dict | None:
    """the kernel this thread's last batched launch chose (brdf_hip_last_batch_launch): its code 0..6 (BATCH_KERNELS), the waves per
    SIMD of the chosen instance, the workgroups launched and the lane scheduler's quorum / maxwait; None before the first batch"""
    kernel, waves, grid, quorum, maxwait = C.c_int(-1), C.c_int(0), C.c_longlong(0), C.c_int(0), C.c_int(0)
    if lib.brdf_hip_last_batch_launch(C.byref(kernel), C.byref(waves), C.byref(grid), C.byref(quorum), C.byref(maxwait)) != 0:
        return None
    return {"kernel": kernel.value, "waves_per_simd": waves.value, "grid": grid.value, "quorum": quorum.value, "maxwait": maxwait.value}


def fit_batch_multi(method: int, model: int, angles, x, p0, *, devices=None, lb=None, ub=None, itmax=100, opts=None):
    """S independent fits over several GPUs of this process (brdf_hip_fit_batch_multi): HOST arrays angles [S,3,n], x [S,n],
    p0 [S,3] (not modified).  `devices`: HIP ordinals, one contiguous shard of ceil(S/len) fits each (dist.shard_range; an
    ordinal may repeat); None: every visible device once.  Returns numpy (p [S,3], info [S,10], ret [S] int32), bit-identical
    to one device's brdf_hip_fit_batch.  The GIL is released during the call."""
    angles = np.ascontiguousarray(angles, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    _require(x.ndim == 2, "x must be [S, n]")
    S, n = x.shape
    _require(angles.shape == (S, 3, n), "angles must be [S, 3, n]")
    p = np.array(p0, dtype=np.float64, order="C").reshape(-1)
    _require(p.size == 3 * S, "p0 must be [S, 3]")
    p = p.reshape(S, 3)
    info = np.zeros((S, 10))
    ret = np.zeros(S, dtype=np.int32)
    lb_a, ub_a, op_a = _f64(lb, 3), _f64(ub, 3), _f64(opts, 5)
    dev_list, ndev = None, 0
    if devices is not None:
        devices = [int(d) for d in devices]
        dev_list, ndev = (C.c_int * max(1, len(devices)))(*devices), len(devices)
    rc = lib.brdf_hip_fit_batch_multi(method, model, _dptr(angles), _dptr(x), S, n, _dptr(p), _dptr(lb_a), _dptr(ub_a), itmax,
                                      _dptr(op_a), _dptr(info), ret.ctypes.data_as(C.POINTER(C.c_int)), dev_list, ndev)
    if rc < 0:
        raise RuntimeError(f"brdf_hip_fit_batch_multi failed: {last_error()}")
    return p, info, ret


def last_multi_stats() -> list:
    """per shard of this thread's last fit_batch_multi(): device, first fit, fit count and upload / fit / download
    milliseconds as the device's stream saw them"""
    out = []
    dev, first, count, ms = C.c_int(0), C.c_longlong(0), C.c_longlong(0), (C.c_double * 3)()
    while lib.brdf_hip_last_multi_stats(len(out), C.byref(dev), C.byref(first), C.byref(count), ms) == 0:
        out.append({"device": dev.value, "first": first.value, "count": count.value, "upload_ms": ms[0], "fit_ms": ms[1],
                    "download_ms": ms[2]})
    return out


def model_eval(model: int, angles, p):
    """hx = model(p; samples) on the device (kernel K1 alone).  angles: CUDA float64 [3,n]."""
    import torch
    _require(angles.is_cuda and angles.dtype == torch.float64 and angles.numel() % 3 == 0, "bad argument: " 'angles.is_cuda and angles.dtype == torch.float64 and angles.numel() % 3 == 0')
    angles = angles.contiguous()
    n = angles.numel() // 3
    hx = torch.empty(n, dtype=torch.float64, device=angles.device)
    pa = _f64(p, 3)
    _call("brdf_hip_model_eval_dev", angles.device, model, angles.data_ptr(), n, _dptr(pa), hx.data_ptr(), _STREAM)
    return hx


def led_table() -> np.ndarray:
    """CBRDFdata::InitLEDs (brdfdata.cpp:683-752): the capture rig's 16 LED positions, [16, 3]."""
    out = np.zeros(48)
    lib.brdf_hip_led_table(_dptr(out))
    return out.reshape(16, 3)


def _check_indices(idx, upper: int, what: str, lower: int = 0) -> None:
    """Range check of an index tensor.  The two reductions synchronise with the device; callers that keep a stream busy
    and vouch for their indices pass validate=False to the entry point instead."""
    if idx.numel() == 0:
        return
    lo, hi = int(idx.min()), int(idx.max())
    _require(lo >= lower and hi < upper, f"{what} (range [{lo}, {hi}], allowed [{lower}, {upper}))")


def cosines(vertices, faces, face_normals, leds, view_origin, *, surfels=None, rv_mode: int = 0, validate: bool = True):
    """vectors -> cosines on the device (GetCosLN / GetCosNH / GetCosRV, brdfdata.cpp:799-943) for a batch of surfels.
    vertices [nv,3] float64, faces [nf,3] int32, face_normals [nf,3] float64: CUDA tensors; surfels: CUDA int32 [S]
    (face index per surfel) or None (surfel s = face s); leds [L,3], view_origin [3]: host.  Returns CUDA float64
    [S, 3, L] -- the batched fitter's `angles` layout."""
    import torch
    vertices, faces, face_normals = vertices.contiguous(), faces.contiguous(), face_normals.contiguous()
    _require(vertices.is_cuda and faces.is_cuda and face_normals.is_cuda, "bad argument: " 'vertices.is_cuda and faces.is_cuda and face_normals.is_cuda')
    _require(vertices.dtype == torch.float64 and face_normals.dtype == torch.float64 and faces.dtype == torch.int32, "bad argument: " 'vertices.dtype == torch.float64 and face_normals.dtype == torch.float64 and faces.dtype == torch.int32')
    _require(vertices.shape[-1] == 3 and faces.shape[-1] == 3 and tuple(face_normals.shape) == (faces.shape[0], 3), "bad argument: " 'vertices.shape[-1] == 3 and faces.shape[-1] == 3 and tuple(face_normals.shape) == (faces.shape[0], 3)')
    if validate:
        _check_indices(faces, vertices.shape[0], "face index outside the vertex array")
    if surfels is not None:
        surfels = surfels.contiguous()
        _require(surfels.is_cuda and surfels.dtype == torch.int32, "bad argument: " 'surfels.is_cuda and surfels.dtype == torch.int32')
        if validate:
            _check_indices(surfels, faces.shape[0], "surfel index outside the face array")
    S = int(surfels.numel()) if surfels is not None else int(faces.shape[0])
    la = np.ascontiguousarray(leds, dtype=np.float64).reshape(-1, 3)
    L = la.shape[0]
    va = _f64(view_origin, 3)
    out = torch.empty((S, 3, L), dtype=torch.float64, device=vertices.device)
    _call("brdf_hip_cosines_dev", vertices.device, vertices.data_ptr(), faces.data_ptr(), face_normals.data_ptr(),
          surfels.data_ptr() if surfels is not None else None, S, _dptr(la), L, _dptr(va), rv_mode, out.data_ptr(), _STREAM)
    return out


def fit_capture_masked(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, *, v_min: int = 0, v_max: int = 255,
                       cos_min: float = -2.0, surface_count=None, **kwargs):
    """fit_capture(want_stats=True) with a validity rule (brdf_hip_fit_capture_masked_dev): light i of a (pixel, channel) fit takes
    part iff v_min <= its 8-bit intensity <= v_max and every cosine plane the model reads is > cos_min; the fit is levmar on the
    valid samples alone (a ragged fit).  The defaults switch both tests off: then every output is bit-identical to fit_capture's, except
    that a NaN cosine is never a sample: on a face with NaN cosines the fit is refused (count 0) where fit_capture stops it with reason 7.
    Returns (brdf_surfaces, avg, pixels, FitStats, surface_count [nf,3] int32 CUDA: the sample count of each stored fit; a fit of
    fewer than 3 samples is refused and leaves p0 in brdf_surfaces).  Keyword arguments as fit_capture."""
    import torch
    nf = int(faces.shape[0])
    if surface_count is None:
        surface_count = torch.zeros((nf, 3), dtype=torch.int32, device=images.device)
    _require(surface_count.is_cuda and surface_count.dtype == torch.int32 and tuple(surface_count.shape) == (nf, 3) and surface_count.is_contiguous(),
             "surface_count: contiguous CUDA int32 [nf,3]")
    kwargs["want_stats"] = True
    out = fit_capture(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin,
                      _mask=(int(v_min), int(v_max), float(cos_min), surface_count), **kwargs)
    return (*out, surface_count)


def _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, p0, lb, ub, itmax, opts, validate):
    """What fit_capture and fit_capture_single share: the checks of the capture and the mesh, and the arguments the two entries have in
    common, model ... opts.  Returns (those arguments, the tensors they point into, nf)."""
    import torch
    images, pixel_map = images.contiguous(), pixel_map.contiguous()
    vertices, faces, face_normals = vertices.contiguous(), faces.contiguous(), face_normals.contiguous()
    _require(images.is_cuda and pixel_map.is_cuda and vertices.is_cuda and faces.is_cuda and face_normals.is_cuda, "bad argument: " 'images.is_cuda and pixel_map.is_cuda and vertices.is_cuda and faces.is_cuda and face_normals.is_cuda')
    _require(images.dtype == torch.uint8 and pixel_map.dtype == torch.int32 and faces.dtype == torch.int32, "bad argument: " 'images.dtype == torch.uint8 and pixel_map.dtype == torch.int32 and faces.dtype == torch.int32')
    _require(vertices.dtype == torch.float64 and face_normals.dtype == torch.float64, "bad argument: " 'vertices.dtype == torch.float64 and face_normals.dtype == torch.float64')
    _require(images.dim() == 4 and images.shape[3] == 3 and tuple(pixel_map.shape) == tuple(images.shape[1:3]), "bad argument: " 'images.dim() == 4 and images.shape[3] == 3 and tuple(pixel_map.shape) == tuple(images.shape[1:3])')  # [L,H,W,3] BGR, [H,W]
    _require(tuple(face_normals.shape) == (faces.shape[0], 3) and vertices.shape[-1] == 3, "bad argument: " 'tuple(face_normals.shape) == (faces.shape[0], 3) and vertices.shape[-1] == 3')
    if validate:  # (-1 = no face under the pixel)
        _check_indices(pixel_map, faces.shape[0], "pixel map names a face that does not exist", lower=-1)
        _check_indices(faces, vertices.shape[0], "face index outside the vertex array")
    L, H, W = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    nf = int(faces.shape[0])
    la = np.ascontiguousarray(leds, dtype=np.float64).reshape(-1, 3)
    _require(la.shape[0] == L, "bad argument: " 'la.shape[0] == L')
    va, pa, lba, uba, oa = _f64(view_origin, 3), _f64(p0, 3), _f64(lb, 3), _f64(ub, 3), _f64(opts, 5)
    args = (model, images.data_ptr(), L, H, W, pixel_map.data_ptr(), vertices.data_ptr(), faces.data_ptr(), face_normals.data_ptr(), nf,
            _dptr(la), _dptr(va), rv_mode, _dptr(pa), _dptr(lba), _dptr(uba), itmax, _dptr(oa))
    return args, (images, pixel_map, vertices, faces, face_normals), nf


def fit_capture(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, *, rv_mode: int = 0,
                p0=(0.5, 1.0, 1.0), lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0), itmax: int = 100, opts=None, brdf_surfaces=None,
                validate: bool = True, want_stats: bool = False, surface_stats: FitStats | None = None, _mask=None):
    """The pixel loop of CBRDFdata::CalcBRDFEquation (brdfdata.cpp:1188-1227) on the device.  images: CUDA uint8
    [L,H,W,3] (BGR), pixel_map: CUDA int32 [H,W] (face index or -1), mesh as in cosines().  Returns (brdf_surfaces
    CUDA float64 [nf,3,3] = {kd,ks,n} per face and channel, avg[3], number of pixels that carried a face).
    want_stats=True (brdf_hip_fit_capture_stats_dev): a fourth value, FitStats with covar [nf,3,3,3], stats [nf,3,8],
    rank [nf,3] of the fits that were stored (`surface_stats`: maps to write into; faces no pixel carries keep their
    values, zeros by default)."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, p0, lb, ub, itmax, opts,
                                   validate)
    dev = keep[0].device
    if brdf_surfaces is None:
        brdf_surfaces = torch.zeros((nf, 3, 3), dtype=torch.float64, device=dev)
    avg = np.zeros(3)
    npx = C.c_longlong(0)
    args += (brdf_surfaces.data_ptr(), _dptr(avg), C.byref(npx), _STREAM)
    if not want_stats:
        _call("brdf_hip_fit_capture_dev", dev, *args)
        return brdf_surfaces, avg, npx.value
    st = surface_stats
    if st is None:
        st = _zero_stats((nf, 3), dev)
    _require(tuple(st.covar.shape) == (nf, 3, 3, 3) and tuple(st.stats.shape) == (nf, 3, 8) and tuple(st.rank.shape) == (nf, 3),
             "surface_stats: covar [nf,3,3,3], stats [nf,3,8], rank [nf,3]")
    _require(st.covar.dtype == torch.float64 and st.stats.dtype == torch.float64 and st.rank.dtype == torch.int32,
             "surface_stats: float64 covar and stats, int32 rank")
    _require(st.covar.is_contiguous() and st.stats.is_contiguous() and st.rank.is_contiguous() and st.covar.is_cuda and st.stats.is_cuda
             and st.rank.is_cuda, "surface_stats: contiguous CUDA tensors")
    args += (st.covar.data_ptr(), st.stats.data_ptr(), st.rank.data_ptr())
    if _mask is not None:  # fit_capture_masked
        _call("brdf_hip_fit_capture_masked_dev", dev, *args, _mask[0], _mask[1], _mask[2], _mask[3].data_ptr())
    else:
        _call("brdf_hip_fit_capture_stats_dev", dev, *args)
    return brdf_surfaces, avg, npx.value, st


class CaptureFaces(NamedTuple):
    """What fit_capture_faces returns: the [nf,3] maps (CUDA tensors) and the call's host scalars."""
    surfaces: object     # [nf,3,3] float64: {kd, ks, n} per face and channel
    info: object         # [nf,3,10] float64: levmar's info[]
    ret: object          # [nf,3] int32: iterations, or -1
    stats: FitStats | None  # covar [nf,3,3,3], stats [nf,3,8], rank [nf,3]; None without want_stats
    count: object        # [nf,3] int32: the samples of the fit
    face_pixels: object  # [nf] int32: the pixels that carry the face (0 where none)
    avg: np.ndarray      # [3]
    n_pixels: int
    n_faces: int


def fit_capture_faces(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, *, v_min: int = 0, v_max: int = 255,
                      cos_min: float = -2.0, rv_mode: int = 0, p0=(0.5, 1.0, 1.0), lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0),
                      itmax: int = 100, opts=None, workspace_bytes: int = 0, want_stats: bool = True, validate: bool = True,
                      out: CaptureFaces | None = None) -> CaptureFaces:
    """The capture with ONE fit per (face, channel) over the samples of ALL the face's pixels (brdf_hip_fit_capture_faces_dev), where
    fit_capture fits every pixel (n = L) and keeps the face's last one.  Arguments as fit_capture; the validity rule as
    fit_capture_masked (the defaults switch it off).  Fit (face, channel)'s samples are the face's pixels in the reference's walk
    (x outer, y inner), the lights inside a pixel, those the rule leaves -- group_capture_samples is this definition as code -- and its
    result has the bytes fit_batch_packed / fit_stats_batch_packed give for that sample set: k - 3 degrees of freedom with k samples;
    k < 3: ret -1, zero info, p0 in surfaces.  Faces no pixel carries keep what the maps held: zeros, or the values of `out`, an
    earlier result (or one built by hand) whose tensors are written into.  A face of more than 4096 / L pixels runs through the
    single-fit path, one such fit after the other.  Memory: 32 bytes per candidate sample (3 channels x pixels x L) at most, plus the
    packed calls' workspace_bytes (0: 1 GiB).  The call waits for the stream."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, p0, lb, ub, itmax, opts,
                                   validate)
    dev = keep[0].device
    if out is None:
        def z(*shape, dtype=torch.float64):
            return torch.zeros((nf, *shape), dtype=dtype, device=dev)
        out = CaptureFaces(z(3, 3), z(3, 10), z(3, dtype=torch.int32), _zero_stats((nf, 3), dev) if want_stats else None, z(3, dtype=torch.int32),
                           z(dtype=torch.int32), None, 0, 0)
    _require(not want_stats or out.stats is not None, "out: want_stats needs out.stats")
    st = out.stats if want_stats else None
    maps = [(out.surfaces, (nf, 3, 3), torch.float64), (out.info, (nf, 3, 10), torch.float64), (out.ret, (nf, 3), torch.int32),
            (out.count, (nf, 3), torch.int32), (out.face_pixels, (nf,), torch.int32)]
    if st is not None:
        maps += [(st.covar, (nf, 3, 3, 3), torch.float64), (st.stats, (nf, 3, 8), torch.float64), (st.rank, (nf, 3), torch.int32)]
    for t, shape, dtype in maps:
        _require(t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous(),
                 f"out: contiguous CUDA {dtype} {list(shape)} tensors on the capture's device")
    avg = np.zeros(3)
    npx, nfc = C.c_longlong(0), C.c_longlong(0)
    _call("brdf_hip_fit_capture_faces_dev", dev, *args, int(v_min), int(v_max), float(cos_min), int(workspace_bytes), out.surfaces.data_ptr(),
          out.info.data_ptr(), out.ret.data_ptr(), None if st is None else st.covar.data_ptr(), None if st is None else st.stats.data_ptr(),
          None if st is None else st.rank.data_ptr(), out.count.data_ptr(), out.face_pixels.data_ptr(), _dptr(avg), C.byref(npx), C.byref(nfc),
          _STREAM)
    return CaptureFaces(out.surfaces, out.info, out.ret, st, out.count, out.face_pixels, avg, npx.value, nfc.value)


class CaptureFacesClipped(NamedTuple):
    """What fit_capture_faces_clipped returns: CaptureFaces' fields and the clip's two maps."""
    surfaces: object
    info: object
    ret: object
    stats: FitStats | None
    count: object        # [nf,3] int32: the fit's candidate samples under the validity rule
    face_pixels: object
    avg: np.ndarray
    n_pixels: int
    n_faces: int
    kept: object         # [nf,3] int32: the samples of the fit's returned set
    rounds: object       # [nf,3] int32: rounds_used


def fit_capture_faces_clipped(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, *, kappa: float, sigma_min: float,
                              rounds: int, v_min: int = 0, v_max: int = 255, cos_min: float = -2.0, rv_mode: int = 0, p0=(0.5, 1.0, 1.0),
                              lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0), itmax: int = 100, opts=None, workspace_bytes: int = 0,
                              want_stats: bool = True, validate: bool = True, out: CaptureFacesClipped | None = None) -> CaptureFacesClipped:
    """fit_capture_faces with fit_batch_packed_clipped in place of the packed fit and statistics
    (brdf_hip_fit_capture_faces_clipped_dev): everything in front of the fit and the scatter behind it are fit_capture_faces'.  `count`
    keeps its meaning, `kept` is the returned sample set's size and `rounds` rounds_used; faces no pixel carries keep zeros in both.
    The statistics are taken over the returned sets.  rounds = 0 gives fit_capture_faces' bytes in every map and scalar.  `out`: an
    earlier result (or one built by hand) whose tensors are written into, as in fit_capture_faces."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, p0, lb, ub, itmax, opts,
                                   validate)
    dev = keep[0].device

    def z(*shape, dtype=torch.float64):
        return torch.zeros((nf, *shape), dtype=dtype, device=dev)
    if out is None:
        out = CaptureFacesClipped(z(3, 3), z(3, 10), z(3, dtype=torch.int32), _zero_stats((nf, 3), dev) if want_stats else None, z(3, dtype=torch.int32),
                                  z(dtype=torch.int32), None, 0, 0, z(3, dtype=torch.int32), z(3, dtype=torch.int32))
    _require(not want_stats or out.stats is not None, "out: want_stats needs out.stats")
    surfaces, info, ret, count, face_pixels, kept, used = out.surfaces, out.info, out.ret, out.count, out.face_pixels, out.kept, out.rounds
    st = out.stats if want_stats else None
    maps = [(surfaces, (nf, 3, 3), torch.float64), (info, (nf, 3, 10), torch.float64), (face_pixels, (nf,), torch.int32)]
    maps += [(t, (nf, 3), torch.int32) for t in (ret, count, kept, used)]
    if st is not None:
        maps += [(st.covar, (nf, 3, 3, 3), torch.float64), (st.stats, (nf, 3, 8), torch.float64), (st.rank, (nf, 3), torch.int32)]
    for t, shape, dtype in maps:
        _require(t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous(),
                 f"out: contiguous CUDA {dtype} {list(shape)} tensors on the capture's device")
    avg = np.zeros(3)
    npx, nfc = C.c_longlong(0), C.c_longlong(0)
    _call("brdf_hip_fit_capture_faces_clipped_dev", dev, *args, int(v_min), int(v_max), float(cos_min), int(workspace_bytes), surfaces.data_ptr(),
          info.data_ptr(), ret.data_ptr(), None if st is None else st.covar.data_ptr(), None if st is None else st.stats.data_ptr(),
          None if st is None else st.rank.data_ptr(), count.data_ptr(), face_pixels.data_ptr(), _dptr(avg), C.byref(npx), C.byref(nfc), _STREAM,
          float(kappa), float(sigma_min), int(rounds), kept.data_ptr(), used.data_ptr())
    return CaptureFacesClipped(surfaces, info, ret, st, count, face_pixels, avg, npx.value, nfc.value, kept, used)


def group_capture_samples(images, pixel_map, face_angles, model: int, *, v_min: int = 0, v_max: int = 255, cos_min: float = -2.0):
    """The host twin of fit_capture_faces' grouping (NumPy, no device): its definition as code.  images [L,H,W,3] uint8, pixel_map
    [H,W] (entries outside [0, nf) are background), face_angles [nf,3,L] (the faces' cosine planes).  One fit per carried face and
    channel, ordered by ascending face, then channel; its candidates are the face's pixels in the reference's walk (x outer, y inner),
    within a pixel the lights 0 ... L-1; a candidate is a sample iff v_min <= image_i(H-1-y, x)[c] <= v_max and every plane the model
    reads is > cos_min (a NaN is not).  Returns (angles [3 * total] float64, x [total], offsets [fits + 1] int64 -- the packed layout
    fit_batch_packed reads --, fit_face [fits], fit_channel [fits], face_pixels [nf] int32)."""
    images, pixel_map = np.asarray(images), np.asarray(pixel_map)
    face_angles = np.ascontiguousarray(face_angles, dtype=np.float64)
    _require(images.ndim == 4 and images.shape[3] == 3 and images.dtype == np.uint8 and pixel_map.shape == images.shape[1:3],
             "images [L,H,W,3] uint8, pixel_map [H,W]")
    L, H, W = images.shape[:3]
    _require(face_angles.ndim == 3 and face_angles.shape[1:] == (3, L), "face_angles [nf,3,L]")
    _require(model in (MODEL_PHONG, MODEL_BLINN_PHONG, MODEL_WARD), "unknown model")
    nf = face_angles.shape[0]
    walk = pixel_map.T.reshape(-1)  # the reference's walk: index x * H + y
    carried = np.flatnonzero((walk > -1) & (walk < nf))
    face = walk[carried].astype(np.int64)
    face_pixels = np.bincount(face, minlength=nf).astype(np.int32)
    order = np.argsort(face, kind="stable")  # by face, walk order kept inside a face
    g, face = carried[order], face[order]
    value = images[:, H - 1 - g % H, g // H, :].astype(np.int64)  # [L, pixels, 3]
    reads = [True, model != MODEL_PHONG, model != MODEL_BLINN_PHONG]  # the planes the model reads
    cos_ok = np.all([face_angles[face, k, :] > cos_min for k in range(3) if reads[k]], axis=0)  # [pixels, L]
    angles, x, offsets, fit_face, fit_channel = [], [], [0], [], []
    first = np.concatenate([[0], np.cumsum(face_pixels[face_pixels > 0])])
    for r, f in enumerate(np.flatnonzero(face_pixels)):
        rows = slice(first[r], first[r + 1])
        for c in range(3):
            v = value[:, rows, c].T  # [the face's pixels, L]: the candidates in their order
            valid = cos_ok[rows] & (v >= v_min) & (v <= v_max)
            angles.append(np.broadcast_to(face_angles[f][:, None, :], (3,) + v.shape)[:, valid].reshape(-1))
            x.append(v[valid] / 255.0)
            offsets.append(offsets[-1] + int(valid.sum()))
            fit_face.append(f)
            fit_channel.append(c)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)  # noqa: E731
    return (np.ascontiguousarray(cat(angles), dtype=np.float64), np.ascontiguousarray(cat(x), dtype=np.float64), np.array(offsets, dtype=np.int64),
            np.array(fit_face, dtype=np.int32), np.array(fit_channel, dtype=np.int32), face_pixels)


class CaptureMeans(NamedTuple):
    """What fit_capture_means returns: fit_capture_faces' maps and one more."""
    surfaces: object     # [nf,3,3] float64: {kd, ks, n} per face and channel
    info: object         # [nf,3,10] float64: levmar's info[] of the weighted fit (info[1]: the weighted objective, without `within`)
    ret: object          # [nf,3] int32: iterations, or -1
    stats: FitStats | None  # the full-sample statistics: covar [nf,3,3,3], stats [nf,3,8], rank [nf,3]; None without want_stats
    count: object        # [nf,3] int32: k, the samples of the fit
    lights: object       # [nf,3] int32: the lights with a sample, the weighted fit's n
    face_pixels: object  # [nf] int32: the pixels that carry the face (0 where none)
    avg: np.ndarray      # [3]
    n_pixels: int
    n_faces: int


def fit_capture_means(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, *, v_min: int = 0, v_max: int = 255,
                      cos_min: float = -2.0, rv_mode: int = 0, p0=(0.5, 1.0, 1.0), lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0),
                      itmax: int = 100, opts=None, want_stats: bool = True, validate: bool = True, out: CaptureMeans | None = None) -> CaptureMeans:
    """fit_capture_faces as a weighted fit of per-light means (brdf_hip_fit_capture_means_dev; L <= 16): all pixels of a face share its
    cosines, so the fit of a face's k samples and the fit of its at most L per-light means, weighted by the lights' sample counts, have
    the same minimiser -- capture_light_means is the definition as code.  Same candidates and validity rule as fit_capture_faces.
    `info` is the weighted fit's; `stats` (sumsq, covariance with k - 3 degrees of freedom, sigma, rho, R2) are the full-sample ones.
    Fewer than 3 lights with a sample: ret -1, zero info, p0 in surfaces, rank 0.  The call waits for the stream."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, p0, lb, ub, itmax, opts,
                                   validate)
    dev = keep[0].device
    if out is None:
        def z(*shape, dtype=torch.float64):
            return torch.zeros((nf, *shape), dtype=dtype, device=dev)
        out = CaptureMeans(z(3, 3), z(3, 10), z(3, dtype=torch.int32), _zero_stats((nf, 3), dev) if want_stats else None, z(3, dtype=torch.int32),
                           z(3, dtype=torch.int32), z(dtype=torch.int32), None, 0, 0)
    _require(not want_stats or out.stats is not None, "out: want_stats needs out.stats")
    st = out.stats if want_stats else None
    maps = [(out.surfaces, (nf, 3, 3), torch.float64), (out.info, (nf, 3, 10), torch.float64), (out.ret, (nf, 3), torch.int32),
            (out.count, (nf, 3), torch.int32), (out.lights, (nf, 3), torch.int32), (out.face_pixels, (nf,), torch.int32)]
    if st is not None:
        maps += [(st.covar, (nf, 3, 3, 3), torch.float64), (st.stats, (nf, 3, 8), torch.float64), (st.rank, (nf, 3), torch.int32)]
    for t, shape, dtype in maps:
        _require(t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous(),
                 f"out: contiguous CUDA {dtype} {list(shape)} tensors on the capture's device")
    avg = np.zeros(3)
    npx, nfc = C.c_longlong(0), C.c_longlong(0)
    _call("brdf_hip_fit_capture_means_dev", dev, *args, int(v_min), int(v_max), float(cos_min), out.surfaces.data_ptr(), out.info.data_ptr(),
          out.ret.data_ptr(), None if st is None else st.covar.data_ptr(), None if st is None else st.stats.data_ptr(),
          None if st is None else st.rank.data_ptr(), out.count.data_ptr(), out.lights.data_ptr(), out.face_pixels.data_ptr(), _dptr(avg),
          C.byref(npx), C.byref(nfc), _STREAM)
    return CaptureMeans(out.surfaces, out.info, out.ret, st, out.count, out.lights, out.face_pixels, avg, npx.value, nfc.value)


class CaptureMeansClipped(NamedTuple):
    """What fit_capture_means_clipped returns: CaptureMeans' fields and the clip's four maps."""
    surfaces: object
    info: object
    ret: object
    stats: FitStats | None  # over the returned sample sets
    count: object        # [nf,3] int32: the fit's samples under the validity rule, before any clip
    lights: object       # [nf,3] int32: the lights with a sample in the returned set
    face_pixels: object
    avg: np.ndarray
    n_pixels: int
    n_faces: int
    kept: object         # [nf,3] int32: k of the returned set
    rounds: object       # [nf,3] int32: the last clip round that refitted the fit (0: none)
    vlo: object          # [nf,3,L] uint8: the returned set's grey-level interval per light of the capture, lowest level
    vhi: object          # [nf,3,L] uint8: highest level (vlo = 1, vhi = 0: no level)


def fit_capture_means_clipped(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, *, kappa: float, sigma_min: float,
                              rounds: int, v_min: int = 0, v_max: int = 255, cos_min: float = -2.0, rv_mode: int = 0, p0=(0.5, 1.0, 1.0),
                              lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0), itmax: int = 100, opts=None, want_stats: bool = True,
                              validate: bool = True, out: CaptureMeansClipped | None = None) -> CaptureMeansClipped:
    """fit_capture_means with sigma clipping (brdf_hip_fit_capture_means_clipped_dev; L <= 16): fit, drop the samples further than
    kappa * sigma from the fit, fit the survivors' per-light means again from the current p, at most `rounds` times or until nothing
    more is dropped.  All pixels of a face share its cosines, so a round's survivors under one light are an interval of grey levels:
    the clip state is `vlo`, `vhi`, and a round accumulates the integer sums again under them -- clip_light_means is one round as
    NumPy code, capture_light_means(v_lo=, v_hi=) the rows under given intervals.  sigma = max(sqrt(sumsq / (k - 3)), sigma_min) with
    the full-sample sumsq of the weighted statistics pass (k == 3: sigma_min; SIGMA_MIN_8BIT is recommended); a fit that is refused,
    ends with ret < 0, drops nothing or would keep fewer than 3 lights is settled and keeps its samples.  `count` stays the unclipped
    sample count, `kept` and `lights` are the returned set's, `stats` are taken over it.  rounds = 0 or kappa = inf give
    fit_capture_means' bytes in every map it has.  `out`: an earlier result (or one built by hand) whose tensors are written into."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, p0, lb, ub, itmax, opts,
                                   validate)
    dev = keep[0].device
    L = int(keep[0].shape[0])

    def z(*shape, dtype=torch.float64):
        return torch.zeros((nf, *shape), dtype=dtype, device=dev)
    if out is None:
        i32, u8 = torch.int32, torch.uint8
        out = CaptureMeansClipped(z(3, 3), z(3, 10), z(3, dtype=i32), _zero_stats((nf, 3), dev) if want_stats else None, z(3, dtype=i32), z(3, dtype=i32),
                                  z(dtype=i32), None, 0, 0, z(3, dtype=i32), z(3, dtype=i32), z(3, L, dtype=u8), z(3, L, dtype=u8))
    _require(not want_stats or out.stats is not None, "out: want_stats needs out.stats")
    st = out.stats if want_stats else None
    maps = [(out.surfaces, (nf, 3, 3), torch.float64), (out.info, (nf, 3, 10), torch.float64), (out.face_pixels, (nf,), torch.int32),
            (out.vlo, (nf, 3, L), torch.uint8), (out.vhi, (nf, 3, L), torch.uint8)]
    maps += [(t, (nf, 3), torch.int32) for t in (out.ret, out.count, out.lights, out.kept, out.rounds)]
    if st is not None:
        maps += [(st.covar, (nf, 3, 3, 3), torch.float64), (st.stats, (nf, 3, 8), torch.float64), (st.rank, (nf, 3), torch.int32)]
    for t, shape, dtype in maps:
        _require(t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous(),
                 f"out: contiguous CUDA {dtype} {list(shape)} tensors on the capture's device")
    avg = np.zeros(3)
    npx, nfc = C.c_longlong(0), C.c_longlong(0)
    _call("brdf_hip_fit_capture_means_clipped_dev", dev, *args, int(v_min), int(v_max), float(cos_min), out.surfaces.data_ptr(), out.info.data_ptr(),
          out.ret.data_ptr(), None if st is None else st.covar.data_ptr(), None if st is None else st.stats.data_ptr(),
          None if st is None else st.rank.data_ptr(), out.count.data_ptr(), out.lights.data_ptr(), out.face_pixels.data_ptr(), _dptr(avg),
          C.byref(npx), C.byref(nfc), _STREAM, float(kappa), float(sigma_min), int(rounds), out.kept.data_ptr(), out.rounds.data_ptr(),
          out.vlo.data_ptr(), out.vhi.data_ptr())
    return CaptureMeansClipped(out.surfaces, out.info, out.ret, st, out.count, out.lights, out.face_pixels, avg, npx.value, nfc.value, out.kept,
                               out.rounds, out.vlo, out.vhi)


class LightMeans(NamedTuple):
    """What capture_light_means returns: the weighted batch of fit_capture_means, rows of stride L (NumPy)."""
    angles: np.ndarray       # [fits,3,L] float64: the face's cosines at the lights with a sample, ascending; NaN behind counts
    x: np.ndarray            # [fits,L] float64: the lights' means S1 / (255 c)
    w: np.ndarray            # [fits,L] float64: the lights' sample counts c
    counts: np.ndarray       # [fits] int32: the lights with a sample
    k: np.ndarray            # [fits] int32: the samples, sum c
    within: np.ndarray       # [fits] float64: sum_l (c S2 - S1^2) / (65025 c)
    fit_face: np.ndarray     # [fits] int32
    fit_channel: np.ndarray  # [fits] int32
    face_pixels: np.ndarray  # [nf] int32


def capture_light_means(images, pixel_map, face_angles, model: int, *, v_min: int = 0, v_max: int = 255, cos_min: float = -2.0, v_lo=None,
                        v_hi=None) -> LightMeans:
    """The host twin of fit_capture_means' accumulation (NumPy, no device): its definition as code.  Arguments, fits (ascending face,
    then channel), candidates and validity rule as group_capture_samples.  Per fit and light l with c_l > 0 valid values v:
    x_l = sum v / (255 c_l), w_l = c_l; the lights with a sample in ascending order at the front of rows of stride L; k = sum c_l;
    within = sum_l (c_l sum v^2 - (sum v)^2) / (65025 c_l), the numerator in integers, added in ascending light order.
    v_lo, v_hi ([fits,L], optional, both or neither): the grey-level intervals of fit_capture_means_clipped -- a valid value v under
    light l is a sample iff v_lo[s, l] <= v <= v_hi[s, l]; without them every valid value is."""
    images, pixel_map = np.asarray(images), np.asarray(pixel_map)
    face_angles = np.ascontiguousarray(face_angles, dtype=np.float64)
    _require(images.ndim == 4 and images.shape[3] == 3 and images.dtype == np.uint8 and pixel_map.shape == images.shape[1:3],
             "images [L,H,W,3] uint8, pixel_map [H,W]")
    L, H, W = images.shape[:3]
    _require(face_angles.ndim == 3 and face_angles.shape[1:] == (3, L), "face_angles [nf,3,L]")
    _require(model in (MODEL_PHONG, MODEL_BLINN_PHONG, MODEL_WARD), "unknown model")
    nf = face_angles.shape[0]
    reads = [True, model != MODEL_PHONG, model != MODEL_BLINN_PHONG]  # the planes the model reads
    face_pixels = np.zeros(nf, dtype=np.int32)
    values = {}  # face -> [L, pixels, 3] int64
    for f in range(nf):
        ys, xs = np.nonzero(pixel_map == f)
        face_pixels[f] = ys.size
        if ys.size:
            values[f] = images[:, H - 1 - ys, xs, :].astype(np.int64)
    fits = 3 * len(values)
    _require((v_lo is None) == (v_hi is None), "v_lo and v_hi: both or neither")
    if v_lo is not None:
        v_lo, v_hi = np.asarray(v_lo).astype(np.int64), np.asarray(v_hi).astype(np.int64)
        _require(v_lo.shape == (fits, L) and v_hi.shape == (fits, L), "v_lo, v_hi [fits,L]")
    angles, x, w = np.full((fits, 3, L), np.nan), np.full((fits, L), np.nan), np.full((fits, L), np.nan)
    counts, k, within = np.zeros(fits, dtype=np.int32), np.zeros(fits, dtype=np.int32), np.zeros(fits)
    fit_face, fit_channel = np.zeros(fits, dtype=np.int32), np.zeros(fits, dtype=np.int32)
    s = 0
    for f in sorted(values):
        cos_ok = np.all([face_angles[f, j, :] > cos_min for j in range(3) if reads[j]], axis=0)  # [L]
        for ch in range(3):
            fit_face[s], fit_channel[s] = f, ch
            n = 0
            for l in range(L):
                v = values[f][l, :, ch]
                v = v[(v >= v_min) & (v <= v_max)] if cos_ok[l] else v[:0]
                if v_lo is not None:
                    v = v[(v >= v_lo[s, l]) & (v <= v_hi[s, l])]
                c = int(v.size)
                if c == 0:
                    continue
                s1, s2 = int(v.sum()), int((v * v).sum())
                angles[s, :, n] = face_angles[f, :, l]
                x[s, n] = float(s1) / (255.0 * float(c))
                w[s, n] = float(c)
                within[s] += float(c * s2 - s1 * s1) / (65025.0 * float(c))
                k[s] += c
                n += 1
            counts[s] = n
            s += 1
    return LightMeans(angles, x, w, counts, k, within, fit_face, fit_channel, face_pixels)


def initial_light_intervals(face_angles, fit_face, model: int, *, v_min: int = 0, v_max: int = 255, cos_min: float = -2.0):
    """The intervals fit_capture_means_clipped starts from (NumPy): per fit of fit_face [fits] and light, [v_min, v_max] clamped to
    0 ... 255 where every plane the model reads is > cos_min (a NaN is not), and the empty interval lo = 1, hi = 0 elsewhere.
    Returns (v_lo, v_hi), uint8 [fits,L]."""
    face_angles = np.asarray(face_angles, dtype=np.float64)
    reads = [True, model != MODEL_PHONG, model != MODEL_BLINN_PHONG]
    a = face_angles[np.asarray(fit_face, dtype=np.int64)]  # [fits,3,L]
    with np.errstate(invalid="ignore"):
        cos_ok = np.all([a[:, j, :] > cos_min for j in range(3) if reads[j]], axis=0)
    lo, hi = int(np.clip(v_min, 0, 255)), int(np.clip(v_max, 0, 255))
    return np.where(cos_ok, lo, 1).astype(np.uint8), np.where(cos_ok, hi, 0).astype(np.uint8)


def clip_light_means(images, pixel_map, face_angles, model: int, p, sumsq, ret, v_lo, v_hi, *, kappa: float, sigma_min: float, v_min: int = 0,
                     v_max: int = 255, cos_min: float = -2.0):
    """ONE clip round of fit_capture_means_clipped's definition, as NumPy code on the host (no device).  The capture and the rule as
    capture_light_means; v_lo, v_hi [fits,L] the fits' CURRENT intervals (initial_light_intervals before the first round), p [fits,3]
    their current parameters, sumsq [fits] the weighted statistics pass's stats[:, 0] at p over the current rows with extra_ss = within
    and nobs = k, ret [fits] the fits' ret.  Returns (new v_lo, new v_hi, settled [fits] bool).  For a fit with ret < 0, fewer than 3
    lights with a sample or a sumsq that is not finite: settled, its intervals as they came.  Otherwise sigma = max(sqrt(sumsq /
    (k - 3)), sigma_min) (k == 3: sigma_min), grey level v under light l survives iff |v / 255.0 - f_l(p)| <= kappa * sigma (a NaN
    does not), and a light's new interval runs from the smallest to the largest surviving v inside the old one (empty, lo = 1 and
    hi = 0, if none survives).  No sample dropped, or fewer than 3 lights keep a sample: settled, the intervals as they came.  The
    caller marks settled fits and never passes them as unsettled again: here every fit given is looked at."""
    from . import synth
    face_angles = np.ascontiguousarray(face_angles, dtype=np.float64)
    v_lo, v_hi = np.asarray(v_lo), np.asarray(v_hi)
    cur = capture_light_means(images, pixel_map, face_angles, model, v_min=v_min, v_max=v_max, cos_min=cos_min, v_lo=v_lo, v_hi=v_hi)
    fits, L = v_lo.shape
    p, sumsq, ret = np.asarray(p, dtype=np.float64), np.asarray(sumsq, dtype=np.float64), np.asarray(ret)
    _require(p.shape == (fits, 3) and sumsq.shape == (fits,) and ret.shape == (fits,), "p [fits,3], sumsq [fits], ret [fits]")
    new_lo, new_hi = v_lo.astype(np.uint8).copy(), v_hi.astype(np.uint8).copy()
    settled = np.ones(fits, dtype=bool)
    for s in range(fits):
        k = int(cur.k[s])
        if ret[s] < 0 or cur.counts[s] < 3 or not np.isfinite(sumsq[s]):
            continue
        a = face_angles[cur.fit_face[s]]  # [3,L]: by the capture's light index
        grey = np.arange(256)
        with np.errstate(all="ignore"):
            sigma = max(float(np.sqrt(sumsq[s] / (k - 3))), float(sigma_min)) if k > 3 else float(sigma_min)
            f = synth.model_value(model, p[s], a[0], a[1], a[2])  # [L]
            ok = np.abs(grey[None, :] / 255.0 - f[:, None]) <= np.float64(kappa) * np.float64(sigma)  # [L,256] (False for a NaN)
        ok &= (grey[None, :] >= v_lo[s].astype(np.int64)[:, None]) & (grey[None, :] <= v_hi[s].astype(np.int64)[:, None])
        any_ok = ok.any(axis=1)
        lo = np.where(any_ok, ok.argmax(axis=1), 1)
        hi = np.where(any_ok, 255 - ok[:, ::-1].argmax(axis=1), 0)
        sub = _light_sums(images, pixel_map, face_angles, model, cur.fit_face[s], cur.fit_channel[s], lo, hi, v_min, v_max, cos_min)
        if int(sub.sum()) >= k or int((sub > 0).sum()) < 3:
            continue
        new_lo[s], new_hi[s] = lo, hi
        settled[s] = False
    return new_lo, new_hi, settled


def _light_sums(images, pixel_map, face_angles, model, face, channel, lo, hi, v_min, v_max, cos_min):
    """the samples per light of fit (face, channel) under the rule and the intervals lo, hi [L]"""
    images, pixel_map = np.asarray(images), np.asarray(pixel_map)
    L, H = images.shape[:2]
    reads = [True, model != MODEL_PHONG, model != MODEL_BLINN_PHONG]
    with np.errstate(invalid="ignore"):
        cos_ok = np.all([face_angles[face, j, :] > cos_min for j in range(3) if reads[j]], axis=0)
    ys, xs = np.nonzero(pixel_map == face)
    v = images[:, H - 1 - ys, xs, channel].astype(np.int64)  # [L, pixels]
    ok = (v >= v_min) & (v <= v_max) & cos_ok[:, None] & (v >= np.asarray(lo)[:, None]) & (v <= np.asarray(hi)[:, None])
    return ok.sum(axis=1)


def fit_capture_single(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, *, rv_mode: int = 0,
                       p0=(0.0, 0.0, 0.0), lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0), itmax: int = 2000,
                       opts=(1e-3, 1e-15, 1e-10, 1e-50, 1.0), validate: bool = True):
    """CalcBRDFEquation_SingleBRDF (brdfdata.cpp:1138-1186) on the device: one {kd, ks, n} per colour channel for the
    whole object.  Defaults are the reference's call-site values (brdfdata.cpp:1002, :1046-1056).  Returns
    (single_brdf [3,3], info [3,10], faces used)."""
    args, keep, _ = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, p0, lb, ub, itmax, opts,
                                  validate)
    out, info = np.zeros(9), np.zeros(30)
    nfu = C.c_longlong(0)
    _call("brdf_hip_fit_capture_single_dev", keep[0].device, *args, _dptr(out), _dptr(info), C.byref(nfu), _STREAM)
    return out.reshape(3, 3), info.reshape(3, 10), nfu.value


class CaptureSingleFaces(NamedTuple):
    """What fit_capture_single_faces returns: the three channels' fits (NumPy), the face maps (CUDA tensors) and the host scalars."""
    single_brdf: np.ndarray  # [3,3] float64: {kd, ks, n} per channel (B, G, R)
    info: np.ndarray         # [3,10] float64: levmar's info[]
    ret: np.ndarray          # [3] int32: iterations, or -1
    count: np.ndarray        # [3] int64: K_c, the samples of the channel's fit
    stats: FitStats | None   # host covar [3,3,3], stats [3,8], rank [3]; None without want_stats
    face_sumsq: object       # [nf,3] float64: the face's sum of squared residuals against the channel's fit
    face_count: object       # [nf,3] int32: the face's samples in the channel
    face_pixels: object      # [nf] int32: the pixels that carry the face (0 where none)
    n_pixels: int
    n_faces: int


def fit_capture_single_faces(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, *, v_min: int = 0, v_max: int = 255,
                             cos_min: float = -2.0, rv_mode: int = 0, p0=(0.5, 1.0, 1.0), lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0),
                             itmax: int = 100, opts=None, want_stats: bool = True, validate: bool = True,
                             out: CaptureSingleFaces | None = None) -> CaptureSingleFaces:
    """ONE fit per colour channel for the whole object over the valid samples of EVERY pixel of every carried face
    (brdf_hip_fit_capture_single_faces_dev), where fit_capture_single takes each face's last pixel and knows no validity rule.
    Arguments as fit_capture; the validity rule as fit_capture_masked (the defaults switch it off).  Channel c's samples are those of
    fit_capture_faces' fits (face, c), ascending faces one behind the other -- group_capture_single_samples is this definition as
    code -- and single_brdf / info / ret have the bytes of fit_single(METHOD_BC_DIF, ...) on them, stats those of fit_stats_batch
    with S = 1.  A channel of fewer than 3 samples is refused: ret -1, zero info, p0, rank 0.  face_sumsq[f, c] is the face's sum of
    squared residuals against channel c's fit, face_count[f, c] its samples; faces no pixel carries keep what the maps held: zeros, or
    the values of `out`, an earlier result (or one built by hand) whose three tensors are written into.  The call waits for the
    stream."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, p0, lb, ub, itmax, opts,
                                   validate)
    _require(args[13] is not None, "p0 is required")
    dev = keep[0].device
    if out is None:
        face_sumsq = torch.zeros((nf, 3), dtype=torch.float64, device=dev)
        face_count = torch.zeros((nf, 3), dtype=torch.int32, device=dev)
        face_pixels = torch.zeros((nf,), dtype=torch.int32, device=dev)
    else:
        face_sumsq, face_count, face_pixels = out.face_sumsq, out.face_count, out.face_pixels
    for t, shape, dtype in ((face_sumsq, (nf, 3), torch.float64), (face_count, (nf, 3), torch.int32), (face_pixels, (nf,), torch.int32)):
        _require(t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous(),
                 f"out: contiguous CUDA {dtype} {list(shape)} tensors on the capture's device")
    single, info, ret, count = np.zeros((3, 3)), np.zeros((3, 10)), np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int64)
    st = _zero_stats((3,)) if want_stats else None
    npx, nfc = C.c_longlong(0), C.c_longlong(0)
    name = "brdf_hip_fit_capture_single_faces_dev"
    with torch.cuda.device(dev):  # (not _call: the entry returns the number of refused or failed channels)
        rc = getattr(lib, name)(*args, int(v_min), int(v_max), float(cos_min), _dptr(single), _dptr(info), _iptr(ret),
                                None if st is None else _dptr(st.covar), None if st is None else _dptr(st.stats),
                                None if st is None else _iptr(st.rank), count.ctypes.data_as(C.POINTER(C.c_longlong)), face_sumsq.data_ptr(),
                                face_count.data_ptr(), face_pixels.data_ptr(), C.byref(npx), C.byref(nfc), _stream_handle(torch))
    if rc < 0:
        raise RuntimeError(f"{name} failed: {last_error()}")
    return CaptureSingleFaces(single, info, ret, count, st, face_sumsq, face_count, face_pixels, npx.value, nfc.value)


class SingleSamples(NamedTuple):
    """What group_capture_single_samples returns (NumPy)."""
    channels: tuple          # per channel (angles [3,K_c] float64, x [K_c] float64, face_offsets [F+1] int64: where a face's samples start)
    faces: np.ndarray        # [F] int32: the carried faces, ascending
    face_pixels: np.ndarray  # [nf] int32


def group_capture_single_samples(images, pixel_map, face_angles, model: int, *, v_min: int = 0, v_max: int = 255,
                                 cos_min: float = -2.0) -> SingleSamples:
    """The host twin of fit_capture_single_faces' sample sets (NumPy, no device): its definition as code.  Arguments, candidates and
    validity rule as group_capture_samples; channel c's sample set is the concatenation, over the carried faces in ascending order, of
    the sample sets group_capture_samples gives for (face, c), laid out as a single fit reads it."""
    a, x, off, fit_face, fit_channel, face_pixels = group_capture_samples(images, pixel_map, face_angles, model, v_min=v_min, v_max=v_max,
                                                                          cos_min=cos_min)
    carried = np.ascontiguousarray(fit_face[0::3], dtype=np.int32)  # (fits: ascending face, then channel)
    channels = []
    for c in range(3):
        planes, xs, face_offsets = [np.zeros((3, 0))], [np.zeros(0)], [0]
        for s in range(c, len(fit_face), 3):
            k = int(off[s + 1] - off[s])
            planes.append(a[3 * off[s]:3 * off[s + 1]].reshape(3, k))
            xs.append(x[off[s]:off[s + 1]])
            face_offsets.append(face_offsets[-1] + k)
        channels.append((np.ascontiguousarray(np.concatenate(planes, axis=1)), np.ascontiguousarray(np.concatenate(xs)),
                         np.array(face_offsets, dtype=np.int64)))
    return SingleSamples(tuple(channels), carried, face_pixels)


# ---- K materials per object: residuals against M materials, one fit per (label, channel), Lloyd's iteration around the two ----------
def _materials_tensor(materials, dev, torch):
    """[M,3,3] float64 on `dev`: the caller's contiguous CUDA tensor itself (the labelled entries write into it), or an upload"""
    if not torch.is_tensor(materials):
        materials = torch.from_numpy(np.ascontiguousarray(materials, dtype=np.float64)).to(dev)
    _require(materials.is_cuda and materials.device == dev and materials.dtype == torch.float64 and materials.dim() == 3
             and tuple(materials.shape[1:]) == (3, 3) and materials.shape[0] >= 1 and materials.is_contiguous(),
             "materials: [M,3,3] float64 (material, channel, parameter), contiguous, on the capture's device")
    return materials


class FaceResiduals(NamedTuple):
    """What capture_face_residuals returns (CUDA tensors and the host scalars)."""
    face_sumsq: object   # [nf,M,3] float64
    face_count: object   # [nf,3] int32
    face_pixels: object  # [nf] int32
    n_pixels: int
    n_faces: int


def capture_face_residuals(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, materials, *, v_min: int = 0,
                           v_max: int = 255, cos_min: float = -2.0, rv_mode: int = 0, validate: bool = True,
                           out: FaceResiduals | None = None) -> FaceResiduals:
    """The carried faces' sums of squared residuals against M candidate materials in one read of the samples
    (brdf_hip_capture_face_residuals_dev).  Capture and validity rule as fit_capture_single_faces; materials [M,3,3] (material, channel,
    {kd, ks, n}), a CUDA tensor or NumPy.  face_sumsq[f, m, c] is the sum over the face's valid samples of channel c of
    (x - f(materials[m, c]))^2 with fit_capture_single_faces' summation: column m has the bytes that call writes to its face_sumsq when
    its single_brdf equals materials[m], whatever M is and wherever m stands.  A sum that is not finite is stored as it comes.  Faces no
    pixel carries keep what the maps held: zeros, or the values of `out`."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, None, None, None, 0, None,
                                   validate)
    dev = keep[0].device
    materials = _materials_tensor(materials, dev, torch)
    M = int(materials.shape[0])
    if out is None:
        out = FaceResiduals(torch.zeros((nf, M, 3), dtype=torch.float64, device=dev), torch.zeros((nf, 3), dtype=torch.int32, device=dev),
                            torch.zeros((nf,), dtype=torch.int32, device=dev), 0, 0)
    for t, shape, dtype in ((out.face_sumsq, (nf, M, 3), torch.float64), (out.face_count, (nf, 3), torch.int32), (out.face_pixels, (nf,), torch.int32)):
        _require(t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous(),
                 f"out: contiguous CUDA {dtype} {list(shape)} tensors on the capture's device")
    npx, nfc = C.c_longlong(0), C.c_longlong(0)
    _call("brdf_hip_capture_face_residuals_dev", dev, *args[:13], int(v_min), int(v_max), float(cos_min), materials.data_ptr(), M,
          out.face_sumsq.data_ptr(), out.face_count.data_ptr(), out.face_pixels.data_ptr(), C.byref(npx), C.byref(nfc), _STREAM)
    return FaceResiduals(out.face_sumsq, out.face_count, out.face_pixels, npx.value, nfc.value)


class CaptureLabelled(NamedTuple):
    """What fit_capture_labelled returns: rows [label, channel] (CUDA tensors) and the host scalars."""
    materials: object    # [K,3,3] float64: {kd, ks, n} per label and channel
    info: object         # [K,3,10] float64
    ret: object          # [K,3] int32
    stats: FitStats | None  # covar [K,3,3,3], stats [K,3,8], rank [K,3]; None without want_stats
    count: object        # [K,3] int32: the samples of the fit
    label_faces: object  # [K] int32: the carried faces of the label
    face_pixels: object  # [nf] int32
    n_pixels: int
    n_faces: int


def _labelled_maps(K, nf, dev, want_stats, torch):
    i32 = torch.int32
    return (torch.zeros((K, 3, 10), dtype=torch.float64, device=dev), torch.zeros((K, 3), dtype=i32, device=dev),
            _zero_stats((K, 3), dev) if want_stats else None, torch.zeros((K, 3), dtype=i32, device=dev), torch.zeros((K,), dtype=i32, device=dev),
            torch.zeros((nf,), dtype=i32, device=dev))


def fit_capture_labelled(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, labels, materials, *, v_min: int = 0,
                         v_max: int = 255, cos_min: float = -2.0, rv_mode: int = 0, lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0), itmax: int = 100,
                         opts=None, workspace_bytes: int = 0, want_stats: bool = True, validate: bool = True) -> CaptureLabelled:
    """ONE fit per (label, channel) over the valid samples of the faces that carry the label (brdf_hip_fit_capture_labelled_dev).
    labels [nf] int32 (CUDA tensor or NumPy): a face whose label is outside [0, K) takes part in nothing.  materials [K,3,3]: the
    starting points; a contiguous CUDA tensor is overwritten with the results, as fit_batch_packed's p0 is.  Fit (k, c)'s samples are
    the carried faces with label k in ascending face index, a face's pixels in the reference's walk, the lights inside a pixel, those
    the rule leaves for channel c -- group_capture_label_samples is this definition as code -- and the 3 K fits are rows c * K + k of
    one packed batch: every map has the bytes fit_batch_packed / fit_stats_batch_packed give for that batch from the same starts.
    Fewer than 3 samples: ret -1, zero info, the material untouched, rank 0.  The call waits for the stream."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, None, lb, ub, itmax, opts,
                                   validate)
    dev = keep[0].device
    materials = _materials_tensor(materials, dev, torch)
    K = int(materials.shape[0])
    if not torch.is_tensor(labels):
        labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
    _require(labels.is_cuda and labels.device == dev and labels.dtype == torch.int32 and tuple(labels.shape) == (nf,) and labels.is_contiguous(),
             "labels: [nf] int32, contiguous, on the capture's device")
    info, ret, st, count, label_faces, face_pixels = _labelled_maps(K, nf, dev, want_stats, torch)
    npx, nfc = C.c_longlong(0), C.c_longlong(0)
    _call("brdf_hip_fit_capture_labelled_dev", dev, *args[:13], *args[14:18], int(v_min), int(v_max), float(cos_min), int(workspace_bytes),
          labels.data_ptr(), K, materials.data_ptr(), info.data_ptr(), ret.data_ptr(), None if st is None else st.covar.data_ptr(),
          None if st is None else st.stats.data_ptr(), None if st is None else st.rank.data_ptr(), count.data_ptr(), label_faces.data_ptr(),
          face_pixels.data_ptr(), C.byref(npx), C.byref(nfc), _STREAM)
    return CaptureLabelled(materials, info, ret, st, count, label_faces, face_pixels, npx.value, nfc.value)


class CaptureMaterials(NamedTuple):
    """What fit_capture_materials returns: the materials' rows [label, channel], the face maps (CUDA tensors) and the host scalars."""
    materials: object    # [K,3,3] float64
    labels: object       # [nf] int32: the face's material; -1: no pixel carries the face, or no material could take it
    face_sumsq: object   # [nf,3] float64: against the face's own material (+inf on a carried face with label -1)
    face_count: object   # [nf,3] int32
    info: object         # [K,3,10]: the last refit's; zeros if none ran
    ret: object          # [K,3]: the last refit's; -1 if none ran
    stats: FitStats | None
    count: object        # [K,3] int32
    label_faces: object  # [K] int32
    face_pixels: object  # [nf] int32
    rounds_used: int     # the refits
    settled: bool        # the last assignment moved no label
    changed: np.ndarray  # [assignments] int64: the faces whose label changed, per assignment
    n_pixels: int
    n_faces: int


def fit_capture_materials(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, seeds, *, rounds: int = 20,
                          v_min: int = 0, v_max: int = 255, cos_min: float = -2.0, rv_mode: int = 0, lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0),
                          itmax: int = 100, opts=None, workspace_bytes: int = 0, want_stats: bool = True, validate: bool = True) -> CaptureMaterials:
    """K materials and a label per face (brdf_hip_fit_capture_materials_dev): Lloyd's iteration with levmar as the centroid step.
    seeds [K,3,3] (seed_materials gives a deterministic set; the caller's tensor is not written).  All labels start at -1; then
    (1) assign every carried face to the material of least cost (s[f,k,0] + s[f,k,1]) + s[f,k,2] over capture_face_residuals' sums, a
    cost that is not finite counting as +inf, the lowest k on a tie, the label staying where every cost is +inf -- assign_materials is
    this step as NumPy code; (2) nothing changed: settled; `rounds` (0 ... 64) refits done: stop; (3) refit every material over its
    faces from the current materials (fit_capture_labelled); after refit number `rounds` the loop ends without another assignment,
    otherwise (1).  So `materials` are always fit_capture_labelled's bytes on `labels` from the materials of the round before;
    rounds = 0 returns the seeds and one assignment.  face_sumsq / face_count come from one last residual pass."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, None, lb, ub, itmax, opts,
                                   validate)
    dev = keep[0].device
    materials = _materials_tensor(seeds, dev, torch).clone()
    K = int(materials.shape[0])
    _require(0 <= int(rounds) <= 64, "rounds: 0 ... 64")
    labels = torch.full((nf,), -1, dtype=torch.int32, device=dev)
    face_sumsq = torch.zeros((nf, 3), dtype=torch.float64, device=dev)
    face_count = torch.zeros((nf, 3), dtype=torch.int32, device=dev)
    info, ret, st, count, label_faces, face_pixels = _labelled_maps(K, nf, dev, want_stats, torch)
    used, settled = C.c_int(0), C.c_int(0)
    changed = np.full(int(rounds) + 1, -1, dtype=np.int64)
    npx, nfc = C.c_longlong(0), C.c_longlong(0)
    _call("brdf_hip_fit_capture_materials_dev", dev, *args[:13], *args[14:18], int(v_min), int(v_max), float(cos_min), int(workspace_bytes), K,
          int(rounds), materials.data_ptr(), labels.data_ptr(), face_sumsq.data_ptr(), face_count.data_ptr(), info.data_ptr(), ret.data_ptr(),
          None if st is None else st.covar.data_ptr(), None if st is None else st.stats.data_ptr(), None if st is None else st.rank.data_ptr(),
          count.data_ptr(), label_faces.data_ptr(), face_pixels.data_ptr(), C.byref(used), C.byref(settled),
          changed.ctypes.data_as(C.POINTER(C.c_longlong)), C.byref(npx), C.byref(nfc), _STREAM)
    return CaptureMaterials(materials, labels, face_sumsq, face_count, info, ret, st, count, label_faces, face_pixels, used.value, bool(settled.value),
                            changed[changed >= 0], npx.value, nfc.value)


class LabelSamples(NamedTuple):
    """What group_capture_label_samples returns (NumPy): the packed batch fit_capture_labelled fits, rows channel * K + label."""
    angles: np.ndarray       # [3 * total] float64
    x: np.ndarray            # [total] float64
    offsets: np.ndarray      # [3 K + 1] int64
    label_faces: np.ndarray  # [K] int32: the carried faces of the label
    face_pixels: np.ndarray  # [nf] int32


def group_capture_label_samples(images, pixel_map, face_angles, model: int, labels, K: int, *, v_min: int = 0, v_max: int = 255,
                                cos_min: float = -2.0) -> LabelSamples:
    """The host twin of fit_capture_labelled's sample sets (NumPy, no device): its definition as code.  Arguments, candidates and
    validity rule as group_capture_samples; labels [nf].  Fit (k, c) -- row c * K + k of the packed batch -- is the concatenation, over
    the carried faces with label k in ascending order, of the sample sets group_capture_samples gives for (face, c).  A face whose
    label is outside [0, K) takes part in nothing."""
    a, x, off, fit_face, _, face_pixels = group_capture_samples(images, pixel_map, face_angles, model, v_min=v_min, v_max=v_max, cos_min=cos_min)
    labels = np.asarray(labels).astype(np.int64)
    _require(labels.shape == (face_pixels.size,) and K >= 1, "labels [nf], K >= 1")
    carried = fit_face[0::3].astype(np.int64)  # (fits: ascending face, then channel)
    label_faces = np.zeros(K, dtype=np.int32)
    planes, xs, offsets = [], [], [0]
    for c in range(3):
        for k in range(K):
            rows = np.flatnonzero(labels[carried] == k)
            if c == 0:
                label_faces[k] = rows.size
            fit_planes, n = [np.zeros((3, 0))], 0
            for r in rows:
                s = 3 * int(r) + c
                ks = int(off[s + 1] - off[s])
                fit_planes.append(a[3 * off[s]:3 * off[s + 1]].reshape(3, ks))
                xs.append(x[off[s]:off[s + 1]])
                n += ks
            planes.append(np.concatenate(fit_planes, axis=1).reshape(-1))
            offsets.append(offsets[-1] + n)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)  # noqa: E731
    return LabelSamples(np.ascontiguousarray(cat(planes), dtype=np.float64), np.ascontiguousarray(cat(xs), dtype=np.float64),
                        np.array(offsets, dtype=np.int64), label_faces, face_pixels)


def assign_materials(face_sumsq, labels, carried=None):
    """ONE assignment of fit_capture_materials as NumPy code.  face_sumsq [nf,K,3] (capture_face_residuals'), labels [nf] the current
    labels, carried [nf] bool (optional): the faces a pixel carries -- the others are never assigned.  cost[f, k] =
    (s[f,k,0] + s[f,k,1]) + s[f,k,2], in that order; a cost that is not finite is +inf; the new label is the least cost, the lowest k on
    a tie; every cost +inf: the label stays.  Returns (new labels [nf] int32, the number of faces whose label changed)."""
    s = np.asarray(face_sumsq, dtype=np.float64)
    labels = np.asarray(labels).astype(np.int32)
    _require(s.ndim == 3 and s.shape[2] == 3 and s.shape[1] >= 1 and labels.shape == (s.shape[0],), "face_sumsq [nf,K,3], labels [nf]")
    with np.errstate(all="ignore"):
        cost = (s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]
    cost = np.where(np.isfinite(cost), cost, np.inf)
    best = np.argmin(cost, axis=1).astype(np.int32)  # (the first of equal costs)
    takes = np.isfinite(cost[np.arange(cost.shape[0]), best])
    if carried is not None:
        takes &= np.asarray(carried, dtype=bool)
    new = np.where(takes, best, labels).astype(np.int32)
    return new, int((new != labels).sum())


def seed_materials(K: int, model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, *, face_fits=None, min_count: int = 16,
                   **capture):
    """K deterministic seeds for fit_capture_materials, [K,3,3] NumPy.  Seed 0 is fit_capture_single_faces' result.  Seed j is the
    per-face fit (`face_fits`: a fit_capture_faces result; computed here if None) of the face with the largest per-sample residual
    against its nearest current seed -- the least of its costs (assign_materials') over capture_face_residuals' sums against seeds
    0 ... j-1, divided by its samples of all three channels.  Only faces whose three fits have ret >= 0 and at least `min_count`
    samples are eligible, and a face gives one seed at most; the lowest face index wins a tie.  **capture: the captures' keyword arguments (rule, rv_mode, p0, lb, ub,
    itmax, opts, validate), passed on."""
    _require(K >= 1, "K >= 1")
    rule = {k: capture[k] for k in ("v_min", "v_max", "cos_min", "rv_mode", "validate") if k in capture}
    single = fit_capture_single_faces(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, want_stats=False, **capture)
    seeds = [np.array(single.single_brdf, dtype=np.float64)]
    if K == 1:
        return np.stack(seeds)
    if face_fits is None:
        face_fits = fit_capture_faces(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, want_stats=False, **capture)
    surfaces, ret, count = (t.cpu().numpy() for t in (face_fits.surfaces, face_fits.ret, face_fits.count))
    eligible = (ret >= 0).all(axis=1) & (count >= min_count).all(axis=1) & (face_fits.face_pixels.cpu().numpy() > 0)
    _require(bool(eligible.any()), "no face has three fits with ret >= 0 and min_count samples")
    samples = np.maximum(count.sum(axis=1), 1).astype(np.float64)
    for _ in range(1, K):
        res = capture_face_residuals(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, np.stack(seeds), **rule)
        s = res.face_sumsq.cpu().numpy()
        with np.errstate(all="ignore"):
            cost = (s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]
        nearest = np.where(np.isfinite(cost), cost, np.inf).min(axis=1) / samples
        nearest = np.where(eligible & np.isfinite(nearest), nearest, -np.inf)
        f = int(np.argmax(nearest))  # (the first of equal values)
        _require(bool(eligible[f]), "fewer eligible faces than seeds")
        eligible[f] = False
        seeds.append(np.array(surfaces[f], dtype=np.float64))
    return np.stack(seeds)


def host_dlevmar(method: int, model: int, angles: np.ndarray, x: np.ndarray, p0, *, lb=None, ub=None, dscl=None,
                 itmax=100, opts=None, want_covar=False) -> FitResult:
    """The drop-in call exactly as brdfdata.cpp:1058/1119 makes it: HOST arrays, a BRDFFunc-style callback
    (here the library's own BRDFFunc_hip) and a struct extraData payload."""
    angles = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.size
    p = _f64(p0, 3).copy()
    info = np.zeros(10)
    covar = np.zeros(9) if want_covar else None
    ed = ExtraData(_dptr(angles), model)
    func = C.cast(lib.BRDFFunc_hip, C.c_void_p)
    lb_a, ub_a, ds_a, op_a = _f64(lb, 3), _f64(ub, 3), _f64(dscl, 3), _f64(opts, 5)
    if method == METHOD_DIF:
        ret = lib.dlevmar_dif(func, _dptr(p), _dptr(x), 3, n, itmax, _dptr(op_a), _dptr(info), None, _dptr(covar),
                              C.byref(ed))
    elif method == METHOD_DER:  # dlevmar_der(BRDFFunc_hip, BRDFJac_hip, ...)
        ret = lib.dlevmar_der(func, C.cast(lib.BRDFJac_hip, C.c_void_p), _dptr(p), _dptr(x), 3, n, itmax, _dptr(op_a), _dptr(info),
                              None, _dptr(covar), C.byref(ed))
    elif method == METHOD_BC_DER:  # dlevmar_bc_der(BRDFFunc_hip, BRDFJac_hip, ...): the analytic Jacobian, all on the device
        ret = lib.dlevmar_bc_der(func, C.cast(lib.BRDFJac_hip, C.c_void_p), _dptr(p), _dptr(x), 3, n, _dptr(lb_a), _dptr(ub_a),
                                 _dptr(ds_a), itmax, _dptr(op_a), _dptr(info), None, _dptr(covar), C.byref(ed))
    else:
        ret = lib.dlevmar_bc_dif(func, _dptr(p), _dptr(x), 3, n, _dptr(lb_a), _dptr(ub_a), _dptr(ds_a), itmax,
                                 _dptr(op_a), _dptr(info), None, _dptr(covar), C.byref(ed))
    return FitResult(ret, p, info, None if covar is None else covar.reshape(3, 3))


def model_jacobian(model: int, angles: np.ndarray, p) -> np.ndarray:
    """BRDFJac_hip through host pointers: the analytic Jacobian [n, 3] of a built-in model."""
    a = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
    n = a.size // 3
    jac = np.zeros(3 * n)
    pa = _f64(p, 3).copy()
    ed = ExtraData(_dptr(a), model)
    lib.BRDFJac_hip(_dptr(pa), _dptr(jac), 3, n, C.byref(ed))
    return jac.reshape(n, 3)


def chkjac(model: int, angles: np.ndarray, p) -> np.ndarray:
    """dlevmar_chkjac (misc_core.c:250-321) on BRDFFunc_hip / BRDFJac_hip: err[n], ~1 where the Jacobian row is right."""
    a = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
    n = a.size // 3
    err = np.zeros(n)
    pa = _f64(p, 3).copy()
    ed = ExtraData(_dptr(a), model)
    lib.dlevmar_chkjac(C.cast(lib.BRDFFunc_hip, C.c_void_p), C.cast(lib.BRDFJac_hip, C.c_void_p), _dptr(pa), 3, n, C.byref(ed),
                       _dptr(err))
    return err


def last_fit_stats() -> dict:
    a, b, c = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
    us = C.c_double(0.0)
    lib.brdf_hip_last_fit_stats(C.byref(a), C.byref(b), C.byref(c), C.byref(us))
    st = (C.c_longlong * 8)()
    lib.brdf_hip_last_fit_stamps(st)
    # fused_steps: LM steps the resident dlevmar_dif kernel took through DifMachine::fused_trial_step (the mailbox's stamps[0],
    # which carries no time stamp; 0 for every other regime and with BRDF_HIP_DIF_FUSED=0)
    return {"passes": a.value, "jac_passes": b.value, "eval_passes": c.value, "device_us": us.value, "fused_steps": int(st[0]),
            "launches": lib.brdf_hip_last_fit_launches(), "kernel_us": lib.brdf_hip_last_fit_kernel_us()}


def set_launch_timing(on: bool) -> None:
    """resident fits bracket their launch with a HIP event pair on the launch stream; last_fit_stats()["kernel_us"] /
    last_channels_stats()["kernel_us"] then hold the kernel's duration (-1 otherwise)"""
    lib.brdf_hip_set_launch_timing(1 if on else 0)


# ---- rendering a fitted capture: predicted images, residual maps, held-out lights -----------------------------------------------------
def _grey_levels(values: np.ndarray) -> np.ndarray:
    """The grey level of a model value: t = 255.0 * v + 0.5; q = !(t >= 0) ? 0 : (t >= 256.0 ? 255 : (int)t).  A NaN gives 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = 255.0 * np.asarray(values, dtype=np.float64) + 0.5
        q = np.zeros(t.shape, dtype=np.uint8)
        inside = (t >= 0.0) & (t < 256.0)
        q[inside] = t[inside].astype(np.int64)
        q[t >= 256.0] = 255
    return q


def render_capture_host(face_values, pixel_map, background: int, out=None) -> np.ndarray:
    """The host twin of capture_render's images (NumPy, no device): their definition as code.  face_values [nf,3,Lr] float64 (the
    model per face, channel and light), pixel_map [H,W].  Returns uint8 [Lr,H,W,3]: map pixel (y, x) with a face in [0, nf) writes the
    grey level of (face, c, l) to [l, H-1-y, x, c]; any other pixel receives `background` (0 ... 255), or with background = -1 keeps
    what `out` held (zeros without one)."""
    face_values, pixel_map = np.asarray(face_values, dtype=np.float64), np.asarray(pixel_map)
    _require(face_values.ndim == 3 and face_values.shape[1] == 3 and pixel_map.ndim == 2, "face_values [nf,3,Lr], pixel_map [H,W]")
    _require(-1 <= int(background) <= 255, "background: -1 or 0 ... 255")
    nf, _, Lr = face_values.shape
    H, W = pixel_map.shape
    if out is None:
        out = np.zeros((Lr, H, W, 3), dtype=np.uint8)
    _require(out.shape == (Lr, H, W, 3) and out.dtype == np.uint8, "out: uint8 [Lr,H,W,3]")
    grey = _grey_levels(face_values)  # [nf,3,Lr]
    flipped = pixel_map[::-1]         # image row r is map row H - 1 - r
    carried = (flipped > -1) & (flipped < nf)
    if int(background) >= 0:
        out[:, ~carried, :] = int(background)
    out[:, carried, :] = grey[flipped[carried]].transpose(2, 0, 1)  # [pixels,3,Lr] -> [Lr,pixels,3]
    return out


class RenderResidualsHost(NamedTuple):
    """What render_residuals_host returns (NumPy): capture_render_residuals' integer maps."""
    light_count: np.ndarray       # [Lr,3] int64
    light_sum: np.ndarray         # [Lr,3] int64
    light_sumsq: np.ndarray       # [Lr,3] int64
    face_light_count: np.ndarray  # [nf,3,Lr] int32
    face_light_sum: np.ndarray    # [nf,3,Lr] int64
    face_light_sumsq: np.ndarray  # [nf,3,Lr] int64
    abs_max: np.ndarray           # [H,W,3] uint8
    worst_light: np.ndarray       # [H,W,3] uint8


def render_residuals_host(images, pixel_map, face_angles, model: int, face_values, *, v_min: int = 0, v_max: int = 255,
                          cos_min: float = -2.0) -> RenderResidualsHost:
    """The host twin of capture_render_residuals (NumPy, no device): its definition as code.  images [Lr,H,W,3] uint8, pixel_map [H,W],
    face_angles [nf,3,Lr] (the faces' cosine planes under these lights), face_values [nf,3,Lr].  A candidate (carried pixel, light l,
    channel c) is compared iff v_min <= image_l(H-1-y, x)[c] <= v_max and every plane the model reads is > cos_min (a NaN is not);
    d = measured - grey level of (face, c, l).  Sums of 1, d, d^2 per (light, channel) and per (face, channel, light); per pixel, at
    map coordinates, max |d| over the compared lights and the lowest light that attains it (0 and 255 where nothing is compared)."""
    images, pixel_map = np.asarray(images), np.asarray(pixel_map)
    face_angles, face_values = np.asarray(face_angles, dtype=np.float64), np.asarray(face_values, dtype=np.float64)
    _require(images.ndim == 4 and images.shape[3] == 3 and images.dtype == np.uint8 and pixel_map.shape == images.shape[1:3],
             "images [Lr,H,W,3] uint8, pixel_map [H,W]")
    L, H, W = images.shape[:3]
    _require(face_angles.ndim == 3 and face_angles.shape[1:] == (3, L) and face_values.shape == face_angles.shape,
             "face_angles, face_values [nf,3,Lr]")
    _require(model in (MODEL_PHONG, MODEL_BLINN_PHONG, MODEL_WARD), "unknown model")
    nf = face_angles.shape[0]
    ys, xs = np.nonzero((pixel_map > -1) & (pixel_map < nf))
    face = pixel_map[ys, xs].astype(np.int64)
    measured = images[:, H - 1 - ys, xs, :].astype(np.int64).transpose(1, 2, 0)  # [pixels,3,Lr]
    reads = [True, model != MODEL_PHONG, model != MODEL_BLINN_PHONG]  # the planes the model reads
    with np.errstate(invalid="ignore"):
        cos_ok = np.all([face_angles[face, k, :] > cos_min for k in range(3) if reads[k]], axis=0)  # [pixels,Lr]
    compared = cos_ok[:, None, :] & (measured >= v_min) & (measured <= v_max)
    d = np.where(compared, measured - _grey_levels(face_values)[face].astype(np.int64), 0)
    n = compared.astype(np.int64)
    fl = [np.zeros((nf, 3, L), dtype=np.int64) for _ in range(3)]
    for acc, term in zip(fl, (n, d, d * d)):
        np.add.at(acc, face, term)
    mag = np.where(compared, np.abs(d), -1)  # [pixels,3,Lr]
    worst = np.argmax(mag, axis=2)           # the first (lowest) light of the maximum
    top = np.take_along_axis(mag, worst[:, :, None], axis=2)[:, :, 0]
    abs_max, worst_light = np.zeros((H, W, 3), dtype=np.uint8), np.full((H, W, 3), 255, dtype=np.uint8)
    abs_max[ys, xs] = np.where(top >= 0, top, 0)
    worst_light[ys, xs] = np.where(top >= 0, worst, 255)
    return RenderResidualsHost(fl[0].sum(axis=0).T.copy(), fl[1].sum(axis=0).T.copy(), fl[2].sum(axis=0).T.copy(), fl[0].astype(np.int32), fl[1],
                               fl[2], abs_max, worst_light)


def _psnr(count, sumsq):
    """10 log10(255^2 count / sumsq): inf at sumsq = 0, NaN at count = 0"""
    count, sumsq = np.asarray(count, dtype=np.float64), np.asarray(sumsq, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 10.0 * np.log10(65025.0 * count / sumsq)
    out = np.where(sumsq == 0, np.inf, out)
    return np.where(count == 0, np.nan, out)


class CaptureRender(NamedTuple):
    """What capture_render returns (CUDA tensors)."""
    face_values: object  # [nf,3,Lr] float64: the model per face, channel and light; None where not asked for
    rendered: object     # [Lr,H,W,3] uint8 BGR, the captures' layout; None where not asked for


def _render_args(model, pixel_map, vertices, faces, face_normals, leds, view_origin, surfaces, validate):
    import torch
    pixel_map, vertices, faces, face_normals = pixel_map.contiguous(), vertices.contiguous(), faces.contiguous(), face_normals.contiguous()
    _require(pixel_map.is_cuda and vertices.is_cuda and faces.is_cuda and face_normals.is_cuda, "pixel_map, vertices, faces, face_normals: CUDA tensors")
    _require(pixel_map.dtype == torch.int32 and pixel_map.dim() == 2 and faces.dtype == torch.int32, "pixel_map int32 [H,W], faces int32")
    _require(vertices.dtype == torch.float64 and face_normals.dtype == torch.float64, "vertices, face_normals: float64")
    _require(tuple(face_normals.shape) == (faces.shape[0], 3) and vertices.shape[-1] == 3 and faces.shape[-1] == 3, "faces, face_normals [nf,3], vertices [nv,3]")
    if validate:
        _check_indices(faces, vertices.shape[0], "face index outside the vertex array")
    nf, dev = int(faces.shape[0]), pixel_map.device
    la = np.ascontiguousarray(leds, dtype=np.float64).reshape(-1, 3)
    if not torch.is_tensor(surfaces):
        surfaces = torch.from_numpy(np.ascontiguousarray(surfaces, dtype=np.float64)).to(dev)
    surfaces = surfaces.contiguous()
    _require(surfaces.is_cuda and surfaces.device == dev and surfaces.dtype == torch.float64 and tuple(surfaces.shape) == (nf, 3, 3),
             "surfaces: [nf,3,3] float64 on the map's device")
    return pixel_map, vertices, faces, face_normals, la, _f64(view_origin, 3), surfaces, nf, dev


def _out_tensor(t, shape, dtype, dev, what, torch, fill=0):
    if t is None:
        return torch.full(shape, fill, dtype=dtype, device=dev)
    _require(torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous(),
             f"{what}: contiguous CUDA {dtype} {list(shape)} on the capture's device")
    return t


def capture_render(model: int, pixel_map, vertices, faces, face_normals, leds, view_origin, surfaces, *, background: int = 0, rv_mode: int = 0,
                   want_values: bool = True, want_images: bool = True, rendered=None, validate: bool = True) -> CaptureRender:
    """Shade the mesh with fitted parameters (brdf_hip_capture_render_dev): the model at surfaces [nf,3,3] under leds [Lr,3] -- the
    fitted lights, some of them, or new positions, 1 <= Lr <= 64 -- as face_values [nf,3,Lr] (the bytes of model_eval on cosines'
    planes) and as 8-bit BGR images [Lr,H,W,3] in the captures' layout: map pixel (y, x) writes image row H-1-y.  Grey level:
    t = 255.0 * v + 0.5, clamped to 0 ... 255, NaN -> 0 (render_capture_host is the definition as code).  Pixels that carry no face
    receive `background`, or with background = -1 keep what `rendered` (a tensor to write into) held."""
    import torch
    pixel_map, vertices, faces, face_normals, la, va, surfaces, nf, dev = _render_args(model, pixel_map, vertices, faces, face_normals, leds,
                                                                                       view_origin, surfaces, validate)
    H, W, Lr = int(pixel_map.shape[0]), int(pixel_map.shape[1]), int(la.shape[0])
    values = torch.empty((nf, 3, Lr), dtype=torch.float64, device=dev) if want_values else None
    if want_images or rendered is not None:
        rendered = _out_tensor(rendered, (Lr, H, W, 3), torch.uint8, dev, "rendered", torch)
    _call("brdf_hip_capture_render_dev", dev, int(model), H, W, pixel_map.data_ptr(), vertices.data_ptr(), faces.data_ptr(), face_normals.data_ptr(), nf,
          _dptr(la), Lr, _dptr(va), int(rv_mode), surfaces.data_ptr(), int(background), None if values is None else values.data_ptr(),
          None if rendered is None else rendered.data_ptr(), _STREAM)
    return CaptureRender(values, rendered)


class CaptureRenderResiduals(NamedTuple):
    """What capture_render_residuals returns (CUDA tensors and the host scalar): d = measured - rendered grey level over the compared
    candidates."""
    light_count: object       # [Lr,3] int64: the compared candidates per light and channel
    light_sum: object         # [Lr,3] int64: sum d
    light_sumsq: object       # [Lr,3] int64: sum d^2
    face_light_count: object  # [nf,3,Lr] int32
    face_light_sum: object    # [nf,3,Lr] int64
    face_light_sumsq: object  # [nf,3,Lr] int64
    abs_max: object           # [H,W,3] uint8 at map coordinates: max |d| over the pixel's compared lights
    worst_light: object       # [H,W,3] uint8: the lowest light that attains it; 255 where nothing is compared
    face_values: object       # [nf,3,Lr] float64
    n_pixels: int

    def psnr(self):
        """10 log10(255^2 count / sumsq) in dB: (per light and channel [Lr,3], over all lights and channels).  inf at sumsq = 0, NaN at
        count = 0."""
        n, s = self.light_count.cpu().numpy(), self.light_sumsq.cpu().numpy()
        return _psnr(n, s), float(_psnr(n.sum(), s.sum()))


def capture_render_residuals(model: int, images, pixel_map, vertices, faces, face_normals, leds, view_origin, surfaces, *, v_min: int = 0,
                             v_max: int = 255, cos_min: float = -2.0, rv_mode: int = 0, validate: bool = True,
                             out: CaptureRenderResiduals | None = None) -> CaptureRenderResiduals:
    """Where a fit disagrees with images, in grey levels (brdf_hip_capture_render_residuals_dev): images [Lr,H,W,3] taken under leds
    [Lr,3] -- the fitted lights or held-out ones -- against capture_render's grey levels at surfaces [nf,3,3], without an image being
    rendered.  The validity rule as fit_capture_masked (the defaults switch it off; a NaN cosine is never a sample).  Every map is
    integer and written whole; two calls give the same bytes; render_residuals_host is the definition as code.  `out`: an earlier
    result whose tensors are written into."""
    import torch
    args, keep, nf = _capture_args(model, images, pixel_map, vertices, faces, face_normals, leds, view_origin, rv_mode, None, None, None, 0, None,
                                   validate)
    dev = keep[0].device
    Lr, H, W = args[2], args[3], args[4]
    if not torch.is_tensor(surfaces):
        surfaces = torch.from_numpy(np.ascontiguousarray(surfaces, dtype=np.float64)).to(dev)
    surfaces = surfaces.contiguous()
    _require(surfaces.is_cuda and surfaces.device == dev and surfaces.dtype == torch.float64 and tuple(surfaces.shape) == (nf, 3, 3),
             "surfaces: [nf,3,3] float64 on the capture's device")
    o = out if out is not None else CaptureRenderResiduals(*([None] * 9), 0)
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    maps = (_out_tensor(o.light_count, (Lr, 3), i64, dev, "light_count", torch), _out_tensor(o.light_sum, (Lr, 3), i64, dev, "light_sum", torch),
            _out_tensor(o.light_sumsq, (Lr, 3), i64, dev, "light_sumsq", torch),
            _out_tensor(o.face_light_count, (nf, 3, Lr), i32, dev, "face_light_count", torch),
            _out_tensor(o.face_light_sum, (nf, 3, Lr), i64, dev, "face_light_sum", torch),
            _out_tensor(o.face_light_sumsq, (nf, 3, Lr), i64, dev, "face_light_sumsq", torch),
            _out_tensor(o.abs_max, (H, W, 3), u8, dev, "abs_max", torch), _out_tensor(o.worst_light, (H, W, 3), u8, dev, "worst_light", torch, 255),
            _out_tensor(o.face_values, (nf, 3, Lr), torch.float64, dev, "face_values", torch))
    npx = C.c_longlong(0)
    _call("brdf_hip_capture_render_residuals_dev", dev, *args[:13], surfaces.data_ptr(), int(v_min), int(v_max), float(cos_min),
          *(t.data_ptr() for t in maps), C.byref(npx), _STREAM)
    return CaptureRenderResiduals(*maps, npx.value)


def surfaces_from_materials(face_label, materials, fill=(0.0, 0.0, 0.0), *, out=None):
    """surfaces [nf,3,3] = materials[face_label] where the label is inside [0, K), `fill` = {kd, ks, n} in each channel elsewhere
    (brdf_hip_surfaces_from_materials_dev): fit_capture_labelled / fit_capture_materials results -- or, with K = 1 and all labels 0, a
    single BRDF -- as the surfaces capture_render and capture_render_residuals read.  face_label: CUDA int32 [nf]; materials [K,3,3]
    CUDA tensor or NumPy."""
    import torch
    _require(torch.is_tensor(face_label) and face_label.is_cuda and face_label.dtype == torch.int32 and face_label.dim() == 1 and face_label.is_contiguous(),
             "face_label: contiguous CUDA int32 [nf]")
    dev, nf = face_label.device, int(face_label.shape[0])
    materials = _materials_tensor(materials, dev, torch)
    surfaces = _out_tensor(out, (nf, 3, 3), torch.float64, dev, "out", torch)
    _call("brdf_hip_surfaces_from_materials_dev", dev, face_label.data_ptr(), nf, materials.data_ptr(), int(materials.shape[0]), _dptr(_f64(fill, 3)),
          surfaces.data_ptr(), _STREAM)
    return surfaces
