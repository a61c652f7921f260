"""Sigma-clipped packed batches (brdf_hip_fit_batch_packed_clipped_dev) on the device.

The first five tests use the SHAPE BATCH: 48 fits cut from tests.weighted_yardstick.quantised_surfels(model, 48, n=4100) to 0 samples
(first, two next to each other in the middle, and last in the batch), 1, 2, 3, 4, 5, 16, 17, 64, 65, 255, 256, 257 and 300 samples
(three of each), 40 and 100, one fit of 1024, one of 1025 and one of 4097 samples (class 5, which runs where it lies); offsets[0] = 5; outliers planted as in the
prototype (x += 0.25, capped at 1, re-quantised): every sample of a fit of 16 and more with probability 0.06, one sample below that.

  (1) rounds = 0 and kappa = inf: the bytes of fit_batch_packed + fit_stats_batch_packed, a mask of ones, kept = k, rounds_used = 0
  (2) the replay at kappa = 2.5 and 0.5: fit_batch_packed / fit_stats_batch_packed on the device alternate with brdf_amd.clip_samples on
      the host, the survivors repacked -- every output of the entry has the replay's bytes.  A fit whose twin finds a sample with
      | |e| - kappa sigma | < 1e-9 sigma is left out; at most 2 % of the fits may be
  (3) one call, two halves, a workspace of several chunks per class, a second call: the same bytes
  (4) the invariant: fit_stats_batch_packed on the masked samples at the returned p gives the returned statistics' bytes
  (5) the host-pointer entry: the device entry's bytes
  (6) against the reference: the clip loop around the compiled reference's dlevmar_bc_dif on the CPU, and once more with every model
      value moved by +-1 ulp; the entry agrees with the reference on all but two of the masks and parameters the reference agrees
      with its own perturbed twin on
  (7) recovery of the surfel's truth: the entry's share of fits within 5 % is the reference loop's minus two fits at most"""
import ctypes as C
import functools

import numpy as np
import pytest

from brdf_amd import synth
from tests import oracle_libs as L
from tests import stats_yardstick as Y
from tests import weighted_yardstick as WY

pytestmark = pytest.mark.gpu
METHOD = 1  # dlevmar_bc_dif
SIGMA_MIN = 1.0 / (255.0 * np.sqrt(12.0))
ROUNDS = 3
_BASE = (1, 2, 3, 4, 5, 16, 17, 64, 65, 255, 256, 257, 300)
SIZES = (0,) + _BASE + (40, 1024) + _BASE[:6] + (0, 0) + _BASE[6:] + (100, 1025) + _BASE + (4097, 0)
PAD = 5  # offsets[0]
OUTPUTS = ("p", "info", "ret", "covar", "stats", "rank", "kept", "rounds_used", "mask")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def plant_outliers(x, rng, all_from=16):
    """the prototype's outliers on x [k]: x += 0.25, capped at 1, re-quantised; -> (x, planted [k] bool)"""
    k = x.size
    planted = rng.random(k) < 0.06 if k >= all_from else np.arange(k) == (rng.integers(k) if k else 0)
    x = np.where(planted, np.round(np.minimum(x + 0.25, 1.0) * 255.0) / 255.0, x)
    return x, planted


@functools.lru_cache(maxsize=None)
def shape_batch(model):
    assert len(SIZES) == 48 and SIZES[0] == SIZES[-1] == SIZES[22] == SIZES[23] == 0
    angles, x = WY.quantised_surfels(model, len(SIZES), n=4100)
    rng = np.random.default_rng(700 + model)
    pa, px, offsets = [np.full(3 * PAD, np.nan)], [np.full(PAD, np.nan)], [PAD]
    for s, k in enumerate(SIZES):
        xs, _ = plant_outliers(x[s, :k], rng)
        pa.append(angles[s, :, :k].reshape(-1))
        px.append(xs)
        offsets.append(offsets[-1] + k)
    return np.concatenate(pa), np.concatenate(px), np.array(offsets, dtype=np.int64)


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _p0(gpu, model, S):
    return _dev(gpu, np.tile(np.array(synth.P0[model]), (S, 1)))


def _fit_kw(model):
    lb, ub = synth.bounds(model)
    return dict(lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)


def _clipped(gpu, model, a, x, off, kappa, rounds=ROUNDS, sigma_min=SIGMA_MIN, p0=None, **kw):
    torch, brdf_amd, _ = gpu
    S = len(off) - 1
    r = brdf_amd.fit_batch_packed_clipped(METHOD, model, _dev(gpu, a), _dev(gpu, x), _dev(gpu, off), _p0(gpu, model, S) if p0 is None else _dev(gpu, p0),
                                          kappa=kappa, sigma_min=sigma_min, rounds=rounds, **_fit_kw(model), **kw)
    torch.cuda.synchronize()
    return dict(p=r.p.cpu().numpy(), info=r.info.cpu().numpy(), ret=r.ret.cpu().numpy(), covar=r.stats.covar.cpu().numpy(),
                stats=r.stats.stats.cpu().numpy(), rank=r.stats.rank.cpu().numpy(), kept=r.kept.cpu().numpy(), rounds_used=r.rounds_used.cpu().numpy(),
                mask=r.mask.cpu().numpy())


def _packed_fit(gpu, model, a, x, off, p):
    torch, brdf_amd, _ = gpu
    p, info, ret = brdf_amd.fit_batch_packed(METHOD, model, _dev(gpu, a), _dev(gpu, x), _dev(gpu, off), _dev(gpu, p), **_fit_kw(model))
    torch.cuda.synchronize()
    return p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()


def _packed_stats(gpu, model, a, x, off, p):
    torch, brdf_amd, _ = gpu
    st = brdf_amd.fit_stats_batch_packed(METHOD, model, _dev(gpu, a), _dev(gpu, x), _dev(gpu, off), _dev(gpu, p), opts=synth.OPTS)
    torch.cuda.synchronize()
    return st.covar.cpu().numpy(), st.stats.cpu().numpy(), st.rank.cpu().numpy()


def _repack(a, x, off, keep):
    """the survivors of a packed batch (keep by position off[s] - off[0] + i), in their order: a batch with offsets[0] = 0"""
    pa, px, no = [], [], [0]
    for s in range(len(off) - 1):
        o, k = off[s], off[s + 1] - off[s]
        m = keep[o - off[0]:o - off[0] + k]
        pa.append(a[3 * o:3 * o + 3 * k].reshape(3, k)[:, m].reshape(-1))
        px.append(x[o:o + k][m])
        no.append(no[-1] + int(m.sum()))
    return np.concatenate(pa) if pa else np.zeros(0), np.concatenate(px) if px else np.zeros(0), np.array(no, dtype=np.int64)


def _same(got, want, names=OUTPUTS, rows=None, label=""):
    for name in names:
        g, w = got[name], want[name]
        if rows is not None and name != "mask":
            g, w = g[rows], w[rows]
        assert g.dtype == w.dtype and g.shape == w.shape and np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (label, name)


# ---- (1) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2])
def test_no_rounds_and_an_infinite_kappa_are_the_packed_calls(gpu, model):
    a, x, off = shape_batch(model)
    S, k = len(off) - 1, np.diff(off)
    p, info, ret = _packed_fit(gpu, model, a, x, off, np.tile(np.array(synth.P0[model]), (S, 1)))
    covar, stats, rank = _packed_stats(gpu, model, a, x, off, p)
    want = dict(p=p, info=info, ret=ret, covar=covar, stats=stats, rank=rank, kept=k.astype(np.int32), rounds_used=np.zeros(S, dtype=np.int32),
                mask=np.ones(off[-1] - off[0], dtype=np.uint8))
    assert (ret[k >= 3] >= 0).any() and np.all(ret[k < 3] == -1)
    _same(_clipped(gpu, model, a, x, off, kappa=2.5, rounds=0), want, label="rounds = 0")
    _same(_clipped(gpu, model, a, x, off, kappa=np.inf, rounds=3), want, label="kappa = inf")


# ---- (2) -------------------------------------------------------------------------------------------------------------------------
def replay(gpu, model, a, x, off, kappa, sigma_min=SIGMA_MIN, rounds=ROUNDS):
    """the definition, round by round: the packed calls on the device, brdf_amd.clip_samples on the host.  -> (the outputs, the fits
    a sample of which the twin found within 1e-9 sigma of its threshold)"""
    _, brdf_amd, _ = gpu
    S = len(off) - 1
    p, info, ret = _packed_fit(gpu, model, a, x, off, np.tile(np.array(synth.P0[model]), (S, 1)))
    mask = np.ones(off[-1] - off[0], dtype=bool)
    settled, used, near = np.zeros(S, dtype=bool), np.zeros(S, dtype=np.int32), np.zeros(S, dtype=bool)
    ca, cx, co = a, x, off
    for r in range(1, rounds + 1):
        _, stats, _ = _packed_stats(gpu, model, ca, cx, co, p)
        keep, done = brdf_amd.clip_samples(model, ca, cx, co, p, stats[:, 0], ret, kappa=kappa, sigma_min=sigma_min)
        for s in range(S):
            o, k = co[s] - co[0], co[s + 1] - co[s]
            if settled[s]:  # settled in an earlier round: not looked at again
                keep[o:o + k] = True
                continue
            if ret[s] >= 0 and k >= 3 and np.isfinite(stats[s, 0]):
                sigma = max(np.sqrt(stats[s, 0] / (k - 3)), sigma_min) if k > 3 else sigma_min
                pl = ca[3 * co[s]:3 * co[s] + 3 * k].reshape(3, k)
                e = np.abs(cx[co[s]:co[s] + k] - synth.model_value(model, p[s], pl[0], pl[1], pl[2]))
                near[s] |= bool((np.abs(e - kappa * sigma) < 1e-9 * sigma).any())
            settled[s] = done[s]
        active = ~settled
        if not active.any():
            break
        mask[mask] = keep  # the current samples are the mask's ones, in order
        ca, cx, co = _repack(ca, cx, co, keep)
        p2, info2, ret2 = _packed_fit(gpu, model, ca, cx, co, p)
        p[active], info[active], ret[active], used[active] = p2[active], info2[active], ret2[active], r
    covar, stats, rank = _packed_stats(gpu, model, ca, cx, co, p)
    return dict(p=p, info=info, ret=ret, covar=covar, stats=stats, rank=rank, kept=np.diff(co).astype(np.int32), rounds_used=used,
                mask=mask.astype(np.uint8)), near


@pytest.mark.parametrize("kappa", [2.5, 0.5])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_replay_of_the_definition(gpu, model, kappa):
    a, x, off = shape_batch(model)
    S, k = len(off) - 1, np.diff(off)
    want, near = replay(gpu, model, a, x, off, kappa)
    got = _clipped(gpu, model, a, x, off, kappa=kappa)
    print(f"model {model} kappa {kappa}: kept {int(want['kept'].sum())} of {int(k.sum())} samples, rounds_used {np.bincount(want['rounds_used'], minlength=4)}, "
          f"left out {int(near.sum())} of {S} fits")
    assert near.sum() <= 0.02 * S, np.flatnonzero(near)  # the cap: change the fixture, not the cap
    rows = np.flatnonzero(~near)
    _same(got, want, rows=rows, label=f"kappa {kappa}")
    pos_ok = np.repeat(~near, k)  # the mask, fit by fit
    assert np.array_equal(got["mask"][pos_ok], want["mask"][pos_ok])
    assert (want["rounds_used"] > 0).sum() >= 10 and np.all(want["kept"] <= k) and np.all(want["kept"][k < 3] == k[k < 3])
    assert np.all(want["kept"][k >= 3] >= 3)
    if kappa == 0.5:  # heavy clipping, and the guard: some fit would have kept fewer than 3 samples and keeps all its current ones
        assert want["kept"].sum() < 0.8 * k.sum()
        assert (want["kept"][(k >= 3) & (k <= 5)] == k[(k >= 3) & (k <= 5)]).any()
    # the per-round record of the call
    _, brdf_amd, _ = gpu
    rec = brdf_amd.last_clip_stats()
    assert 1 <= len(rec) <= ROUNDS and rec[0]["active"] == int((got["rounds_used"] >= 1).sum())
    assert sum(r["clipped"] for r in rec) == int(k.sum() - got["kept"].sum())


# ---- (3) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2])
def test_halves_chunks_and_a_second_call_give_the_same_bytes(gpu, model):
    _, brdf_amd, _ = gpu
    a, x, off = shape_batch(model)
    S = len(off) - 1
    whole = _clipped(gpu, model, a, x, off, kappa=2.5)
    _same(_clipped(gpu, model, a, x, off, kappa=2.5), whole, label="second call")
    small = _clipped(gpu, model, a, x, off, kappa=2.5, workspace_bytes=3000)
    chunks = brdf_amd.last_packed_stats()
    assert sum(c["chunks"] > 1 for c in chunks[:5]) >= 3, chunks
    _same(small, whole, label="chunks")
    h = S // 2
    first, second = _clipped(gpu, model, a, x, off[:h + 1], kappa=2.5), _clipped(gpu, model, a, x, off[h:], kappa=2.5)
    for name in OUTPUTS:
        joined = np.concatenate([first[name], second[name]])
        assert joined.tobytes() == whole[name].tobytes(), name


# ---- (4) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2])
def test_returned_statistics_are_those_of_the_returned_sample_set(gpu, model):
    a, x, off = shape_batch(model)
    k = np.diff(off)
    got = _clipped(gpu, model, a, x, off, kappa=2.5)
    ma, mx, mo = _repack(a, x, off, got["mask"].astype(bool))
    assert np.array_equal(np.diff(mo), got["kept"]) and (got["kept"] < k).sum() >= 10
    covar, stats, rank = _packed_stats(gpu, model, ma, mx, mo, got["p"])
    assert covar.tobytes() == got["covar"].tobytes() and stats.tobytes() == got["stats"].tobytes() and rank.tobytes() == got["rank"].tobytes()


# ---- (5) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2])
def test_host_pointer_entry_has_the_device_entrys_bytes(gpu, model):
    from brdf_amd._lib import D, I, lib
    a, x, off = shape_batch(model)
    S, total = len(off) - 1, int(off[-1] - off[0])
    want = _clipped(gpu, model, a, x, off, kappa=2.5)
    lb, ub = (np.array(v, dtype=np.float64) for v in synth.bounds(model))
    opts = np.array(synth.OPTS)
    got = dict(p=np.tile(np.array(synth.P0[model]), (S, 1)), info=np.zeros((S, 10)), ret=np.zeros(S, dtype=np.int32), covar=np.zeros((S, 3, 3)),
               stats=np.zeros((S, 8)), rank=np.zeros(S, dtype=np.int32), kept=np.zeros(S, dtype=np.int32), rounds_used=np.zeros(S, dtype=np.int32),
               mask=np.zeros(total, dtype=np.uint8))
    d = lambda v: v.ctypes.data_as(D)  # noqa: E731
    i = lambda v: v.ctypes.data_as(I)  # noqa: E731
    rc = lib.brdf_hip_fit_batch_packed_clipped(METHOD, model, d(a), d(x), off.ctypes.data_as(C.POINTER(C.c_longlong)), S, d(got["p"]), d(lb), d(ub),
                                               synth.ITMAX, d(opts), 2.5, SIGMA_MIN, ROUNDS, d(got["info"]), i(got["ret"]), d(got["covar"]),
                                               d(got["stats"]), i(got["rank"]), i(got["kept"]), i(got["rounds_used"]),
                                               got["mask"].ctypes.data_as(C.POINTER(C.c_ubyte)), 0)
    assert rc == int((want["ret"] < 0).sum()) > 0  # the refused fits
    _same(got, want, label="host entry")


# ---- (6), (7) --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prototype_fixture(model, n):
    """64 fits of n samples of quantised_surfels, first = 4000, with the prototype's outliers; -> (angles [64,3,n], x [64,n], planted)"""
    angles, x = WY.quantised_surfels(model, 64, first=4000, n=n)
    rng = np.random.default_rng(900 + 10 * model + (n == 40))
    planted = np.zeros(x.shape, dtype=bool)
    x = x.copy()
    for s in range(64):
        x[s], planted[s] = plant_outliers(x[s], rng, all_from=0)
    return angles, x, planted


def _reference_fit(model, angles, x, p0, sign):
    """dlevmar_bc_dif of the compiled reference (oracle/_ref where it was built, the oracle's restatement otherwise) on the samples
    given; sign [n] or None: every model value moved by sign ulp"""
    a, xx = L.f64(angles), L.f64(x)
    n = xx.size
    ed = Y._Extra(L.ptr(a), model)

    def func(p, hx, m, nn, adata):
        L.orc.orc_brdf_func(p, hx, m, nn, C.c_void_p(adata))
        if sign is not None:
            out = np.ctypeslib.as_array(hx, shape=(nn,))
            out[:] = np.nextafter(out, sign * np.inf)

    cb = WY._FUNC(func)
    lb, ub = synth.bounds(model)
    p, info = L.f64(p0).copy(), np.zeros(10)
    r = WY._BC_DIF(cb, L.ptr(p), L.ptr(xx), 3, n, L.ptr(L.f64(lb)), L.ptr(L.f64(ub)), None, synth.ITMAX, L.ptr(L.f64(synth.OPTS)), L.ptr(info), None,
                   None, C.byref(ed))
    return int(r), p


@functools.lru_cache(maxsize=None)
def reference_loop(model, n, seed, kappa=2.5):
    """the clip loop of the definition around the reference's fit, fit by fit; seed: None, or the seed of the +-1 ulp perturbation
    of every model value.  -> (final masks [64,n], p [64,3], p after round 0 [64,3])"""
    angles, x, _ = prototype_fixture(model, n)
    masks, ps, p_first = np.ones(x.shape, dtype=bool), np.zeros((64, 3)), np.zeros((64, 3))
    rng = np.random.default_rng(seed) if seed is not None else None
    for s in range(64):
        sign = None if rng is None else np.where(rng.random(n) < 0.5, -1.0, 1.0)
        idx = np.arange(n)
        ret, p = _reference_fit(model, angles[s], x[s], synth.P0[model], sign)
        p_first[s] = p
        for _ in range(ROUNDS):
            if ret < 0:
                break
            f = L.model_values(model, angles[s][:, idx], p)
            if sign is not None:
                f = np.nextafter(f, sign[idx] * np.inf)
            e = x[s, idx] - f
            k = idx.size
            sumsq = float(e @ e)
            if not np.isfinite(sumsq):
                break
            sigma = max(np.sqrt(sumsq / (k - 3)), SIGMA_MIN) if k > 3 else SIGMA_MIN
            ok = np.abs(e) <= kappa * sigma
            if ok.all() or ok.sum() < 3:
                break
            idx = idx[ok]
            ret, p = _reference_fit(model, np.ascontiguousarray(angles[s][:, idx]), x[s, idx], p, None if sign is None else sign[idx])
        masks[s] = np.isin(np.arange(n), idx)
        ps[s] = p
    return masks, ps, p_first


def _device_loop(gpu, model, n):
    angles, x, _ = prototype_fixture(model, n)
    a, xx, off = (np.ascontiguousarray(angles.reshape(-1)), np.ascontiguousarray(x.reshape(-1)), np.arange(65, dtype=np.int64) * n)
    got = _clipped(gpu, model, a, xx, off, kappa=2.5)
    return got["mask"].reshape(64, n).astype(bool), got["p"]


def _agreement(masks_a, p_a, masks_b, p_b):
    same = np.all(masks_a == masks_b, axis=1)
    return int(same.sum()), int(sum(L.rel_err(p_a[s], p_b[s]) <= 1e-5 for s in np.flatnonzero(same)))


@pytest.mark.parametrize("n", [256, 40])
@pytest.mark.parametrize("model", [1, 2])
def test_fit_by_fit_against_the_reference_loop(gpu, model, n):
    """Figures printed by this test on the MI355X (A_mask, A_p of the reference against its perturbed twin; the entry's agreement):
    see DESIGN.md, "Sigma-clipped fits"."""
    m_ref, p_ref, _ = reference_loop(model, n, None)
    m_twin, p_twin, _ = reference_loop(model, n, 12345)
    a_mask, a_p = _agreement(m_ref, p_ref, m_twin, p_twin)
    m_dev, p_dev = _device_loop(gpu, model, n)
    d_mask, d_p = _agreement(m_ref, p_ref, m_dev, p_dev)
    print(f"model {model} n {n}: reference against its +-1 ulp twin A_mask {a_mask} A_p {a_p} of 64; the entry against the reference: masks {d_mask} "
          f"parameters {d_p}")
    assert d_mask >= a_mask - 2 and d_p >= a_p - 2, (a_mask, a_p, d_mask, d_p)


@pytest.mark.parametrize("model", [1, 2])
def test_clipping_recovers_the_truth_as_the_reference_loop_does(gpu, model):
    truth = synth.surfel_truth(model, 4000, 64)
    _, p_ref, p_first = reference_loop(model, 256, None)
    _, p_dev = _device_loop(gpu, model, 256)
    within = lambda p: int(sum(L.rel_err(p[s], truth[s]) <= 0.05 for s in range(64)))  # noqa: E731
    plain, ref, dev = within(p_first), within(p_ref), within(p_dev)
    masks, _, planted = reference_loop(model, 256, None)[0], None, prototype_fixture(model, 256)[2]
    print(f"model {model}: fits within 5 % of the truth: plain reference fit {plain}, reference clip loop {ref}, the entry {dev} of 64; planted outliers "
          f"removed by the reference loop {int((planted & ~masks).sum())} of {int(planted.sum())}")
    assert ref > plain  # guards the fixture, not the library
    assert dev >= ref - 2


# ---- the optional outputs, and offsets the clip rounds refuse --------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 2])
def test_outputs_the_caller_leaves_out_do_not_show(gpu, model):
    """d_ret, d_kept, d_rounds_used and d_stats NULL (the call keeps its own), d_covar without d_stats, no d_info: the outputs that are
    asked for have the full call's bytes"""
    from brdf_amd._lib import D, lib
    torch, brdf_amd, dev = gpu
    a, x, off = shape_batch(model)
    S, total = len(off) - 1, int(off[-1] - off[0])
    want = _clipped(gpu, model, a, x, off, kappa=2.5)
    lb, ub = (np.array(v, dtype=np.float64) for v in synth.bounds(model))
    opts = np.array(synth.OPTS)
    d = lambda v: v.ctypes.data_as(D)  # noqa: E731
    da, dx, do = _dev(gpu, a), _dev(gpu, x), _dev(gpu, off)

    def call(**outs):
        p = _p0(gpu, model, S)
        ptr = lambda name: outs[name].data_ptr() if name in outs else None  # noqa: E731
        with torch.cuda.device(dev):
            rc = lib.brdf_hip_fit_batch_packed_clipped_dev(METHOD, model, da.data_ptr(), dx.data_ptr(), do.data_ptr(), S, p.data_ptr(), d(lb), d(ub),
                                                           synth.ITMAX, d(opts), 2.5, SIGMA_MIN, ROUNDS, ptr("info"), ptr("ret"), ptr("covar"), ptr("stats"),
                                                           ptr("rank"), ptr("kept"), ptr("rounds_used"), ptr("mask"), 0,
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0, brdf_amd.last_error()
        return p.cpu().numpy(), {k: v.cpu().numpy() for k, v in outs.items()}

    p, _ = call()  # nothing but p
    assert p.tobytes() == want["p"].tobytes()
    p, got = call(covar=torch.zeros((S, 3, 3), dtype=torch.float64, device=dev), mask=torch.zeros(total, dtype=torch.uint8, device=dev))
    assert p.tobytes() == want["p"].tobytes() and got["covar"].tobytes() == want["covar"].tobytes() and got["mask"].tobytes() == want["mask"].tobytes()
    p, got = call(info=torch.zeros((S, 10), dtype=torch.float64, device=dev), rank=torch.zeros(S, dtype=torch.int32, device=dev),
                  kept=torch.zeros(S, dtype=torch.int32, device=dev))
    assert p.tobytes() == want["p"].tobytes()
    for name in ("info", "rank", "kept"):
        assert got[name].tobytes() == want[name].tobytes(), name


def test_clip_rounds_refuse_offsets_that_descend(gpu):
    """the packed calls read a descending pair of offsets as a count of 0; the clip rounds give every sample position one fit, so the
    clipped call refuses such a batch before it writes anything -- with rounds = 0 it is the packed calls, which take it"""
    torch, brdf_amd, dev = gpu
    a, x, _ = shape_batch(1)
    off = np.array([5, 15, 5, 15], dtype=np.int64)
    p0 = np.tile(np.array(synth.P0[1]), (3, 1))
    args = (METHOD, 1, _dev(gpu, a), _dev(gpu, x), _dev(gpu, off))
    p = _dev(gpu, p0)
    with pytest.raises(RuntimeError, match="offsets descend.*at fit 1"):
        brdf_amd.fit_batch_packed_clipped(*args, p, kappa=2.5, sigma_min=SIGMA_MIN, rounds=2, validate=False, **_fit_kw(1))
    torch.cuda.synchronize()
    assert p.cpu().numpy().tobytes() == p0.tobytes()
    r = brdf_amd.fit_batch_packed_clipped(*args, _dev(gpu, p0), kappa=2.5, sigma_min=SIGMA_MIN, rounds=0, validate=False, **_fit_kw(1))
    torch.cuda.synchronize()
    assert list(r.kept.cpu().numpy()) == [10, 0, 10] and list(r.ret.cpu().numpy() < 0) == [False, True, False] and r.mask.cpu().numpy().all()
