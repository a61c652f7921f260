"""Per-sample weights in the n <= 16 size class (brdf_hip_fit_batch_weighted_dev, brdf_hip_fit_stats_batch_weighted_dev).

Fit s is levmar on sqrt(w) f against sqrt(w) x.  The yardstick (tests/weighted_yardstick.py) poses exactly that problem to the compiled
reference's dlevmar_bc_dif through a ctypes callback (orc_dlevmar_bc_dif where oracle/_ref is absent); it is computed once per module.

  1. unit weights return the bytes of the unweighted ragged calls (fit and statistics), counts 0 ... 16, cosines of 0.0 included;
  2. fit by fit against the reference, on the bars of test_sixteen_sample_fits_fit_by_fit_against_the_oracle;
  3. refusals (a negative or NaN weight, a count of 2), a weight of 0, nothing behind the count is read;
  4. the batch in one call and in two halves: the same bytes;
  5. the statistics at the reference's p against the reference's dlevmar_covar on J^T W J, with and without extra_ss / nobs."""
import numpy as np
import pytest

from brdf_amd import synth
from tests import stats_yardstick as Y
from tests import weighted_yardstick as WY

pytestmark = pytest.mark.gpu
S_FIT = 768


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _weighted(gpu, method, model, angles, x, w, counts=None, p0=None):
    torch, brdf_amd, _ = gpu
    S = x.shape[0]
    lb, ub = synth.bounds(model)
    p0 = np.tile(np.array(synth.P0[model]), (S, 1)) if p0 is None else p0
    p, info, ret = brdf_amd.fit_batch_weighted(method, model, _dev(gpu, angles), _dev(gpu, x), _dev(gpu, w), _dev(gpu, p0), lb=lb, ub=ub,
                                               itmax=synth.ITMAX, opts=synth.OPTS, counts=None if counts is None else _dev(gpu, counts))
    torch.cuda.synchronize()
    return p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()


def _figures(label, got, ref, S):
    both, close, near, worst = WY.parity_figures(got[2], got[0], got[1], ref[0], ref[1], ref[2])
    print(f"{label}: {both}/{S} converge on both sides, {close}/{both} of them within 1e-5 on p, {near}/{S} objectives within 1e-6, "
          f"worst objective excess {worst:.3e}")
    assert both >= 0.7 * S and close >= 0.97 * both, (label, close, both)
    assert near >= 0.99 * S and worst <= 0.3, (label, near, worst)


@pytest.mark.parametrize("stride", [16, 5])
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_unit_weights_are_the_unweighted_calls_bytes(gpu, model, method, stride):
    torch, brdf_amd, _ = gpu
    S = 200
    angles, x = WY.quantised_surfels(model, S)
    angles, x = np.ascontiguousarray(angles[:, :, :stride]), np.ascontiguousarray(x[:, :stride])
    angles[::7, 0, 1] = 0.0  # a cosine of 0.0: these fits take the exact twin
    counts = (np.arange(S) % (stride + 1)).astype(np.int32)
    lb, ub = synth.bounds(model)
    p0 = np.tile(np.array(synth.P0[model]), (S, 1))
    da, dx, dc = _dev(gpu, angles), _dev(gpu, x), _dev(gpu, counts)
    want = brdf_amd.fit_batch(method, model, da, dx, _dev(gpu, p0), lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS, counts=dc)
    got = brdf_amd.fit_batch_weighted(method, model, da, dx, torch.ones_like(dx), _dev(gpu, p0), lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS,
                                      counts=dc)
    torch.cuda.synchronize()
    for g, w_, name in zip(got, want, ("p", "info", "ret")):
        assert g.cpu().numpy().tobytes() == w_.cpu().numpy().tobytes(), name
    ret = want[2].cpu().numpy()
    assert (ret[counts < 3] == -1).all() and (ret[counts >= 3] >= 0).any()
    st_want = brdf_amd.fit_stats_batch(method, model, da, dx, want[0], opts=synth.OPTS, counts=dc)
    st_got = brdf_amd.fit_stats_batch_weighted(method, model, da, dx, torch.ones_like(dx), want[0], opts=synth.OPTS, counts=dc)
    torch.cuda.synchronize()
    for name in ("covar", "stats", "rank"):
        assert getattr(st_got, name).cpu().numpy().tobytes() == getattr(st_want, name).cpu().numpy().tobytes(), name
    # without counts: the uniform calls
    want_u = brdf_amd.fit_batch(method, model, da, dx, _dev(gpu, p0), lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
    got_u = brdf_amd.fit_batch_weighted(method, model, da, dx, torch.ones_like(dx), _dev(gpu, p0), lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
    st_want_u = brdf_amd.fit_stats_batch(method, model, da, dx, want_u[0], opts=synth.OPTS)
    st_got_u = brdf_amd.fit_stats_batch_weighted(method, model, da, dx, torch.ones_like(dx), want_u[0], opts=synth.OPTS)
    torch.cuda.synchronize()
    for g, w_, name in zip(got_u, want_u, ("p", "info", "ret")):
        assert g.cpu().numpy().tobytes() == w_.cpu().numpy().tobytes(), name
    for name in ("covar", "stats", "rank"):
        assert getattr(st_got_u, name).cpu().numpy().tobytes() == getattr(st_want_u, name).cpu().numpy().tobytes(), name


@pytest.mark.parametrize("model", [0, 1, 2])
def test_weighted_fits_fit_by_fit_against_the_reference(gpu, model):
    """S = 768 fits of 16 8-bit samples with integer weights in [1, 300], dlevmar_bc_dif, synth's options and box.  The bars are
    test_sixteen_sample_fits_fit_by_fit_against_the_oracle's: the sources of difference (the last bit of pow / exp on ill-conditioned
    fits) are the same."""
    angles, x, w, ret_ref, p_ref, info_ref = WY.reference_case(model, S_FIT)
    got = _weighted(gpu, 1, model, angles, x, w)
    _figures(f"weighted n=16 model {model}", got, (ret_ref, p_ref, info_ref), S_FIT)


@pytest.mark.parametrize("model", [0, 1, 2])
def test_batch_composition_does_not_show(gpu, model):
    angles, x, w = WY.reference_case(model, S_FIT)[:3]
    whole = _weighted(gpu, 1, model, angles, x, w)
    h = S_FIT // 2
    a, b = _weighted(gpu, 1, model, angles[:h], x[:h], w[:h]), _weighted(gpu, 1, model, angles[h:], x[h:], w[h:])
    for k in range(3):
        assert whole[k].tobytes() == np.concatenate([a[k], b[k]]).tobytes(), k


def test_refusals_zero_weights_and_padding(gpu):
    model, S = 1, 128
    angles, x, w = (v[:S].copy() for v in WY.reference_case(model, S_FIT)[:3])
    base = _weighted(gpu, 1, model, angles, x, w)
    # a negative weight, a NaN weight, a count of 2: refused as n < m is; the neighbours keep their bytes
    w_bad, counts = w.copy(), np.full(S, 16, dtype=np.int32)
    w_bad[10, 3], w_bad[20, 15], counts[30] = -1.0, np.nan, 2
    w_bad[40, 7] = np.inf
    p0 = np.tile(np.array(synth.P0[model]), (S, 1)) + 0.125 * np.arange(S)[:, None] / S  # (a start of its own per fit: "p untouched" shows)
    base_p0 = _weighted(gpu, 1, model, angles, x, w, p0=p0)
    got = _weighted(gpu, 1, model, angles, x, w_bad, counts=counts, p0=p0)
    refused = np.zeros(S, dtype=bool)
    refused[[10, 20, 30, 40]] = True
    assert (got[2][refused] == -1).all() and not got[1][refused].any() and got[0][refused].tobytes() == p0[refused].tobytes()
    for k in range(3):
        assert got[k][~refused].tobytes() == base_p0[k][~refused].tobytes(), k
    # nothing behind counts[s] is read: NaN there (planes, measurements, weights) changes no byte
    counts = (3 + np.arange(S) % 14).astype(np.int32)
    first = _weighted(gpu, 1, model, angles, x, w, counts=counts)
    behind = np.arange(16)[None, :] >= counts[:, None]
    a2, x2, w2 = angles.copy(), x.copy(), w.copy()
    x2[behind], w2[behind] = np.nan, np.nan
    a2[np.broadcast_to(behind[:, None, :], a2.shape)] = np.nan
    again = _weighted(gpu, 1, model, a2, x2, w2, counts=counts)
    for k in range(3):
        assert again[k].tobytes() == first[k].tobytes(), k
    # ... and the counted fits are the reference's fits of those samples
    _figures("weighted ragged model 1", first, WY.weighted_fits(model, angles, x, w, counts), S)
    # a weight of 0 on one sample: the reference's fit with that weight 0 and n unchanged
    w0 = w.copy()
    w0[np.arange(S), np.arange(S) % 16] = 0.0
    zero = _weighted(gpu, 1, model, angles, x, w0)
    _figures("weighted, one zero weight per fit, model 1", zero, WY.weighted_fits(model, angles, x, w0), S)
    assert zero[0].tobytes() != base[0].tobytes()


@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_weighted_statistics_against_the_reference(gpu, model, method, with_extra):
    torch, brdf_amd, _ = gpu
    S = 256
    angles, x, w, _, p_ref, _ = WY.reference_case(model, S_FIT)
    angles, x, w, p_ref = angles[:S], x[:S], w[:S], p_ref[:S]
    extra = nobs = None
    if with_extra:
        rng = np.random.default_rng(7 + model)
        extra = rng.uniform(0.0, 0.05, size=S)
        nobs = w.sum(axis=1).astype(np.int32)  # the weights as group sizes: every observation counts
    st = brdf_amd.fit_stats_batch_weighted(method, model, _dev(gpu, angles), _dev(gpu, x), _dev(gpu, w), _dev(gpu, p_ref), opts=synth.OPTS,
                                           extra_ss=None if extra is None else _dev(gpu, extra), nobs=None if nobs is None else _dev(gpu, nobs))
    torch.cuda.synchronize()
    kind = Y.jac_kind(method, synth.OPTS)
    WY.compare_weighted_stats(kind, model, angles, x, w, p_ref, st.covar.cpu().numpy(), st.stats.cpu().numpy(), st.rank.cpu().numpy(), nobs=nobs,
                              extra_ss=extra, max_left_out=0.35, label=f"method {method} extra {with_extra}")
