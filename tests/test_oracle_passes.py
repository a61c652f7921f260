"""Per-pass parity without a GPU (tests/pass_problems.py): the case tables meet their conditions with the oracle alone; the
oracle equals the compiled reference bit for bit at these itmax / opts; and the product's LM machines, driven on the host
(tests/cpp/host_machine.cpp: "hm" with the reference's model expression, "hm_fast" with the prepared-sample path), pass the very
comparison tests/test_gpu_passes.py makes on the device -- itmax = 0 and the cases of every GPU regime included."""
import collections

import numpy as np
import pytest

from brdf_amd import synth
from tests import oracle_libs as L
from tests import pass_problems as P


def _fit(which, case):
    angles, x, p0, _, _ = P.problem(case.problem)
    lb, ub = P.box(case)
    return L.brdf_fit(which, case.method, case.problem[1], angles, x, p0, case.itmax, case.opts, lb, ub)


def _fit_covar(which, case):
    angles, x, p0, _, _ = P.problem(case.problem)
    lb, ub = P.box(case)
    return L.brdf_fit_covar(which, case.method, case.problem[1], angles, x, p0, case.itmax, case.opts, lb, ub, P.scaling(case))


def _conditions(name, rows):
    """the 10 % / no-empty-cell conditions of `rows` with the reference alone, for ret / p / info and for the covariance;
    -> (compared, uncompared, largest tolerance per field)"""
    cells, covar_cells = collections.defaultdict(lambda: [0, 0]), collections.defaultdict(lambda: [0, 0])
    worst = {f: 0.0 for f in P.FIELDS + ("covar",)}
    for cell, case in rows:
        y = P.yardstick(case)
        ok = P.admitted(case)
        cells[cell][0 if ok else 1] += 1
        covar_cells[cell][0 if P.covar_judged(case) else 1] += 1
        if ok and case.itmax > 0:  # (a converged case: only p and info[1] are judged, p against CAP_INFO)
            for f in ("p", "info1") if P.converged(case) else P.FIELDS:
                worst[f] = max(worst[f], y.tol[f])
        if y.covar_rule == "compare":
            worst["covar"] = max(worst["covar"], y.tol["covar"])
    comp, unc = sum(c[0] for c in cells.values()), sum(c[1] for c in cells.values())
    cj, cl = sum(c[0] for c in covar_cells.values()), sum(c[1] for c in covar_cells.values())
    print(f"{name}: {comp} compared, {unc} uncompared ({100.0 * unc / (comp + unc):.1f} %); covar: {cj} judged, {cl} left out "
          f"({100.0 * cl / (cj + cl):.1f} %); largest tolerance: " + ", ".join(f"{f} {v:.2g}" for f, v in worst.items()))
    assert unc <= P.MAX_UNCOMPARED * (comp + unc), (name, comp, unc)
    assert all(c[0] > 0 for c in cells.values()), (name, dict(cells))
    assert cl <= P.MAX_UNCOMPARED * (cj + cl), (name, "covar", cj, cl)
    assert all(c[0] > 0 for c in covar_cells.values()), (name, "covar", dict(covar_cells))
    cap_p = P.CAP_INFO if all(P.converged(c) for _, c in rows) else P.CAP_P
    assert worst["p"] <= cap_p and all(worst[f] <= P.CAP_P for f in ("info0", "info1")) and all(worst[f] <= P.CAP_INFO for f in ("info2", "info3", "info4", "covar"))
    return comp, unc, worst


@pytest.mark.parametrize("table", list(P.tables()))
def test_tables_meet_their_conditions(table):
    comp, unc, _ = _conditions(table, P.tables()[table])
    assert comp + unc >= 12


def test_stop_rule_table_holds_every_reason_and_start_point_stops():
    cases = [c for _, c in P.tables()["stop rules"]]
    reasons = collections.Counter(int(P.yardstick(c).info[6]) for c in cases)
    assert reasons[1] >= 10 and reasons[2] >= 10 and reasons[6] >= 10, reasons
    assert all(P.yardstick(c).info[5] <= P.MAX_STOP_ITERATIONS for c in cases)
    at_start = P.start_point_stops(cases)
    assert at_start[1] and at_start[6], dict(at_start)
    y = P.yardstick(at_start[1][0])
    assert y.info[8] == 1 and y.comparable  # reason 1 at iteration 0: one Jacobian, no step
    y = P.yardstick(at_start[6][0])
    assert y.info[7] == 1 and y.info[8] == 0 and y.comparable  # reason 6 at iteration 0: one evaluation, no Jacobian


def test_gpu_case_lists_meet_their_conditions():
    """every list tests/test_gpu_passes.py compares, before any GPU run"""
    for regime, sizes in P.SINGLE_REGIMES.items():
        if regime != "short_last_workgroup":  # (n = 262145: eight cases, judged on the GPU machine)
            _conditions(f"single fits, {regime}", [r for n in sizes for r in P.single_cases(n)])
    _conditions("switches", P.switch_cases())
    _conditions("diagonal scaling", P.dscl_cases())
    _conditions("converged fits", P.converged_cases())
    zeros = [c for _, c in P.zero_covar_cases()]
    assert all(P.yardstick(c).covar_rule == "zeros" for c in zeros) and sum(c.itmax == 0 for c in zeros) == 12
    assert sum(c.itmax > 0 and P.yardstick(c).info[8] == 0 for c in zeros) >= 8 and sum(P.yardstick(c).info[8] > 0 for c in zeros) >= 16
    for _, case in P.singular_cases():  # J'J singular exactly: the oracle says so and its NaN fill survives, with and without noise
        y = P.yardstick(case)
        assert y.comparable and y.covar_rule == "zeros" and y.info[8] == 1 and np.all(np.isnan(y.covar)), (P.describe(case), y)
        assert np.all(np.isnan(_fit_covar("orc", case)[3]))
    _conditions("channels", [(P.METHOD[method], c) for model in P.CHANNEL_TRUTHS for method in range(4)
                             for row in P.channel_cases(model, method) for c in row])
    for model in P.CHANNEL_TRUTHS:
        for method in range(4):
            rows = P.channel_cases(model, method)
            if method in (1, 2):  # the shared launch: one of each stop reason, at different iterations, one at the start point
                ends = [(int(P.yardstick(c).info[5]), int(P.yardstick(c).info[6])) for c in rows[0]]
                assert ends[0] == (0, 6) and ends[1][1] == 1 and ends[2][1] == 2 and len({e[0] for e in ends}) == 3, ends
    for kernel, (_, sizes, methods) in P.BATCH_KERNELS.items():
        rows = P.batch_rows(kernel)
        _conditions(f"batch kernel {kernel}", rows)  # (a test's cases: every size and setting of the kernel)
        for n in sizes:  # every batch with a cap holds fits that are over at the start among fits that are not; for every method, a
            itmax, opts = P.batch_settings(n)[0]  # batch mixes fits over at the start, fits that stop early and fits that reach the cap
            for m in methods:
                mixed = 0
                for model in (0, 1, 2):
                    its = {int(P.yardstick(P.Case(key, m, itmax, opts)).info[5]) for key in P.batch_items(model, n)}
                    assert 0 in its and len(its) >= 2, (kernel, n, model, m, its)
                    mixed += int(0 in its and itmax in its and any(0 < k < itmax for k in its))
                assert mixed >= 1, (kernel, n, m)


@pytest.mark.skipif(L.ref is None, reason="the reference's levmar lives in oracle/_ref")
def test_oracle_equals_the_compiled_reference_at_these_settings():
    """the restatement is pinned at the default settings elsewhere; here at itmax 0..3, opts = NULL, tau, delta (central differences
    included) and the loosened stop rules: ret, p and info[] bit for bit (info[2], info[4] where the reference defines them)"""
    sample = []
    for table, rows in P.tables().items():
        sample += [c for _, c in rows][::5 if table != "itmax = 0" else 1]
    sample += [c for n in (64, 5000) for _, c in P.single_cases(n)][::7]
    assert len(sample) >= 200
    for case in sample:
        a, b = _fit("orc", case), _fit("ref", case)
        ia, ib = a[2].copy(), b[2].copy()
        if ib[8] == 0:
            ia[[2, 4]] = ib[[2, 4]] = 0.0
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(ia, ib, equal_nan=True), (P.describe(case), a, b)


@pytest.mark.parametrize("which", ["hm", "hm_fast"])
def test_host_driven_machines_pass_the_gpu_comparison(which):
    """the product's DifMachine / BcMachine / DerMachine with reference-order sums, covariance and dscl included.  hm: the oracle's
    expressions, so without dscl it must equal the oracle bit for bit wherever the reference defines the result (and return nine
    zeros where the reference writes no covariance); hm_fast, and hm with dscl: within the case's tolerance"""
    rows = [r for rows in P.tables().values() for r in rows]
    rows += [r for n in (64, 1000, 4096, 5000) for r in P.single_cases(n)]
    for model in P.CHANNEL_TRUTHS:
        for method in range(4):
            rows += [(P.METHOD[method], c) for row in P.channel_cases(model, method) for c in row]
    for kernel in P.BATCH_KERNELS:
        rows += P.batch_rows(kernel)
    rows += P.dscl_cases() + P.converged_cases() + P.singular_cases()
    rows = list(dict.fromkeys(rows))
    tally = P.Tally(f"host-driven machines, {which}")
    for cell, case in rows:
        got = _fit_covar(which, case)
        tally.add(cell, case, got)
        if which == "hm" and case.itmax > 0 and case.dscl is None:
            y = P.yardstick(case)
            keep = [i for i in range(10) if f"info{i}" not in P.undefined(y.info)]
            assert got[0] == y.ret and np.array_equal(got[1], y.p) and np.array_equal(got[2][keep], y.info[keep], equal_nan=True), (P.describe(case), got, y)
            if y.covar_rule == "zeros":  # (nothing defined in the reference: nine zeros here)
                assert got[3].tobytes() == np.zeros((3, 3)).tobytes(), (P.describe(case), got[3])
            else:  # (a J'J that is singular to round-off alone gives inf / NaN on both sides)
                assert np.array_equal(got[3], y.covar, equal_nan=True), (P.describe(case), got[3], y.covar)
    tally.check()


def test_speculation_does_not_show_in_the_host_machines():
    """BcMachine's multi-candidate projected-gradient search and speculative Jacobian passes, DifMachine's chained trials: the
    results of fits that end early -- counters included -- are those of one evaluation at a time, byte for byte"""
    cases = [c for _, c in P.switch_cases()]
    try:
        plain = [_fit("hm", c) for c in cases]
        for setter, value in ((L.hm.hm_set_bc_multi, 8), (L.hm.hm_set_dif_multi, 8), (L.hm.hm_set_bc_spec_jac, 1)):
            setter(value)
            for c, a in zip(cases, plain):
                b = _fit("hm", c)
                assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), (setter.__name__, P.describe(c), a, b)
            setter(1 if value == 8 else 0)
    finally:
        L.hm.hm_set_bc_multi(1)
        L.hm.hm_set_dif_multi(1)
        L.hm.hm_set_bc_spec_jac(0)
