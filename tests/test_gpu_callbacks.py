"""The host-callback path (brdf_amd/csrc/generic_fit.hip) on the GPU against the compiled reference's own dlevmar_* / slevmar_*
on the same callback (tests/callback_problems.py): bit for bit where one lane forms the sums in the reference's order
(n m <= 65536: the small loop, the 32-row blocked loop, the switch between them, partial last blocks, the upper edge), pass by pass
within each case's own tolerance where the 256-lane tree does (n m > 65536), and the two utilities on either side of that limit.

Not judged: p, info[1..4] and covar of the float tree branch -- under permutation of the samples the reference's own slevmar_*
moves by 1e-4 to 2e-2 there, more than a dropped sample; only its info[0] is held (test_float_tree_first_residual_norm)."""
import ctypes as C

import numpy as np
import pytest

from tests import callback_problems as K
from tests import oracle_libs as L

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(L.ref is None, reason="the wide problem's callbacks and the yardstick live in oracle/_ref")]


@pytest.fixture(scope="module")
def lib():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from brdf_amd._lib import lib
    return lib


def _err():
    import brdf_amd
    return brdf_amd.last_error()


# ---- A: reference order, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.exact_cases(), ids=K.case_id)
def test_reference_order_sums_replay_the_reference_bit_for_bit(lib, c):
    want = K.run(L.ref, c)
    got = K.run(lib, c)
    assert K.identical(c, got, want) is None, (K.identical(c, got, want), _err())
    assert want[0] >= 0 or c.itmax == 0


# ---- B: the tree, pass by pass ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", K.SHAPES_B)
def test_tree_sums_pass_by_pass(lib, m, n):
    """itmax = 1, 2, 3: all four entries forward, dif and bc_dif central, bc_dif and bc_der with dscl"""
    tally = K.Tally(f"tree ({m}, {n})")
    for c in K.tree_cases(m, n):
        tally.add(c, K.run(lib, c))
    tally.check()


@pytest.mark.parametrize("c", K.converged_cases(), ids=K.case_id)
def test_tree_fits_run_to_convergence(lib, c):
    """der in full; dif, bc_dif, bc_der: ret >= 0, p and info[1] (the reference's own iteration counts move under permutation)"""
    y = K.yardstick(c)
    assert y.tol["p"] <= K.CAP_CONVERGED_P and y.tol["info1"] <= K.CAP_P and (c.entry != "der" or (y.stable and y.tol["covar"] <= K.CAP_COVAR)), y.tol
    got = K.run(lib, c)
    print(K.describe(c), "got", got[2].tolist(), "reference", y.info.tolist())
    assert K.compare_converged(c, got) is None, (K.compare_converged(c, got), _err())


@pytest.mark.parametrize("c", K.float_tree_cases(), ids=K.case_id)
def test_float_tree_first_residual_norm(lib, c):
    """the one field of the float tree branch that is judged: info[0] = ||x - f(p0)||^2 against a float64 sum over the float
    callback's values, within 8 x the float reference's own spread under permutation.  p, info[1..4] and covar are not judged."""
    want, tol = K.float_tree_info0(c)
    got = K.run(lib, c)
    print(K.describe(c), "info[0]", got[2][0], "float64 sum", want, "difference", abs(got[2][0] - want) / want, "tolerance", tol)
    assert got[0] >= 0, _err()
    assert abs(float(got[2][0]) - want) <= tol * want


# ---- C: the utilities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", ["d", "s"])
def test_r2_on_either_side_of_the_limit(lib, real):
    """n = 65536: the reference's descending loops by one lane, equal to the reference's own value; n = 65537: the tree, within
    1e-12 of float64 numpy, the bar of test_r2_through_the_product_abi (float: 64 * 2^-24, the floor of the double yardstick in float
    units and 4 x sqrt(265) units, the random-walk size of the rounding of a 257-term lane sum and eight tree levels in each of two
    sums; the reference's own sequential float sums are 280 units off there); x == NULL: the value of the reference's x == 0 branch
    (taken from the reference on a vector of zeros: with NULL itself the reference reads x before it tests it, misc_core.c:634-638)"""
    assert K.r2(lib, 65536, real) == K.r2(L.ref, 65536, real)
    x, p0 = K.problem(3, 65537, real)[:2]
    x, hx = x.astype(np.float64), K.values(real, p0, 65537).astype(np.float64)
    want = 1.0 - np.sum((x - hx) ** 2) / np.sum((x - x.mean()) ** 2)
    got = K.r2(lib, 65537, real)
    print(real, "R2", got, "numpy", want)
    if real == "d":
        assert abs(got - want) <= 1e-12 * abs(want)
    else:
        assert abs(got - want) <= 64 * 2.0 ** -24 * abs(want)
    assert K.r2(lib, 100, real, null_x=True) == K.r2(L.ref, 100, real, zero_x=True) == -np.inf
    assert K.r2(lib, 100, real, zero_x=True) == -np.inf


@pytest.mark.parametrize("n", [1000, 70001])
def test_chkjac_on_a_host_callback(lib, n):
    """dlevmar_chkjac's row kernel (more than one block, a short last one; n beyond 65536) against the reference's, on the bar of
    the BRDF check in tests/test_gpu_parity.py: err is a log10 of rounding noise, so the vectors agree in what they say, within 0.1"""
    err, err_ref = K.chkjac(lib, 5, n), K.chkjac(L.ref, 5, n)
    assert err_ref.min() > 0.5 and err.min() > 0.5 and np.max(np.abs(err - err_ref)) <= 0.1
    jf = K.scaled_column_jac(1, 1.01)  # column 1 one per cent off: both sides flag the same rows
    bad, bad_ref = K.chkjac(lib, 5, n, C.cast(jf, C.c_void_p)), K.chkjac(L.ref, 5, n, C.cast(jf, C.c_void_p))
    assert np.array_equal(bad < 0.5, bad_ref < 0.5) and np.count_nonzero(bad_ref < 0.5) > n // 2
    assert np.max(np.abs(bad - bad_ref)) <= 0.1
