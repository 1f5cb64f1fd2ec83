"""bbg_g1_sum / bbg_g1_sum_device / bbg_g1_normalize (k_g1_sum and k_normalize in csrc/msm.hip) on the MI355X over designed inputs.

k_g1_sum produces the final answer of every sharded MSM (the C binding's g1_sum, bbg_multi_msm, parallel.py), and the rest of the suite
only ever hands it 2 to 9 generic MSM partials.  The cases of tests/tools/g1_sum_cases.py run its serial loop (n > 256), every tree width
up to 256, n = 0 and n = 1, and -- by design, on points [k_i] G with known k_i -- tree and serial steps whose operands are the same group
element (the doubling branch of xyzz_add), opposite elements (its infinity branch), the same element under two Jacobian representations
(another Z, or a coordinate lifted by q), and inputs flagged as infinity in several patterns.

Every expectation is the closed form [sum k_i mod r] G, held to oracle.g1_sum on the CPU side (tests/test_g1_sum_cases_cpu.py); every
comparison is bit-exact on canonical Montgomery words, after the oracle's Jacobian -> affine conversion of the library's 12 words."""
import numpy as np
import pytest

import coarse_inputs as ci
import fixed_base_model as fb
import g1_sum_cases as gc

pytestmark = pytest.mark.gpu


def check_sum(oracle, got, c):
    assert got.shape == (12,)
    if c.spec.total == 0:
        assert int(got[3]) >> 63 == 1, f"{c.name}: the sum is the point at infinity, the flag is not set"
    else:
        assert int(got[3]) >> 63 == 0, f"{c.name}: a finite sum came back flagged as infinity"
        ci.assert_coarse_jacobian(got, c.name)
    assert np.array_equal(oracle.jac_to_affine(got), c.want), c.name


@pytest.mark.parametrize("name", gc.NAMES)
def test_g1_sum_case(bbg, oracle, name):
    c = gc.case(oracle, name)
    check_sum(oracle, bbg.g1_sum(c.jac), c)


@pytest.mark.parametrize("name", gc.DEVICE_NAMES)
def test_g1_sum_device_case(bbg, oracle, name):
    """The same through bbg_g1_sum_device on buffers of the caller's: the result buffer starts out as a finite non-answer."""
    c = gc.case(oracle, name)
    d_in, d_out = bbg.dev_alloc(max(c.n, 1) * 96), bbg.dev_alloc(96)
    try:
        if c.n:
            bbg.dev_upload(d_in, c.jac)
        bbg.dev_upload(d_out, np.full(12, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
        bbg.g1_sum_device(d_in, c.n, d_out)
        check_sum(oracle, bbg.dev_download(d_out, (12,)), c)
    finally:
        bbg.dev_free(d_in)
        bbg.dev_free(d_out)


@pytest.mark.parametrize("n", gc.NORMALIZE_SIZES)
def test_g1_normalize_mixed_entries(bbg, oracle, n):
    """Rescaled, plain, lifted and flagged entries mixed, across whole and partial blocks of 128: every finite output is [k_i] G bit for
    bit and canonical, every flagged input gives the affine infinity of include/bbg.h."""
    jac, want, kinds = gc.normalize_case(oracle, n)
    got = bbg.g1_normalize(jac)
    assert got.shape == (n, 8)
    for i in np.flatnonzero(~(got == want).all(axis=1))[:4]:
        raise AssertionError(f"n = {n}: entry {int(i)} ({kinds[i]}) differs")
    flagged = np.array([kd == "flagged" for kd in kinds], dtype=bool)
    ci.assert_canonical(got[~flagged].reshape(-1, 4), 1, f"n = {n}")
    assert (got[flagged] == fb.aff_infinity()).all()
