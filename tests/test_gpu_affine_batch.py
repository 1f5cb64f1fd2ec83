"""The batched XYZZ -> affine conversion (aff_batch_park / aff_batch_invert / aff_batch_finish, csrc/curve.hip.h) through every kernel
that uses it, at the shapes where a chunked conversion can go wrong: tails of every chunk size (16 points per thread in the linear
string, 4 in the hashed one, 4 in the two batch multiplications, one thread per point in the window-table build), and chunks whose
members are partly finite and partly at infinity.

Every comparison is bit-exact on canonical Montgomery affine words against the C oracle; an infinite result is the promised aff_inf()
encoding.  (The Lagrange normalisation's short chunks and its infinite output are tests/test_gpu_lagrange_srs.py's.)"""
import itertools

import numpy as np
import pytest

import coarse_inputs as ci
import fixed_base_model as fb
import lagrange_model as lm
import var_base_model as vb

pytestmark = pytest.mark.gpu

R = vb.R_MOD
N = 7  # one full chunk of four and a tail of three
TAIL_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 33]
# (first four positions) x (tail): True = finite.  All 16 patterns of the full chunk, each with an all-infinite and a mixed tail.
PATTERNS = [head + tail for head in itertools.product((False, True), repeat=4) for tail in ((False, False, False), (True, False, True))]
SCALARS = [0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % R, 3, R - 1, 0x1_0000_0001, (1 << 253) + 12345, 255, R - 256]


def mont(vals):
    return ci.to_words([ci.to_mont(v % R, 0) for v in vals])


@pytest.fixture(scope="module")
def products(oracle):
    """Seven scalars, seven finite points, and both kinds of product by the oracle: computed once and left unchanged."""
    words = mont(SCALARS)
    G = lm.canon_points(oracle, oracle.g1_generator())[0]
    points = np.stack([lm.canon_points(oracle, oracle.g1_mul(G, w))[0] for w in mont([2, 5, 77, R - 2, 1 << 200, 0xABCDEF, 11])])
    fixed = np.stack([lm.canon_points(oracle, oracle.g1_mul(G, w))[0] for w in words])
    variable = np.stack([lm.canon_points(oracle, oracle.g1_mul(p, w))[0] for p, w in zip(points, words)])
    return words, points, fixed, variable


def masked(finite_values, pattern):
    return np.stack([v if f else fb.aff_infinity() for v, f in zip(finite_values, pattern)])


@pytest.mark.parametrize("n", TAIL_SIZES)
def test_synthetic_strings_at_chunk_tails(bbg, oracle, n):
    a, s = 0x123456789ABCDEF, 0xFEDCBA987654321
    srs = bbg.srs_synth_linear(a, s, n)
    got = srs.read()
    srs.free()
    assert np.array_equal(got, oracle.srs_linear(a, s, n)), f"linear string, n = {n}"
    srs = bbg.srs_synth_hashed(0xBB254, n)
    got = srs.read()
    srs.free()
    assert np.array_equal(got, oracle.srs_hashed(0xBB254, n)), f"hashed string, n = {n}"


def test_fixed_base_mixed_chunks(bbg, products):
    """Zero scalars (results at infinity) in every pattern over a full chunk, beside an all-zero and a mixed tail."""
    words, _, fixed, _ = products
    zero = np.zeros(4, dtype=np.uint64)
    for pattern in PATTERNS:
        scalars = np.stack([w if f else zero for w, f in zip(words, pattern)])
        got = bbg.g1_fixed_base_mul(scalars)
        want = masked(fixed, pattern)
        bad = [i for i in range(N) if not np.array_equal(got[i], want[i])]
        assert not bad, f"finite pattern {pattern}: positions {bad} differ"


def device_mul_in_place(bbg, points, scalars):
    n = points.shape[0]
    d_p, d_s = bbg.dev_alloc(n * 64), bbg.dev_alloc(n * 32)
    try:
        bbg.dev_upload(d_p, points)
        bbg.dev_upload(d_s, scalars)
        bbg.g1_batch_mul_device(d_p, d_s, n, d_p)
        return bbg.dev_download(d_p, (n, 8))
    finally:
        bbg.dev_free(d_p)
        bbg.dev_free(d_s)


@pytest.mark.parametrize("glv", [1, 0])
def test_variable_base_mixed_chunks(bbg, products, glv):
    """The same patterns with infinite POINTS (every scalar non-zero), under both multiplication kernels, and once with out = points."""
    words, points, _, variable = products
    bbg.set_option("batch_mul_glv", glv)
    try:
        for pattern in PATTERNS:
            pts = masked(points, pattern)
            want = masked(variable, pattern)
            got = bbg.g1_batch_mul(pts, words)
            bad = [i for i in range(N) if not np.array_equal(got[i], want[i])]
            assert not bad, f"batch_mul_glv = {glv}, finite pattern {pattern}: positions {bad} differ"
        pattern = PATTERNS[2 * 0b0110 + 1]  # inf, P, P, inf | P, inf, P
        got = device_mul_in_place(bbg, masked(points, pattern), words)
        assert np.array_equal(got, masked(variable, pattern)), f"batch_mul_glv = {glv}, in place"
    finally:
        bbg.set_option("batch_mul_glv", 1)


@pytest.mark.parametrize("n", [5, 129])
def test_small_registered_srs_and_msm(pkg, bbg, oracle, n):
    """The window-table build on a one-block launch with a partly filled block (5) and on a second, one-thread block (129): an MSM over
    the whole string reads every window of every point."""
    points = oracle.srs_hashed(0xAFF1 + n, n)
    srs = bbg.srs_register(points)
    try:
        assert np.array_equal(srs.read(), points)
        scalars = pkg.synthetic_scalars(0xAFF1 + 3 * n, n)
        got = oracle.jac_to_affine(bbg.msm(srs, scalars))
    finally:
        srs.free()
    assert np.array_equal(got, oracle.pippenger(scalars, points)), f"MSM over a freshly registered string of {n} points"
