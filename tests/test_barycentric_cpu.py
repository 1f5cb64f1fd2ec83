"""Lagrange-form evaluation / opening / batch inversion: what can be checked without a GPU.

tests/tools/barycentric_model.py states the formulas of csrc/barycentric.hip on Python integers.  Here the model is proven against the C
oracle's coefficient route (inverse NTT, then Horner / the Kate recurrence), on values and points over the whole input range [0, 2r); the
GPU tests (tests/test_gpu_barycentric.py) then use the oracle route at their own sizes and the inputs asserted here."""
import ctypes
import os
import re

import numpy as np
import pytest

import barycentric_model as bm
import coarse_inputs as ci

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = bm.R_MOD
IFFT, FFT = 1, 0
NEW_SYMBOLS = ("bbg_fr_batch_invert_device", "bbg_poly_evaluate_lagrange_device", "bbg_poly_evaluate_lagrange",
               "bbg_kate_opening_lagrange_device", "bbg_prover_evaluate_lagrange")


def points(lg):
    """Off-domain evaluation points as Montgomery words: canonical, and the second representative z + r of the first."""
    zs = bm.mont_words(bm.Z_INTS)
    return list(zs) + [bm.second_representative(zs[0])[0]]


def test_shared_points_are_off_every_domain():
    """Every off-domain z of either test file, at every size either evaluates at (and the prover's 2^6 / 2^10): z^n != 1."""
    for lg in sorted(set(bm.SIZES_CPU + bm.SIZES_GPU + (6, 10))):
        for z in bm.Z_INTS:
            assert bm.off_domain(z, lg), (lg, hex(z))
    assert bm.X_INT % R != 0 and all(bm.off_domain(bm.X_INT, lg) for lg in (10,))
    assert bm.E_BLK == 1 << bm.LOG_E_BLK and bm.G == bm.E_BLK


def test_model_root_is_the_oracles(oracle):
    for lg in sorted(set(bm.SIZES_CPU + bm.SIZES_GPU)):
        assert np.array_equal(bm.canon(oracle, oracle.root_of_unity(lg)), bm.mont_words([ci.root_of_unity(lg)])[0])


@pytest.mark.parametrize("lg", bm.SIZES_CPU)
def test_model_evaluation_equals_coefficient_route(oracle, lg):
    n = 1 << lg
    evals = bm.coarse_poly(0xBA51 + lg, n)
    assert not ci.below(evals, R).all() or n < 64, "the values should reach beyond r"
    coeffs = oracle.ntt(evals, IFFT)
    w = oracle.root_of_unity(lg)
    for z in points(lg):
        want = bm.canon(oracle, oracle.poly_eval(coeffs, z))
        assert np.array_equal(bm.evaluate(evals, lg, z), want), (lg, "F(z)")
        want = bm.canon(oracle, oracle.poly_eval(coeffs, oracle.fe_mul(0, z.reshape(1, 4), w.reshape(1, 4))[0]))
        assert np.array_equal(bm.evaluate(evals, lg, z, shifted=True), want), (lg, "F(z w)")


@pytest.mark.parametrize("lg", bm.SIZES_CPU)
def test_model_opening_equals_coefficient_route(oracle, lg):
    n = 1 << lg
    evals = bm.coarse_poly(0xBA52 + lg, n)
    coeffs = oracle.ntt(evals, IFFT)
    std = [ci.from_mont(v % R, 0) for v in ci.to_ints(evals)]
    w = ci.root_of_unity(lg)
    for z in points(lg):
        got_w, got_f = bm.opening(evals, lg, z)
        assert np.array_equal(got_f, bm.canon(oracle, oracle.poly_eval(coeffs, z)))
        # by definition: W(w^i) (w^i - z) = f_i - F(z) at every point of the domain
        zi, fz = ci.from_mont(ci.to_ints(z)[0] % R, 0), ci.from_mont(ci.to_ints(got_f)[0], 0)
        for i, wv in enumerate(ci.to_ints(got_w)):
            assert ci.from_mont(wv, 0) * (pow(w, i, R) - zi) % R == (std[i] - fz) % R, (lg, i)
        if zi == 0:
            continue  # the reference's recurrence multiplies by -1/z (polynomial_arithmetic.cpp:727-750): it has no answer at z = 0
        dest, f = oracle.kate_opening(coeffs, z)
        dest = bm.canon(oracle, dest)
        assert not dest[n - 1].any(), "W has degree n - 2: its top coefficient is zero"
        assert np.array_equal(got_f, bm.canon(oracle, f))
        assert np.array_equal(got_w, bm.canon(oracle, oracle.ntt(dest, FFT))), lg


@pytest.mark.parametrize("lg", bm.SIZES_CPU)
def test_model_point_on_the_domain(oracle, lg):
    n = 1 << lg
    evals = bm.coarse_poly(0xBA53 + lg, n)
    canon = bm.canon(oracle, evals)
    for j in (0, 1, n - 1):
        z = bm.mont_words([pow(ci.root_of_unity(lg), j, R)])[0]
        assert np.array_equal(bm.evaluate(evals, lg, z), canon[j])
        assert np.array_equal(bm.evaluate(evals, lg, z, shifted=True), canon[(j + 1) % n])
        with pytest.raises(AssertionError):
            bm.opening(evals, lg, z)


def test_model_batch_invert_zero_rule(oracle):
    vals = bm.coarse_poly(0xBA54, 96)
    vals[5], vals[6] = 0, ci.to_words([R])[0]
    got = bm.batch_invert(vals)
    want = bm.canon(oracle, oracle.fe_inv(0, vals))
    assert not got[5].any() and not got[6].any()
    live = np.array([v % R != 0 for v in ci.to_ints(vals)])
    assert np.array_equal(got[live], want[live])
    one = bm.mont_words([1])[0]
    assert all(np.array_equal(bm.canon(oracle, oracle.fe_mul(0, vals[i:i + 1], got[i:i + 1]))[0], one) for i in np.flatnonzero(live))


def test_entry_points_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "bbg.h")).read()
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert name in pkg.binding.EXPORTED_SYMBOLS, name
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
    for method in ("fr_batch_invert_device", "poly_evaluate_lagrange_device", "poly_evaluate_lagrange", "kate_opening_lagrange_device"):
        assert callable(getattr(pkg.binding.Bbg, method))
    assert '"fr_batch_invert", "barycentric"' in header
