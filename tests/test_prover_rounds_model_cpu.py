"""tests/tools/prover_rounds_model.py (the oracle-built model tests/test_gpu_prover_rounds.py holds the device to) against Python integers:
Horner evaluation (coarse_inputs.horner), term-by-term sums, and the defining identity of an opening quotient, W(X) (X - z) = F(X) - F(z),
coefficient by coefficient.  Inputs carry p - 1 and coarse representatives x + p; every output must be canonical."""
import numpy as np
import pytest

import coarse_inputs as ci
import prover_rounds_model as prm

P = ci.R_MOD
SIZES = (3, 6)  # n = 8 and 64


def words(seed, count):
    """count Montgomery words over [0, 2p) with p - 1 first and a coarse x + p second (coarse_ints splices its catalogue in as well)."""
    vals = ci.coarse_ints(seed, count, 0)
    vals[0] = P - 1
    if count > 1:
        vals[1] = vals[1] % P + P
    return ci.to_words(vals)


def points(lg):
    """name -> Montgomery words of an evaluation point: generic, zero, one, a domain point, a coarse representative."""
    generic = ci.to_mont(0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % P, 0)
    return {"generic": generic, "zero": 0, "one": ci.to_mont(1, 0), "domain": ci.to_mont(pow(ci.root_of_unity(lg), 5, P), 0), "coarse": generic + P}


def word(v):
    return ci.to_words([v])[0]


def test_the_root_is_the_integer_model_s():
    for lg in SIZES:
        assert ci.to_ints(prm.canon(prm.oracle().root_of_unity(lg))) == [ci.to_mont(ci.root_of_unity(lg), 0)]


@pytest.mark.parametrize("lg", SIZES)
def test_evaluations_are_horner_sums(lg):
    n = 1 << lg
    lengths = [n, n + 1, 4 * n, n, 4 * n, n + 1, 1]
    arrays = [words(0x5A00 + 16 * lg + k, m) for k, m in enumerate(lengths)]
    shifted = [k % 3 == 1 for k in range(len(arrays))]
    w = ci.to_mont(ci.root_of_unity(lg), 0)
    for name, z in points(lg).items():
        zw = ci.mont_mul(z % P, w, 0)
        want = [ci.horner(ci.to_ints(a), zw if s else z % P) for a, s in zip(arrays, shifted)]
        got = prm.evaluations(arrays, shifted, word(z), lg)
        assert ci.to_ints(got) == want, name
        assert ci.below(got, P).all()
        plain = prm.evaluations(arrays, None, word(z), lg)
        assert ci.to_ints(plain) == [ci.horner(ci.to_ints(a), z % P) for a in arrays], name
    # at a domain point an n-coefficient polynomial takes the value its transform has there
    a = arrays[0]
    at_w5 = prm.evaluations([a], [0], word(points(lg)["domain"]), lg)[0]
    assert ci.to_ints(at_w5)[0] == ci.dft(ci.to_ints(a), 0)[5]


@pytest.mark.parametrize("count", (1, 5, 32))
@pytest.mark.parametrize("lg", SIZES)
def test_linearisation_is_the_term_by_term_sum(lg, count):
    n = 1 << lg
    arrays = [words(0x5B00 + 64 * lg + k, n) for k in range(count)]
    scalars = words(0x5B80 + lg, count)
    for k, v in enumerate((ci.to_ints(scalars)[0] % P + P, 0, ci.to_mont(1, 0), P - 1)[:count]):
        scalars[k] = word(v)
    z = points(lg)["generic"]
    r, r_eval = prm.linearisation(arrays, scalars, word(z))
    ints, sc = [ci.to_ints(a) for a in arrays], ci.to_ints(scalars)
    want = [sum(ci.mont_mul(a[i], s, 0) for a, s in zip(ints, sc)) % P for i in range(n)]
    assert ci.to_ints(r) == want
    assert ci.to_ints(r_eval) == [ci.horner(want, z)]
    assert ci.below(r, P).all() and ci.below(r_eval, P).all()


@pytest.mark.parametrize("with_top", (False, True))
@pytest.mark.parametrize("count_zeta,count_omega", [(0, 1), (1, 5), (14, 32), (32, 1)])
@pytest.mark.parametrize("lg", SIZES)
def test_openings_satisfy_the_quotient_identity(lg, count_zeta, count_omega, with_top):
    n = 1 << lg
    t = words(0x5C00 + lg, 4 * n)
    az = [words(0x5C10 + 64 * lg + k, n) for k in range(count_zeta)]
    ao = [words(0x5D10 + 64 * lg + k, n) for k in range(count_omega)]
    nz, no = words(0x5E00 + lg, max(count_zeta, 2))[:count_zeta], words(0x5E40 + lg, max(count_omega, 2))[:count_omega]
    pts = points(lg)
    z = pts["coarse"]
    zo = ci.mont_mul(z % P, ci.to_mont(ci.root_of_unity(lg), 0), 0)
    top_scalar = ci.to_mont(pow(ci.from_mont(z % P, 0), 2 * n, P), 0)
    top = (word(top_scalar), t[3 * n]) if with_top else None
    f, f_shifted = prm.opened_polynomials(t[:n], az, nz, ao, no, top)
    # F and F' themselves, term by term
    t_int = ci.to_ints(t)
    want_f = [(t_int[i] + sum(ci.mont_mul(a[i], s, 0) for a, s in zip([ci.to_ints(a) for a in az], ci.to_ints(nz)))) % P for i in range(n)]
    if with_top:
        want_f.append(ci.mont_mul(top_scalar, t_int[3 * n], 0))
    want_fs = [sum(ci.mont_mul(a[i], s, 0) for a, s in zip([ci.to_ints(a) for a in ao], ci.to_ints(no))) % P for i in range(n)]
    assert ci.to_ints(f) == want_f and ci.to_ints(f_shifted) == want_fs
    assert len(f) == n + (1 if with_top else 0)
    if count_zeta == 0 and not with_top:
        assert np.array_equal(f, prm.canon(t[:n])), "no terms: F = t_low"
    w, w_shifted = prm.openings(t[:n], az, nz, ao, no, word(z), word(zo), top)
    assert w.shape == (n, 4) and w_shifted.shape == (n, 4)
    assert ci.below(w, P).all() and ci.below(w_shifted, P).all()
    for quotient, poly, point in ((ci.to_ints(w), want_f, z % P), (ci.to_ints(w_shifted), want_fs, zo)):
        value = ci.horner(poly, point)
        q = quotient + [0] * (len(poly) + 1 - len(quotient))  # the coefficients the model leaves out are zeros
        assert (-ci.mont_mul(point, q[0], 0)) % P == (poly[0] - value) % P
        for i in range(1, len(poly)):
            assert (q[i - 1] - ci.mont_mul(point, q[i], 0)) % P == poly[i], i
        assert q[len(poly) - 1] == 0, "an exact division leaves no top coefficient"
