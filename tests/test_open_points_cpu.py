"""The integer models of bbg_open_points and bbg_kzg_verify_reduce (tests/tools/open_points_model.py) against coefficient-form division,
which is oracle.kate_opening of oracle.ntt(., IFFT): the quotient values and y off the domain, the on-domain identity for q_m, and the
reduction's closed form with every point a multiple of G.  No GPU."""
import random

import numpy as np
import pytest

import open_points_model as om
import pairing_model as pm

R = om.R
IFFT = 1


def rand(rng):
    return rng.randrange(R)


def coefficient_route(oracle, f, z):
    """(y, quotient values) from the VALUES f through the oracle: inverse transform, coefficient-form division, forward transform."""
    coeffs = oracle.ntt(pm.fr_words(f), IFFT)
    dest, y = oracle.kate_opening(coeffs, pm.fr_words([z])[0])
    return oracle.canon(0, y).reshape(4), oracle.canon(0, oracle.ntt(dest, 0)), oracle.canon(0, dest)


def test_model_root_is_the_oracles(oracle):
    for lg in (1, 4, 11, 28):
        assert np.array_equal(oracle.canon(0, oracle.root_of_unity(lg)).reshape(4), pm.fr_words([om.root(lg)])[0])


@pytest.mark.parametrize("lg", [1, 4, 10, 11])
def test_off_the_domain(oracle, lg):
    rng = random.Random(0x09E2 + lg)
    n = 1 << lg
    f = [rand(rng) for _ in range(n)]
    z = rand(rng)
    y, q, hit = om.open_values(f, z, lg)
    assert hit == om.NO_HIT
    want_y, want_q, dest = coefficient_route(oracle, f, z)
    assert np.array_equal(pm.fr_words([y])[0], want_y)
    assert np.array_equal(pm.fr_words(q), want_q)
    assert not dest[n - 1].any(), "the quotient has degree n - 2"


@pytest.mark.parametrize("lg", [4, 11])
def test_on_domain_identity(oracle, lg):
    """q_m = - w^-m sum_(i != m) (f_m - f_i) / d_i: the model's S0 / S1 form, the identity spelt out, and coefficient-form division agree,
    for m in {0, 1, n/2, n - 1}."""
    rng = random.Random(0x09E3 + lg)
    n = 1 << lg
    f = [rand(rng) for _ in range(n)]
    w = om.root(lg)
    for m in (0, 1, n // 2, n - 1):
        z = pow(w, m, R)
        y, q, hit = om.open_values(f, z, lg)
        assert hit == m and y == f[m]
        assert q[m] == om.hit_identity(f, m, lg)
        want_y, want_q, dest = coefficient_route(oracle, f, z)
        assert np.array_equal(pm.fr_words([y])[0], want_y), m
        assert np.array_equal(pm.fr_words(q), want_q), m
        assert not dest[n - 1].any()
        assert sum(pow(w, i, R) * q[i] for i in range(n)) % R == 0, "the top coefficient of the quotient vanishes"


def test_division_model_is_the_oracles(oracle):
    rng = random.Random(0x09E4)
    coeffs = [rand(rng) for _ in range(64)]
    z = rand(rng)
    y, q = om.divide(coeffs, z)
    dest, f = oracle.kate_opening(pm.fr_words(coeffs), pm.fr_words([z])[0])
    assert np.array_equal(oracle.canon(0, f).reshape(4), pm.fr_words([y])[0]) and np.array_equal(oracle.canon(0, dest), pm.fr_words(q))
    vals = om.values(coeffs[:16], 4)
    assert np.array_equal(pm.fr_words(vals), oracle.canon(0, oracle.ntt(pm.fr_words(coeffs[:16]), 0)))


def test_fast_scalar_multiplication_is_the_pairing_models():
    import open_points_cases as oc
    rng = random.Random(0x09E6)
    for s in [0, 1, 2, 3, R - 1, R - 2, R, R + 5] + [rand(rng) for _ in range(6)]:
        assert oc.g1_mul_g(s) == pm.g1_mul(pm.G1, s % R), s


@pytest.mark.parametrize("rho_kind", ["random", "zero", "one"])
def test_reduction_closed_form(rho_kind):
    rng = random.Random(0x09E5)
    x = rand(rng)
    N = 7
    polys = [[rand(rng) for _ in range(8)] for _ in range(N)]
    polys[3] = [0] * 8                     # the zero polynomial: commitment and proof at infinity
    polys[5] = polys[1]                    # one polynomial at two points
    zs = [rand(rng) for _ in range(N)]
    zs[6] = zs[2]                          # one point twice
    rho = {"random": rand(rng), "zero": 0, "one": 1}[rho_kind]
    c, y, w = om.kzg_honest(x, polys, zs)
    assert c[3] == 0 and w[3] == 0
    l, r = om.kzg_closed_form(c, zs, y, w, rho)
    assert x * l % R == r, "x L = R for honest openings"
    points, scalars = om.kzg_packed(c, zs, y, w, rho)
    assert len(points) == len(scalars) == 2 * N + 1
    assert sum(p * s for p, s in zip(points, scalars)) % R == r, "the packed layout sums to the same R"
    assert sum(p * s for p, s in zip(points[N:2 * N], scalars[:N])) % R == l, "the proofs' window with the powers of rho sums to L"
    # one changed y, z, C or pi breaks x L = R (rho = 0 sees opening 0 only)
    k = 0 if rho_kind == "zero" else 4
    for what in "yzcw":
        c2, z2, y2, w2 = list(c), list(zs), list(y), list(w)
        {"y": y2, "z": z2, "c": c2, "w": w2}[what][k] += 1
        l2, r2 = om.kzg_closed_form(c2, z2, y2, w2, rho)
        assert x * l2 % R != r2, what
