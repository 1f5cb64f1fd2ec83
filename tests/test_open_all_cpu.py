"""CPU side of bbg_g1_ntt / bbg_open_all: the host model (tests/tools/open_all_model.py) against itself and against closed forms, and the
new symbols in the header and the binding.  No GPU."""
import os
import re

import numpy as np
import pytest

import lagrange_model as lm
import open_all_model as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = oa.R_MOD
SEED = 0xBB254
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
NEW_SYMBOLS = ["bbg_g1_ntt", "bbg_g1_ntt_device", "bbg_open_all_prepare", "bbg_open_all_device", "bbg_open_all", "bbg_open_all_device_bytes",
               "bbg_open_all_free"]


def coefficients(seed, n):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_model_routes_agree(oracle, n):
    """The quotient definition and the circulant embedding give the same proofs over a hashed string (no structure to lean on)."""
    srs = oracle.srs_hashed(SEED + n, n)
    f = coefficients(SEED + 10 + n, n)
    want = oa.open_all_definition(oracle, srs, f)
    got, h = oa.open_all_embedding(oracle, srs, f)
    assert oa.is_infinity(h[n - 1]), "h_(n-1) must be the point at infinity"
    assert np.array_equal(got, want)
    assert not any(oa.is_infinity(p) for p in want)
    # f_0 is never read
    f2 = [(f[0] + 12345) % R] + f[1:]
    assert np.array_equal(oa.open_all_definition(oracle, srs, f2), want)


def test_model_matches_the_closed_form(oracle):
    """Over s_j = [x^j] G the proof at w^m is [(f(x) - f(w^m)) / (x - w^m)] G."""
    n = 8
    srs = oracle.srs_powers(lm.ints_to_mont(oracle, [X_INT])[0], n)
    f = coefficients(SEED + 20, n)
    w = lm.root(oracle, 3)
    ks = oa.closed_form_scalars(f, X_INT, w)
    # the fast route of closed_form_scalars against Horner and a plain inversion
    ev = lambda z: sum(c * pow(z, i, R) for i, c in enumerate(f)) % R
    assert ks == [(ev(X_INT) - ev(pow(w, m, R))) * pow(X_INT - pow(w, m, R), -1, R) % R for m in range(n)]
    assert oa.fr_fft(f, w) == oa.fr_ntt(f, w)
    G = oracle.g1_generator()
    want = oa.canon_points(oracle, np.stack([oracle.g1_mul(G, k) for k in lm.ints_to_mont(oracle, ks)]))
    assert np.array_equal(oa.open_all_definition(oracle, srs, f), want)
    assert np.array_equal(oa.open_all_embedding(oracle, srs, f)[0], want)


def test_model_edge_polynomials(oracle):
    n = 8
    srs = oracle.srs_hashed(SEED + 30, n)
    inf = np.tile(oa.aff_infinity(), (n, 1))
    for f in ([0] * n, [7] + [0] * (n - 1)):  # zero and constant: every quotient is zero
        assert np.array_equal(oa.open_all_definition(oracle, srs, f), inf)
        assert np.array_equal(oa.open_all_embedding(oracle, srs, f)[0], inf)
    f = [0, 1] + [0] * (n - 2)  # X: every quotient is 1, every proof s_0
    want = np.tile(oa.canon_points(oracle, srs[:1]), (n, 1))
    assert np.array_equal(oa.open_all_definition(oracle, srs, f), want)
    assert np.array_equal(oa.open_all_embedding(oracle, srs, f)[0], want)


def test_g1_ntt_model_round_trip_and_infinities(oracle):
    n = 8
    pts = oa.canon_points(oracle, oracle.srs_hashed(SEED + 40, n))
    pts[3] = oa.aff_infinity()
    fwd = oa.g1_ntt(oracle, pts)
    assert np.array_equal(oa.g1_ntt(oracle, fwd, inverse=True), pts)
    same = np.tile(pts[0], (n, 1))
    out = oa.g1_ntt(oracle, same)
    assert np.array_equal(out[0], oa.canon_points(oracle, oracle.g1_mul(pts[0], lm.ints_to_mont(oracle, [n])[0]))[0])
    assert np.array_equal(out[1:], np.tile(oa.aff_infinity(), (n - 1, 1)))


def test_header_and_binding_list_the_new_symbols(pkg):
    text = open(os.path.join(ROOT, "include", "bbg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bbg_[a-z0-9_]+)\s*\(", text))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/bbg.h"
        assert sym in pkg.binding.EXPORTED_SYMBOLS, f"{sym} is missing from binding.EXPORTED_SYMBOLS"
    lib = pkg.load_library()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), f"{sym} is not exported by libbbg.so"
    for name in ("g1_ntt", "g1_ntt_device", "open_all_prepare"):
        assert callable(getattr(pkg.Bbg, name))
    for name in ("open", "open_device", "device_bytes", "free"):
        assert callable(getattr(pkg.binding.OpenAll, name))
