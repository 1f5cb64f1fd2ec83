"""CPU side of the cell handle of bbg_open_all (bbg_open_all_prepare_cells): the host model (tests/tools/open_cells_model.py) against itself,
against the all-points model and against the closed form; the designed inputs the GPU tests of the segment sum rely on, proved from the
integers; and the new symbols in the header, the library and the binding.  No GPU."""
import os
import re

import numpy as np
import pytest

import coarse_inputs as ci
import lagrange_model as lm
import open_all_model as oa
import open_cells_model as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = oa.R_MOD
SEED = 0xBB254 + 0xCE11
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
SHAPES = [(2, 1), (3, 1), (3, 2), (4, 2), (6, 3), (7, 6)]  # r = 2, i.e. transforms of 4 points, is the smallest; (7, 6) is l = 64 with r = 2
NEW_SYMBOLS = ["bbg_open_all_prepare_cells", "bbg_open_all_count"]


def coefficients(seed, n):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]


def by_generator(oracle, scalars):
    G = oracle.g1_generator()
    return oa.canon_points(oracle, np.stack([oracle.g1_mul(G, k) for k in lm.ints_to_mont(oracle, scalars)]))


@pytest.mark.parametrize("lg,lc", SHAPES)
def test_model_routes_agree(oracle, lg, lc):
    """The definition, the device's route and, over a powers string, the closed form give the same proofs."""
    n, l = 1 << lg, 1 << lc
    r = n // l
    assert lm.root(oracle, lg) == ci.root_of_unity(lg)
    f = coefficients(SEED + 16 * lg + lc, n)
    hashed = oracle.srs_hashed(SEED + lg, n)
    want = oc.open_cells_definition(oracle, hashed, f, lc)
    got, h = oc.open_cells_embedding(oracle, hashed, f, lc)
    assert want.shape == (r, 8) and not any(oa.is_infinity(p) for p in want)
    assert oa.is_infinity(h[r - 1]), "h_(r-1) must be the point at infinity"
    assert np.array_equal(got, want)
    # f_0 .. f_(l-1) are never read, and neither are the last l points of the string
    f2 = [(v + 12345) % R for v in f[:l]] + f[l:]
    assert np.array_equal(oc.open_cells_definition(oracle, hashed, f2, lc), want)
    cut = hashed.copy()
    cut[n - l:] = oa.aff_infinity()
    assert np.array_equal(oc.open_cells_embedding(oracle, cut, f2, lc)[0], want)

    powers = oracle.srs_powers(lm.ints_to_mont(oracle, [X_INT])[0], n)
    ks = oc.cell_closed_form_scalars(f, X_INT, lc)
    want = by_generator(oracle, ks)
    assert np.array_equal(oc.open_cells_definition(oracle, powers, f, lc), want)
    assert np.array_equal(oc.open_cells_embedding(oracle, powers, f, lc)[0], want)


def test_closed_form_against_plain_division():
    """cell_closed_form_scalars and cell_quotient_coeffs against each other: q_m(x) (x^l - phi^m) + I_m(x) = f(x), deg I_m < l."""
    lg, lc = 5, 2
    n, l = 1 << lg, 1 << lc
    f = coefficients(SEED + 50, n)
    phi = pow(ci.root_of_unity(lg), l, R)
    ks = oc.cell_closed_form_scalars(f, X_INT, lc)
    rem = oc.cell_remainders(f, lc)
    for m in range(n // l):
        a = pow(phi, m, R)
        q = oc.cell_quotient_coeffs(f, l, a)
        assert len(q) == n - l and oc.horner(q, X_INT) == ks[m]
        # f = q (X^l - a) + I, coefficient by coefficient
        back = [0] * n
        for j, v in enumerate(q):
            back[j + l] = (back[j + l] + v) % R
            back[j] = (back[j] - a * v) % R
        for b in range(l):
            back[b] = (back[b] + rem[m][b]) % R
        assert back == f
        # the cell's values are f on the coset w^(m + r t)
        w = ci.root_of_unity(lg)
        for t in range(l):
            z = pow(w, m + (n // l) * t, R)
            assert oc.horner(f, z) == oc.horner(rem[m], z)


@pytest.mark.parametrize("lg", [1, 2, 3])
def test_log2cell_zero_is_the_all_points_opening(oracle, lg):
    n = 1 << lg
    srs = oracle.srs_hashed(SEED + 60 + lg, n)
    f = coefficients(SEED + 70 + lg, n)
    want = oa.open_all_definition(oracle, srs, f)
    assert np.array_equal(oc.open_cells_definition(oracle, srs, f, 0), want)
    assert np.array_equal(oc.open_cells_embedding(oracle, srs, f, 0)[0], want)
    assert oc.cell_quotient_coeffs(f, 1, 7) == oa.quotient_coeffs(f, 7)
    w = ci.root_of_unity(lg)
    assert oc.cell_closed_form_scalars(f, X_INT, 0) == oa.closed_form_scalars(f, X_INT, w)


@pytest.mark.parametrize("lg", [1, 2, 3, 4, 5, 6])
def test_cell_layouts_at_log2cell_zero_are_the_all_points_ones(lg):
    """The string layout and the coefficient scatter of the cell handle at l = 1 are s^ and c^ of the all-points construction: the one
    layout kernel and the one scatter kernel of csrc/open_all.hip serve both kinds of handle on this identity."""
    n = 1 << lg
    assert oc.string_layout(n, 0) == [n - 2 - i for i in range(n - 1)] + [None] * (n + 1)
    f = coefficients(SEED + 110 + lg, n)
    tagged = np.zeros((n, 8), dtype=np.uint64)  # point j carries its index, so that s^ can be read back as indices
    tagged[:, 0] = np.arange(n)
    s_hat, c_hat = oa.embedding(tagged, f)
    assert oc.class_embedding(f, 0, 0) == c_hat
    assert [None if oa.is_infinity(p) else int(p[0]) for p in s_hat] == oc.string_layout(n, 0)


def signs(kind, l, seed):
    rng = np.random.default_rng(seed)
    if kind == "plus":
        return [1] * l
    if kind == "alternating":
        return [1, -1] * (l // 2)
    if kind == "halves":
        return [1] * (l // 2) + [-1] * (l // 2)
    if kind == "balanced":
        e = [1] * (l // 2) + [-1] * (l // 2)
        rng.shuffle(e)
        return [int(v) for v in e]
    e = [1] * (l // 2 + 1) + [-1] * (l // 2 - 1)  # unbalanced: sum 2
    rng.shuffle(e)
    return [int(v) for v in e]


@pytest.mark.parametrize("lg,lc", [(4, 2), (8, 4), (9, 6)])
def test_designed_inputs_from_the_integers(oracle, lg, lc):
    """Over s_j = [x^j] G and with f_(l i + b) = eps_b x^(-b) g_i, the l products the segment sum adds at output index i are
    [eps_b C_i S_i] G: equal or opposite, whatever b.  C_i S_i is non-zero at all 2r indices for these seeds, so no segment is trivially
    a run of infinities, and a balanced eps makes every proof the point at infinity."""
    n, l = 1 << lg, 1 << lc
    r = n // l
    g = coefficients(SEED + 80 + lg, r)
    C, S = oc.designed_factors(g, X_INT, lc)
    assert sum(1 for c, s in zip(C, S) if c * s % R) == 2 * r
    for kind in ("plus", "alternating", "halves", "balanced", "unbalanced"):
        eps = signs(kind, l, SEED + 90 + lg)
        f = oc.designed_coeffs(g, X_INT, eps, lc)
        prod = oc.product_scalars(f, X_INT, lc)
        for b in range(l):
            assert prod[b] == [eps[b] * c * s % R for c, s in zip(C, S)], f"{kind}: residue class {b}"
        ks = oc.cell_closed_form_scalars(f, X_INT, lc)
        # the proofs are sum(eps) times those of eps = (1, 0, .., 0)
        base = oc.cell_closed_form_scalars(oc.designed_coeffs(g, X_INT, [1] + [0] * (l - 1), lc), X_INT, lc)
        assert ks == [sum(eps) * k % R for k in base]
        assert all(ks) == (sum(eps) != 0) and any(ks) == (sum(eps) != 0)
    if lg == 4:
        f = oc.designed_coeffs(g, X_INT, signs("unbalanced", l, SEED + 90 + lg), lc)
        powers = oracle.srs_powers(lm.ints_to_mont(oracle, [X_INT])[0], n)
        want = by_generator(oracle, oc.cell_closed_form_scalars(f, X_INT, lc))
        assert np.array_equal(oc.open_cells_definition(oracle, powers, f, lc), want)
        assert np.array_equal(oc.open_cells_embedding(oracle, powers, f, lc)[0], want)
        f = oc.designed_coeffs(g, X_INT, signs("balanced", l, SEED + 90 + lg), lc)
        assert np.array_equal(oc.open_cells_embedding(oracle, powers, f, lc)[0], np.tile(oa.aff_infinity(), (r, 1)))


def test_model_edge_polynomials(oracle):
    lg, lc = 4, 2
    n, l = 1 << lg, 1 << lc
    r = n // l
    srs = oracle.srs_hashed(SEED + 100, n)
    inf = np.tile(oa.aff_infinity(), (r, 1))
    for f in ([0] * n, coefficients(SEED + 101, l) + [0] * (n - l)):  # zero, and degree below l: every quotient is zero
        assert np.array_equal(oc.open_cells_definition(oracle, srs, f, lc), inf)
        assert np.array_equal(oc.open_cells_embedding(oracle, srs, f, lc)[0], inf)
    c = 0x1234567
    f = [0] * l + [c] + [0] * (n - l - 1)  # c X^l: every quotient is c, every proof [c] s_0
    want = np.tile(oa.canon_points(oracle, oracle.g1_mul(srs[0], lm.ints_to_mont(oracle, [c])[0])), (r, 1))
    assert np.array_equal(oc.open_cells_definition(oracle, srs, f, lc), want)
    assert np.array_equal(oc.open_cells_embedding(oracle, srs, f, lc)[0], want)


def test_header_library_and_binding_list_the_new_symbols(pkg):
    text = open(os.path.join(ROOT, "include", "bbg.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bbg_[a-z0-9_]+)\s*\(", code))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/bbg.h"
        assert sym in pkg.binding.EXPORTED_SYMBOLS, f"{sym} is missing from binding.EXPORTED_SYMBOLS"
    assert re.search(r"bbg_open_all_prepare_cells\(bbg_ctx\* ctx, bbg_srs\* srs, unsigned log2n, unsigned log2cell, struct bbg_open_all\*\* out\)", code)
    assert re.search(r"bbg_open_all_count\(const struct bbg_open_all\* h, size_t\* proofs\)", code)
    # the header says where a cell's values come from and what verification needs
    flat = re.sub(r"[\s*]+", " ", comments)
    assert "stride r" in flat and "bbg_ntt" in flat and "[x^l]_2" in flat
    lib = pkg.load_library()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), f"{sym} is not exported by libbbg.so"
    import inspect
    assert "log2cell" in inspect.signature(pkg.Bbg.open_all_prepare).parameters
    assert inspect.signature(pkg.Bbg.open_all_prepare).parameters["log2cell"].default == 0
    assert isinstance(pkg.binding.OpenAll.count, property)
