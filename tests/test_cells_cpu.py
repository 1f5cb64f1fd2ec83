"""CPU side of the cells of a polynomial as data (bbg_cells_values, bbg_cells_recover): the host model's definition (Lagrange interpolation
through the K l points) against the route the device takes, the two r-periodic identities of Z against its product, and the new symbols in
the header, the library and the binding.  No GPU."""
import os
import re

import numpy as np
import pytest

import cells_model as cm
import coarse_inputs as ci

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = cm.R_MOD
SEED = 0xBB254 + 0xCE115
SHAPES = [(2, 1), (3, 1), (3, 2), (4, 2), (6, 3)]
NEW_SYMBOLS = ["bbg_cells_values_device", "bbg_cells_values", "bbg_cells_recover_device", "bbg_cells_recover"]
NEW_METHODS = ["cells_values", "cells_values_device", "cells_recover", "cells_recover_device"]


def id_sets(r, seed):
    """{name: ids}: all, one cell, first half, second half, even cells, a seeded random subset in shuffled order."""
    rng = np.random.default_rng(seed)
    size = int(rng.integers(1, r + 1))
    sets = {"all": list(range(r)), "one": [int(rng.integers(0, r))], "first_half": list(range(r // 2)), "second_half": list(range(r // 2, r)),
            "even": list(range(0, r, 2)), "random": [int(v) for v in rng.permutation(r)[:size]]}
    return sets


@pytest.mark.parametrize("lg,lc", SHAPES)
def test_definition_against_route(oracle, lg, lc):
    n, l, r = cm.shape(lg, lc)
    values = cm.random_ints(SEED + 16 * lg + lc, n)  # any values: the interpolant exists whatever they are
    for name, ids in id_sets(r, SEED + 100 + 16 * lg + lc).items():
        K = len(ids)
        known = cm.known_values(values, ids, lc)
        got = cm.recover_route(oracle, ids, known, lg, lc)
        assert len(got) == n and not any(got[K * l:]), f"({lg}, {lc}) {name}: coefficients from K l up must be zero"
        if K * l <= 64:
            want = cm.interpolate_definition(cm.cell_points(lg, lc, ids), known)
            assert got[:K * l] == want, f"({lg}, {lc}) {name}: the route differs from Lagrange interpolation"
        # and the interpolant takes the known values on the known cells
        back = cm.cell_values(oracle, got, lc)
        assert cm.known_values(back, ids, lc) == known, f"({lg}, {lc}) {name}"


@pytest.mark.parametrize("lg,lc", SHAPES)
def test_recovers_a_low_degree_polynomial(oracle, lg, lc):
    n, l, r = cm.shape(lg, lc)
    for name, ids in id_sets(r, SEED + 200 + 16 * lg + lc).items():
        K = len(ids)
        f = cm.random_ints(SEED + 300 + lg, K * l)
        f[-1] = f[-1] or 1  # degree exactly K l - 1
        f += [0] * (n - K * l)
        known = cm.known_values(cm.cell_values(oracle, f, lc), ids, lc)
        assert cm.recover_route(oracle, ids, known, lg, lc) == f, f"({lg}, {lc}) {name}"


@pytest.mark.parametrize("lg,lc", SHAPES)
def test_z_identities_against_the_direct_product(lg, lc):
    """Z(w^i) = Zdom[i mod r] and Z(g w^i) = Zcos[i mod r] for every i < n; Zdom vanishes exactly on the missing cells, Zcos nowhere."""
    n, l, r = cm.shape(lg, lc)
    w = ci.root_of_unity(lg)
    for name, ids in id_sets(r, SEED + 400 + 16 * lg + lc).items():
        zdom, zcos = cm.z_tables(lg, lc, ids)
        for i in range(n):
            x = pow(w, i, R)
            assert cm.z_direct(lg, lc, ids, x) == zdom[i % r], f"({lg}, {lc}) {name}: Z(w^{i})"
            assert cm.z_direct(lg, lc, ids, cm.GEN * x % R) == zcos[i % r], f"({lg}, {lc}) {name}: Z(g w^{i})"
        assert [j for j in range(r) if zdom[j] == 0] == sorted(set(range(r)) - set(ids))
        assert all(zcos)
        if name == "all":
            assert zdom == [1] * r and zcos == [1] * r  # the empty product
    if r >= 2:  # missing = the even cells: Z = X^(n/2) - 1, which is (-1)^j - 1 on cell j
        zdom, zcos = cm.z_tables(lg, lc, list(range(1, r, 2)))
        assert zdom == [(pow(w, (j * (n // 2)) % n, R) - 1) % R for j in range(r)] == [0, R - 2] * (r // 2)
        gn2 = pow(cm.GEN, n // 2, R)
        assert zcos == [(gn2 * (1 if j % 2 == 0 else R - 1) - 1) % R for j in range(r)]


def test_cell_values_are_the_polynomial_on_the_cosets(oracle):
    lg, lc = 5, 2
    n, l, r = cm.shape(lg, lc)
    f = cm.random_ints(SEED + 500, n)
    w = ci.root_of_unity(lg)
    values = cm.cell_values(oracle, f, lc)
    for m in range(r):
        for t in range(l):
            x, acc = pow(w, m + r * t, R), 0
            for c in reversed(f):
                acc = (acc * x + c) % R
            assert values[m * l + t] == acc
    assert cm.unmont(cm.mont(values)) == values


def test_header_library_and_binding_list_the_new_symbols(pkg):
    text = open(os.path.join(ROOT, "include", "bbg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bbg_[a-z0-9_]+)\s*\(", code))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/bbg.h"
        assert sym in pkg.binding.EXPORTED_SYMBOLS, f"{sym} is missing from binding.EXPORTED_SYMBOLS"
    lib = pkg.load_library()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), f"{sym} is not exported by libbbg.so"


def test_binding_has_the_four_methods(pkg):
    for name in NEW_METHODS:
        assert callable(getattr(pkg.Bbg, name, None)), f"Bbg.{name} is missing"
