"""CPU side of bbg_cells_verify_reduce (a batch of cell proofs reduced to the two points of one pairing check): the identity A_b = r g_b
the device's route stands on, proved on integers; the host model's two routes against each other; [x^l] L = R for honest batches and its
failure after every single corruption; and the new symbols in the header and the binding.  No GPU."""
import os
import re

import numpy as np
import pytest

import cells_model as cm
import cells_verify_model as vm
import open_all_model as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = cm.R_MOD
SEED = 0xBB254 + 0x7E81F
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
SHAPES = [(2, 1), (4, 2), (6, 3), (3, 0)]
NEW_SYMBOLS = ["bbg_cells_verify_reduce_device", "bbg_cells_verify_reduce"]
NEW_METHODS = ["cells_verify_reduce", "cells_verify_reduce_device"]


def some_cells(seed, r, ncom, K):
    """K (c, m) pairs with a duplicate pair, repeated cells, and (for K < r) cells nobody samples."""
    rng = np.random.default_rng(seed)
    cells = [(int(rng.integers(0, ncom)), int(rng.integers(0, r))) for _ in range(K)]
    if K >= 2:
        cells[-1] = cells[0]
    return cells


def batch(oracle, lg, lc, ncom, K, seed):
    n, l, r = cm.shape(lg, lc)
    polys = [cm.random_ints(seed + 7 * c, n) for c in range(ncom)]
    com, cids, mids, values, proofs = vm.honest_batch(oracle, polys, X_INT, lc, some_cells(seed + 1, r, ncom, K))
    srs = vm.scalar_times_generator(oracle, [pow(X_INT, j, R) for j in range(l)])
    return srs, com, cids, mids, values, proofs


# 1 ------------------------------------------------------------------------------------------------ A_b = r g_b
@pytest.mark.parametrize("lg,lc", SHAPES)
def test_interpolant_sum_is_r_times_the_low_block(lg, lc):
    n, l, r = cm.shape(lg, lc)
    for K in (1, 2, r, 2 * r + 1):
        rng = np.random.default_rng(SEED + 100 * lg + 10 * lc + K)
        mids = [int(rng.integers(0, r)) for _ in range(K)]  # duplicates and gaps as they fall
        values = cm.random_ints(SEED + 1 + 16 * lg + K, K * l)  # any values: no polynomial behind them
        rho = cm.random_ints(SEED + 2 + K, 1)[0]
        want = vm.interpolant_sum_definition(lg, lc, mids, values, rho)
        got, g = vm.interpolant_sum_route(lg, lc, mids, values, rho)
        assert got == want, f"({lg}, {lc}), K = {K}: r g_b differs from the sum of the Lagrange interpolants"
        # the step of the proof: g mod (X^l - phi^m) interpolates E on cell m, sampled or not
        E = vm.folded_values(lg, lc, mids, values, rho)
        for m in range(r):
            pts = cm.cell_points(lg, lc, [m])
            assert vm.cell_interpolant_from_blocks(g, lg, lc, m) == cm.interpolate_definition(pts, [E[m + r * t] for t in range(l)]), (lg, lc, K, m)
    if l == 1:  # the check the issue names: A_0 = sum_k rho^k v_k
        assert got == [sum(p * v for p, v in zip(vm.powers(rho, K), values)) % R]


def test_rho_zero_keeps_cell_zero_only():
    lg, lc = 4, 2
    n, l, r = cm.shape(lg, lc)
    mids, values = [3, 1, 3], cm.random_ints(SEED + 5, 3 * l)
    assert vm.powers(0, 3) == [1, 0, 0]
    assert vm.interpolant_sum_route(lg, lc, mids, values, 0)[0] == vm.interpolant_sum_definition(lg, lc, mids[:1], values[:l], 1)


# 2 ------------------------------------------------------------------------------------------------ the two routes, and the closed form
@pytest.mark.parametrize("lg,lc", SHAPES)
def test_routes_agree_and_honest_batches_verify(oracle, lg, lc):
    n, l, r = cm.shape(lg, lc)
    for ncom, K in ((1, 1), (2, 5), (3, r + 2)):
        srs, com, cids, mids, values, proofs = batch(oracle, lg, lc, ncom, K, SEED + 1000 * lg + 100 * lc + K)
        rho = cm.random_ints(SEED + 3 + K, 1)[0]
        L, R_ = vm.reduce_definition(oracle, srs, lg, lc, com, cids, mids, values, proofs, rho)
        L2, R2 = vm.reduce_route(oracle, srs, lg, lc, com, cids, mids, values, proofs, rho)
        assert np.array_equal(L, L2) and np.array_equal(R_, R2), f"({lg}, {lc}), ncom = {ncom}, K = {K}: the two routes differ"
        assert not oa.is_infinity(L) and vm.holds(oracle, L, R_, X_INT, lc), f"({lg}, {lc}), ncom = {ncom}, K = {K}: an honest batch must verify"


def corruptions(oracle, lg, lc, com, cids, mids, values, proofs):
    """{name: (com, cids, mids, values, proofs)} with exactly one thing changed."""
    n, l, r = cm.shape(lg, lc)
    other = vm.scalar_times_generator(oracle, [12345])[0]
    v2 = list(values)
    v2[l + 0] = (v2[l + 0] + 1) % R
    p2, c2 = proofs.copy(), com.copy()
    p2[1], c2[cids[2]] = other, other
    m2, i2 = list(mids), list(cids)
    m2[2] = (m2[2] + 1) % r
    i2[1] = (i2[1] + 1) % com.shape[0]
    return {"one value": (com, cids, mids, v2, proofs), "one proof": (com, cids, mids, values, p2), "one commitment": (c2, cids, mids, values, proofs),
            "one cell id": (com, cids, m2, values, proofs), "one commitment id": (com, i2, mids, values, proofs)}


@pytest.mark.parametrize("lg,lc", SHAPES)
def test_every_single_corruption_fails(oracle, lg, lc):
    srs, com, cids, mids, values, proofs = batch(oracle, lg, lc, 2, 4, SEED + 50 * lg + lc)
    rho = cm.random_ints(SEED + 4, 1)[0]
    for name, (a, b, c, d, e) in corruptions(oracle, lg, lc, com, cids, mids, values, proofs).items():
        L, R_ = vm.reduce_route(oracle, srs, lg, lc, a, b, c, d, e, rho)
        assert not vm.holds(oracle, L, R_, X_INT, lc), f"({lg}, {lc}): the batch verifies with {name} changed"


def test_cancellation_and_infinities(oracle):
    lg, lc = 4, 2
    n, l, r = cm.shape(lg, lc)
    srs, com, cids, mids, values, proofs = batch(oracle, lg, lc, 1, 1, SEED + 9)
    twice = (com, cids * 2, mids * 2, values * 2, np.concatenate([proofs, proofs]))
    L, R_ = vm.reduce_route(oracle, srs, lg, lc, *twice, R - 1)  # rho = -1: the two copies cancel
    assert oa.is_infinity(L) and oa.is_infinity(R_)
    # a polynomial of degree < l: every proof is infinity, and L is
    low = cm.random_ints(SEED + 10, l) + [0] * (n - l)
    com, cids, mids, values, proofs = vm.honest_batch(oracle, [low], X_INT, lc, [(0, 1), (0, 2)])
    assert all(oa.is_infinity(p) for p in proofs)
    L, R_ = vm.reduce_definition(oracle, srs, lg, lc, com, cids, mids, values, proofs, 77)
    assert oa.is_infinity(L) and oa.is_infinity(R_), "C - [I] = infinity for every cell of a polynomial of degree < l"


# 3 ------------------------------------------------------------------------------------------------ header, binding
def test_header_and_binding_have_the_new_entry_points(pkg):
    with open(os.path.join(ROOT, "include", "bbg.h")) as f:
        header = f.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} is not declared in include/bbg.h"
        assert sym in pkg.binding.EXPORTED_SYMBOLS, f"{sym} is not in binding.EXPORTED_SYMBOLS"
    for name in NEW_METHODS:
        assert callable(getattr(pkg.Bbg, name, None)), f"Bbg.{name} is missing"
    assert "This library does not verify" not in header
    for scope in ("cells_verify_powers", "cells_verify_fold", "cells_verify_mul", "cells_verify_segsum", "cells_verify_phi", "cells_verify_finish"):
        assert f'"{scope}"' in header, f"profile name {scope} is not documented in include/bbg.h"
