"""The wave-cooperative pairing product (csrc/pairing_wave.hip, csrc/fq12_wave.hip.h) without a GPU: its dataflow on integers
(tests/tools/pairing_wave_model.py) against the integer model of the reference's pairing, the lane schedule against the product it has to
form, and the four new symbols in the header and the binding."""
import os
import re

import numpy as np
import pytest

import pairing_model as pm
import pairing_wave_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["bbg_pairing_product_wave_device", "bbg_pairing_product_wave", "bbg_cells_verify_device", "bbg_cells_verify"]
NEW_METHODS = ["pairing_product_wave", "pairing_product_wave_device", "cells_verify", "cells_verify_device"]
B = [7, pm.R - 3, 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % pm.R]


def random_f12(seed):
    rng = np.random.default_rng(seed)
    v = [int.from_bytes(rng.bytes(40), "little") % pm.P for _ in range(12)]
    two = [(v[2 * i], v[2 * i + 1]) for i in range(6)]
    return (tuple(two[:3]), tuple(two[3:]))


@pytest.fixture(scope="module")
def tables():
    return [pm.precompute_miller_lines(pm.g2_mul(pm.G2, b)) for b in B]


def test_w_basis_is_the_reference_tower():
    x = random_f12(11)
    assert wm.from_w(wm.to_w(x)) == x
    assert [wm.ref_component(i) for i in range(6)] == [0, 3, 1, 4, 2, 5], "c0 = (a0, a2, a4), c1 = (a1, a3, a5)"
    # w itself is a_1 = 1, w^2 = v is a_2 = 1, and w^6 = xi
    w = (pm.F6_ZERO, pm.F6_ONE)
    assert wm.to_w(w) == [0, 0, 1, 0] + [0] * 8 and wm.to_w(pm.f12_sqr(w)) == [0] * 4 + [1, 0] + [0] * 6
    assert wm.to_w(pm.f12_pow(w, 6)) == list(pm.XI) + [0] * 10
    # a line (o, vw, vv) sits at w^0, w^3, w^4
    o, vw, vv = (3, 4), (5, 6), (7, 8)
    coeff = wm.to_w(((o, pm.F2_ZERO, vv), (pm.F2_ZERO, vw, pm.F2_ZERO)))
    assert coeff == [3, 4, 0, 0, 0, 0, 5, 6, 7, 8, 0, 0] and [wm.line_power(jj) for jj in range(3)] == [0, 3, 4]


@pytest.mark.parametrize("sparse", [False, True])
def test_lane_schedule_forms_every_term_once(sparse):
    powers = [0, 3, 4] if sparse else list(range(6))
    busy = [wm.product_lane(lane, sparse) for lane in range(wm.LANES)]
    formed = [(i, j) for i, _, j in filter(None, busy)]
    assert len(formed) == 6 * len(powers) <= wm.LANES and all(t is None for t in busy[len(formed):]), "the busy lanes are the first ones"
    assert sorted(formed) == sorted((i, j) for i in range(6) for j in powers), "every a_i b_j exactly once"
    assert all(j == (wm.line_power(jj) if sparse else jj) for _, jj, j in filter(None, busy))
    read = []
    for c in range(12):
        terms = wm.sum_terms(c, sparse)
        assert len(terms) == len(powers) and all(h == c & 1 for _, h in terms)
        for e, _ in terms:
            i, j = divmod(e, 6)
            assert (i, j) in formed and (i + j) % 6 == c >> 1, "a term of coefficient k has i + j = k mod 6"
        read += terms
    assert len(set(read)) == 12 * len(powers), "every half of every formed product is read exactly once"


def test_products_against_the_tower():
    x, y = random_f12(12), random_f12(13)
    w = wm.Wave()
    w.slot[1], w.slot[2] = wm.to_w(x), wm.to_w(y)
    w.mul(3, 1, w.slot[2], False)
    assert wm.from_w(w.slot[3]) == pm.f12_mul(x, y)
    w.mul(1, 1, w.slot[1], False)  # the result on top of both operands
    assert wm.from_w(w.slot[1]) == pm.f12_sqr(x)
    line = ((3, 4), (5, 6), (7, 8))
    w.slot[0] = wm.to_w(y)
    w.pt = [(11, 13)]
    w.scale_line(line, 0)
    w.mul(0, 0, w.line, True)
    assert wm.from_w(w.slot[0]) == pm.f12_sparse_mul(y, (line[0], pm.f2_mul_fq(line[1], 13), pm.f2_mul_fq(line[2], 11)))


def test_conj_frobenius_inverse_and_cyclotomic_square():
    x = random_f12(14)
    w = wm.Wave()
    w.slot[0] = wm.to_w(x)
    w.conj(1, 0)
    assert wm.from_w(w.slot[1]) == pm.f12_conj(x)
    for k in (1, 2, 3):
        w.frobenius(2, 0, k)
        assert wm.from_w(w.slot[2]) == pm.f12_frobenius(x, k), k
    w.inv(3, 0)
    assert wm.from_w(w.slot[3]) == pm.f12_inv(x)
    # OP_CSQR as the product of x with itself: the Granger-Scott square on the cyclotomic subgroup, where the program uses it
    u = pm.final_exponentiation_easy_part(x)
    w.slot[4] = wm.to_w(u)
    w.mul(4, 4, w.slot[4], False)
    assert wm.from_w(w.slot[4]) == pm.f12_cyclotomic_sqr(u)


def test_kernel_tables_are_the_generators():
    gen = wm._generator()
    assert wm.FINAL_PROGRAM == gen.final_exponentiation_program() and len(wm.FINAL_PROGRAM) == 295
    first, it = 0, 0
    for bit in pm.LOOP_BITS:
        first |= 1 << it
        it += 2 if bit else 1
    assert wm.LINE_OPENS_STEP == [(first >> (32 * i)) & 0xFFFFFFFF for i in range(3)]


@pytest.mark.parametrize("pairs", [1, 2, 3])
def test_model_pairing_is_the_reference_pairing(tables, pairs):
    scalars = [5, pm.R - 11, 0x123456789ABCDEF][:pairs]
    points = [pm.g1_mul(pm.G1, a) for a in scalars]
    value, status = wm.pairing_product(points, tables[:pairs])
    assert value == pm.reduced_ate_pairing_batch_precomputed(points, tables[:pairs]) and status == 0


def test_model_pairing_edges(tables):
    a = 0xABCDEF
    pa, pna = pm.g1_mul(pm.G1, a), pm.g1_mul(pm.G1, pm.R - a)
    same = [tables[0], tables[0]]
    assert wm.pairing_product([pa, pna], same) == (pm.F12_ONE, 1), "one by design"
    value, status = wm.pairing_product([pa, None, pna], tables)
    assert value == pm.reduced_ate_pairing_batch_precomputed([pa, None, pna], tables) and status == 0, "a pair at infinity is the factor one"
    assert wm.pairing_product([None, None, None], tables) == (pm.F12_ONE, 1), "every pair at infinity: one"
    assert wm.pairing_product([(pa[0], (pa[1] + 1) % pm.P), pna], same)[1] == 2, "a point off the curve"


def test_symbols_in_header_and_binding(pkg):
    header = open(os.path.join(ROOT, "include", "bbg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", code), f"{sym} is not declared in include/bbg.h"
        assert sym in pkg.binding.EXPORTED_SYMBOLS, f"{sym} is not in binding.EXPORTED_SYMBOLS"
    for method in NEW_METHODS:
        assert callable(getattr(pkg.Bbg, method, None)), f"Bbg.{method} is missing"
