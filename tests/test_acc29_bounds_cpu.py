"""The bounds of the bucket accumulation's mixed addition on 29-bit limbs (csrc/curve29.hip.h xyzz29_madd) after its sums moved into the
products: P = U2 - X1, R = S2 - Y1 and X3 = R^2 - PPP - 2Q are added in the high columns of the product that precedes them and leave
through its output masks, with no subtraction pass and no carry pass of their own.

tests/tools/acc29_model.py restates that sequence with Python integers.  Here it runs (a) against the oracle's field arithmetic on random
chains, negative digits included, (b) from accumulators with every limb at its stated maximum, through the `neg` path and with
coordinates next to p, and (c) as a pure bound computation: every product of the addition, all operand limbs at their maxima at once,
stays below 2^63 in every column."""
import math
import random

import numpy as np

import acc29_model as m
import coarse_inputs as ci

P = m.P


def _oracle_mul(oracle):
    """a * b / R' mod p through the oracle's Montgomery product (a * b / 2^256), for integer residues."""
    r_corr = pow(2, 256 - 261, P)  # a b / 2^261 = (a b / 2^256) * 2^-5

    def mul(a, b):
        w = oracle.fe_mul(1, ci.to_words([a % P]), ci.to_words([b % P]))
        return ci.to_ints(oracle.canon(1, w))[0] * r_corr % P
    return mul


def _check(acc, ref):
    for a, r in zip(acc, ref):
        assert m.val(a) % P == r


def _exit_bounds(acc):
    x3, y3, zz3, zzz3 = acc
    assert m.val(x3) < 21 * P and m.val(y3) < 8 * P and m.val(zz3) < 2 * P and m.val(zzz3) < 2 * P
    assert all(l <= m.M29 for c in acc for l in c[:8])  # exact limbs: every coordinate leaves a product's output masks


def test_model_against_oracle_field_arithmetic(oracle):
    assert ci.Q_MOD == P
    mul = _oracle_mul(oracle)
    a, b = 0x1234567 << 200 | 99, P - 5
    assert mul(a, b) == a * b * pow(m.R1, -1, P) % P
    rng = random.Random(0xACC29)
    for chain in range(6):
        px, py, ng = rng.randrange(1, P), rng.randrange(1, P), bool(rng.getrandbits(1))
        x2, y2 = m.aff_from_table(px, py, ng)
        acc = m.start(x2, y2)
        ref = [m.val(c) % P for c in acc]
        assert ref[1] == (-py if ng else py) * 32 % P
        for step in range(12):
            px, py, ng = rng.randrange(1, P), rng.randrange(1, P), bool(rng.getrandbits(1))
            if step % 4 == 1:
                py = P - 1 - rng.randrange(4)   # y next to p
            if step % 4 == 3:
                px, py = P - 1, 1 + rng.randrange(4)
            x2, y2 = m.aff_from_table(px, py, ng)
            acc, ref = m.madd(acc, x2, y2), m.madd_mod(ref, m.val(x2) % P, m.val(y2) % P, mul)
            _check(acc, ref)
            _exit_bounds(acc)


def test_long_chains_of_negative_digits():
    """Runs in which every digit is negative (y -> p - y on the table words), against plain modular arithmetic."""
    ri = pow(m.R1, -1, P)
    mul = lambda a, b: a * b * ri % P
    rng = random.Random(7)
    for chain in range(10):
        x2, y2 = m.aff_from_table(rng.randrange(1, P), rng.randrange(1, P), True)
        acc = m.start(x2, y2)
        ref = [m.val(c) % P for c in acc]
        for step in range(60):
            py = rng.choice([1, 2, P - 1, P - 2, rng.randrange(1, P)])
            x2, y2 = m.aff_from_table(rng.choice([0, 1, P - 1, rng.randrange(P)]), py, True)
            assert m.val(y2) == (P - py) << 5
            acc, ref = m.madd(acc, x2, y2), m.madd_mod(ref, m.val(x2) % P, m.val(y2) % P, mul)
            _check(acc, ref)
            _exit_bounds(acc)


def test_addition_from_every_limb_at_its_maximum():
    """Accumulators with all limbs at the header's entry maximum (2^29 + 7) and at the kernel's own (2^29 - 1), top limbs at the value
    bounds (X, Y < 32p, ZZ, ZZZ < 1.4p), against table points at the ends of the range, both signs."""
    ri = pow(m.R1, -1, P)
    mul = lambda a, b: a * b * ri % P
    x_top = ((32 * P) >> 232) - 2
    z_top = (14 * P // 10) >> 232
    for full in (m.M29 + 8, m.M29):
        acc = [[full] * 8 + [x_top], [full] * 8 + [x_top], [full] * 8 + [z_top], [full] * 8 + [z_top]]
        ref = [m.val(a) % P for a in acc]
        for px, py in ((P - 1, P - 1), (1, 1), (P - 1, 1), (0, P - 1), ((1 << 253) - 1, (1 << 253) + 12345)):
            for ng in (False, True):
                x2, y2 = m.aff_from_table(px, py, ng)
                out = m.madd(acc, x2, y2)
                _check(out, m.madd_mod(ref, m.val(x2) % P, m.val(y2) % P, mul))
                _exit_bounds(out)
                _check(m.madd(out, x2, y2), m.madd_mod([m.val(c) % P for c in out], m.val(x2) % P, m.val(y2) % P, mul))


def test_every_column_of_every_product_stays_below_2_63():
    bounds = m.madd_bounds()
    assert len(bounds) == 9  # 8M + 2S in nine reductions: Y3 is one double product
    for name, worst in bounds.items():
        print(f"{name:32s} largest column 2^{math.log2(worst):.3f}")
        assert worst < 1 << 63, name
    # the carry pass that stays: T = Q - X3 + 24p uncarried has limbs up to 2^29 + 2^30 + 2^29, and column 8 of Y3 leaves 63 bits
    t_raw = [m.M29 + s for s in m.spread(24, 30)[:8]] + [m.top(26.6)]
    assert m.column_max([(m.exact(35.3), t_raw), (m.spread(64, 30), m.exact(2.8))]) >= 1 << 63
    # and the one the issue proposed to drop on X3: uncarried limbs up to 2^29 + 2^31 + 2^29 against PP's exact ones in Q = X1 PP
    x_raw = [m.M29 + s for s in m.spread(12, 31)[:8]] + [m.top(20.4)]
    assert m.column_max([(x_raw, m.exact(8.4))]) >= 1 << 63
    # the model's own runs never came near the bound either
    assert m.STATS["max_column"] < 1 << 63
