"""Operand vectors and expected result rows for bbg_limb29_op (csrc/limb29_check.hip): the device primitives of the 29-bit-limb arithmetic
against the integer models, on the same raw limbs (test tooling for tests/test_limb29_vectors_cpu.py and tests/test_gpu_limb29.py).

For every op of the harness this module holds
  * the op number, operand and result row counts (restating BBG_L29_OPS / BBG_L29_PAIRS of csrc/limb29_check.hip; the GPU test compares them
    with bbg_limb29_op_shape);
  * a MODEL: the op computed limb by limb with Python integers, asserting on every overflow, negative limb and stated bound.  Where the
    suite already has one it is imported from where it lives -- tests/test_limb29_model.py (Fq), tests/test_ntt29_model.py (Fr),
    tests/tools/acc29_model.py (the ADD / Z0 jobs and the mixed addition), tests/test_w29_model.py (up / dot).  Those are written for one
    field each, so the same statements, field as a parameter, are restated in class Field below (with the models the suite lacked: f29_norm,
    f29_to_fe, f29_div32_to_fe, f29_mul_ilp, xyzz29_finish); every vector goes through BOTH and the rows must agree;
  * a CHECK: the op's residue identity and value bound with plain % arithmetic on val() of the operands, not through the model;
  * deterministic VECTORS: the corners of the op's contract as its header comment states them, the values 0, 1, p - 1, p, 2p - 1 and the
    entry bound minus 1, both sides of every row boundary of the table-driven ops, and at most 512 random vectors inside the contract.

A row is 9 words.  A limb value uses all nine; an 8 x u32 field element uses words 0..7 (32-bit words), word 8 is 0."""
import itertools
import os
import random
import sys

_TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _TESTS not in sys.path:
    sys.path.insert(0, _TESTS)

import acc29_model as accm  # noqa: E402
import test_limb29_model as fqm  # noqa: E402
import test_ntt29_model as nttm  # noqa: E402
import test_w29_model as w29m  # noqa: E402

M29 = (1 << 29) - 1
R1 = 1 << 261
U32, U64 = 1 << 32, 1 << 64
FR, FQ = 0, 1
N_RANDOM = 192  # per op (the issue allows 512)

# the (M, E) pairs of f29_sub (op 100 + i), f29_neg (200 + i), n29_bfly (300 + i): BBG_L29_PAIRS of csrc/limb29_check.hip.
PAIRS = [(3, 30), (4, 30), (6, 30), (7, 30), (7, 31), (13, 30), (12, 31), (24, 30), (34, 30), (64, 30), (65, 30), (52, 30)]
# Template argument lists of f29_sub / f29_neg / n29_bfly that the sources give by a constant expression instead of literals, and the pairs each
# stands for (listed by hand; the CPU test finds the literal lists itself and requires every other spelling it meets to be a key here).
TEMPLATE_EXPRESSIONS = {
    "KB, E": [],         # n29_bfly's own parameters, handed to f29_sub (ntt29.hip.h)
    "K, E": [],          # f29_neg's own parameters, handed to f29_sub (field29.hip.h)
    "Pr::M, Pr::E": [],  # the conformance kernels themselves (limb29_check.hip): the pairs of this table
    "M::KP": [(3, 30), (4, 30)],   # N29M<0>::KP = 3, N29M<1>::KP = N29M<2>::KP = 4 (ntt29.hip.h)
    "M::KPP": [(4, 30), (6, 30)],  # N29M<0>::KPP = 4, N29M<1>::KPP = 6
    # w29::sub: M = (B::vq + 63) / 64 + 1, E = max(30, bitlen(B::lm + 1)) of the subtrahend's type.  The pairs the widget kernels of
    # quotient29.hip.h instantiate, read off tests/test_w29_model.py's sub() while it evaluates those kernels: a class-0 load (3), a
    # product (4), the permutation widget's denominators (7), dbl(e) of the logic widget (52), a class-1 load (65)
    "M, E": [(3, 30), (4, 30), (7, 30), (52, 30), (65, 30)],
}


def limbs(v):
    assert 0 <= v < (1 << (29 * 8 + 32))
    return [(v >> (29 * j)) & M29 for j in range(8)] + [v >> 232]


def val(a):
    return sum(x << (29 * i) for i, x in enumerate(a))


def fe_val(row):  # 8 x u32 words
    assert row[8] == 0 and all(0 <= w < U32 for w in row)
    return sum(w << (32 * i) for i, w in enumerate(row[:8]))


def fe_row(v):
    assert 0 <= v < (1 << 256)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0]


STATS = {"max_column": 0, "rows": set()}  # what the model run of the current vector reached (reset per vector by build())


class Field:
    """The limb arithmetic of csrc/field29.hip.h for the field with modulus p: the statements of tests/test_limb29_model.py and
    tests/tools/acc29_model.py with the field as a parameter, plus the operations those lack."""

    def __init__(self, p):
        self.p = p
        self.inv29 = (-pow(p, -1, 1 << 29)) % (1 << 29)
        self.p29 = limbs(p)
        self.ninv5 = (-pow(p, -1, 32)) % 32
        self.one = limbs(R1 % p)

    def from_fe(self, x, shift):  # f29_from_fe<P, S>
        assert 0 <= x < (1 << 256)
        return limbs(x << shift)

    def carry(self, a):  # f29_carry
        assert all(0 <= x < U32 for x in a)
        r = [a[0] & M29] + [(a[i] & M29) + (a[i - 1] >> 29) for i in range(1, 8)] + [a[8] + (a[7] >> 29)]
        assert all(x < U32 for x in r) and val(r) == val(a)
        assert max(r[:8]) < (1 << 29) + 8
        return r

    def norm(self, a):  # f29_norm: sequential carries, exact limbs
        assert all(0 <= x < U32 for x in a)
        r, c = [], 0
        for i in range(8):
            t = a[i] + c
            assert t < U32, "limb overflow in f29_norm"
            r.append(t & M29)
            c = t >> 29
        assert a[8] + c < U32, "top limb overflow in f29_norm"
        r.append(a[8] + c)
        assert val(r) == val(a) and max(r[:8]) <= M29
        return r

    def to_fe(self, a):  # f29_to_fe: the 8 words of a value < 2^256
        v = val(self.norm(a))
        assert v < (1 << 256), "f29_to_fe of a value that does not fit 8 words"
        return v

    def div32_to_fe(self, a):  # f29_div32_to_fe: (x + m p) / 32 with m = -x / p mod 32 from the table of the 32 multiples of p
        assert val(a) < R1 - 31 * self.p
        m = (a[0] * self.ninv5) & 31
        STATS["rows"].add(m)
        row = limbs(m * self.p)
        assert row[8] < (1 << 27) and max(row[:8]) <= M29
        t = [x + y for x, y in zip(a, row)]
        assert all(x < U32 for x in t), "limb overflow adding the table row"
        n = self.norm(t)
        tv = val(n)
        assert tv % 32 == 0 and tv >> 5 < (1 << 256)
        return tv >> 5

    def add(self, a, b):  # f29_add
        r = [x + y for x, y in zip(a, b)]
        assert all(x < U32 for x in r), "limb overflow in f29_add"
        return r

    def spread(self, mult, e):  # Spread29<P, J, M, E>
        q = limbs(mult * self.p)
        up, down = 1 << e, 1 << (e - 29)
        s = [q[0] + up] + [q[j] + up - down for j in range(1, 8)] + [q[8] - down]
        assert val(s) == mult * self.p and s[8] >= 0 and all(x < U32 for x in s)
        return s

    def sub(self, a, b, mult, e=30):  # f29_sub<M, E>
        r = []
        for x, y, c in zip(a, b, self.spread(mult, e)):
            assert c - y >= 0, "subtrahend limb above the spread constant"
            assert x + (c - y) < U32, "limb overflow in f29_sub"
            r.append(x + (c - y))
        assert val(r) == val(a) - val(b) + mult * self.p
        return r

    def neg(self, b, mult, e=30):  # f29_neg<M, E>
        return self.sub([0] * 9, b, mult, e)

    def mont(self, chains, add=None, limit=U64):
        """Product scanning over 29-bit limbs: one reduction over the sum of a * b of all chains; add: 9 limbs added to the result through
        columns 9 .. 16 and the top limb (F29Job ADD).  limit: 2^64 for the plain products (v_mad_u64_u32 wraps there), 2^63 for the
        accumulation's jobs (acc29_model.COLUMN_LIMIT: their contract keeps one bit in hand)."""
        acc, m, r = 0, [0] * 9, [0] * 9
        for a, b in chains:
            assert all(0 <= x < U32 for x in a + b)
        for k in range(17):
            lo, hi = max(0, k - 8), min(k, 8)
            for a, b in chains:
                acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
            if add is not None and k >= 9:
                assert 0 <= add[k - 9] < U32
                acc += add[k - 9]
            acc += sum(m[i] * self.p29[k - i] for i in range(lo, hi + 1 if k > 8 else k))
            if k <= 8:
                m[k] = ((acc & 0xFFFFFFFF) * self.inv29) & M29
                acc += m[k] * self.p29[0]
                assert acc & M29 == 0
            else:
                r[k - 9] = acc & M29
            STATS["max_column"] = max(STATS["max_column"], acc)
            assert acc < limit, "column sum overflow"
            acc >>= 29
        r[8] = acc + (add[8] if add is not None else 0)
        assert r[8] < U32, "top limb overflow"
        want = sum(val(a) * val(b) for a, b in chains)
        extra = val(add) if add is not None else 0
        assert (val(r) * R1 - want - extra * R1) % self.p == 0 and val(r) < want // R1 + self.p + 1 + extra
        return r

    def mul_ilp(self, a, b):
        """f29_mul_ilp: every column in an accumulator of its own, the nine digit steps add m p to nine columns each; same columns and
        digits as f29_mul, but the sums that must fit 64 bits are the per-column ones (a column's a b terms + its m p terms, without the
        carried-in value, which joins only in the digit chain)."""
        t = [sum(a[i] * b[k - i] for i in range(9) if 0 <= k - i <= 8) for k in range(17)]
        assert all(x < U64 for x in t)
        STATS["max_column"] = max(STATS["max_column"], max(t))
        cy = 0
        for i in range(9):
            ti = t[i] + cy
            assert ti < U64, "column overflow (digit chain)"
            m = ((ti & 0xFFFFFFFF) * self.inv29) & M29
            s = ti + m * self.p29[0]
            assert s < U64 and s & M29 == 0
            STATS["max_column"] = max(STATS["max_column"], s)
            cy = s >> 29
            for j in range(1, 9):
                t[i + j] += m * self.p29[j]
                assert t[i + j] < U64, "column overflow (m p)"
        r = []
        for k in range(8):
            v = t[9 + k] + cy
            assert v < U64, "column overflow (result chain)"
            STATS["max_column"] = max(STATS["max_column"], v)
            r.append(v & M29)
            cy = v >> 29
        assert cy < U32
        r.append(cy)
        assert (val(r) * R1 - val(a) * val(b)) % self.p == 0 and val(r) < val(a) * val(b) // R1 + self.p + 1
        return r

    def doubled(self, a):  # the doubled operand of the squares (a.v[i] << 1 in 32 bits)
        assert all(2 * x < U32 for x in a), "doubled operand leaves 32 bits"

    def sqr(self, a, limit=U64):
        self.doubled(a)
        return self.mont([(a, a)], limit=limit)

    def mul_sub2(self, a, b, c, d, limit=U64):  # a b + (64p - c) d
        r = self.mont([(a, b), (self.neg(c, 64, 30), d)], limit=limit)
        assert (val(r) * R1 - (val(a) * val(b) - val(c) * val(d))) % self.p == 0
        return r

    # ---- the mixed addition of the bucket accumulation (curve29.hip.h), as tests/tools/acc29_model.py states it
    def madd(self, acc, x2, y2):
        lim = accm.COLUMN_LIMIT
        x1, y1, zz1, zzz1 = acc
        p_ = self.mont([(x2, zz1)], self.neg(x1, 34), lim)
        r_ = self.mont([(y2, zzz1)], self.neg(y1, 34), lim)
        pp = self.sqr(p_, lim)
        ppp, q = self.mont([(p_, pp)], limit=lim), self.mont([(x1, pp)], limit=lim)
        s = [a + 2 * b for a, b in zip(ppp, q)]
        self.doubled(r_)
        x3 = self.mont([(r_, r_)], self.neg(s, 12, 31), lim)
        zz3 = self.mont([(zz1, pp)], limit=lim)
        t = self.carry(self.sub(q, x3, 24))
        y3 = self.mont([(r_, t), (self.neg(y1, 64, 30), ppp)], limit=lim)
        zzz3 = self.mont([(zzz1, ppp)], limit=lim)
        return [x3, y3, zz3, zzz3]

    def finish(self, acc):  # xyzz29_finish: four conversions and the flag "ZZ is not a multiple of p"
        out = [self.div32_to_fe(a) for a in acc]
        for v in out:
            assert v < 2 * self.p  # fe_is_zero reduces once
        return out, 1 if out[2] % self.p else 0


FIELDS = {FR: Field(nttm.P), FQ: Field(fqm.P)}
assert accm.P == fqm.P and w29m.P == nttm.P


# ---------------------------------------------------------------------------------------------- operand domains
class Lz:
    """Lazily reduced limb values: value < vmult * p, limbs below the top <= lmax."""

    def __init__(self, vmult, lmax=M29, vmin=0, extra=()):
        self.vmult, self.lmax, self.vmin, self.extra = vmult, lmax, vmin, list(extra)

    def topmax(self, f, low):  # largest top limb that keeps [low] * 8 + [top] below the value bound
        return (self.vmult * f.p - 1 - val([low] * 8 + [0])) >> 232

    def fat(self, f):  # every limb below the top at the largest allowed value, the top limb at the value bound
        t = self.topmax(f, self.lmax)
        return [[self.lmax] * 8 + [t]] if t >= 0 else [limbs(self.vmult * f.p - 1)]

    def corners(self, f):
        p, bound = f.p, self.vmult * f.p
        out = [limbs(v) for v in (0, 1, p - 1, p, 2 * p - 1, bound - 1) if self.vmin <= v < bound]
        t = self.topmax(f, self.lmax)
        if t >= 0:
            out.append([self.lmax] * 8 + [t])      # every limb below the top at the largest allowed value, the top limb at the value bound
            out.append([self.lmax] * 8 + [0])
            out.append([self.lmax - 1, self.lmax] * 4 + [t])
        out.append([0] * 8 + [(bound - 1) >> 232])  # the top limb at the value bound on its own
        out = [a for a in out if self.vmin <= val(a) < bound]
        return out + [list(a) for a in self.extra]

    def rand(self, f, rng):
        bound = self.vmult * f.p
        while True:
            if rng.random() < 0.5:
                a = limbs(rng.randrange(self.vmin, bound))
                if self.lmax > M29:  # move weight down: a limb just over 29 bits, as a carry pass leaves it
                    k = rng.randrange(8)
                    c = min(a[k + 1], (self.lmax - a[k]) >> 29, rng.randrange(1, 8))
                    a[k + 1] -= c
                    a[k] += c << 29
            else:
                a = [rng.randrange(self.lmax + 1) for _ in range(8)] + [rng.randrange(max(1, self.topmax(f, self.lmax) + 1))]
            if self.vmin <= val(a) < bound and max(a[:8]) <= self.lmax:
                return a


class FeDom:
    """8 x u32 field elements below bound (an integer)"""

    def __init__(self, bound_of, extra_of=lambda p: ()):
        self.bound_of, self.extra_of = bound_of, extra_of

    def corners(self, f):
        p, bound = f.p, self.bound_of(f.p)
        vs = [0, 1, p - 1, p, 2 * p - 1, bound - 1] + list(self.extra_of(p))
        return [fe_row(v) for v in dict.fromkeys(vs) if 0 <= v < bound]

    def rand(self, f, rng):
        return fe_row(rng.randrange(self.bound_of(f.p)))


class Fixed:
    """an operand domain given by explicit rows"""

    def __init__(self, rows_of, rand_of):
        self.rows_of, self.rand_of = rows_of, rand_of

    def corners(self, f):
        return [list(r) for r in self.rows_of(f)]

    def rand(self, f, rng):
        return list(self.rand_of(f, rng))


CARRIED = M29 + 8  # the largest limb f29_carry leaves


# ---------------------------------------------------------------------------------------------- the ops
class Op:
    def __init__(self, op, name, fields, nin, nout, model, check, regimes, **flags):
        self.op, self.name, self.fields, self.nin, self.nout = op, name, fields, nin, nout
        self.model, self.check, self.regimes, self.flags = model, check, regimes, flags


OPS = {}


def _op(op, name, fields, nin, nout, model, check, regimes, **flags):
    assert op not in OPS
    OPS[op] = Op(op, name, fields, nin, nout, model, check, regimes, **flags)


BOTH = (FR, FQ)


def _residue(f, got, want_times_r1):
    """val(result) * R' == want (mod p)"""
    assert (val(got) * R1 - want_times_r1) % f.p == 0, "residue"


# ---- representation
_any256 = FeDom(lambda p: 1 << 256, lambda p: ((1 << 255), (1 << 256) - (1 << 29), 0x1FFFFFFF, 0xFFFFFFFF))
_op(0, "f29_from_fe<P,0>", BOTH, 1, 1, lambda f, a: [f.from_fe(fe_val(a[0]), 0)],
    lambda f, a, r: _assert(val(r[0]) == fe_val(a[0]) and max(r[0]) <= M29), [(_any256,)])
_op(1, "f29_from_fe<P,5>", BOTH, 1, 1, lambda f, a: [f.from_fe(fe_val(a[0]), 5)],
    lambda f, a, r: _assert(val(r[0]) == fe_val(a[0]) << 5 and max(r[0]) <= M29), [(_any256,)])


def _assert(cond):
    assert cond


# f29_carry: "limbs < 2^32 in": every limb at 2^32 - 1 below the top, the top limb with room for the carry into it
_lz_any32 = Lz(1 << 6, U32 - 1, extra=[[U32 - 1] * 8 + [U32 - 8], [U32 - 1] * 8 + [0], [M29] * 8 + [7]])
_op(2, "f29_carry", BOTH, 1, 1, lambda f, a: [f.carry(a[0])],
    lambda f, a, r: _assert(val(r[0]) == val(a[0]) and max(r[0][:8]) < (1 << 29) + 8), [(_lz_any32,)])
# f29_norm: sequential carries; a limb plus the carry into it must stay below 2^32
_lz_norm = Lz(1 << 6, U32 - 8, extra=[[U32 - 8] * 8 + [U32 - 8], [M29, M29 + 1] * 4 + [5], [M29] * 8 + [0], [1] + [M29] * 7 + [0]])
_op(3, "f29_norm", BOTH, 1, 1, lambda f, a: [f.norm(a[0])],
    lambda f, a, r: _assert(val(r[0]) == val(a[0]) and max(r[0][:8]) <= M29), [(_lz_norm,)])
# f29_to_fe: any lazily reduced value below 2^256
_lz_fe = Fixed(lambda f: [limbs(v) for v in (0, 1, f.p - 1, f.p, 2 * f.p - 1, (1 << 256) - 1)]
               + [[CARRIED] * 8 + [(1 << 24) - 2], [U32 - 8] * 8 + [0], [M29, M29 + 1] * 4 + [5]],
               lambda f, rng: Lz(4, CARRIED).rand(f, rng))
_op(4, "f29_to_fe", BOTH, 1, 1, lambda f, a: [fe_row(f.to_fe(a[0]))],
    lambda f, a, r: _assert(fe_val(r[0]) == val(a[0])), [(_lz_fe,)])


def _div32_rows(f):
    # all 32 five-bit digits (m = a[0] * ninv5 mod 32: the low five bits of limb 0 run through every value), small and at the stated bound
    # (input < 2^261 - 31p; the result must also fit 8 words: (x + 31p) / 32 < 2^256), exact and carried limbs
    out = []
    hi = min(R1 - 31 * f.p, (1 << 261) - 31 * f.p) - 1
    for d in range(32):
        out.append(limbs(d))
        out.append(limbs(hi - 32 - d))
        out.append([CARRIED - 31 + d] + [CARRIED] * 7 + [Lz(21, CARRIED).topmax(f, CARRIED)])
    return out + [limbs(v) for v in (f.p - 1, f.p, 2 * f.p - 1, 21 * f.p - 1, 32 * f.p - 1)]


_lz_div32 = Fixed(_div32_rows, lambda f, rng: Lz(32, CARRIED).rand(f, rng))
_op(5, "f29_div32_to_fe", BOTH, 1, 1, lambda f, a: [fe_row(f.div32_to_fe(a[0]))],
    lambda f, a, r: _assert((fe_val(r[0]) * 32 - val(a[0])) % f.p == 0 and fe_val(r[0]) * 32 < val(a[0]) + 32 * f.p), [(_lz_div32,)], table=32)
_lz_half = Lz(1 << 5, (1 << 31) - 1, extra=[[(1 << 31) - 1] * 9])
_lz_half2 = Lz(1 << 5, 1 << 31, extra=[[1 << 31] * 9])
_op(6, "f29_add", BOTH, 2, 1, lambda f, a: [f.add(a[0], a[1])],
    lambda f, a, r: _assert(val(r[0]) == val(a[0]) + val(a[1])), [(_lz_half, _lz_half2)])


def _up_model(f, a):
    x = a[0]
    w = w29m.W(x, 0, 31 * 64, U32 - 1, val(x) * pow(w29m.R, -1, f.p))
    return [w29m.up(w).l]


# w29::up: class 0 -> class 1, any lazy limbs, top limb below 2^27 (value below 31p here)
_lz_up = Lz(31, U32 - 1, extra=[[U32 - 1] * 8 + [0], [(1 << 24) - 1] * 9, [1 << 24] * 9, [(1 << 29) - 1] * 8 + [(1 << 26)]])
_op(7, "w29::up", (FR,), 1, 1, _up_model, lambda f, a, r: _assert(val(r[0]) == 32 * val(a[0]) and max(r[0][:8]) <= M29 + 256), [(_lz_up,)])

# ---- products.  f29_mul: bitlen(a limbs) + bitlen(b limbs) <= 60, all nine limbs (the top one is a limb of the columns like the others)
_E30 = (1 << 30) - 1
_E31 = (1 << 31) - 1
_lz30 = Lz(64, _E30, extra=[[_E30] * 9])
_lz31 = Lz(64, _E31, extra=[[_E31] * 8 + [M29]])
_lz29 = Lz(64, M29, extra=[[M29] * 9])
_lzc = Lz(32, CARRIED)
_MUL_REGIMES = [(_lz30, _lz30), (_lz31, _lz29), (_lz29, _lz31), (_lzc, _lzc)]


def _chk_mul(f, a, r):
    _residue(f, r[0], val(a[0]) * val(a[1]))
    assert val(r[0]) < val(a[0]) * val(a[1]) // R1 + f.p + 1 and max(r[0][:8]) <= M29


def _chk_sqr(f, a, r):
    _residue(f, r[0], val(a[0]) ** 2)
    assert val(r[0]) < val(a[0]) ** 2 // R1 + f.p + 1 and max(r[0][:8]) <= M29


def _chk_mul_sub2(f, a, r, at=0):
    va, vb, vc, vd = (val(x) for x in a[:4])
    _residue(f, r[at], va * vb - vc * vd)
    assert val(r[at]) < (va * vb + (64 * f.p - vc) * vd) // R1 + f.p + 1 and max(r[at][:8]) <= M29


_op(10, "f29_mul", BOTH, 2, 1, lambda f, a: [f.mont([(a[0], a[1])])], _chk_mul, _MUL_REGIMES, bit63=True)
# f29_sqr: the doubled operand must fit 32 bits and 9 L^2 + 9 2^58 < 2^64: limbs < 2^30
_op(11, "f29_sqr", BOTH, 1, 1, lambda f, a: [f.sqr(a[0])], _chk_sqr, [(_lz30,), (_lzc,)], bit63=True)
# f29_mul_sub2(a, b, c, d): c limbs <= 2^30 - 2, c < 63p, d carried; a b columns beside 9 * 2^60 + 9 * 2^58: bitlen(a) + bitlen(b) <= 59
_lz_c63 = Lz(63, (1 << 30) - 2)
_MS2_REGIMES = [(_lz30, _lz29, _lz_c63, _lzc), (_lz29, _lz30, _lz_c63, _lzc), (Lz(36, CARRIED), Lz(27, CARRIED), Lz(32, CARRIED), Lz(3, M29))]
_op(12, "f29_mul_sub2", BOTH, 4, 1, lambda f, a: [f.mul_sub2(*a)], _chk_mul_sub2, _MS2_REGIMES, bit63=True)
_op(13, "f29_mul_ilp", BOTH, 2, 1, lambda f, a: [f.mul_ilp(a[0], a[1])], _chk_mul, _MUL_REGIMES, bit63=True)

# fe_mul29 / fe_mul29_ilp: 8 x u32 operands < 2p, or < 4p and < p (field.hip.h fe_mul's contract); result a b / 2^256 < 1.76p as 8 words
_fe2p = FeDom(lambda p: 2 * p)
_fe4p = FeDom(lambda p: 4 * p)
_fe1p = FeDom(lambda p: p)


def _fe_mul_model(ilp):
    def model(f, a):
        x, y = f.from_fe(fe_val(a[0]), 5), f.from_fe(fe_val(a[1]), 0)
        return [fe_row(f.to_fe(f.mul_ilp(x, y) if ilp else f.mont([(x, y)])))]
    return model


def _chk_fe_mul(f, a, r):
    va, vb, vr = fe_val(a[0]), fe_val(a[1]), fe_val(r[0])
    assert (vr * (1 << 256) - va * vb) % f.p == 0 and vr * 100 < 176 * f.p


_op(14, "fe_mul29", BOTH, 2, 1, _fe_mul_model(False), _chk_fe_mul, [(_fe2p, _fe2p), (_fe4p, _fe1p)])
_op(15, "fe_mul29_ilp", BOTH, 2, 1, _fe_mul_model(True), _chk_fe_mul, [(_fe2p, _fe2p), (_fe4p, _fe1p)])


def _pair(regs1, regs2):
    return [r1 + r2 for r1, r2 in zip(regs1, itertools.cycle(regs2))]


def _chk_pair(c1, n1, c2):
    def check(f, a, r):
        c1(f, a[:n1], [r[0]])
        c2(f, a[n1:], [r[1]])
    return check


# the interleaved pairs: both results must be what the single-product models give
_op(16, "f29_mul2", BOTH, 4, 2, lambda f, a: [f.mont([(a[0], a[1])]), f.mont([(a[2], a[3])])], _chk_pair(_chk_mul, 2, _chk_mul),
    _pair(_MUL_REGIMES, _MUL_REGIMES[1:] + _MUL_REGIMES[:1]), bit63=True)
_op(17, "f29_sqr2", BOTH, 2, 2, lambda f, a: [f.sqr(a[0]), f.sqr(a[1])], _chk_pair(_chk_sqr, 1, _chk_sqr), [(_lz30, _lzc), (_lzc, _lz30), (_lz30, _lz30)],
    bit63=True)
_op(18, "f29_mul_sub2_mul", BOTH, 6, 2, lambda f, a: [f.mul_sub2(*a[:4]), f.mont([(a[4], a[5])])], _chk_pair(_chk_mul_sub2, 4, _chk_mul),
    _pair(_MS2_REGIMES, _MUL_REGIMES), bit63=True)

# ---- the accumulation's Z0 / ADD jobs: the same products, their contract keeps every column below 2^63 (acc29_model.COLUMN_LIMIT).
# Operand bounds as xyzz29_madd uses them (curve29.hip.h): a table coordinate exact < 32p, ZZ / ZZZ carried < 1.4p (2p here), X1 / Y1
# carried < 32p, P / R exact < 36p, PP exact < 9p, T carried < 27p, PPP exact < 3p; the addends f29_neg<34>(carried < 32p): limbs < 2^31,
# f29_neg<12, 31>(s) with s = PPP + 2 Q < 8p, limbs < 3 * 2^29: limbs < 2^31 + 2^29.
LIM63 = accm.COLUMN_LIMIT
_x32, _x32c, _zz, _pr, _pp, _t27, _ppp = Lz(32, M29), Lz(32, CARRIED), Lz(2, CARRIED), Lz(36, M29), Lz(9, M29), Lz(27, CARRIED), Lz(3, M29)


def _neg_dom(src, mult, e):
    """the addend of an ADD job: f29_neg<mult, e> of every corner / random value of src"""
    return Fixed(lambda f: [f.neg(a, mult, e) for a in src.corners(f)], lambda f, rng: f.neg(src.rand(f, rng), mult, e))


_nx34 = _neg_dom(_x32c, 34, 30)
_s8 = Lz(8, 3 * M29)
_ns12 = _neg_dom(_s8, 12, 31)
_Z_REGIMES = [(_x32, _zz, _x32, _zz), (_pr, _pp, _x32c, _pp), (_zz, _pp, _zz, _ppp)]


def _chk_mul_add(f, a, r, at=0):
    va, vb, vd = val(a[0]), val(a[1]), val(a[2])
    _residue(f, r[at], va * vb + vd * R1)
    assert val(r[at]) < va * vb // R1 + f.p + 1 + vd and max(r[at][:8]) <= M29


def _chk_mul2_add(f, a, r):
    _chk_mul_add(f, a[:3], r, 0)
    _chk_mul_add(f, a[3:], r, 1)


def _chk_sqr_add_mul(f, a, r):
    _chk_mul_add(f, [a[0], a[0], a[1]], r, 0)
    _chk_mul(f, a[2:], [r[1]])


_op(19, "f29_mul2_z", BOTH, 4, 2, lambda f, a: [f.mont([(a[0], a[1])], limit=LIM63), f.mont([(a[2], a[3])], limit=LIM63)],
    _chk_pair(_chk_mul, 2, _chk_mul), _Z_REGIMES, acc_job=True)
_op(20, "f29_mul2_add", BOTH, 6, 2, lambda f, a: [f.mont([(a[0], a[1])], a[2], LIM63), f.mont([(a[3], a[4])], a[5], LIM63)], _chk_mul2_add,
    [(_x32, _zz, _nx34, _x32, _zz, _nx34), (_x32, _zz, _ns12, _pr, _pp, _nx34), (_pr, _pp, _nx34, _x32, _zz, _ns12)], acc_job=True, bit31=(2, 5))
_op(21, "f29_sqr_add_mul", BOTH, 4, 2, lambda f, a: [(f.doubled(a[0]), f.mont([(a[0], a[0])], a[1], LIM63))[1], f.mont([(a[2], a[3])], limit=LIM63)],
    _chk_sqr_add_mul, [(_pr, _ns12, _zz, _pp), (_pr, _nx34, _x32c, _pp)], acc_job=True, bit31=(1,))
_op(22, "f29_mul_sub2_mul_z", BOTH, 6, 2, lambda f, a: [f.mul_sub2(*a[:4], limit=LIM63), f.mont([(a[4], a[5])], limit=LIM63)],
    _chk_pair(_chk_mul_sub2, 4, _chk_mul), [(_pr, _t27, _x32c, _ppp, _zz, _ppp)], acc_job=True)
_op(23, "f29_sqr_z", BOTH, 1, 1, lambda f, a: [f.sqr(a[0], LIM63)], _chk_sqr, [(_pr,), (Lz(36, CARRIED),)], acc_job=True)


# ---- accumulation, Fq
_fe_x = FeDom(lambda p: p, lambda p: (p - 2, (1 << 253) - 1, (1 << 253) + 12345))
_fe_y = Fixed(lambda f: [fe_row(v) for v in (1, 2, f.p - 1, f.p - 2, (1 << 253) - 1, (1 << 253) + 12345)], lambda f, rng: fe_row(rng.randrange(1, f.p)))


def _aff_model(negative):
    def model(f, a):
        x, y = accm.aff_from_table(fe_val(a[0]), fe_val(a[1]), negative)
        assert x == f.from_fe(fe_val(a[0]), 5)
        return [x, y]
    return model


def _chk_aff(negative):
    def check(f, a, r):
        y = fe_val(a[1])
        assert val(r[0]) == fe_val(a[0]) << 5 and val(r[1]) == ((f.p - y) if negative else y) << 5 and max(r[0] + r[1]) <= M29
    return check


_op(30, "aff29_from_table(+)", (FQ,), 2, 2, _aff_model(False), _chk_aff(False), [(_fe_x, _fe_y)])
_op(31, "aff29_from_table(-)", (FQ,), 2, 2, _aff_model(True), _chk_aff(True), [(_fe_x, _fe_y)])
_op(32, "xyzz29_from_affine", (FQ,), 2, 4, lambda f, a: accm.start(a[0], a[1]),
    lambda f, a, r: _assert(r[0] == a[0] and r[1] == a[1] and val(r[2]) == R1 % f.p and r[3] == r[2] and max(r[2]) <= M29), [(_x32, _x32)])


def _madd_model(f, a):
    seen, accm.STATS["max_column"] = accm.STATS["max_column"], 0
    got = accm.madd([list(x) for x in a[:4]], a[4], a[5])
    STATS["max_column"] = accm.STATS["max_column"]
    accm.STATS["max_column"] = max(seen, STATS["max_column"])  # (the model's own record keeps growing for its other users)
    assert got == f.madd([list(x) for x in a[:4]], a[4], a[5])
    return got


def _chk_madd(f, a, r):
    ri = pow(R1, -1, f.p)
    want = accm.madd_mod([val(x) % f.p for x in a[:4]], val(a[4]) % f.p, val(a[5]) % f.p, lambda x, y: x * y * ri % f.p)
    assert [val(x) % f.p for x in r] == want
    # the exit bounds curve29.hip.h states: X < 20.4p, Y < 7.7p, ZZ, ZZZ < 1.1p, exact limbs
    assert val(r[0]) * 10 < 204 * f.p and val(r[1]) * 10 < 77 * f.p and val(r[2]) * 10 < 11 * f.p and val(r[3]) * 10 < 11 * f.p
    assert all(max(x[:8]) <= M29 for x in r)


def _madd_vectors(f):
    """The four extreme-limb accumulators and points of test_limb29_model.test_mixed_addition_from_extreme_limbs, the entry-bound recipe of
    test_mixed_addition_from_the_entry_bounds, canonical chains, and the corners of the table point."""
    p = f.p
    out = []
    full = (1 << 29) + 7
    x_top = ((32 * p) >> 232) - 2
    z_top = (14 * p // 10) >> 232
    acc = [[full] * 8 + [x_top], [full] * 8 + [x_top], [full] * 8 + [z_top], [full] * 8 + [z_top]]
    for px, py in ((p - 1, p - 1), (1, 1), (p - 1, 1), ((1 << 253) - 1, (1 << 253) + 12345)):
        out.append(acc + [limbs(px << 5), limbs(py << 5)])
    rng = random.Random(31)
    for _ in range(100):
        def lazy(bound_num, bound_den):
            v = rng.randrange(bound_num * p // bound_den - (1 << 240), bound_num * p // bound_den)
            a = limbs(v)
            k = rng.randrange(8)
            if a[k + 1] > 0 and a[k] + (1 << 29) < (1 << 29) + 8:
                a[k + 1] -= 1
                a[k] += 1 << 29
            return a
        acc = [lazy(32, 1), lazy(32, 1), lazy(14, 10), lazy(14, 10)]
        for a in acc:
            a[0] |= 7
        px, py = rng.choice([p - 1, rng.randrange(1, p)]), rng.choice([p - 1, rng.randrange(1, p)])
        out.append(acc + [limbs(px << 5), limbs(py << 5)])
    # a run as the kernel sees it: from a table point through a chain of additions (exact limbs, the values an addition leaves)
    rng = random.Random(2929)
    for chain in range(8):
        acc = accm.start(limbs(rng.randrange(1, p) << 5), limbs(rng.randrange(1, p) << 5))
        for step in range(16):
            px, py = rng.randrange(p), rng.randrange(1, p)
            if step % 7 == 3:
                px, py = p - 1, p - 1
            if step % 7 == 5:
                px, py = 0, p - 1
            x2, y2 = limbs(px << 5), limbs(py << 5)
            out.append([list(a) for a in acc] + [x2, y2])
            acc = accm.madd(acc, x2, y2)
    return out


_op(33, "xyzz29_madd", (FQ,), 6, 4, _madd_model, _chk_madd, _madd_vectors, acc_job=True)


def _finish_model(f, a):
    out, flag = f.finish(a)
    return [fe_row(v) for v in out] + [[flag] + [0] * 8]


def _chk_finish(f, a, r):
    for x, y in zip(a, r[:4]):
        assert (fe_val(y) * 32 - val(x)) % f.p == 0 and fe_val(y) * 32 < val(x) + 32 * f.p and fe_val(y) < 2 * f.p
    assert r[4] == [0 if val(a[2]) % f.p == 0 else 1] + [0] * 8


def _finish_vectors(f):
    """The exit values of a mixed addition (X < 20.4p, Y < 7.7p, ZZ, ZZZ < 1.1p, exact limbs) at their bounds, ZZ at every multiple of p it
    can be (the flag) and one unit beside it, all 32 digits in every coordinate."""
    p = f.p
    out = []
    tops = (204 * p // 10 - 1, 77 * p // 10 - 1, 11 * p // 10 - 1, 11 * p // 10 - 1)
    out.append([limbs(v) for v in tops])
    for zz in (0, 1, p - 1, p, p + 1):
        out.append([limbs(tops[0] - 5), limbs(3), limbs(zz), limbs(p - 1)])
    for d in range(32):
        out.append([limbs(tops[0] - d), limbs(d), limbs(p - d), limbs(tops[3] - 7 * d)])
    rng = random.Random(34)
    for _ in range(N_RANDOM):
        out.append([limbs(rng.randrange(t)) for t in tops])
    return out


_op(34, "xyzz29_finish", (FQ,), 4, 5, _finish_model, _chk_finish, _finish_vectors, table=32, table_of=lambda a: a[0])


# ---- NTT, Fr
def _shoup(flag):
    def wrap(fn):
        def run(*args):
            old, nttm.SHOUP = nttm.SHOUP, flag
            try:
                return fn(*args)
            finally:
                nttm.SHOUP = old
        return run
    return wrap


def _reduce_rows(f):
    """ntt29_reduce: value < 32p, limbs < 2^32 - 2^30.  Row k = max(q - 1, 0) with q = (c8 * INV_TOP) >> 32 of the carried top limb c8: for
    every q both sides of the top-limb boundary (the smallest c8 that gives q, and one below it), low limbs empty and full; the values k p - 1,
    k p, k p + 1; uncarried limbs at the limb bound."""
    p = f.p
    out = []
    for q in range(0, 33):
        c8 = -(-(q << 32) // nttm.INV_TOP)  # smallest top limb whose estimate is q
        for top in (c8 - 1, c8):
            for low in (0, M29, CARRIED):
                a = [low] * 8 + [top]
                if top >= 0 and val(a) < 32 * p:
                    out.append(a)
        for v in (q * p - 1, q * p, q * p + 1):
            if 0 <= v < 32 * p:
                out.append(limbs(v))
    lmax = U32 - (1 << 30) - 1
    for top in (0, 5, (31 * p) >> 232):
        a = [lmax] * 8 + [top]
        if val(a) < 32 * p:
            out.append(a)
    return out


def _reduce_model(f, a):
    r = nttm.reduce(a[0])
    c = nttm.carry(a[0])
    q = (c[8] * nttm.INV_TOP) >> 32
    STATS["rows"].add(q - 1 if q > 1 else 0)
    return [r]


_lz_red = Fixed(_reduce_rows, lambda f, rng: Lz(32, U32 - (1 << 30) - 1).rand(f, rng) if rng.random() < 0.3 else Lz(32, CARRIED).rand(f, rng))
_op(40, "ntt29_reduce", (FR,), 1, 1, _reduce_model,
    lambda f, a, r: _assert((val(r[0]) - val(a[0])) % f.p == 0 and val(r[0]) < 3 * f.p and max(r[0][:8]) < (1 << 29) + 8
                            and (val(r[0]) == val(a[0]) if val(a[0]) < 2 * f.p else val(r[0]) >= f.p)), [(_lz_red,)], table=31)


def _finish29_rows(f):
    """n29_finish: row q = the quotient estimate itself.  The NTT hands it V < 25 with limbs < 2^31 + 8; the typed layer (w29::finish) any
    class-0 value with V <= 31 ("the q p table has 32 rows"): the contract here.  Both sides of the top-limb boundary of every q, low limbs
    empty and full; the values q p - 1, q p, q p + 1."""
    p = f.p
    out = []
    for q in range(0, 33):
        c8 = -(-(q << 32) // nttm.INV_TOP)
        for top in (c8 - 1, c8):
            for low in (0, M29, CARRIED):
                a = [low] * 8 + [top]
                if top >= 0 and val(a) <= 31 * p:
                    out.append(a)
        for v in (q * p - 1, q * p, q * p + 1):
            if 0 <= v <= 31 * p:
                out.append(limbs(v))
    lmax = (1 << 31) + 7
    for top in (0, 5, (25 * p) >> 232):
        out.append([lmax] * 8 + [top])
    return out


def _finish29_model(f, a):
    x = a[0]
    assert val(x) <= 31 * f.p and max(x[:8]) < (1 << 31) + 8
    c = nttm.carry(x)
    q = (c[8] * nttm.INV_TOP) >> 32
    STATS["rows"].add(q)
    if val(x) * 1000 < 25000 * f.p + f.p:
        v = nttm.finish(x)  # the NTT's statement (V < 25)
    else:                   # the typed layer's (V <= 31: test_w29_model.finish), the same signed pass
        v = w29m.finish(w29m.W(x, 0, 31 * 64, (1 << 31) + 7, val(x) * pow(w29m.R, -1, f.p)))
    return [fe_row(v)]


_lz_fin = Fixed(_finish29_rows, lambda f, rng: Lz(25, (1 << 31) + 7).rand(f, rng) if rng.random() < 0.3 else Lz(31, CARRIED).rand(f, rng))
_op(41, "n29_finish", (FR,), 1, 1, _finish29_model,
    lambda f, a, r: _assert((fe_val(r[0]) - val(a[0])) % f.p == 0 and fe_val(r[0]) < 2 * f.p), [(_lz_fin,)], table=31)
_lz25 = Lz(25, (1 << 31) + 7)
_op(42, "n29_finish_mul", (FR,), 2, 1, lambda f, a: [fe_row(nttm.finish(a[0], fe_val(a[1])))],
    lambda f, a, r: _assert((fe_val(r[0]) * R1 - val(a[0]) * (fe_val(a[1]) << 5)) % f.p == 0 and fe_val(r[0]) < 2 * f.p), [(_lz25, _fe2p)])


# f29_mulc(x, {w, wq}): x limbs <= 2^31 + 2^29, x < 64p; w < p exact, wq = floor(w 2^261 / p)
def _const_rows(f, w):
    return [limbs(w), limbs(w * R1 // f.p)]


_lz_c = Lz(64, (1 << 31) + (1 << 29))
_W_CORNERS = lambda p: (0, 1, 2, p - 1, p - 2, (p - 1) // 2, 1 << 253)  # noqa: E731
_w_dom = Fixed(lambda f: [limbs(w) for w in _W_CORNERS(f.p)], lambda f, rng: limbs(rng.randrange(f.p)))


def _chk_mulc(f, a, r, at=0):
    x, w = val(a[0]), val(a[1])
    assert val(a[2]) == w * R1 // f.p
    assert (val(r[at]) - x * w) % f.p == 0 and val(r[at]) * 169 < (2 * 169 + x // f.p + 1) * f.p and max(r[at]) <= M29


def _mulc_vectors(n):
    def make(f):
        rng = random.Random(4300 + n)
        xs = _lz_c.corners(f)
        ws = [w for w in _W_CORNERS(f.p)]
        vecs = [[x] + _const_rows(f, w) for x in xs for w in ws]
        vecs += [[_lz_c.rand(f, rng)] + _const_rows(f, rng.randrange(f.p)) for _ in range(N_RANDOM)]
        if n == 1:
            return vecs
        other = vecs[1:] + vecs[:1]
        return [a + b for a, b in zip(vecs, other)]
    return make


_op(43, "f29_mulc", (FR,), 3, 1, lambda f, a: [nttm.mulc(a[0], a[1])], _chk_mulc, _mulc_vectors(1))
_op(44, "f29_mulc2", (FR,), 6, 2, lambda f, a: [nttm.mulc(a[0], a[1]), nttm.mulc(a[3], a[4])],
    lambda f, a, r: (_chk_mulc(f, a[:3], r, 0), _chk_mulc(f, a[3:], r, 1)), _mulc_vectors(2))


def _step_inputs(f, rng, trial):
    """eight registers: carried, V < 3"""
    p = f.p
    big = 3 * p - 1
    fat = limbs(big)
    for i in range(8, 0, -1):  # test_ntt29_model.test_step8_at_the_entry_bounds: weight moved down where the limb stays below 2^29 + 8
        if fat[i] > 0 and fat[i - 1] + (1 << 29) < (1 << 29) + 8:
            fat[i] -= 1
            fat[i - 1] += 1 << 29
    full = [CARRIED] * 8 + [Lz(3, CARRIED).topmax(f, CARRIED)]
    fixed = [[fat] * 8, [limbs(big)] * 8, [limbs(0)] * 8, [limbs(big)] + [limbs(0)] * 7, [limbs(0)] * 7 + [limbs(big)], [full] * 8,
             [limbs(v) for v in (0, 1, p - 1, p, 2 * p - 1, big, p + 1, 2 * p)]]
    if trial < len(fixed):
        return [list(a) for a in fixed[trial]]
    return [Lz(3, CARRIED).rand(f, rng) for _ in range(8)]


def _step_vectors(sh, nw, ntw, n=96):
    def make(f):
        rng = random.Random(5000 + 10 * nw + ntw + sh)
        out = []
        for trial in range(n):
            x = _step_inputs(f, rng, trial)
            ws = [f.p - 1] * (nw + ntw) if trial < 7 and trial % 2 == 0 else [rng.randrange(f.p) for _ in range(nw + ntw)]
            rows = []
            for w in ws:
                rows += _const_rows(f, w) if sh else [limbs(w)]
            out.append(x + rows)
        return out
    return make


def _tw(a, sh, i):  # multiplier i of a step vector (after the eight registers): its w limbs
    return a[8 + (2 * i if sh else i)]


def _step8_model(sh, have_tw):
    @_shoup(bool(sh))
    def model(f, a):
        x = a[:8]
        w = [_tw(a, sh, i) for i in range(3)]
        if have_tw:
            return nttm.step8(x, w[0], w[1], w[2], [None] + [_tw(a, sh, 3 + i) for i in range(7)])
        return [nttm.reduce(r) for r in nttm.step8_raw(x, w[0], w[1], w[2])]
    return model


def _bf_mod(f, x, pairs, rinv):
    x = list(x)
    for i, j, w in pairs:
        u, d = (x[i] + x[j]) % f.p, (x[i] - x[j]) % f.p
        x[i], x[j] = u, d if w is None else d * w * rinv % f.p
    return x


def _chk_step8(sh, have_tw, reduced=True):
    def check(f, a, r):
        rinv = 1 if sh else pow(R1, -1, f.p)
        w1, w2, w3 = (val(_tw(a, sh, i)) for i in range(3))
        ref = _bf_mod(f, [val(x) % f.p for x in a[:8]],
                      [(0, 4, None), (1, 5, w1), (2, 6, w2), (3, 7, w3), (0, 2, None), (1, 3, w2), (4, 6, None), (5, 7, w2),
                       (0, 1, None), (2, 3, None), (4, 5, None), (6, 7, None)], rinv)
        if have_tw:
            ref = [ref[0]] + [ref[j] * val(_tw(a, sh, 2 + j)) * rinv % f.p for j in range(1, 8)]
        assert [val(x) % f.p for x in r] == ref
        if have_tw:
            assert val(r[0]) < 3 * f.p and all(val(x) * 100 < (215 if sh else 115) * f.p + f.p for x in r[1:])
        elif reduced:
            assert all(val(x) < 3 * f.p and max(x[:8]) < (1 << 29) + 8 for x in r)
        else:
            assert all(val(x) < 25 * f.p and max(x) < (1 << 31) + 8 for x in r)
    return check


_op(50, "n29_step8<0,true>", (FR,), 18, 8, _step8_model(0, True), _chk_step8(0, True), _step_vectors(0, 3, 7))
_op(51, "n29_step8<0,false>", (FR,), 11, 8, _step8_model(0, False), _chk_step8(0, False), _step_vectors(0, 3, 0))
_op(52, "n29_step8<1,true>", (FR,), 28, 8, _step8_model(1, True), _chk_step8(1, True), _step_vectors(1, 3, 7))
_op(53, "n29_step8<1,false>", (FR,), 14, 8, _step8_model(1, False), _chk_step8(1, False), _step_vectors(1, 3, 0))


def _step4_model(sh):
    return _shoup(bool(sh))(lambda f, a: nttm.step4(a[:8], _tw(a, sh, 0)))


def _chk_step4(sh):
    def check(f, a, r):
        rinv = 1 if sh else pow(R1, -1, f.p)
        w2 = val(_tw(a, sh, 0))
        ref = _bf_mod(f, [val(x) % f.p for x in a[:8]], [(0, 2, None), (1, 3, w2), (4, 6, None), (5, 7, w2), (0, 1, None), (2, 3, None),
                                                        (4, 5, None), (6, 7, None)], rinv)
        assert [val(x) % f.p for x in r] == ref and all(val(x) < 13 * f.p and max(x) < (1 << 31) + 8 for x in r)
    return check


_op(54, "n29_step4<0>", (FR,), 9, 8, _step4_model(0), _chk_step4(0), _step_vectors(0, 1, 0))
_op(55, "n29_step4<1>", (FR,), 10, 8, _step4_model(1), _chk_step4(1), _step_vectors(1, 1, 0))
_op(56, "n29_step2", (FR,), 8, 8, lambda f, a: nttm.step2(a),
    lambda f, a, r: _assert([val(x) % f.p for x in r] == _bf_mod(f, [val(x) % f.p for x in a], [(i, i + 1, None) for i in (0, 2, 4, 6)], 1)
                            and all(val(x) < 7 * f.p and max(x) < (1 << 31) + 8 for x in r)), _step_vectors(0, 0, 0))
_op(57, "n29_step8_raw<0>", (FR,), 11, 8, _shoup(False)(lambda f, a: nttm.step8_raw(a[:8], a[8], a[9], a[10])), _chk_step8(0, False, False),
    _step_vectors(0, 3, 0))
_op(58, "n29_step8_raw<1>", (FR,), 14, 8, _shoup(True)(lambda f, a: nttm.step8_raw(a[:8], a[8], a[10], a[12])), _chk_step8(1, False, False),
    _step_vectors(1, 3, 0))


# ---- the typed layer: the five-term dot of k_quotient29_turbo_fixed_base_gate.  The operand TYPES (class, V bound in 1/64, limb bound) are
# derived as the kernel derives them, by running the model's own operations on placeholder operands.
def _gate_types():
    m = w29m
    top = 2 * m.P - 1
    l0, l1 = m.ld(top, 0), m.ld(top, 1)
    sq = m.sqr(l1)
    acc = m.mul(m.carry(m.sub(sq, l1)), m.carry(m.sub(sq, l1)))
    nw = m.carry(m.neg(l0))
    m10 = m.mul(l1, l0)
    xid = m.dot((l0, sq), (nw, sq), (nw, l1), (m10, l1))
    xid17 = m.add(xid, l0)
    ym = m.carry(m.sub(l0, m10))
    yid = m.dot((l0, l1), (ym, l1))
    i3 = m.dot((l0, l1), (nw, l1))
    init = m.dot((m10, l1), (m.neg(m10), l1), (i3, l1))
    return [(w.cls, w.vq, w.lm) for w in (acc, l0, nw, l1, xid17, l1, yid, l1, init, l1)]


GATE_TYPES = _gate_types()


def _w_of(f, row, typ):
    cls, vq, lm = typ
    return w29m.W(row, cls, vq, lm, val(row) * pow(w29m.R * pow(32, cls, f.p), -1, f.p))


def _dot_model(f, a):
    ws = [_w_of(f, row, typ) for row, typ in zip(a, GATE_TYPES)]  # (W() asserts the limbs against the type's bounds)
    return [w29m.dot(*[(ws[2 * i], ws[2 * i + 1]) for i in range(5)]).l]


def _dot_dom(typ):
    cls, vq, lm = typ
    top = (vq * w29m.PTOP1 + 63) // 64 + 2

    def corners(f):
        out = [limbs(v) for v in (0, 1, f.p - 1, f.p, 2 * f.p - 1, vq * f.p // 64) if v * 64 <= vq * f.p]
        t = (vq * f.p // 64 - val([lm] * 8 + [0])) >> 232
        if t >= 0:
            out.append([lm] * 8 + [min(t, top)])
        return out

    def rand(f, rng):
        while True:
            a = [rng.randrange(lm + 1) for _ in range(8)] + [rng.randrange(top + 1)]
            if val(a) * 64 <= vq * f.p:
                return a
    return Fixed(corners, rand)


def _chk_dot(f, a, r):
    want = sum(val(a[2 * i]) * val(a[2 * i + 1]) for i in range(5))
    _residue(f, r[0], want)
    assert val(r[0]) < want // R1 + f.p + 1 and max(r[0][:8]) <= M29


_op(60, "w29::dot (gate)", (FR,), 10, 1, _dot_model, _chk_dot, [tuple(_dot_dom(t) for t in GATE_TYPES)])


# ---- f29_sub / f29_neg / n29_bfly for every (M, E) pair
def _sub_dom(f_mult, e):
    """the subtrahend: limbs <= 2^E - 2, value below M p with the top-limb margin (top limb <= that of M p minus 2^(E - 29))"""
    lmax = (1 << e) - 2

    def corners(f):
        top = ((f_mult * f.p) >> 232) - (1 << (e - 29))
        out = [limbs(v) for v in (0, 1, f.p - 1, f.p, 2 * f.p - 1, (f_mult - 1) * f.p - 1) if (v >> 232) <= top]
        out += [[lmax] * 8 + [top], [lmax] * 8 + [0], [0] * 8 + [top], [lmax, 0] * 4 + [top]]
        return out

    def rand(f, rng):
        top = ((f_mult * f.p) >> 232) - (1 << (e - 29))
        if rng.random() < 0.5:
            return [rng.randrange(lmax + 1) for _ in range(8)] + [rng.randrange(top + 1)]
        return limbs(rng.randrange((f_mult - 1) * f.p))
    return Fixed(corners, rand)


def _minuend_dom(mult, e):
    """the minuend: any limbs that keep a + spread - b below 2^32 (spread limb < 2^E + 2^29)"""
    lmax = U32 - 1 - (1 << e) - (1 << 29)
    return Lz(64, lmax, extra=[[lmax] * 8 + [U32 - 1 - ((mult + 1) << 22)]])


for _i, (_m, _e) in enumerate(PAIRS):
    def _mk(i, m, e):
        _op(100 + i, "f29_sub<%d,%d>" % (m, e), BOTH, 2, 1, lambda f, a: [f.sub(a[0], a[1], m, e)],
            lambda f, a, r: _assert(val(r[0]) == val(a[0]) - val(a[1]) + m * f.p), [(_minuend_dom(m, e), _sub_dom(m, e))], bit31=(0,), out31=True)
        _op(200 + i, "f29_neg<%d,%d>" % (m, e), BOTH, 1, 1, lambda f, a: [f.neg(a[0], m, e)],
            lambda f, a, r: _assert(val(r[0]) == m * f.p - val(a[0])), [(_sub_dom(m, e),)], out31=(e == 31))
        _op(300 + i, "n29_bfly<%d,%d>" % (m, e), (FR,), 2, 2, lambda f, a: [nttm.add(a[0], a[1]), nttm.sub(a[0], a[1], m, e)],
            lambda f, a, r: _assert(val(r[0]) == val(a[0]) + val(a[1]) and val(r[1]) == val(a[0]) - val(a[1]) + m * f.p),
            [(Lz(64, U32 - 1 - (1 << e) - (1 << 29)), _sub_dom(m, e))], bit31=(0,) if e == 30 else (), out31=True)
    _mk(_i, _m, _e)


# ---------------------------------------------------------------------------------------------- existing models, by field
def _existing(which, op):
    """The same op through the model the suite already had for this field (None where it has none): rows must equal Field's."""
    if which == FQ:
        t = {2: lambda a: [fqm.carry(a[0])], 10: lambda a: [fqm.mul(a[0], a[1])], 11: lambda a: [fqm.sqr(a[0])],
             12: lambda a: [fqm.mul_sub2(*a)], 16: lambda a: [fqm.mul(a[0], a[1]), fqm.mul(a[2], a[3])], 17: lambda a: [fqm.sqr(a[0]), fqm.sqr(a[1])],
             18: lambda a: [fqm.mul_sub2(*a[:4]), fqm.mul(a[4], a[5])],
             19: lambda a: [accm.mont([(a[0], a[1])]), accm.mont([(a[2], a[3])])],
             20: lambda a: [accm.mont([(a[0], a[1])], a[2]), accm.mont([(a[3], a[4])], a[5])],
             21: lambda a: [accm.mont([(a[0], a[0])], a[1]), accm.mont([(a[2], a[3])])],
             22: lambda a: [accm.mont([(a[0], a[1]), (accm.neg(a[2], 64, 30), a[3])]), accm.mont([(a[4], a[5])])],
             23: lambda a: [accm.mont([(a[0], a[0])])]}
        if op in t:
            return t[op]
        if 100 <= op < 100 + len(PAIRS):
            m, e = PAIRS[op - 100]
            return lambda a: [accm.sub(a[0], a[1], m, e)]
        if 200 <= op < 200 + len(PAIRS):
            m, e = PAIRS[op - 200]
            return lambda a: [accm.neg(a[0], m, e)]
    else:
        t = {2: lambda a: [nttm.carry(a[0])], 6: lambda a: [nttm.add(a[0], a[1])], 10: lambda a: [nttm.mul(a[0], a[1])],
             16: lambda a: [nttm.mul(a[0], a[1]), nttm.mul(a[2], a[3])]}
        if op in t:
            return t[op]
        if 100 <= op < 100 + len(PAIRS):
            m, e = PAIRS[op - 100]
            return lambda a: [nttm.sub(a[0], a[1], m, e)]
    return None


# ---------------------------------------------------------------------------------------------- building the vectors
def operands_of(which, op):
    """the deterministic operand vectors of an op: a list of vectors, each a list of nin rows of 9 ints"""
    o, f = OPS[op], FIELDS[which]
    if callable(o.regimes):
        return [[list(r) for r in v] for v in o.regimes(f)]
    rng = random.Random(1000 * op + which)
    out = []
    for regime in o.regimes:
        corners = [d.corners(f) for d in regime]
        total = 1
        for c in corners:
            total *= len(c)
        if total <= 400:
            combos = list(itertools.product(*corners))
        else:  # every corner of every operand against the others' same-numbered corner, then random combinations of corners
            n = max(len(c) for c in corners)
            combos = [tuple(c[i % len(c)] for c in corners) for i in range(n)]
            combos += [tuple(c[(i + 3 * k) % len(c)] for k, c in enumerate(corners)) for i in range(n)]
            combos += [tuple(rng.choice(c) for c in corners) for _ in range(160)]
            # every limb-valued operand at its largest at once, against every corner of the others (addends, 8-word values)
            others = max([len(c) for d, c in zip(regime, corners) if not isinstance(d, Lz)] or [1])
            combos += [tuple(d.fat(f)[0] if isinstance(d, Lz) else c[i % len(c)] for d, c in zip(regime, corners)) for i in range(others)]
        out += [[list(r) for r in v] for v in combos]
        out += [[d.rand(f, rng) for d in regime] for _ in range(N_RANDOM // len(o.regimes))]
    return out


class Built:
    """operands, expected rows and what the model run reached, for one (which, op)"""

    def __init__(self, which, op):
        o, f = OPS[op], FIELDS[which]
        self.which, self.op, self.name = which, op, o.name
        self.operands, self.expected, self.max_column, self.rows = [], [], 0, set()
        other = _existing(which, op)
        for v in operands_of(which, op):
            assert len(v) == o.nin
            STATS["max_column"], STATS["rows"] = 0, set()
            r = o.model(f, v)  # (a model assertion here = a vector outside the op's contract: every vector must be inside)
            if other is not None:
                assert other(v) == r, "the suite's model of this field and Field disagree: %s %r" % (o.name, v)
            assert len(r) == o.nout and all(len(x) == 9 and all(0 <= y < U32 for y in x) for x in r)
            self.operands.append(v)
            self.expected.append(r)
            self.max_column = max(self.max_column, STATS["max_column"])
            self.rows |= STATS["rows"]


_CACHE = {}


def cases():
    """every (which, op) of the harness"""
    return [(w, op) for op in sorted(OPS) for w in OPS[op].fields]


def build(which, op):
    if (which, op) not in _CACHE:
        _CACHE[(which, op)] = Built(which, op)
    return _CACHE[(which, op)]


def case_id(case):
    return "%s-%s" % ("Fr" if case[0] == FR else "Fq", OPS[case[1]].name.replace(" ", ""))
