"""Vectors and expected results of the pairing-arithmetic conformance test (bbg_tower_op, csrc/tower_check.hip): for every device function of
csrc/fq_tower.hip.h, fq12_wave.hip.h and g2.hip.h the operand rows (RAW Montgomery words as integers anywhere in the tower's coarse range
[0, 2p]) and what the integer models (pairing_model.py, pairing_wave_model.py; plain residues mod p) say the result is.  Nothing here comes
from a device.

OPS restates the X-macro table BBG_TOWER_OPS of csrc/tower_check.hip (tests/test_tower_vectors_cpu.py scans the source, the GPU test asks
bbg_tower_op_shape).  Per op three groups of vectors, each with a name:
  corner:*     the corner set C = {0, 1, R mod p (the Montgomery one), p - 1, p, p + 1, 2p - 1, 2p}: every operand row takes every corner once
               while the others are random, all rows equal to one corner; the unary Fq2 ops all |C|^2 pairs; the binary Fq2 ops every
               operand whose four coefficients come from the reduced set {0, p - 1, p, 2p - 1, 2p} (625);
  designed:*   the conditions a generic input does not meet (a Karatsuba sum that wraps exactly at 2p, a borrowing fe_sub, every
               representative of zero and of one and their near misses, single non-zero components for the Frobenius constants and for the
               wrap of the w-basis product, the exceptional branches of g2_madd, ...);
  random:*     64 seeded vectors, half with every row in [0, p), half in [p, 2p).

A result row has a kind: "res" (the raw row is <= 2p and its residue is the model's), "canon" (the words are the model's canonical words),
"same" (the raw words are the operand's), "bool" (word 0 is the model's 0 / 1, the rest 0), "point" (the six rows are a Jacobian point that
normalises to the model's affine point; z = 0 is infinity).  Expected rows are Montgomery residues below p; for "point" ops the expectation
is five rows: infinity flag, x.c0, x.c1, y.c0, y.c1."""
import functools
import itertools
import random
from collections import namedtuple

import pairing_model as pm
import pairing_wave_model as pwm

P = pm.P
MONT = pm.MONT
MINV = pow(MONT, -1, P)
NINV = (-pow(P, -1, MONT)) % MONT
RM = MONT % P  # the Montgomery form of one
CORNERS = [0, 1, RM, P - 1, P, P + 1, 2 * P - 1, 2 * P]
CORNER_NAMES = ["0", "1", "R", "p-1", "p", "p+1", "2p-1", "2p"]
REDUCED = [0, P - 1, P, 2 * P - 1, 2 * P]
ZEROS = [0, P, 2 * P]
ONES = [RM, RM + P]
N_RANDOM = 64


def raw(v, lift=0):
    """The Montgomery word of the plain residue v, in [0, p) or with lift = 1 in [p, 2p)."""
    return v % P * MONT % P + lift * P


def plain(r):
    return r * MINV % P


def mont_mul_raw(a, b):
    """fe_mul on raw words: (a b + m p) / 2^256 with no final subtraction, below 2p for a, b <= 2p."""
    t = a * b
    return (t + (t * NINV % MONT) * P) >> 256


# ------------------------------------------------------------------------------------------------ shapes of flat plain lists
def F2(v, i=0):
    return (v[i], v[i + 1])


def F6(v, i=0):
    return (F2(v, i), F2(v, i + 2), F2(v, i + 4))


def F12(v, i=0):
    return (F6(v, i), F6(v, i + 6))


def flat6(a):
    return [c for two in a for c in two]


flat12 = pm.f12_flat


def f4_sqr(a, b):
    """(a + b s)^2 in Fq2[s] / (s^2 - xi), by the definition."""
    return pm.f2_add(pm.f2_sqr(a), pm.f2_mul_xi(pm.f2_sqr(b))), pm.f2_mul_fq(pm.f2_mul(a, b), 2)


def jac(q, z):
    """The affine point q in Jacobian coordinates with the given z (plain)."""
    z2 = pm.f2_sqr(z)
    return [*pm.f2_mul(q[0], z2), *pm.f2_mul(q[1], pm.f2_mul(z2, z)), *z]


def jac_affine(v):
    """The affine point of plain Jacobian coordinates x, y, z; None for z = 0."""
    x, y, z = F2(v, 0), F2(v, 2), F2(v, 4)
    if z == pm.F2_ZERO:
        return None
    zi = pm.f2_inv(z)
    zi2 = pm.f2_sqr(zi)
    return (pm.f2_mul(x, zi2), pm.f2_mul(y, pm.f2_mul(zi2, zi)))


def point_rows(q):
    return [1, 0, 0, 0, 0] if q is None else [0, *q[0], *q[1]]


def _wave(slot1, slot2=None):
    w = pwm.Wave()
    w.slot[1] = list(slot1)
    if slot2 is not None:
        w.slot[2] = list(slot2)
    return w


def _w_mul(v, d, sparse):
    w = _wave(v[:12], None if sparse else v[12:24])
    w.mul(d, 1, v[12:18] if sparse else w.slot[2], sparse)
    return w.slot[d]


def _w_unary(v, what, *args):
    w = _wave(v)
    getattr(w, what)(3, 1, *args)
    return w.slot[3]


def _w_store_is_one(v):
    value = pwm.from_w(v)
    return flat12(value) + [int(value == pm.F12_ONE)]


def _line_double(v):
    cur, line = pm.doubling_step((F2(v, 0), F2(v, 2), F2(v, 4)))
    return flat6(cur) + flat6(line)


def _line_add(v):
    cur, line = pm.mixed_addition_step((F2(v, 0), F2(v, 2)), (F2(v, 4), F2(v, 6), F2(v, 8)))
    return flat6(cur) + flat6(line)


def _mul_by_q(v):
    q = pm.mul_by_q((F2(v, 0), F2(v, 2)))
    return [*q[0], *q[1]]


Op = namedtuple("Op", "name nin nout kinds model")


def _op(name, nin, nout, model, kinds="res"):
    return Op(name, nin, nout, [kinds] * nout if isinstance(kinds, str) else kinds, model)


# number: (name, operand rows, result rows, kinds, the model on plain residues)
OPS = {
    0: _op("f2_add", 4, 2, lambda v: pm.f2_add(F2(v), F2(v, 2))),
    1: _op("f2_sub", 4, 2, lambda v: pm.f2_sub(F2(v), F2(v, 2))),
    2: _op("f2_neg", 2, 2, lambda v: pm.f2_neg(F2(v))),
    3: _op("f2_dbl", 2, 2, lambda v: pm.f2_add(F2(v), F2(v))),
    4: _op("f2_conj", 2, 2, lambda v: pm.f2_conj(F2(v))),
    5: _op("f2_mul", 4, 2, lambda v: pm.f2_mul(F2(v), F2(v, 2))),
    6: _op("f2_sqr", 2, 2, lambda v: pm.f2_sqr(F2(v))),
    7: _op("f2_mul_fq", 3, 2, lambda v: pm.f2_mul_fq(F2(v), v[2])),
    8: _op("f2_mul_xi", 2, 2, lambda v: pm.f2_mul_xi(F2(v))),
    9: _op("f2_inv", 2, 2, lambda v: pm.f2_inv(F2(v))),
    10: _op("f2_canon", 2, 2, lambda v: F2(v), "canon"),
    11: _op("f2_is_zero", 2, 1, lambda v: [int(F2(v) == pm.F2_ZERO)], "bool"),
    12: _op("f2_eq", 4, 1, lambda v: [int(F2(v) == F2(v, 2))], "bool"),
    13: _op("fq_canon", 1, 1, lambda v: [v[0]], "canon"),
    20: _op("f6_add", 12, 6, lambda v: flat6(pm.f6_add(F6(v), F6(v, 6)))),
    21: _op("f6_sub", 12, 6, lambda v: flat6(pm.f6_sub(F6(v), F6(v, 6)))),
    22: _op("f6_neg", 6, 6, lambda v: flat6(pm.f6_neg(F6(v)))),
    23: _op("f6_mul_v", 6, 6, lambda v: flat6(pm.f6_mul_v(F6(v)))),
    24: _op("f6_mul", 12, 6, lambda v: flat6(pm.f6_mul(F6(v), F6(v, 6)))),
    25: _op("f6_sqr", 6, 6, lambda v: flat6(pm.f6_sqr(F6(v)))),
    26: _op("f6_inv", 6, 6, lambda v: flat6(pm.f6_inv(F6(v)))),
    30: _op("f12_mul", 24, 12, lambda v: flat12(pm.f12_mul(F12(v), F12(v, 12)))),
    31: _op("f12_sqr", 12, 12, lambda v: flat12(pm.f12_sqr(F12(v)))),
    32: _op("f12_conj", 12, 12, lambda v: flat12(pm.f12_conj(F12(v)))),
    33: _op("f12_inv", 12, 12, lambda v: flat12(pm.f12_inv(F12(v)))),
    34: _op("f4_sqr", 4, 4, lambda v: [c for two in f4_sqr(F2(v), F2(v, 2)) for c in two]),
    35: _op("f12_cyclotomic_sqr", 12, 12, lambda v: flat12(pm.f12_cyclotomic_sqr(F12(v)))),
    36: _op("f12_frobenius(1)", 12, 12, lambda v: flat12(pm.f12_frobenius(F12(v), 1))),
    37: _op("f12_frobenius(2)", 12, 12, lambda v: flat12(pm.f12_frobenius(F12(v), 2))),
    38: _op("f12_frobenius(3)", 12, 12, lambda v: flat12(pm.f12_frobenius(F12(v), 3))),
    39: _op("f12_sparse_mul", 18, 12, lambda v: flat12(pm.f12_sparse_mul(F12(v), (F2(v, 12), F2(v, 14), F2(v, 16))))),
    40: _op("f12_is_one", 12, 1, lambda v: [int(F12(v) == pm.F12_ONE)], "bool"),
    41: _op("f12_store", 12, 12, lambda v: list(v), "canon"),
    42: _op("f12_load_lanes(f12_store_lanes)", 12, 12, lambda v: list(v), "same"),
    50: _op("w12_mul<false>", 24, 12, lambda v: _w_mul(v, 3, False)),
    51: _op("w12_mul<false>(d=a)", 24, 12, lambda v: _w_mul(v, 1, False)),
    52: _op("w12_mul<true>", 18, 12, lambda v: _w_mul(v, 3, True)),
    53: _op("w12_conj", 12, 12, lambda v: _w_unary(v, "conj")),
    54: _op("w12_frobenius(1)", 12, 12, lambda v: _w_unary(v, "frobenius", 1)),
    55: _op("w12_frobenius(2)", 12, 12, lambda v: _w_unary(v, "frobenius", 2)),
    56: _op("w12_frobenius(3)", 12, 12, lambda v: _w_unary(v, "frobenius", 3)),
    57: _op("w12_inv", 12, 12, lambda v: _w_unary(v, "inv")),
    58: _op("w12_set_one", 12, 12, lambda v: [1] + [0] * 11, "canon"),
    59: _op("w12_store_is_one", 12, 13, _w_store_is_one, ["canon"] * 12 + ["bool"]),
    60: _op("g2_on_twist", 4, 1, lambda v: [int(pm.g2_on_twist((F2(v), F2(v, 2))))], "bool"),
    61: _op("g2_dbl", 6, 6, lambda v: point_rows(pm.g2_add(jac_affine(v), jac_affine(v))), "point"),
    62: _op("g2_madd", 10, 6, lambda v: point_rows(pm.g2_add(jac_affine(v), (F2(v, 6), F2(v, 8)))), "point"),
    63: _op("line_double", 6, 12, _line_double, ["res"] * 6 + ["canon"] * 6),
    64: _op("line_add", 10, 12, _line_add, ["res"] * 6 + ["canon"] * 6),
    65: _op("g2_mul_by_q", 4, 4, _mul_by_q),
}
UNARY_F2 = (2, 3, 4, 6, 8, 9, 10, 11)       # all |C|^2 operands
BINARY_F2 = (0, 1, 5, 12, 34)               # every operand over the reduced set: 625
WAVE_OPS = tuple(range(50, 60))

# Device functions of the three headers that no op names, and why that is enough.  A function added to a header without an op fails
# tests/test_tower_vectors_cpu.py::test_every_device_function_has_an_op.
EXEMPT = {
    "f2_zero": "a constant", "f2_one": "a constant", "f6_zero": "a constant", "f6_one": "a constant", "f12_one": "a constant",
    "f2_load": "a copy: canonical memory to registers", "f2_store": "a copy; runs under f12_store and the stored lines",
    "fq_load_lanes": "a copy; runs under f12_load_lanes", "fq_store_lanes": "a copy; runs under f12_store_lanes",
    "f2_load_lanes": "a copy; runs under f12_load_lanes", "f2_store_lanes": "a copy; runs under f12_store_lanes",
    "f2_3t_minus_2z": "a step of f12_cyclotomic_sqr, which has an op", "f2_3t_plus_2z": "a step of f12_cyclotomic_sqr, which has an op",
    "f12_frob_part": "a step of f12_frobenius and w12_frobenius, which have ops",
    "w12_ref_component": "index arithmetic", "w12_line_power": "index arithmetic",
    "line_store": "runs under line_double and line_add, whose stored lines are compared word for word",
    "g2_aff_is_inf": "g2_aff_*: the memory format of bbg_g2_mul, compared bit for bit by tests/test_gpu_pairing.py",
    "g2_aff_load": "g2_aff_*", "g2_aff_store": "g2_aff_*",
}


# ------------------------------------------------------------------------------------------------ vectors
def _rand_rows(rng, n):
    return [rng.randrange(2 * P + 1) for _ in range(n)]


def _corner_vectors(op, rng):
    o = OPS[op]
    out = []
    for pos in range(o.nin):
        for c, cn in zip(CORNERS, CORNER_NAMES):
            v = _rand_rows(rng, o.nin)
            v[pos] = c
            out.append(("corner:pos%d=%s" % (pos, cn), v))
    for c, cn in zip(CORNERS, CORNER_NAMES):
        out.append(("corner:all=%s" % cn, [c] * o.nin))
    if op in UNARY_F2:
        out += [("corner:pair%d" % i, list(v)) for i, v in enumerate(itertools.product(CORNERS, repeat=2))]
    if op in BINARY_F2:
        out += [("corner:reduced%d" % i, list(v)) for i, v in enumerate(itertools.product(REDUCED, repeat=4))]
    if op == 7:
        out += [("corner:reduced%d" % i, list(v)) for i, v in enumerate(itertools.product(REDUCED, repeat=3))]
    return out


def _random_vectors(op, rng):
    n = OPS[op].nin
    return [("random:%d" % i, [rng.randrange(P) + (P if i >= N_RANDOM // 2 else 0) for _ in range(n)]) for i in range(N_RANDOM)]


def _rp(rng):
    return rng.randrange(1, P)


def _rp2(rng):
    return (_rp(rng), _rp(rng))


def _raws(vals, lift=0):
    return [raw(v, lift) for v in vals]


@functools.lru_cache(maxsize=None)
def cyclotomic_elements():
    """Four random Fq12 through the easy part of the final exponentiation: elements of the cyclotomic subgroup (plain residues)."""
    rng = random.Random(0x7035)
    return [pm.final_exponentiation_easy_part(F12([_rp(rng) for _ in range(12)])) for _ in range(4)]


@functools.lru_cache(maxsize=None)
def g2_points():
    """The generator, three multiples of it, and a point of the twist outside the subgroup of order r."""
    return [pm.G2, pm.g2_mul(pm.G2, 5), pm.g2_mul(pm.G2, 0xC0FFEE1234567), pm.g2_mul(pm.G2, pm.R - 2), pm.g2_point_outside_subgroup()]


def _zero_mixes(rng, n, count):
    """Representatives of zero over n coefficients drawn from {0, p, 2p}: the three constant ones, then `count` random mixes (all 3^n if few)."""
    if 3 ** n <= count:
        return [list(v) for v in itertools.product(ZEROS, repeat=n)]
    return [[z] * n for z in ZEROS] + [[rng.choice(ZEROS) for _ in range(n)] for _ in range(count)]


def _one_mixes(rng, n, count):
    return [[o] + z[1:] for z in _zero_mixes(rng, n, count) for o in ONES]


def _inv_designed(rng, n, embed):
    """n coefficients; embed(k) the plain coefficients of the Fq element k."""
    out = [("designed:zero:%d" % i, z) for i, z in enumerate(_zero_mixes(rng, n, 30))]
    k = _rp(rng)
    for name, vals in (("one", embed(1)), ("minus_one", embed(P - 1)), ("fq", embed(k))):
        out.append(("designed:unit:%s" % name, _raws(vals)))
        out.append(("designed:unit:%s:lifted" % name, _raws(vals, 1)))
    return out


def _is_one_designed(rng, n):
    out = [("designed:true:%d" % i, v) for i, v in enumerate(_one_mixes(rng, n, 20))]
    one = [RM] + [0] * (n - 1)
    for k in range(1, n):
        out.append(("designed:false:coefficient%d=1" % k, one[:k] + [1] + one[k + 1:]))
    out.append(("designed:false:word1_for_R", [1] + [0] * (n - 1)))
    out.append(("designed:false:R+1", [RM + 1] + [0] * (n - 1)))
    out.append(("designed:false:R+1:lifted", [RM + 1 + P] + [P] * (n - 1)))
    for last in (1, P - 1, P + 1, 2 * P - 1, rng.randrange(2, P)):
        out.append(("designed:false:last=%d" % (last % 1000), one[:-1] + [last]))
        out.append(("designed:false:only_last=%d" % (last % 1000), [0] * (n - 1) + [last]))
    out.append(("designed:false:zero", [0] * n))
    out.append(("designed:false:2R", [2 * RM % P] + [0] * (n - 1)))
    return out


def _single_component(rng, to_rows):
    """Fq12 elements with exactly one non-zero Fq2 component (reference component c = 0 .. 5), in three shapes."""
    out = []
    for c in range(6):
        for shape, val in (("both", _rp2(rng)), ("c0", (_rp(rng), 0)), ("c1", (0, _rp(rng)))):
            six = [pm.F2_ZERO] * 6
            six[c] = val
            a = (tuple(six[:3]), tuple(six[3:]))
            out.append(("designed:single:component%d:%s" % (c, shape), _raws(to_rows(a))))
            out.append(("designed:single:component%d:%s:lifted" % (c, shape), _raws(to_rows(a), 1)))
    return out


def _sparse_designed(rng):
    out = []
    for zi, zn in enumerate(("o", "vw", "vv")):
        for z, zname in zip(ZEROS, ("0", "p", "2p")):
            a = _rand_rows(rng, 12)
            line = _rand_rows(rng, 6)
            line[2 * zi] = line[2 * zi + 1] = z
            out.append(("designed:line:%s=%s" % (zn, zname), a + line))
    for i, one in enumerate(_one_mixes(rng, 12, 4)):
        out.append(("designed:acc_one:%d" % i, one + _rand_rows(rng, 6)))  # the constant term is coefficient 0 in both bases
    for c, cn in zip(CORNERS, CORNER_NAMES):
        out.append(("designed:acc_one:line=%s" % cn, [RM + P] + [2 * P] * 11 + [c] * 6))
        for zi, zn in enumerate(("o", "vw", "vv")):
            line = [c] * 6
            line[2 * zi] = line[2 * zi + 1] = 2 * P
            out.append(("designed:line:%s=2p:rest=%s" % (zn, cn), [c] * 12 + line))
    return out


def _w_pairs():
    out = []
    for i in range(6):
        for j in range(6):
            for val, vn in ((RM, "R"), (2 * P - 1, "2p-1")):
                a, b = [0] * 12, [0] * 12
                a[2 * i] = a[2 * i + 1] = b[2 * j] = b[2 * j + 1] = val
                out.append(("designed:pair:%d,%d:%s" % (i, j, vn), a + b))
    return out


def _lift_variants(rows):
    """The rows as they are, each row once lifted by p, all rows lifted."""
    out = [("", list(rows))]
    for k in range(len(rows)):
        out.append((":lift%d" % k, [r + P if i == k else r for i, r in enumerate(rows)]))
    out.append((":lifted", [r + P for r in rows]))
    return out


def _aff_rows(q, lift=0):
    return _raws([*q[0], *q[1]], lift)


def _designed_vectors(op, rng):
    name = OPS[op].name
    out = []
    if op == 5:  # f2_mul
        for side in (0, 2):
            for extra, tag in ((0, "2p"), (1, "2p+1")):
                for i in range(4):
                    v = _rand_rows(rng, 4)
                    v[side] = rng.randrange(1 + extra, 2 * P)
                    v[side + 1] = 2 * P + extra - v[side]
                    out.append(("designed:sum_%s:%s:%d" % (tag, "ab"[side // 2], i), v))
        while sum(n.startswith("designed:t0_lt_t1") for n, _ in out) < 8:
            v = _rand_rows(rng, 4)
            if mont_mul_raw(v[0], v[2]) < mont_mul_raw(v[1], v[3]):
                out.append(("designed:t0_lt_t1:%d" % len(out), v))
        for i in range(8):
            a0, a1, b0 = _rp(rng), _rp(rng), _rp(rng)
            b1 = a0 * b0 * pow(a1, -1, P) % P
            out.append(("designed:t0_eq_t1:%d" % i, [raw(a0, i & 1), raw(a1, (i >> 1) & 1), raw(b0, (i >> 2) & 1), raw(b1, i & 1)]))
    elif op == 6:  # f2_sqr
        for i in range(4):
            x = _rp(rng)
            out.append(("designed:c0_eq_c1:%d" % i, [raw(x, i & 1), raw(x, i >> 1)]))
            out.append(("designed:c0_eq_neg_c1:%d" % i, [raw(x, i & 1), raw(-x, i >> 1)]))
        x = rng.randrange(1, 2 * P)
        out.append(("designed:c0_eq_neg_c1:raw", [x, 2 * P - x]))
    elif op == 9:
        out += _inv_designed(rng, 2, lambda k: [k, 0])
    elif op == 26:
        out += _inv_designed(rng, 6, lambda k: [k] + [0] * 5)
    elif op in (33, 57):
        out += _inv_designed(rng, 12, lambda k: [k] + [0] * 11)
    elif op == 11:  # f2_is_zero
        out += [("designed:true:%d" % i, z) for i, z in enumerate(_zero_mixes(rng, 2, 9))]
        for z, zn in zip(ZEROS, ("0", "p", "2p")):
            for miss, mn in ((1, "1"), (RM, "R"), (RM + 1, "R+1"), (P - 1, "p-1"), (P + 1, "p+1"), (2 * P - 1, "2p-1")):
                out.append(("designed:false:c0=%s:c1=%s" % (mn, zn), [miss, z]))
                out.append(("designed:false:c0=%s:last=%s" % (zn, mn), [z, miss]))
    elif op == 12:  # f2_eq
        for i in range(16):
            a = _rp2(rng)
            out.append(("designed:true:%d" % i, [raw(a[0], i & 1), raw(a[1], (i >> 1) & 1), raw(a[0], (i >> 2) & 1), raw(a[1], (i >> 3) & 1)]))
            k = i & 3
            v = [raw(a[0], i & 1), raw(a[1], (i >> 1) & 1), raw(a[0], (i >> 2) & 1), raw(a[1], (i >> 3) & 1)]
            v[k] += 1 if v[k] < 2 * P else -1
            out.append(("designed:false:coefficient%d_off_by_one:%d" % (k, i), v))
        out += [("designed:true:zero:%d" % i, z) for i, z in enumerate(_zero_mixes(rng, 4, 81))]
    elif op in (40, 59):
        out += _is_one_designed(rng, 12)
    elif op == 35:  # f12_cyclotomic_sqr
        for i, e in enumerate(cyclotomic_elements()):
            out.append(("designed:cyclotomic:%d" % i, _raws(flat12(e), 0)))
        out.append(("designed:cyclotomic:0:lifted", _raws(flat12(cyclotomic_elements()[0]), 1)))
        out.append(("designed:cyclotomic:one", [RM] + [0] * 11))
    elif op in (36, 37, 38):
        out += _single_component(rng, flat12)
    elif op in (54, 55, 56):
        out += _single_component(rng, pwm.to_w)
    elif op in (39, 52):
        out += _sparse_designed(rng)
    elif op in (50, 51):
        out += _w_pairs()
    elif op == 60:  # g2_on_twist
        g, m, _, _, outside = g2_points()
        out.append(("designed:true:generator", _aff_rows(g)))
        out.append(("designed:true:multiple:lifted", _aff_rows(m, 1)))
        out.append(("designed:true:outside_subgroup", _aff_rows(outside)))
        for tag, q in (("generator", g), ("multiple", m)):
            rows = _aff_rows(q)
            for k, cn in enumerate(("x.c0", "x.c1", "y.c0", "y.c1")):
                out.append(("designed:false:%s:%s+1" % (tag, cn), [r + 1 if i == k else r for i, r in enumerate(rows)]))
                out.append(("designed:false:%s:%s-1:lifted" % (tag, cn), [r + P - 1 if i == k else r + P for i, r in enumerate(rows)]))
    elif op == 61:  # g2_dbl
        g, m, big, _, _ = g2_points()
        for i, z in enumerate(_zero_mixes(rng, 2, 9)):
            out.append(("designed:infinity:%d" % i, _rand_rows(rng, 4) + z))
        for tag, q in (("generator", g), ("multiple", big)):
            for sfx, rows in _lift_variants(_raws(jac(q, _rp2(rng)))):
                out.append(("designed:generic:%s%s" % (tag, sfx), rows))
        out.append(("designed:generic:z=1", _raws(jac(m, pm.F2_ONE))))
    elif op == 62:  # g2_madd
        g, m, big, near, _ = g2_points()
        for i, z in enumerate(_zero_mixes(rng, 2, 9)):
            out.append(("designed:p_infinite:%d" % i, _rand_rows(rng, 4) + z + _aff_rows(m, i & 1)))
        for tag, q in (("generator", g), ("multiple", big)):
            for sfx, rows in _lift_variants(_raws(jac(q, _rp2(rng)))):
                out.append(("designed:p_eq_q:%s%s" % (tag, sfx), rows + _aff_rows(q)))
                out.append(("designed:p_eq_minus_q:%s%s" % (tag, sfx), rows + _aff_rows(pm.g2_neg(q))))
            out.append(("designed:p_eq_q:%s:q_lifted" % tag, _raws(jac(q, _rp2(rng))) + _aff_rows(q, 1)))
            out.append(("designed:p_eq_minus_q:%s:q_lifted" % tag, _raws(jac(q, _rp2(rng))) + _aff_rows(pm.g2_neg(q), 1)))
        out.append(("designed:generic:sum", _raws(jac(m, _rp2(rng))) + _aff_rows(big)))
        out.append(("designed:generic:sum:lifted", _raws(jac(big, _rp2(rng)), 1) + _aff_rows(g, 1)))
        out.append(("designed:generic:z=1", _raws(jac(near, pm.F2_ONE)) + _aff_rows(g)))   # (r - 2) G + G = -G
    elif op in (63, 64):  # the first steps of the Miller loop of the generator and of one other point
        g, _, big, _, _ = g2_points()
        for tag, q in (("generator", g), ("other", big)):
            cur, doubles, adds = (q[0], q[1], pm.F2_ONE), 0, 0
            for bit in pm.LOOP_BITS:
                if doubles >= 3 and adds >= 3:
                    break
                if op == 63 and doubles < 3:
                    out.append(("designed:step:%s:%d" % (tag, doubles), _raws(flat6(cur))))
                    out.append(("designed:step:%s:%d:lifted" % (tag, doubles), _raws(flat6(cur), 1)))
                cur, _ = pm.doubling_step(cur)
                doubles += 1
                if bit:
                    base = q if bit == 1 else pm.g2_neg(q)
                    if op == 64 and adds < 3:
                        out.append(("designed:step:%s:%d" % (tag, adds), _aff_rows(base) + _raws(flat6(cur))))
                        out.append(("designed:step:%s:%d:lifted" % (tag, adds), _aff_rows(base, 1) + _raws(flat6(cur), 1)))
                    cur, _ = pm.mixed_addition_step(base, cur)
                    adds += 1
    elif op == 65:
        g, _, big, _, _ = g2_points()
        for tag, q in (("generator", g), ("other", big)):
            out.append(("designed:%s" % tag, _aff_rows(q)))
            out.append(("designed:%s:lifted" % tag, _aff_rows(q, 1)))
    assert all(n.startswith("designed:") for n, _ in out), name
    return out


Built = namedtuple("Built", "op names operands expected")


@functools.lru_cache(maxsize=None)
def build(op):
    """The vectors of one op: names, operand rows (raw integers) and expected rows (Montgomery residues below p; see the module text)."""
    o = OPS[op]
    rng = random.Random(0x70BE5 + op)
    vectors = _corner_vectors(op, rng) + _designed_vectors(op, rng) + _random_vectors(op, rng)
    names, operands, expected = [], [], []
    for name, v in vectors:
        assert len(v) == o.nin, (o.name, name, len(v))
        res = list(o.model([plain(r) for r in v]))
        kinds = ["flag"] + ["canon"] * 4 if o.kinds[0] == "point" else o.kinds
        assert len(res) == len(kinds), (o.name, name)
        names.append(name)
        operands.append(v)
        expected.append([r if k in ("bool", "flag") else raw(r) for r, k in zip(res, kinds)])
    return Built(op, names, operands, expected)


def rows_to_words(rows):
    """A list of vectors of integers below 2^256 as nested lists of eight 32-bit words."""
    return [[[(r >> (32 * w)) & 0xFFFFFFFF for w in range(8)] for r in v] for v in rows]


def words_to_int(words):
    return sum(int(w) << (32 * i) for i, w in enumerate(words))


def check(op, operands, expected, got):
    """None, or what is wrong with the result rows `got` (integers) of one vector, the first differing row named."""
    o = OPS[op]
    for k, g in enumerate(got):
        if o.kinds[k] not in ("bool",) and g > 2 * P:
            return "result row %d is above 2p: %#x" % (k, g)
    if o.kinds[0] == "point":
        q = jac_affine([plain(g) for g in got])
        want = None if expected[0] else ((plain(expected[1]), plain(expected[2])), (plain(expected[3]), plain(expected[4])))
        if q != want:
            return "the point (X, Y, Z) normalises to %s, the model's sum is %s" % (q, want)
        return None
    for k, (kind, g, e) in enumerate(zip(o.kinds, got, expected)):
        if kind == "res" and g % P != e:
            return "result row %d: residue %#x, the model's %#x (raw %#x)" % (k, g % P, e, g)
        if kind == "canon" and g != e:
            return "result row %d: words %#x, the model's canonical %#x" % (k, g, e)
        if kind == "bool" and g != e:
            return "result row %d: boolean row %#x, the model's %d" % (k, g, e)
        if kind == "same" and (g != operands[k] or g % P != e):
            return "result row %d: raw words %#x, the operand's %#x" % (k, g, operands[k])
    return None
