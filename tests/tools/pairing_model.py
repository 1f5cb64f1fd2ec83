"""Integer model of the BN254 pairing as the reference computes it (ecc/curves/bn254/pairing_impl.hpp, fields/field2/6/12.hpp): the tower
Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v) with xi = 9 + u, the group law of the twist y^2 = x^3 + 3/xi, the
line functions of the flipped Miller loop, the loop itself (one pair and a batch), both halves of the final exponentiation, and the bytes of
pairing::miller_lines.  Python integers only, plain residues (not Montgomery form); to_words() makes the Montgomery words of the device.

Every constant is DERIVED here from the BN parameter z, the modulus p(z) and xi; scripts/gen_pairing_consts.py renders the same values
into csrc/pairing_consts.hip.h.  The one constant that is a convention and not a consequence is the generator of G2: it is the point of
the alt_bn128 curve description (EIP-197), checked here to lie on the twist and in the subgroup of order r.

Fq2 = (c0, c1), Fq6 = (c0, c1, c2) of Fq2, Fq12 = (c0, c1) of Fq6; a G2 point is None (infinity) or (x, y) of Fq2."""
import numpy as np

Z = 4965661367192848881  # the BN parameter: p = 36 z^4 + 36 z^3 + 24 z^2 + 6 z + 1, r = 36 z^4 + 36 z^3 + 18 z^2 + 6 z + 1
P = 36 * Z**4 + 36 * Z**3 + 24 * Z**2 + 6 * Z + 1
R = 36 * Z**4 + 36 * Z**3 + 18 * Z**2 + 6 * Z + 1
MONT = 1 << 256
XI = (9, 1)
G1 = (1, 2)
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
       11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930,
       4082367875863433681332203403145435568316851327593401208105741076214120093531))
assert P == 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
assert R == 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
LINES = 87
LINES_BYTES = LINES * 3 * 64


# ------------------------------------------------------------------------------------------------ Fq2
F2_ZERO, F2_ONE = (0, 0), (1, 0)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_sqr(a):
    return ((a[0] + a[1]) * (a[0] - a[1]) % P, 2 * a[0] * a[1] % P)


def f2_mul_fq(a, k):
    return (a[0] * k % P, a[1] * k % P)


def f2_conj(a):  # the Frobenius map of Fq2
    return (a[0], -a[1] % P)


def f2_inv(a):
    t = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * t % P, -a[1] * t % P)


def f2_mul_xi(a):  # (9 + u) a
    return ((9 * a[0] - a[1]) % P, (9 * a[1] + a[0]) % P)


def f2_pow(a, e):
    out = F2_ONE
    for bit in bin(e)[2:]:
        out = f2_sqr(out)
        if bit == "1":
            out = f2_mul(out, a)
    return out


def f2_sqrt(a):
    """A square root of a in Fq2, or None (p = 3 mod 4: through the norm and two square roots in Fq)."""
    if a == F2_ZERO:
        return F2_ZERO
    n = (a[0] * a[0] + a[1] * a[1]) % P
    s = pow(n, (P + 1) // 4, P)
    if s * s % P != n:
        return None
    inv2 = (P + 1) // 2
    for t in ((a[0] + s) * inv2 % P, (a[0] - s) * inv2 % P):
        x0 = pow(t, (P + 1) // 4, P)
        if x0 * x0 % P == t and x0:
            x = (x0, a[1] * pow(2 * x0, P - 2, P) % P)
            if f2_sqr(x) == a:
                return x
    if a[1] == 0:  # a in Fq and not a square there: a = (u y)^2 with y^2 = -a
        y = pow(-a[0] % P, (P + 1) // 4, P)
        if f2_sqr((0, y)) == a:
            return (0, y)
    return None


# ------------------------------------------------------------------------------------------------ the derived constants
TWO_INV = (P + 1) // 2
TWIST_B = f2_mul_fq(f2_inv(XI), 3)                    # b' = 3 / xi
TWIST_MUL_BY_Q_X = f2_pow(XI, (P - 1) // 3)           # pi(x, y) = (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2)) on the twist
TWIST_MUL_BY_Q_Y = f2_pow(XI, (P - 1) // 2)
FROB6_C1 = {k: f2_pow(XI, (P**k - 1) // 3) for k in (1, 2, 3)}      # v^(p^k) = xi^((p^k - 1)/3) v
FROB6_C2 = {k: f2_pow(XI, 2 * (P**k - 1) // 3) for k in (1, 2, 3)}  # (v^2)^(p^k)
FROB12 = {k: f2_pow(XI, (P**k - 1) // 6) for k in (1, 2, 3)}        # w^(p^k) = xi^((p^k - 1)/6) w


def naf(n):
    """The non-adjacent form of n > 0, least significant digit first, digits in {-1, 0, 1}."""
    out = []
    while n:
        d = 0
        if n & 1:
            d = 2 - (n & 3)
            n -= d
        out.append(d)
        n >>= 1
    return out


# the Miller loop starts from Q, the leading bit 2^64 of 6 z + 2, and walks what is below it in non-adjacent form, 64 digits from the top:
# 0, 1 (add Q) or 3 (add -Q)
_LOOP = 6 * Z + 2
_LOW = naf(_LOOP - (1 << (_LOOP.bit_length() - 1)))
LOOP_BITS = [{0: 0, 1: 1, -1: 3}[d] for d in reversed(_LOW + [0] * (_LOOP.bit_length() - 1 - len(_LOW)))]
# the exponentiation by z walks the bits of z below the leading one
NEG_Z_LOOP_BITS = [int(b) for b in bin(Z)[3:]]
assert len(LOOP_BITS) == 64 and len(NEG_Z_LOOP_BITS) == 62
assert len(LOOP_BITS) + sum(1 for b in LOOP_BITS if b) + 2 == LINES


# ------------------------------------------------------------------------------------------------ Fq6, Fq12
F6_ZERO, F6_ONE = (F2_ZERO,) * 3, (F2_ONE, F2_ZERO, F2_ZERO)
F12_ONE = (F6_ONE, F6_ZERO)


def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def f6_neg(a):
    return tuple(f2_neg(x) for x in a)


def f6_mul(a, b):
    t0, t1, t2 = f2_mul(a[0], b[0]), f2_mul(a[1], b[1]), f2_mul(a[2], b[2])
    t3 = f2_mul(f2_add(a[0], a[2]), f2_add(b[0], b[2]))
    t4 = f2_mul(f2_add(a[0], a[1]), f2_add(b[0], b[1]))
    t5 = f2_mul(f2_add(a[1], a[2]), f2_add(b[1], b[2]))
    return (f2_add(t0, f2_mul_xi(f2_sub(t5, f2_add(t1, t2)))),
            f2_add(f2_sub(t4, f2_add(t0, t1)), f2_mul_xi(t2)),
            f2_sub(f2_add(t3, t1), f2_add(t0, t2)))


def f6_sqr(a):
    return f6_mul(a, a)


def f6_mul_v(a):  # times v: field12::mul_by_non_residue
    return (f2_mul_xi(a[2]), a[0], a[1])


def f6_mul_f2(a, k):
    return tuple(f2_mul(x, k) for x in a)


def f6_inv(a):
    c0 = f2_sub(f2_sqr(a[0]), f2_mul_xi(f2_mul(a[1], a[2])))
    c1 = f2_sub(f2_mul_xi(f2_sqr(a[2])), f2_mul(a[0], a[1]))
    c2 = f2_sub(f2_sqr(a[1]), f2_mul(a[0], a[2]))
    t = f2_inv(f2_add(f2_mul(a[0], c0), f2_mul_xi(f2_add(f2_mul(a[2], c1), f2_mul(a[1], c2)))))
    return (f2_mul(t, c0), f2_mul(t, c1), f2_mul(t, c2))


def f6_frobenius(a, k):
    m = f2_conj if k & 1 else (lambda x: x)
    return (m(a[0]), f2_mul(FROB6_C1[k], m(a[1])), f2_mul(FROB6_C2[k], m(a[2])))


def f12_mul(a, b):
    t0, t1 = f6_mul(a[0], b[0]), f6_mul(a[1], b[1])
    return (f6_add(f6_mul_v(t1), t0), f6_sub(f6_mul(f6_add(a[0], a[1]), f6_add(b[0], b[1])), f6_add(t0, t1)))


def f12_sqr(a):
    t1 = f6_mul(a[0], a[1])
    t0 = f6_mul(f6_add(a[0], a[1]), f6_add(f6_mul_v(a[1]), a[0]))
    return (f6_sub(t0, f6_add(t1, f6_mul_v(t1))), f6_add(t1, t1))


def f12_inv(a):
    t = f6_inv(f6_sub(f6_sqr(a[0]), f6_mul_v(f6_sqr(a[1]))))
    return (f6_mul(a[0], t), f6_neg(f6_mul(a[1], t)))


def f12_conj(a):  # unitary_inverse
    return (a[0], f6_neg(a[1]))


def f12_cyclotomic_sqr(a):
    """The square of an element of the cyclotomic subgroup by Granger and Scott, as csrc/fq_tower.hip.h computes it: three squarings in
    Fq4 = Fq2[s]/(s^2 - xi).  Equal to f12_sqr(a) on the subgroup only."""
    def f4_sqr(x, y):
        m = f2_mul(x, y)
        return f2_sub(f2_mul(f2_add(x, y), f2_add(f2_mul_xi(y), x)), f2_add(m, f2_mul_xi(m))), f2_add(m, m)

    def minus(t, z):  # 3 t - 2 z
        return f2_add(f2_mul_fq(f2_sub(t, z), 2), t)

    def plus(t, z):  # 3 t + 2 z
        return f2_add(f2_mul_fq(f2_add(t, z), 2), t)
    (c00, c01, c02), (c10, c11, c12) = a
    t0, t1 = f4_sqr(c00, c11)
    t2, t3 = f4_sqr(c10, c02)
    t4, t5 = f4_sqr(c01, c12)
    return ((minus(t0, c00), minus(t2, c01), minus(t4, c02)), (plus(f2_mul_xi(t5), c10), plus(t1, c11), plus(t3, c12)))


def f12_frobenius(a, k):
    return (f6_frobenius(a[0], k), f6_mul_f2(f6_frobenius(a[1], k), FROB12[k]))


def f12_pow(a, e):
    out = F12_ONE
    for bit in bin(e)[2:] if e else "":
        out = f12_sqr(out)
        if bit == "1":
            out = f12_mul(out, a)
    return out


def f12_sparse_mul(a, line):
    """a times the sparse element (o, 0, vv) + w (0, vw, 0): field12::self_sparse_mul, by the full product."""
    o, vw, vv = line
    return f12_mul(a, ((o, F2_ZERO, vv), (F2_ZERO, vw, F2_ZERO)))


class PowerTable:
    """g^e for many e below 2^256 by 4-bit windows: 64 multiplications each after 960 once."""

    def __init__(self, g):
        self.rows = []
        base = g
        for _ in range(64):
            row = [F12_ONE, base]
            for _ in range(14):
                row.append(f12_mul(row[-1], base))
            self.rows.append(row)
            base = f12_mul(row[15], base)

    def pow(self, e):
        out = None
        for w in range(64):
            d = (e >> (4 * w)) & 15
            if d:
                out = self.rows[w][d] if out is None else f12_mul(out, self.rows[w][d])
        return F12_ONE if out is None else out


# ------------------------------------------------------------------------------------------------ G2: affine group law on the twist
def g2_on_twist(q):
    return q is None or f2_sqr(q[1]) == f2_add(f2_mul(f2_sqr(q[0]), q[0]), TWIST_B)


def g2_neg(q):
    return None if q is None else (q[0], f2_neg(q[1]))


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if a[1] != b[1] or a[1] == F2_ZERO:
            return None
        lam = f2_mul(f2_mul_fq(f2_sqr(a[0]), 3), f2_inv(f2_mul_fq(a[1], 2)))
    else:
        lam = f2_mul(f2_sub(b[1], a[1]), f2_inv(f2_sub(b[0], a[0])))
    x = f2_sub(f2_sub(f2_sqr(lam), a[0]), b[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(a[0], x)), a[1]))


def g2_mul(q, s):
    out = None
    for bit in bin(s)[2:] if s else "":
        out = g2_add(out, out)
        if bit == "1":
            out = g2_add(out, q)
    return out


def g2_point_outside_subgroup():
    """A point of the twist that is NOT of order r: the twist has r (2p - r) points, so a point found from its x coordinate alone, the
    cofactor not cleared, is outside the subgroup unless chance (one in 2p - r) puts it there."""
    x0 = 1
    while True:
        x = (x0, 1)
        y = f2_sqrt(f2_add(f2_mul(f2_sqr(x), x), TWIST_B))
        if y is not None and g2_mul((x, y), R) is not None:
            return (x, y)
        x0 += 1


# ------------------------------------------------------------------------------------------------ G1 (only what the tests need)
def g1_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], P - 2, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], P - 2, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def g1_mul(a, s):
    out = None
    for bit in bin(s)[2:] if s else "":
        out = g1_add(out, out)
        if bit == "1":
            out = g1_add(out, a)
    return out


# ------------------------------------------------------------------------------------------------ lines (pairing_impl.hpp:23-123)
def doubling_step(cur):
    """(the doubled projective point, the line (o, vw, vv)): doubling_step_for_flipped_miller_loop."""
    x, y, z = cur
    a = f2_mul(f2_mul_fq(x, TWO_INV), y)
    b, c = f2_sqr(y), f2_sqr(z)
    d = f2_add(f2_add(c, c), c)
    e = f2_mul(d, TWIST_B)
    f = f2_add(f2_add(e, e), e)
    g = f2_mul_fq(f2_add(b, f), TWO_INV)
    h = f2_sub(f2_sqr(f2_add(y, z)), f2_add(b, c))
    i = f2_sub(e, b)
    j = f2_sqr(x)
    ee = f2_sqr(e)
    k = f2_sub(b, f)
    nx = f2_mul(a, k)
    k = f2_add(f2_add(ee, ee), ee)
    ny = f2_sub(f2_sqr(g), k)
    nz = f2_mul(b, h)
    return (nx, ny, nz), (f2_mul_xi(i), f2_neg(h), f2_add(f2_add(j, j), j))


def mixed_addition_step(base, cur):
    """(cur + base, the line): mixed_addition_step_for_flipped_miller_loop; base = (x, y) affine."""
    x, y, z = cur
    d = f2_sub(x, f2_mul(base[0], z))
    e = f2_sub(y, f2_mul(base[1], z))
    f, g = f2_sqr(d), f2_sqr(e)
    h = f2_mul(d, f)
    i = f2_mul(x, f)
    j = f2_sub(f2_sub(f2_add(f2_mul(z, g), h), i), i)
    nx = f2_mul(d, j)
    ny = f2_sub(f2_mul(f2_sub(i, j), e), f2_mul(y, h))
    nz = f2_mul(z, h)
    o = f2_mul_xi(f2_sub(f2_mul(e, base[0]), f2_mul(d, base[1])))
    return (nx, ny, nz), (o, d, f2_neg(e))  # (o, vw, vv)


def mul_by_q(q):
    return (f2_mul(TWIST_MUL_BY_Q_X, f2_conj(q[0])), f2_mul(TWIST_MUL_BY_Q_Y, f2_conj(q[1])))


def precompute_miller_lines(q):
    """The 87 lines (o, vw, vv) of the finite point q."""
    lines = []
    neg = (q[0], f2_neg(q[1]))
    cur = (q[0], q[1], F2_ONE)
    for bit in LOOP_BITS:
        cur, line = doubling_step(cur)
        lines.append(line)
        if bit:
            cur, line = mixed_addition_step(q if bit == 1 else neg, cur)
            lines.append(line)
    q1 = mul_by_q(q)
    q2 = mul_by_q(q1)
    cur, line = mixed_addition_step(q1, cur)
    lines.append(line)
    cur, line = mixed_addition_step((q2[0], f2_neg(q2[1])), cur)
    lines.append(line)
    assert len(lines) == LINES
    return lines


def miller_loop_batch(points, tables):
    """miller_loop_batch: points[j] = (x, y) finite G1 points, tables[j] their lines."""
    f = F12_ONE
    it = 0

    def step(f, it):
        for (px, py), lines in zip(points, tables):
            o, vw, vv = lines[it]
            f = f12_sparse_mul(f, (o, f2_mul_fq(vw, py), f2_mul_fq(vv, px)))
        return f
    for bit in LOOP_BITS:
        f = step(f12_sqr(f), it)
        it += 1
        if bit:
            f = step(f, it)
            it += 1
    f = step(f, it)
    return step(f, it + 1)


def miller_loop(point, lines):
    return miller_loop_batch([point], [lines])


def final_exponentiation_easy_part(f):
    a = f12_mul(f12_conj(f), f12_inv(f))
    return f12_mul(a, f12_frobenius(a, 2))


def exp_by_neg_z(f):
    r = f
    for bit in NEG_Z_LOOP_BITS:
        r = f12_sqr(r)
        if bit:
            r = f12_mul(r, f)
    return f12_conj(r)


def final_exponentiation_tricky_part(elt):
    a = exp_by_neg_z(elt)
    b = f12_sqr(a)
    c = f12_sqr(b)
    d = f12_mul(b, c)
    e = exp_by_neg_z(d)
    f = f12_sqr(e)
    g = exp_by_neg_z(f)
    h, i = f12_conj(d), f12_conj(g)
    j = f12_mul(i, e)
    k = f12_mul(j, h)
    l_ = f12_mul(b, k)
    m = f12_mul(e, k)
    n = f12_mul(m, elt)
    o = f12_frobenius(l_, 1)
    p = f12_mul(o, n)
    q = f12_frobenius(k, 2)
    r = f12_mul(p, q)
    t = f12_mul(l_, f12_conj(elt))
    return f12_mul(r, f12_frobenius(t, 3))


def final_exponentiation(f):
    return final_exponentiation_tricky_part(final_exponentiation_easy_part(f))


def reduced_ate_pairing(p, q):
    return final_exponentiation(miller_loop(p, precompute_miller_lines(q)))


def reduced_ate_pairing_batch_precomputed(points, tables):
    """The product over the pairs; a G1 point None (infinity) contributes the factor one."""
    live = [(p, t) for p, t in zip(points, tables) if p is not None]
    return final_exponentiation(miller_loop_batch([p for p, _ in live], [t for _, t in live]))


# ------------------------------------------------------------------------------------------------ words of the device
def fq_words(vals):
    """(len, 4) uint64 Montgomery words of integers mod p."""
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = v % P * MONT % P
        for k in range(4):
            out[i, k] = (m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def fq_ints(words):
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    inv = pow(MONT, -1, P)
    return [sum(int(w[i, k]) << (64 * k) for k in range(4)) * inv % P for i in range(w.shape[0])]


def fr_words(vals, lift=0):
    """(len, 4) uint64 Montgomery words of integers mod r; lift = 1 writes the representative in [r, 2r)."""
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = v % R * MONT % R + lift * R
        for k in range(4):
            out[i, k] = (m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def f2_flat(a):
    return [a[0], a[1]]


def f12_flat(a):
    return [c for six in a for two in six for c in two]


def f12_words(a):
    """The 48 words of an fq12: c0 | c1, each c0 | c1 | c2 of fq2 = c0 | c1."""
    return fq_words(f12_flat(a)).reshape(48)


def f12_from_words(words):
    v = fq_ints(np.ascontiguousarray(words, dtype=np.uint64).reshape(12, 4))
    two = [(v[2 * i], v[2 * i + 1]) for i in range(6)]
    return (tuple(two[:3]), tuple(two[3:]))


G2_INFINITY_WORDS = np.array([0, 0, 0, 1 << 63] + [0] * 12, dtype=np.uint64)  # affine infinity: bit 63 of the top limb of x.c0


def g2_words(q):
    """The 16 words of g2::affine_element x | y; infinity in the reference's affine encoding applied to x.c0."""
    if q is None:
        return G2_INFINITY_WORDS.copy()
    return fq_words(f2_flat(q[0]) + f2_flat(q[1])).reshape(16)


def g2_from_words(words):
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(16)
    if int(w[3]) >> 63:
        return None
    v = fq_ints(w.reshape(4, 4))
    return ((v[0], v[1]), (v[2], v[3]))


G1_INFINITY_WORDS = np.array([0, 0, 0, 1 << 63] + [0] * 4, dtype=np.uint64)


def g1_words(p):
    if p is None:
        return G1_INFINITY_WORDS.copy()
    return fq_words([p[0], p[1]]).reshape(8)


def g1_from_words(words):
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(8)
    if int(w[3]) >> 63:
        return None
    v = fq_ints(w.reshape(2, 4))
    return (v[0], v[1])


def lines_words(lines):
    """pairing::miller_lines: 87 x (o | vw | vv), 2088 words."""
    flat = []
    for o, vw, vv in lines:
        flat += f2_flat(o) + f2_flat(vw) + f2_flat(vv)
    return fq_words(flat).reshape(LINES * 24)
