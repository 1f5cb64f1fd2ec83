"""Big-integer model of the bucket accumulation's mixed addition as csrc/curve29.hip.h runs it: sums folded into the high columns of the
product before them (F29Job ADD), runs started without a zeroed accumulator (test tooling for tests/test_acc29_bounds_cpu.py).

Two views of the same sequence of operations:
  * madd() computes with Python integers limb by limb and asserts what the kernel relies on at every step -- no 32-bit limb overflow, no
    negative limb in a subtraction, every column sum below COLUMN_LIMIT, exact output limbs;
  * madd_bounds() carries only the MAXIMUM each limb of each value can take and evaluates every column with all limbs at that maximum
    at once (an upper bound no input reaches: it ignores that the limbs of one value cannot all be maximal together).
"""
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47  # BN254 Fq
M29 = (1 << 29) - 1
R1 = 1 << 261
INV29 = (-pow(P, -1, 1 << 29)) % (1 << 29)
U32 = 1 << 32
COLUMN_LIMIT = 1 << 63  # v_mad_u64_u32 wraps at 2^64; the accumulation keeps one bit of that in hand


def limbs(v):
    assert 0 <= v < (1 << (29 * 8 + 32))
    return [(v >> (29 * j)) & M29 for j in range(8)] + [v >> 232]


def val(a):
    return sum(x << (29 * i) for i, x in enumerate(a))


P29 = limbs(P)
ONE = limbs(R1 % P)


def spread(mult, e):  # Spread29<P, J, M, E>
    q = limbs(mult * P)
    up, down = 1 << e, 1 << (e - 29)
    s = [q[0] + up] + [q[j] + up - down for j in range(1, 8)] + [q[8] - down]
    assert val(s) == mult * P and s[8] >= 0
    return s


def sub(a, b, mult, e=30):  # f29_sub<M, E>; f29_neg<M, E>(b) is sub(zero, b)
    r = []
    for x, y, c in zip(a, b, spread(mult, e)):
        assert c - y >= 0, "subtrahend limb above the spread constant"
        assert x + (c - y) < U32, "limb overflow in f29_sub"
        r.append(x + (c - y))
    return r


def neg(b, mult, e=30):
    return sub([0] * 9, b, mult, e)


def carry(a):  # f29_carry
    assert all(0 <= x < U32 for x in a)
    r = [a[0] & M29] + [(a[i] & M29) + (a[i - 1] >> 29) for i in range(1, 8)] + [a[8] + (a[7] >> 29)]
    assert all(x < U32 for x in r)
    return r


STATS = {"max_column": 0}


def mont(chains, add=None):
    """One reduction over the sum of a * b of all chains; add: 9 limbs added to the result through columns 9 .. 16 and the top limb."""
    acc, m, r = 0, [0] * 9, [0] * 9
    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        for a, b in chains:
            acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        if add is not None and k >= 9:
            assert 0 <= add[k - 9] < U32
            acc += add[k - 9]
        acc += sum(m[i] * P29[k - i] for i in range(lo, hi + 1 if k > 8 else k))
        if k <= 8:
            m[k] = ((acc & 0xFFFFFFFF) * INV29) & M29
            acc += m[k] * P29[0]
            assert acc & M29 == 0
        else:
            r[k - 9] = acc & M29
        STATS["max_column"] = max(STATS["max_column"], acc)
        assert acc < COLUMN_LIMIT, "column sum leaves 63 bits"
        acc >>= 29
    r[8] = acc + (add[8] if add is not None else 0)
    assert r[8] < U32
    want = sum(val(a) * val(b) for a, b in chains)
    extra = val(add) if add is not None else 0
    assert (val(r) * R1 - want - extra * R1) % P == 0 and val(r) < want // R1 + P + 1 + extra
    return r


def aff_from_table(px, py, negative):  # aff29_from_table: the sign on the 8 x u32 words, then the split at a 5-bit offset
    assert 0 < py < P and 0 <= px < P
    return limbs(px << 5), limbs((P - py if negative else py) << 5)


def start(x2, y2):
    return [list(x2), list(y2), list(ONE), list(ONE)]


def madd(acc, x2, y2):  # xyzz29_madd
    x1, y1, zz1, zzz1 = acc
    p_ = mont([(x2, zz1)], neg(x1, 34))
    r_ = mont([(y2, zzz1)], neg(y1, 34))
    pp = mont([(p_, p_)])
    assert all(2 * x < U32 for x in p_ + r_)  # the doubled operands of the squares
    ppp, q = mont([(p_, pp)]), mont([(x1, pp)])
    s = [a + 2 * b for a, b in zip(ppp, q)]
    x3 = mont([(r_, r_)], neg(s, 12, 31))
    zz3 = mont([(zz1, pp)])
    t = carry(sub(q, x3, 24))
    y3 = mont([(r_, t), (neg(y1, 64, 30), ppp)])
    zzz3 = mont([(zzz1, ppp)])
    return [x3, y3, zz3, zzz3]


def madd_mod(ref, x2, y2, mul):
    """The same formulas on residues; mul(a, b) = a * b / R' mod p supplied by the caller (plain integers or the oracle)."""
    x1, y1, zz1, zzz1 = ref
    u2, s2 = mul(x2, zz1), mul(y2, zzz1)
    p_, r_ = (u2 - x1) % P, (s2 - y1) % P
    pp = mul(p_, p_)
    ppp, q = mul(p_, pp), mul(x1, pp)
    x3 = (mul(r_, r_) - ppp - 2 * q) % P
    y3 = (mul(r_, (q - x3) % P) - mul(y1, ppp)) % P
    return [x3, y3, mul(zz1, pp), mul(zzz1, ppp)]


# ---------------------------------------------------------------------------------------------- worst-case limbs
def top(bound):
    """Top limb of a value below bound * p."""
    return ((int(round(bound * 10)) * P // 10) >> 232) + 1


def exact(bound):  # a product's output: limbs < 2^29, top limb by the value bound
    return [M29] * 8 + [top(bound)]


def column_max(chains, add=None):
    """Largest column sum of a product whose operand limbs are all at the given maxima (digits all 2^29 - 1, carried-in value included)."""
    worst, acc = 0, 0
    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        acc += sum(a[i] * b[k - i] for a, b in chains for i in range(lo, hi + 1))
        acc += sum(M29 * P29[k - i] for i in range(lo, hi + 1))
        if add is not None and k >= 9:
            acc += add[k - 9]
        worst = max(worst, acc)
        acc >>= 29
    return worst


def madd_bounds():
    """{product: largest column sum} of one mixed addition from the entry bounds of curve29.hip.h: X, Y < 32p, ZZ, ZZZ < 1.4p, limbs
    < 2^29 + 8 (what the header states; the kernel's own values have exact limbs); the table point canonical << 5, its y = p - y for a
    negative digit (the same bound).  Value bounds as the comments of xyzz29_madd derive them, rounded up."""
    lazy = lambda bound: [M29 + 8] * 8 + [top(bound)]
    x1, y1, zz1, zzz1 = lazy(32), lazy(32), lazy(1.4), lazy(1.4)
    x2 = y2 = exact(32)
    nx, ny = spread(34, 30), spread(34, 30)          # 34p - X1 <= the constant itself
    out = {"P = U2 + (34p - X1)": column_max([(x2, zz1)], nx), "R = S2 + (34p - Y1)": column_max([(y2, zzz1)], ny)}
    p_, r_ = exact(35.3), exact(35.3)
    pp = exact(8.4)
    out["PP = P^2"] = column_max([(p_, p_)])
    out["PPP = P PP"] = column_max([(p_, pp)])
    out["Q = X1 PP"] = column_max([(x1, pp)])
    out["X3 = R^2 + (12p - PPP - 2Q)"] = column_max([(r_, r_)], spread(12, 31))
    out["ZZ3 = ZZ1 PP"] = column_max([(zz1, pp)])
    t = lazy(26.6)
    ppp = exact(2.8)
    out["Y3 = R T + (64p - Y1) PPP"] = column_max([(r_, t), (spread(64, 30), ppp)])
    out["ZZZ3 = ZZZ1 PPP"] = column_max([(zzz1, ppp)])
    return out
