"""Python-integer model of the scalar recoding behind the variable-base multiplication (csrc/var_base.hip.h), shared by
tests/test_var_base_cpu.py and tests/test_gpu_var_base.py:

* split         k -> (k1, k2) with k = k1 - k2 lambda (mod r), the floors and lattice constants the device code uses.  k1 >= 0 always;
                k2 is SIGNED: it is negative for about one scalar in 2^63 (negative_half_scalar() constructs one).  Where k2 >= 0 the pair
                is what oracle.endo_split returns (the reference truncates t1 = k2 mod r to 128 bits, so it has no answer for a negative k2).
* recode        a half 0 <= h < 2^128 -> (32 odd digits in [-15, 15], most significant first, skew): h + skew = sum_i d_i 16^i.
* recombine     the value the device's 32 rounds and two skew corrections compute, for the check against k mod r.
* gpu_scalars   the scalar list of the GPU parity test with the cases it claims, and case_report() to prove they are there.
"""
import numpy as np

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # BN254 Fr
Q_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583  # BN254 Fq

# cube roots of unity (plain integers): lambda^3 = 1 mod r, beta^3 = 1 mod p, lambda (x, y) = (beta x, y) on G1
LAMBDA = 0xB3C4D79D41A917585BFC41088D8DAAA78B17EA66B99C90DD
BETA = 0x59E26BCEA0D48BACD4F263F1ACDB5C4F5763473177FFFFFE
# short basis (A1, -MB1), (A2, B2) of { (u, v) : u + v lambda = 0 mod r }, A1 = B2
MB1 = 0x6F4D8248EEB859FC8211BBEB7D4F1128
B2 = 0x89D3256894D213E3
A1 = B2
A2 = (R_MOD - B2 * B2) // MB1
G1 = (MB1 << 256) // R_MOD
G2 = (B2 << 256) // R_MOD
WINDOWS = 32
SEED = 0x5CA1AB1E


def constants_ok():
    return (pow(LAMBDA, 3, R_MOD) == 1 and LAMBDA != 1 and pow(BETA, 3, Q_MOD) == 1 and BETA != 1 and A1 * B2 + A2 * MB1 == R_MOD
            and (A1 - MB1 * LAMBDA) % R_MOD == 0 and (A2 + B2 * LAMBDA) % R_MOD == 0)


def split(k):
    """(k1, k2) for a canonical k; k2 signed."""
    assert 0 <= k < R_MOD
    c1, c2 = (G2 * k) >> 256, (G1 * k) >> 256
    k1, k2 = k - c1 * A1 - c2 * A2, c2 * B2 - c1 * MB1
    assert 0 <= k1 < 1 << 128 and abs(k2) < 1 << 128 and (k1 - k2 * LAMBDA - k) % R_MOD == 0
    return k1, k2


def recode(h):
    """(digits, skew): digits most significant first, each odd in [-15, 15], h + skew = sum d_i 16^i."""
    assert 0 <= h < 1 << 128
    skew = 1 - (h & 1)
    h |= 1
    digits = [(h >> 124) | 1]  # the top digit is positive
    for i in range(WINDOWS - 2, -1, -1):
        w = (h >> (4 * i)) & 31  # five bits: bit 4 the sign, bits 3..1 the table index
        digits.append((w | 1) - 16)
    assert all(d & 1 and -15 <= d <= 15 for d in digits)
    return digits, skew


def table_index(d):
    """Entry of T[j] = (2j + 1) P a digit selects."""
    return (abs(d) - 1) // 2


def digits_value(digits):
    acc = 0
    for d in digits:
        acc = 16 * acc + d
    return acc


def recombine(k):
    """What the device computes for k, as a multiple of P mod r: rounds over both halves, then the skew corrections."""
    k1, k2 = split(k)
    d1, s1 = recode(k1)
    d2, s2 = recode(abs(k2))
    sign2 = -1 if k2 < 0 else 1
    acc = 0
    for a, b in zip(d1, d2):
        acc = 16 * acc + a - sign2 * b * LAMBDA
    acc += -s1 + sign2 * s2 * LAMBDA
    return acc % R_MOD


def from_halves(k1, k2):
    """The scalar with these halves, if the split returns them (None otherwise: the pair is outside the split's fundamental domain)."""
    k = (k1 - k2 * LAMBDA) % R_MOD
    return k if split(k) == (k1, k2) else None


def negative_half_scalar():
    """A canonical k whose second half is negative: the first k with c1 = 1 has e1 at its minimum, 2^-65 or so."""
    k = -(-(1 << 256) // G2)
    for d in range(64):
        if split(k + d)[1] < 0:
            return k + d
    raise AssertionError("no negative second half near the first c1 = 1")


def half_bounds():
    """Exact upper bounds (k1_max, |k2|_max) over all canonical k.  With c1 = B2 k / r - e1 and c2 = MB1 k / r - e2 the floors give
    0 <= e1 < 1 + theta2 r / 2^256 and 0 <= e2 < 1 + theta1 r / 2^256 (theta = the fraction dropped from G2, G1), and
    k1 = e1 A1 + e2 A2, k2 = e1 MB1 - e2 B2.  Both bounds are below 2^127: a half of 2^127 or more does not exist for this split, so the
    top digit of a half never exceeds 7 -- the recoding itself is checked up to 2^128 - 1 all the same (tests/test_var_base_cpu.py)."""
    from fractions import Fraction
    e1 = 1 + Fraction((B2 << 256) % R_MOD, 1 << 256)
    e2 = 1 + Fraction((MB1 << 256) % R_MOD, 1 << 256)
    return e1 * A1 + e2 * A2, max(e1 * MB1, e2 * B2)


def gpu_scalars():
    """(names, plain canonical integers) of the GPU parity test: the issue's edge values, constructed halves, random full-width ones."""
    rng = np.random.default_rng(SEED + 1)
    named = [("0", 0), ("1", 1), ("2", 2), ("r - 1", R_MOD - 1), ("lambda", LAMBDA), ("lambda - 1", LAMBDA - 1), ("lambda + 1", LAMBDA + 1),
             ("r - lambda", R_MOD - LAMBDA),  # = 0 - 1 lambda, but (0, 1) lies outside the split's fundamental domain: see case_report
             ("2^127 - 1", (1 << 127) - 1), ("2^127 + 1", (1 << 127) + 1), ("2^128", 1 << 128)]
    for nib in (0x7, 0x8, 0xF):  # 63 nibbles: the widest run of one nibble below r
        named.append((f"nibbles {nib:x}", int(f"{nib:x}" * 63, 16)))
    named.append(("negative k2", negative_half_scalar()))
    # a first half close to its upper bound (top digit 7), by a deterministic search
    for j in range(400):
        k = from_halves((0x7C << 120) + 2 * j + 1, int.from_bytes(rng.bytes(16), "little") % MB1)
        if k is not None:
            named.append(("large k1", k))
            break
    # halves of one repeated digit pattern, where the split returns them
    for nib in (0x1, 0xF, 0x0, 0xE):
        h = int(f"{nib:x}" * 31, 16)
        for k1, k2 in ((h, h), (h | 1, h & ~1), (h & ~1, h | 1)):
            k = from_halves(k1, k2)
            if k is not None:
                named.append((f"halves {k1:x} / {k2:x}", k))
    n_random = 300 - len(named) - 3  # three coarse representatives join in the GPU test
    named += [(f"random {i}", int.from_bytes(rng.bytes(32), "little") % R_MOD) for i in range(n_random)]
    return [n for n, _ in named], [k for _, k in named]


def case_report(ks):
    """Which recoding branches a scalar list reaches.  A zero FIRST half exists for k = 0 only: k1 = e1 A1 + e2 A2 with A1, A2 > 0 and
    e1, e2 >= 0 (half_bounds) vanishes only when both floors are exact, B2 k / r and MB1 k / r integers, i.e. r | k (r is prime and larger
    than B2).  So zero_k1_only can never be set, while a zero second half beside a non-zero first is common (every k < 2^190)."""
    rep = dict(zero_k1=False, zero_k1_only=False, zero_k2=False, zero_k2_only=False, skew1_set=False, skew1_clear=False, skew2_set=False, skew2_clear=False, negative_k2=False,
               max_half=0, digits=set(), top_digits=set())
    for k in ks:
        k1, k2 = split(k)
        rep["zero_k1"] |= k1 == 0
        rep["zero_k2"] |= k2 == 0
        rep["zero_k1_only"] |= k1 == 0 and k2 != 0
        rep["zero_k2_only"] |= k2 == 0 and k1 != 0
        rep["negative_k2"] |= k2 < 0
        rep["max_half"] = max(rep["max_half"], k1, abs(k2))
        for half, name in ((k1, "skew1"), (abs(k2), "skew2")):
            digits, skew = recode(half)
            rep[name + ("_set" if skew else "_clear")] = True
            rep["digits"].update(digits[1:])
            rep["top_digits"].add(digits[0])
    return rep
