"""Inputs over the whole coarse range [0, 2p), range checks on device outputs, and big-integer references (test tooling).

include/bbg.h accepts any representative in [0, 2p) and every kernel is meant to return one; the 29-bit-limb kernels skip carries and
comparisons on the strength of value bounds (tests/test_ntt29_model.py, tests/test_w29_model.py).  inputs.synthetic_scalars stays below
2^252 (~0.33 r), so these helpers supply the rest of the range: the GPU tests in tests/test_gpu_coarse_range.py feed them to the kernels
and check both the canonical value and the < 2p bound of what comes back.

Also the MSM's digit patterns: canonical scalars whose signed-digit recoding (msm_kernels.hip.h recode_digits, window layout
msm_cfg.h MsmCfg<C>) hits the edges random scalars reach only by chance -- the top bucket, the zero digit of a carry, carry chains.
"""
import numpy as np

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001  # Fr (scalars, NTT)
Q_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47  # Fq (point coordinates)
MODULI = (R_MOD, Q_MOD)
MONT_R = 1 << 256
MASK64 = (1 << 64) - 1
COSET_GENERATOR = 5  # Fr's multiplicative generator: the coset shift of the NTT family (as in tests/test_gpu_parity.py)
MSM_WINDOWS = (8, 13, 16, 17, 19, 20, 22)  # every window width libbbg.so compiles (msm_cfg.h BBG_MSM_TABLE_WIDTHS; 8 = msm_tiny.hip)


# ---------------------------------------------------------------------------------------------- words <-> integers
def to_words(vals):
    """Python ints (< 2^256) -> (n, 4) little-endian uint64 limbs."""
    vals = list(vals)
    out = np.empty((len(vals), 4), dtype=np.uint64)
    for k in range(4):
        out[:, k] = np.array([(v >> (64 * k)) & MASK64 for v in vals], dtype=np.uint64)
    return out


def to_ints(words):
    """(n, 4) (or (4,)) uint64 limbs -> list of Python ints."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    cols = [w[:, k].tolist() for k in range(4)]
    return [a | (b << 64) | (c << 128) | (d << 192) for a, b, c, d in zip(*cols)]


def add_int(words, x):
    """words + x (an integer, the same for every row) limb by limb, vectorised; asserts no overflow past 2^256."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    out = np.empty_like(w)
    carry = np.zeros(w.shape[0], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(4):
            xk = np.uint64((x >> (64 * k)) & MASK64)
            s = w[:, k] + xk
            c1 = s < xk
            s2 = s + carry
            c2 = s2 < carry
            out[:, k] = s2
            carry = (c1 | c2).astype(np.uint64)
    assert not carry.any(), "add_int overflowed 2^256"
    return out


def add_words(a, b):
    """a + b as 256-bit integers, vectorised; asserts no overflow past 2^256."""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    out = np.empty_like(a)
    carry = np.zeros(a.shape[0], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(4):
            s = a[:, k] + b[:, k]
            c1 = s < b[:, k]
            s2 = s + carry
            c2 = s2 < carry
            out[:, k] = s2
            carry = (c1 | c2).astype(np.uint64)
    assert not carry.any(), "add_words overflowed 2^256"
    return out


def below(words, bound):
    """Boolean mask: each 256-bit row < bound, compared on all four limbs (not only the top word)."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    lt = np.zeros(w.shape[0], dtype=bool)
    eq = np.ones(w.shape[0], dtype=bool)
    for k in (3, 2, 1, 0):
        bk = np.uint64((bound >> (64 * k)) & MASK64)
        lt |= eq & (w[:, k] < bk)
        eq &= w[:, k] == bk
    return lt


# ---------------------------------------------------------------------------------------------- coarse inputs
def catalogue(which):
    """The fixed edge values of [0, 2p) for Fr (which = 0) or Fq (1)."""
    p = MODULI[which]
    rmod = MONT_R % p
    vals = [0, 1, p - 1, p, p + 1, 2 * p - 1,
            (1 << 252) - 1, 1 << 252, 1 << 253, (1 << 254) - 1, 1 << 254,
            rmod, p + rmod,
            ((2 * p) >> 232 << 232) - 1]  # the largest value below 2p whose eight 29-bit limbs below the top one are all 2^29 - 1
    for j in range(1, 9):  # just below (and at) each 29-bit limb boundary
        vals += [(1 << (29 * j)) - 1, 1 << (29 * j)]
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    assert all(0 <= v < 2 * p for v in out)
    return out


def _splitmix(seed, count):
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def coarse_ints(seed, n, which):
    """n deterministic integers spread uniformly over [0, 2p) (x 2p / 2^256 of a uniform 256-bit x), with the catalogue spliced in at
    seeded positions (all of it when n allows, else a seeded choice of it)."""
    p2 = 2 * MODULI[which]
    raw = _splitmix(seed, 4 * n).reshape(n, 4)
    vals = [(x * p2) >> 256 for x in to_ints(raw)]
    cat = catalogue(which)
    if n:
        rng = np.random.default_rng(seed)
        pos = rng.permutation(n)[:len(cat)]
        for i, v in zip(pos, rng.permutation(len(cat))[:len(pos)]):
            vals[int(i)] = cat[int(v)]
    return vals


def coarse_scalars(seed, n, which=0):
    """coarse_ints as (n, 4) uint64 words."""
    return to_words(coarse_ints(seed, n, which))


def assert_coarse(words, which, what=""):
    """Every 256-bit value is below 2p, on the full 256 bits."""
    ok = below(words, 2 * MODULI[which])
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} value(s) >= 2p, first at {i}: {hex(to_ints(np.reshape(words, (-1, 4))[i])[0])}")


def assert_canonical(words, which, what=""):
    ok = below(words, MODULI[which])
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} value(s) >= p, first at {i}")


def assert_coarse_jacobian(jac, what=""):
    """Jacobian g1::element outputs (x || y || z, infinity = bit 63 of x.data[3]): X, Y, Z each below 2q unless the infinity bit is set."""
    j = np.ascontiguousarray(jac, dtype=np.uint64).reshape(-1, 12)
    live = (j[:, 3] >> np.uint64(63)) == 0
    for c in range(3):
        ok = below(j[:, 4 * c:4 * c + 4], 2 * Q_MOD) | ~live
        assert ok.all(), f"{what}: coordinate {'XYZ'[c]} >= 2q in {int((~ok).sum())} point(s)"


# ---------------------------------------------------------------------------------------------- big-integer references
def mont_mul(a, b, which):
    p = MODULI[which]
    return a * b * pow(MONT_R, -1, p) % p


def mont_add(a, b, which):
    return (a + b) % MODULI[which]


def mont_sub(a, b, which):
    return (a - b) % MODULI[which]


def from_mont(a, which):
    p = MODULI[which]
    return a * pow(MONT_R, -1, p) % p


def to_mont(a, which):
    p = MODULI[which]
    return a * MONT_R % p


def mont_inv(a, which):
    """Montgomery residue of 1 / (a / R); 0 -> 0."""
    p = MODULI[which]
    a %= p
    return 0 if a == 0 else MONT_R * MONT_R * pow(a, -1, p) % p


def root_of_unity(log2n):
    """The standard-form primitive 2^log2n-th root Fr's domains use: 5^((r - 1) / 2^28) raised to 2^(28 - log2n)."""
    w = pow(COSET_GENERATOR, (R_MOD - 1) >> 28, R_MOD)
    return pow(w, 1 << (28 - log2n), R_MOD)


def dft(vals, op):
    """O(n^2) transform of Montgomery-form values (the transform is linear, so the R factor rides along): op 0 fft, 1 ifft, 2 coset fft
    (a_i g^i first), 3 coset ifft (ifft, then g^-j).  Canonical Montgomery-form outputs."""
    p = R_MOD
    n = len(vals)
    lg = n.bit_length() - 1
    w = root_of_unity(lg)
    if op in (1, 3):
        w = pow(w, -1, p)
    a = [v % p for v in vals]
    if op == 2:
        a = [x * pow(COSET_GENERATOR, i, p) % p for i, x in enumerate(a)]
    wp = [pow(w, k, p) for k in range(n)]
    out = [sum(a[i] * wp[(i * j) % n] for i in range(n)) % p for j in range(n)]
    if op in (1, 3):
        ninv = pow(n, -1, p)
        out = [x * ninv % p for x in out]
    if op == 3:
        ginv = pow(COSET_GENERATOR, -1, p)
        out = [x * pow(ginv, j, p) % p for j, x in enumerate(out)]
    return out


def horner(vals, z_mont):
    """Montgomery form of sum a_i z^i for Montgomery-form coefficients a_i and point z."""
    p = R_MOD
    z = from_mont(z_mont, 0)
    acc = 0
    for v in reversed(vals):
        acc = (acc * z + v) % p
    return acc


# ---------------------------------------------------------------------------------------------- MSM window layout and recoding
class MsmLayout:
    """msm_cfg.h MsmCfg<C>: windows of C or C - 1 bits covering exactly 255 bits, narrow windows filed at twice the digit."""

    def __init__(self, c):
        self.c = c
        self.windows = (254 + c) // c
        self.nwide = 255 - self.windows * (c - 1)
        assert 1 <= self.nwide <= self.windows

    def width(self, w):
        return self.c if w < self.nwide else self.c - 1

    def offset(self, w):
        return w * (self.c - 1) + (w if w < self.nwide else self.nwide)

    def scale(self, w):
        return 0 if w < self.nwide else 1


def recode_digits(k, c):
    """Python restatement of recode_digits (msm_kernels.hip.h) on a canonical integer k: the signed digits d_w and the bucket numbers
    |d_w| << scale(w).  k = sum d_w 2^offset(w)."""
    L = MsmLayout(c)
    carry = 0
    digits, buckets = [], []
    for w in range(L.windows):
        full = 1 << L.width(w)
        half = full >> 1
        d = ((k >> L.offset(w)) & (full - 1)) + carry
        neg = d > half
        digits.append(d - full if neg else d)
        buckets.append((full - d if neg else d) << L.scale(w))
        carry = 1 if neg else 0
    return digits, buckets


def digits_value(digits, c):
    L = MsmLayout(c)
    return sum(d << L.offset(w) for w, d in enumerate(digits))


def msm_digit_patterns(c):
    """[(name, k, digits)]: canonical integers k < r built from digit vectors in MsmCfg<C>'s layout, each the recoding's own digits for
    k (d_w in (-2^(w-1), 2^(w-1)], the top one >= 0).  The patterns hit the recoding's edges every time instead of once per 2^C terms."""
    L = MsmLayout(c)
    W = L.windows
    half = [1 << (L.width(w) - 1) for w in range(W)]
    pats = []

    def add(name, digits):
        k = digits_value(digits, c)
        assert 0 <= k < R_MOD, name
        pats.append((name, k, list(digits)))

    # every digit +2^(w-1) (the top bucket) below the top window, whose top bucket would exceed r
    add("top_bucket_all", half[:W - 1] + [0])
    # every chunk 2^(w-1) + 1: the digit -(2^(w-1) - 1) with a carry into the next window, closed by a top digit 1
    add("neg_carry_all", [-(h - 1) for h in half[:W - 1]] + [1])
    # alternating: the top bucket and the largest negative digit in turn
    add("alternating", [half[w] if w % 2 == 0 else -(half[w] - 1) for w in range(W - 1)] + [1])
    # all-ones runs 2^m - 1: a -1 digit, zero digits from chunks 2^w - 1 plus carry, a +1 where the run ends
    ms = sorted({L.offset(w) for w in range(1, W)} | {1, 2, L.c - 1, L.c, L.c + 1, 64, 128, 200, 253})
    for m in ms:
        if m > 253:
            continue
        digits = [0] * W
        if m < L.width(0):
            digits[0] = (1 << m) - 1  # no carry at all
        else:
            digits[0] = -1            # chunk 2^w - 1: digit -1, carry 1; full windows above it: 2^w - 1 + 1 -> digit 0, carry 1
            w = max(v for v in range(W) if L.offset(v) <= m)
            digits[w] = 1 << (m - L.offset(w))  # where the run ends: 2^j - 1 + carry (j = width - 1 gives the top bucket, no carry)
        add(f"ones_{m}", digits)
    for w in range(W):
        add(f"pow_offset_{w}", [1 if v == w else 0 for v in range(W)])
        if w < W - 1:
            add(f"half_offset_{w}", [half[w] if v == w else 0 for v in range(W)])
    add("r_minus_1", recode_digits(R_MOD - 1, c)[0])
    add("half_r", recode_digits((R_MOD - 1) // 2, c)[0])
    top_max = recode_digits(R_MOD - 1, c)[0][W - 1]
    for lower in (half[:W - 1], [0] * (W - 1)):  # the largest top digit, with the top bucket below it where that stays below r
        if digits_value(lower + [top_max], c) < R_MOD:
            add(f"top_window_max_{'half' if lower[0] else 'zero'}", lower + [top_max])
    return pats
