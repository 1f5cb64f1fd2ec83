"""The wire forms of G1 points and Fr scalars (include/bbg.h, bbg_wire_*; csrc/wire.hip) on Python integers, both directions of every form.

A native G1 value is an affine pair (x, y) of integers below Q, or None for the point at infinity; a native Fr value an integer below R.
A wire element is `bytes` of the form's size.  The square root is taken by two routes: `sqrt_candidate` is the power a^((Q + 1) / 4) the
kernel computes, and `is_decoding_of` / `is_non_residue` hold a decoding to the definition -- y^2 = x^3 + 3 with the parity rule, Euler's
criterion for the words that have no point -- without that power.  `window_program` / `window_pow` are the kernel's own program: sliding
windows over (Q + 1) / 4 from the top, a table of odd powers, one squaring per exponent bit and one product per window."""
import numpy as np

import pairing_model as pm

Q, R, MONT = pm.P, pm.R, pm.MONT
G1_COMPRESSED, G1_COMPRESSED_BYTES, G1_BUFFER, FR, FR_BYTES = range(5)
FORMS = (G1_COMPRESSED, G1_COMPRESSED_BYTES, G1_BUFFER, FR, FR_BYTES)
G1_FORMS = (G1_COMPRESSED, G1_COMPRESSED_BYTES, G1_BUFFER)
VALID, INFINITY, MALFORMED, OFF_CURVE = 1, 3, 0, 2
INF_WORD = 1 << 254          # the compressed infinity: bit 254 alone (Q < 2^254, so no finite word sets it)
INF_BUFFER = b"\x80" + bytes(63)
N_MAX = 1 << 28

assert Q % 4 == 3 and R % 4 == 1 and Q < 1 << 254


def sizes(form):
    """(wire bytes, native bytes) per element."""
    return (64 if form == G1_BUFFER else 32, 32 if form in (FR, FR_BYTES) else 64)


def is_bytes_form(form):
    return form in (G1_COMPRESSED_BYTES, G1_BUFFER, FR_BYTES)


# ------------------------------------------------------------------------------------------------ the square root
SQRT_EXP = (Q + 1) // 4
WINDOW = 4  # csrc/wire.hip BBG_WIRE_WINDOW


def sqrt_candidate(a):
    """a^((Q + 1) / 4): a root of a residue; for a non-residue a value that squares to -a."""
    return pow(a % Q, SQRT_EXP, Q)


def window_program(window=WINDOW):
    """The kernel's program (csrc/wire.hip wire_program): from the top bit down a set bit i opens a window i .. l, l >= i - window + 1 the
    lowest set bit in reach, of odd value v.  Returns (first value, start bit, [(l, v) of every later window, in the order they run])."""
    bit = lambda i: (SQRT_EXP >> i) & 1
    i, first, steps = SQRT_EXP.bit_length() - 1, None, []
    while i >= 0:
        if not bit(i):
            i -= 1
            continue
        l = max(i - window + 1, 0)
        while not bit(l):
            l += 1
        v = (SQRT_EXP >> l) & ((1 << (i - l + 1)) - 1)
        if first is None:
            first = (l, v)
        else:
            steps.append((l, v))
        i = l - 1
    return first[1], first[0] - 1, steps


def window_pow(a, window=WINDOW, counts=None):
    """The program run as the kernel runs it: a table of the odd powers a, a^3 .. a^(2^window - 1), one squaring per exponent bit from the
    start bit down, a product behind the squaring of bit l of every window; counts (a dict) receives the number of products of each kind."""
    a %= Q
    first, start, steps = window_program(window)
    a2 = a * a % Q
    table = [a]
    for _ in range((1 << (window - 1)) - 1):
        table.append(table[-1] * a2 % Q)
    at = dict(steps)
    acc = table[(first - 1) // 2]
    for i in range(start, -1, -1):
        acc = acc * acc % Q
        if i in at:
            acc = acc * table[(at[i] - 1) // 2] % Q
    if counts is not None:
        counts.update(table=len(table), squarings=start + 1, products=len(steps))
    return acc


def rhs(x):
    return (x * x * x + 3) % Q


def on_curve(p):
    return p is None or (p[1] * p[1] - rhs(p[0])) % Q == 0


def is_non_residue(a):
    """Euler's criterion: the route that takes no root."""
    return pow(a % Q, (Q - 1) // 2, Q) == Q - 1


def is_decoding_of(word, point):
    """`point` is what the finite compressed word decodes to, by the definition alone."""
    x, parity = word & (INF_WORD - 1), word >> 255
    return point is not None and point[0] == x and 0 <= point[1] < Q and on_curve(point) and (point[1] & 1) == parity


# ------------------------------------------------------------------------------------------------ one element
def word_to_bytes(form, w):
    return w.to_bytes(32, "big" if is_bytes_form(form) else "little")


def word_from_bytes(form, data):
    return int.from_bytes(data, "big" if is_bytes_form(form) else "little")


def compress(point):
    """The reference's uint256_t(P) for a finite point; bit 254 alone for infinity."""
    return INF_WORD if point is None else point[0] | (point[1] & 1) << 255


def decode_word(w):
    """(status, point) of a compressed 256-bit word."""
    if (w >> 254) & 1:
        return (INFINITY, None) if w == INF_WORD else (MALFORMED, None)
    x, parity = w & (INF_WORD - 1), w >> 255
    if x >= Q:
        return MALFORMED, None
    y = sqrt_candidate(rhs(x))
    if y * y % Q != rhs(x):
        return OFF_CURVE, None
    if (y & 1) != parity:
        y = (Q - y) % Q
    return VALID, (x, y)


def decode(form, data):
    """(status, native value) of one wire element; the value of a bad element is what the device writes: infinity, or zero."""
    assert len(data) == sizes(form)[0]
    if form in (FR, FR_BYTES):
        v = word_from_bytes(form, data)
        return (VALID, v) if v < R else (MALFORMED, 0)
    if form == G1_BUFFER:
        if data[0] & 0x80:
            return INFINITY, None
        y, x = int.from_bytes(data[:32], "big"), int.from_bytes(data[32:], "big")
        if data[0] & 0x40 or y >= Q or x >= Q:
            return MALFORMED, None
        return (VALID, (x, y)) if on_curve((x, y)) else (OFF_CURVE, None)
    return decode_word(word_from_bytes(form, data))


def encode(form, value, check=1):
    """(status, wire bytes) of one native value: a point (any integers, taken mod Q), None, or a scalar (taken mod R)."""
    if form in (FR, FR_BYTES):
        return VALID, word_to_bytes(form, value % R)
    st, p = VALID, value
    if p is None:
        st = INFINITY
    else:
        p = (p[0] % Q, p[1] % Q)
        if check and not on_curve(p):
            st, p = OFF_CURVE, None
    if form == G1_BUFFER:
        return st, INF_BUFFER if p is None else p[1].to_bytes(32, "big") + p[0].to_bytes(32, "big")
    return st, word_to_bytes(form, compress(p))


# ------------------------------------------------------------------------------------------------ batches, in the device's own arrays
def _ints(words, k):
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, k, 4)
    return [[sum(int(e[j]) << (64 * j) for j in range(4)) for e in row] for row in w]


def native_words(form, values):
    """The native array of a list of values: (n, 8) canonical Montgomery affine words, or (n, 4) canonical Montgomery Fr words."""
    if form in (FR, FR_BYTES):
        return pm.fr_words(values) if values else np.zeros((0, 4), dtype=np.uint64)
    return np.stack([pm.g1_words(p) for p in values]) if values else np.zeros((0, 8), dtype=np.uint64)


def native_values(form, words):
    """The values of a native array whose entries may be any representative in [0, 2 modulus); infinity as the device reads it."""
    if form in (FR, FR_BYTES):
        inv = pow(MONT, -1, R)
        return [v[0] * inv % R for v in _ints(words, 1)]
    inv = pow(MONT, -1, Q)
    return [None if x >> 255 else (x * inv % Q, y * inv % Q) for x, y in _ints(words, 2)]


def decode_batch(form, data):
    """(native words, status uint32 (n,), bad) of the concatenated wire elements `data`."""
    size = sizes(form)[0]
    assert len(data) % size == 0
    out = [decode(form, data[i:i + size]) for i in range(0, len(data), size)]
    status = np.array([s for s, _ in out], dtype=np.uint32)
    return native_words(form, [v for _, v in out]), status, int(((status == MALFORMED) | (status == OFF_CURVE)).sum())


def encode_batch(form, words, check=1):
    """(wire bytes, status, bad) of a native array."""
    out = [encode(form, v, check) for v in native_values(form, words)]
    status = np.array([s for s, _ in out], dtype=np.uint32)
    return b"".join(b for _, b in out), status, int((status == OFF_CURVE).sum())


def multiples_of_g(n, negate_every=3):
    """[k] G, k = 1 .. n, every `negate_every`-th one negated (0 = none) so that both parities of y occur."""
    out, cur = [], None
    for k in range(1, n + 1):
        cur = pm.g1_add(cur, pm.G1)
        out.append((cur[0], Q - cur[1]) if negate_every and k % negate_every == 0 else cur)
    return out
