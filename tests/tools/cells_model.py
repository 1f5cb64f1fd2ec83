"""CPU model of the cells of a polynomial as data (bbg_cells_values, bbg_cells_recover, csrc/cells.hip), on Python integers
for Fr and the C oracle's ntt for the transforms.

With n = 2^log2n, l = 2^log2cell, r = n / l, w = w_n, phi = w^l and g the domain's coset generator, cell m < r is { w^(m + r t) : t < l }.
Values are plain integers mod r_mod everywhere here (the transforms are linear, so what the oracle takes for Montgomery residues may be any
residues); mont() turns them into the words the C ABI takes.

    cell_values             out[m l + t] = f(w^(m + r t)): the oracle's forward transform, read cell by cell.
    interpolate_definition  the polynomial of degree < k through k points by Lagrange's formula, for at most 64 points.
    z_tables                Zdom[j] = prod_{m missing} (phi^j - phi^m) and Zcos[j] = prod (g^l phi^j - phi^m), j < r, by their products.
    recover_route           the interpolant of degree < K l by the route the device takes: scatter times Zdom, inverse transform, coset
                            transform, division by Zcos, inverse coset transform.  The index identities the kernels rely on are asserted."""
import numpy as np

import coarse_inputs as ci

R_MOD = ci.R_MOD
GEN = ci.COSET_GENERATOR
FFT, IFFT, COSET_FFT, COSET_IFFT = 0, 1, 2, 3


def shape(log2n, log2cell):
    assert 1 <= log2n <= 28 and 0 <= log2cell <= log2n - 1
    return 1 << log2n, 1 << log2cell, 1 << (log2n - log2cell)


def mont(vals):
    """Plain integers -> (len, 4) canonical Montgomery words."""
    return ci.to_words([ci.to_mont(v % R_MOD, 0) for v in vals])


def unmont(words):
    """(len, 4) Montgomery words below 2 r_mod -> plain integers."""
    return [ci.from_mont(v, 0) for v in ci.to_ints(words)]


def transform(oracle, vals, op):
    """The oracle's ntt on plain integers, canonical integers out."""
    return ci.to_ints(oracle.canon(0, oracle.ntt(ci.to_words([v % R_MOD for v in vals]), op)))


def cell_values(oracle, f, log2cell):
    """The n values of the n coefficients f, cell-major: out[m l + t] = f(w^(m + r t))."""
    n = len(f)
    _, l, r = shape(n.bit_length() - 1, log2cell)
    on_domain = transform(oracle, f, FFT)
    return [on_domain[m + r * t] for m in range(r) for t in range(l)]


def known_values(values, ids, log2cell):
    """The cells `ids` of cell-major `values`, one after the other in the order of ids: what bbg_cells_recover takes."""
    l = 1 << log2cell
    return [values[m * l + t] for m in ids for t in range(l)]


def cell_points(log2n, log2cell, ids):
    """The domain points of the cells `ids`, in known_values' order."""
    n, l, r = shape(log2n, log2cell)
    w = ci.root_of_unity(log2n)
    return [pow(w, m + r * t, R_MOD) for m in ids for t in range(l)]


def interpolate_definition(xs, ys):
    """Coefficients c_0 .. c_(k-1) of the polynomial through (xs[i], ys[i]), xs distinct, k <= 64: sum_i ys[i] prod_{j != i} (X - x_j) / (x_i - x_j)."""
    k = len(xs)
    assert k == len(ys) and k <= 64 and len(set(x % R_MOD for x in xs)) == k
    master = [1]  # prod (X - x_j), lowest coefficient first
    for x in xs:
        master = [((master[i - 1] if i else 0) - x * (master[i] if i < len(master) else 0)) % R_MOD for i in range(len(master) + 1)]
    out = [0] * k
    for x, y in zip(xs, ys):
        q, carry = [0] * k, 0  # master / (X - x) by synthetic division, from the top
        for i in range(k, 0, -1):
            carry = (master[i] + carry * x) % R_MOD
            q[i - 1] = carry
        den = 1
        for xj in xs:
            if xj != x:
                den = den * (x - xj) % R_MOD
        scale = y * pow(den, R_MOD - 2, R_MOD) % R_MOD
        out = [(o + scale * c) % R_MOD for o, c in zip(out, q)]
    return out


def z_tables(log2n, log2cell, ids):
    """(Zdom, Zcos), r integers each, by the products over the missing cells (the empty product is 1)."""
    n, l, r = shape(log2n, log2cell)
    assert len(set(ids)) == len(ids) and all(0 <= m < r for m in ids) and len(ids) >= 1
    phi = pow(ci.root_of_unity(log2n), l, R_MOD)
    powers = [pow(phi, j, R_MOD) for j in range(r)]
    known = set(ids)
    roots = [powers[m] for m in range(r) if m not in known]
    gl = pow(GEN, l, R_MOD)

    def product(x):
        acc = 1
        for rt in roots:
            acc = acc * (x - rt) % R_MOD
        return acc
    return [product(powers[j]) for j in range(r)], [product(gl * powers[j] % R_MOD) for j in range(r)]


def z_direct(log2n, log2cell, ids, x):
    """Z(x) = prod_{m missing} (x^l - phi^m) from the definition."""
    n, l, r = shape(log2n, log2cell)
    phi = pow(ci.root_of_unity(log2n), l, R_MOD)
    xl, acc = pow(x, l, R_MOD), 1
    for m in range(r):
        if m not in ids:
            acc = acc * (xl - pow(phi, m, R_MOD)) % R_MOD
    return acc


def recover_route(oracle, ids, values, log2n, log2cell):
    """The n coefficients of the interpolant of degree < K l through the cells `ids` (values: K l integers in known_values' order)."""
    n, l, r = shape(log2n, log2cell)
    K = len(ids)
    assert len(values) == K * l
    zdom, zcos = z_tables(log2n, log2cell, ids)
    slot = [-1] * r
    for k, m in enumerate(ids):
        slot[m] = k
    # 1. scatter: domain index i = m + r t takes cell-major entry slot[m] l + t, times Zdom[i mod r]; i mod r = m
    a = [0] * n
    for m in range(r):
        for t in range(l):
            i = m + r * t
            assert i % r == m and i < n
            if slot[m] >= 0:
                assert zdom[m] != 0
                a[i] = values[slot[m] * l + t] * zdom[i % r] % R_MOD
            else:
                assert zdom[m] == 0  # Z vanishes exactly on the missing cells
    # 2. the coefficients of f* Z
    d = transform(oracle, a, IFFT)
    # 3. on the coset g <w>, where Z is never zero and again r-periodic
    b = transform(oracle, d, COSET_FFT)
    assert all(zcos)
    inv = [pow(v, R_MOD - 2, R_MOD) for v in zcos]
    b = [v * inv[i % r] % R_MOD for i, v in enumerate(b)]
    # 4. back
    f = transform(oracle, b, COSET_IFFT)
    assert not any(f[K * l:]), "the interpolant has degree < K l"
    return f


def random_ints(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R_MOD for _ in range(count)]
