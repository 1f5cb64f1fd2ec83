"""CPU model of the cell handle of bbg_open_all (bbg_open_all_prepare_cells, csrc/open_all.hip), on open_all_model.py, the C oracle's group
operations and Python integers for Fr.

With n = len(f), l = 2^log2cell, r = n / l, w = w_n and phi = w^l, proof m (m < r) is the commitment over s_0 .. s_(n-l-1) to q_m in
f = q_m (X^l - phi^m) + I_m, deg I_m < l.

    cell_quotient_coeffs    the n - l coefficients of the quotient of f by X^l - a.
    open_cells_definition   the proofs by what they ARE: the quotient's coefficients, then one oracle.msm_naive per proof.
    open_cells_embedding    the proofs by the route the device takes: the block layout of the l transformed residue classes of the string,
                            the l Fr transforms, the 2n products scattered by the bit reversal over 2n, the segment sums, an inverse G1
                            transform at 2r and a forward one at r.  The layout identity bitrev_2n(b 2r + i) = bitrev_2r(i) l + bitrev_l(b)
                            is asserted on the way.
    cell_closed_form_scalars
                            (f(x) - I_m(x)) / (x^l - phi^m) for m < r: over a powers string s_j = [x^j] G the proof is this scalar times G.

Designed inputs (the special cases of the segment sum): over a powers string and with f_(l i + b) = eps_b x^(-b) g_i, the l products that
k_open_cells_sum adds at output index i are [eps_b C_i S_i] G -- equal or opposite points, whatever b -- where C = NTT_Fr,2r(c^(g)) and
S = NTT_Fr,2r(x^(l (r-2)), .., x^l, 1, 0, ..).  designed_coeffs builds f, product_scalars computes the 2n discrete logarithms of the
products of ANY f over a powers string by the device's route, designed_factors gives C and S."""
import numpy as np

import coarse_inputs as ci
import lagrange_model as lm
import open_all_model as oa

R_MOD = oa.R_MOD


def bit_reverse(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def shape(n, log2cell):
    lg = n.bit_length() - 1
    assert n >= 2 and 1 << lg == n and 0 <= log2cell <= lg - 1, "n a power of two and at least two cells"
    return lg, 1 << log2cell, n >> log2cell


def cell_quotient_coeffs(f, l, a):
    """q_0 .. q_(n-l-1) of f = q (X^l - a) + I, deg I < l: q_j = f_(j+l) + a q_(j+l)."""
    n = len(f)
    q = [0] * (n - l)
    for j in range(n - l - 1, -1, -1):
        q[j] = (f[j + l] + (a * q[j + l] if j + l < n - l else 0)) % R_MOD
    return q


def open_cells_definition(oracle, pts, f, log2cell, indices=None):
    """out[m] = sum_j q^(m)_j s_j over the first n - l points, for every m < r or for the m in `indices`; plain integer coefficients."""
    n = len(f)
    lg, l, r = shape(n, log2cell)
    s = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 8)[:n - l]
    phi = pow(lm.root(oracle, lg), l, R_MOD)
    ms = range(r) if indices is None else indices
    out = [oracle.msm_naive(lm.ints_to_mont(oracle, cell_quotient_coeffs(f, l, pow(phi, m, R_MOD))), s) for m in ms]
    return oa.canon_points(oracle, np.stack(out))


def class_embedding(f, log2cell, b):
    """c^(b) = (f^(b)_(r-1), r + 1 zeros, f^(b)_1, .., f^(b)_(r-2)) with f^(b)_i = f_(l i + b): 2r integers."""
    _, l, r = shape(len(f), log2cell)
    return [f[l * (r - 1) + b]] + [0] * (r + 1) + [f[l * i + b] for i in range(1, r - 1)]


def string_layout(n, log2cell):
    """What k_open_cells_srs writes, as indices into the string (None = infinity): src[k l + c] = s^(bitrev_l(c))[k], s^(b)[k] =
    s_(l (r-2-k) + b) for k <= r - 2."""
    _, l, r = shape(n, log2cell)
    src = [None] * (2 * n)
    for k in range(2 * r):
        for c in range(l):
            if k <= r - 2:
                src[k * l + c] = l * (r - 2 - k) + bit_reverse(c, log2cell)
    return src


def sum_points(oracle, pts):
    """The sum of a few points, infinities among them, canonical."""
    live = [p for p in pts if not oa.is_infinity(p)]
    if not live:
        return oa.aff_infinity()
    ones = lm.ints_to_mont(oracle, [1] * len(live))
    return oa.canon_points(oracle, oracle.msm_naive(ones, np.stack(live)))[0]


def open_cells_embedding(oracle, pts, f, log2cell):
    """The same proofs by the device's route; also returns h (r points, h_(r-1) = infinity)."""
    n = len(f)
    lg, l, r = shape(n, log2cell)
    lg2r = lg - log2cell + 1
    s = oa.canon_points(oracle, np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 8)[:n - l])
    at = lambda idx: oa.aff_infinity() if idx is None else s[idx]
    src = string_layout(n, log2cell)
    work = [src[bit_reverse(j, lg + 1)] for j in range(2 * n)]  # ecntt_load over 2n
    w2r = lm.root(oracle, lg2r)
    s_hat, c_hat = [None] * (2 * n), [0] * (2 * n)
    for b in range(l):
        block = [work[b * 2 * r + bit_reverse(i, lg2r)] for i in range(2 * r)]  # the block is bit-reversed within itself ..
        assert block == [l * (r - 2 - k) + b if k <= r - 2 else None for k in range(2 * r)]  # .. and is s^(b)
        s_hat[b * 2 * r:(b + 1) * 2 * r] = list(oa.g1_ntt(oracle, np.stack([at(idx) for idx in block])))
        c_hat[b * 2 * r:(b + 1) * 2 * r] = oa.fr_ntt(class_embedding(f, log2cell, b), w2r)
    work2 = [None] * (2 * n)
    for b in range(l):
        for i in range(2 * r):
            j = b * 2 * r + i
            dst = bit_reverse(j, lg + 1)  # k_open_batch_pointwise with log2m = log2(2n)
            assert dst == bit_reverse(i, lg2r) * l + bit_reverse(b, log2cell)
            work2[dst] = oracle.g1_mul(s_hat[j], lm.ints_to_mont(oracle, [c_hat[j]])[0])
    work2 = oa.canon_points(oracle, np.stack(work2))
    sums = [sum_points(oracle, work2[k * l:(k + 1) * l]) for k in range(2 * r)]
    natural = np.stack([sums[bit_reverse(i, lg2r)] for i in range(2 * r)])
    h = oa.g1_ntt(oracle, natural, inverse=True)[:r]
    return oa.g1_ntt(oracle, h), h


def horner(f, x):
    acc = 0
    for c in reversed(f):
        acc = (acc * x + c) % R_MOD
    return acc


def cell_remainders(f, log2cell, w=None):
    """I[m][b] = sum_k f_(b + k l) phi^(m k): the remainder of f modulo X^l - phi^m, for every m < r."""
    n = len(f)
    lg, l, r = shape(n, log2cell)
    w = ci.root_of_unity(lg) if w is None else w
    phi = pow(w, l, R_MOD)
    cols = [oa.fr_fft([f[b + k * l] % R_MOD for k in range(r)], phi) for b in range(l)]
    return [[cols[b][m] for b in range(l)] for m in range(r)]


def cell_closed_form_scalars(f, x, log2cell, w=None):
    """(f(x) - I_m(x)) / (x^l - phi^m) for m < r, plain integers; x^l must not be a power of phi.  w: the domain's root (default: Fr's)."""
    n = len(f)
    lg, l, r = shape(n, log2cell)
    w = ci.root_of_unity(lg) if w is None else w
    phi = pow(w, l, R_MOD)
    fx, xl = horner(f, x), pow(x, l, R_MOD)
    dens, z = [], 1
    for _ in range(r):
        dens.append((xl - z) % R_MOD)
        z = z * phi % R_MOD
    assert all(dens), "x^l lies on the domain of the cells"
    rem = cell_remainders(f, log2cell, w)
    return [(fx - horner(rem[m], x)) * d % R_MOD for m, d in zip(range(r), oa.batch_inverse(dens))]


# ------------------------------------------------------------------------------------------------ designed inputs over a powers string
def designed_coeffs(g, x, eps, log2cell):
    """f_(l i + b) = eps_b x^(-b) g_i for r integers g and l signs eps (+1 / -1, or any integers)."""
    l, r = 1 << log2cell, len(g)
    assert len(eps) == l
    xinv = pow(x, R_MOD - 2, R_MOD)
    f = [0] * (l * r)
    for b in range(l):
        scale = eps[b] * pow(xinv, b, R_MOD) % R_MOD
        for i in range(r):
            f[l * i + b] = scale * g[i] % R_MOD
    return f


def product_scalars(f, x, log2cell, w2r=None):
    """prod[b][i], the discrete logarithm of product (b, i) = c_hat[b 2r + i] * s_hat[b 2r + i] over s_j = [x^j] G, by the device's route on
    integers: NTT_Fr,2r of c^(b) times NTT_Fr,2r of the logarithms of s^(b)."""
    n = len(f)
    lg, l, r = shape(n, log2cell)
    w2r = ci.root_of_unity(lg - log2cell + 1) if w2r is None else w2r
    out = []
    for b in range(l):
        s_b = [pow(x, l * (r - 2 - k) + b, R_MOD) if k <= r - 2 else 0 for k in range(2 * r)]
        c_tr, s_tr = oa.fr_fft(class_embedding(f, log2cell, b), w2r), oa.fr_fft(s_b, w2r)
        out.append([c * s % R_MOD for c, s in zip(c_tr, s_tr)])
    return out


def designed_factors(g, x, log2cell, w2r=None):
    """(C, S): C = NTT_Fr,2r(c^(g)) for the l = 1 embedding of g, S = NTT_Fr,2r(y^(r-2), .., y, 1, then r + 1 zeros), y = x^l."""
    r = len(g)
    lg2r = r.bit_length()
    w2r = ci.root_of_unity(lg2r) if w2r is None else w2r
    y = pow(x, 1 << log2cell, R_MOD)
    c = [g[r - 1]] + [0] * (r + 1) + [g[i] for i in range(1, r - 1)]
    s = [pow(y, r - 2 - k, R_MOD) if k <= r - 2 else 0 for k in range(2 * r)]
    return oa.fr_fft([v % R_MOD for v in c], w2r), oa.fr_fft(s, w2r)
