"""CPU model of bbg_g1_ntt and bbg_open_all, built only from the C oracle's group operations (oracle/bn254_oracle.c) and Python integers
for Fr.

    g1_ntt      out[k] = sum_j w_n^(jk) P_j, or n^-1 sum_j w_n^(-jk) P_j: one oracle.msm_naive per output.
    open_all_definition
                the proofs by what they ARE: for every m the coefficients of (f(X) - f(w^m)) / (X - w^m), then oracle.msm_naive over the
                first n - 1 points.
    open_all_embedding
                the proofs by the route csrc/open_all.hip takes: the circulant embedding of the Toeplitz product, two G1 transforms at 2n,
                one at n.

Points are (n, 8) Montgomery affine words; the point at infinity is the reference's affine encoding (bit 63 of x.data[3], nothing else),
which every helper here keeps as it is.  Shared by tests/test_open_all_cpu.py, tests/test_gpu_g1_ntt.py and tests/test_gpu_open_all.py."""
import numpy as np

import lagrange_model as lm

R_MOD = lm.R_MOD


def aff_infinity():
    p = np.zeros(8, dtype=np.uint64)
    p[3] = np.uint64(1 << 63)
    return p


def is_infinity(p):
    return bool(int(p[3]) >> 63)


def canon_points(oracle, pts):
    """Both coordinates below p; an infinite point becomes exactly aff_infinity()."""
    p = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 8).copy()
    inf = (p[:, 3] >> np.uint64(63)) != 0
    p[inf] = 0  # canon() would reduce the flag bit away
    out = lm.canon_points(oracle, p)
    out[inf] = aff_infinity()
    return out


def g1_ntt(oracle, points, inverse=False):
    """The transform of n = 2^k points by its definition, canonical."""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    n = pts.shape[0]
    lg = n.bit_length() - 1
    assert n >= 2 and 1 << lg == n
    w = lm.root(oracle, lg)
    scale = 1
    if inverse:
        w, scale = pow(w, R_MOD - 2, R_MOD), pow(n, R_MOD - 2, R_MOD)
    wp = [scale * pow(w, e, R_MOD) % R_MOD for e in range(n)]
    live = [j for j in range(n) if not is_infinity(pts[j])]  # an infinite input adds nothing: sparse inputs stay cheap at larger n
    if not live:
        return np.tile(aff_infinity(), (n, 1))
    sel = np.ascontiguousarray(pts[live])
    rows = [lm.ints_to_mont(oracle, [wp[(j * k) % n] for j in live]) for k in range(n)]
    return canon_points(oracle, np.stack([oracle.msm_naive(rows[k], sel) for k in range(n)]))


def quotient_coeffs(f, z):
    """Coefficients q_0 .. q_(n-2) of (f(X) - f(z)) / (X - z): q_(n-2) = f_(n-1), q_j = f_(j+1) + z q_(j+1)."""
    n = len(f)
    q = [0] * (n - 1)
    acc = 0
    for j in range(n - 2, -1, -1):
        acc = (f[j + 1] + z * acc) % R_MOD
        q[j] = acc
    return q


def open_all_definition(oracle, srs_points, f, indices=None):
    """out[m] = sum_j q^(m)_j s_j, for plain integer coefficients f (n = 2^k of them) and at least n - 1 points; for every m < n, or for
    the m in `indices` (one n-term oracle.msm_naive each: all of them is for small n only)."""
    n = len(f)
    lg = n.bit_length() - 1
    assert n >= 2 and 1 << lg == n
    s = np.ascontiguousarray(srs_points, dtype=np.uint64).reshape(-1, 8)[:n - 1]
    w = lm.root(oracle, lg)
    ms = range(n) if indices is None else indices
    out = [oracle.msm_naive(lm.ints_to_mont(oracle, quotient_coeffs(f, pow(w, m, R_MOD))), s) for m in ms]
    return canon_points(oracle, np.stack(out))


def fr_ntt(vals, w):
    n = len(vals)
    wp = [pow(w, e, R_MOD) for e in range(n)]
    return [sum(vals[j] * wp[(j * k) % n] for j in range(n)) % R_MOD for k in range(n)]


def embedding(srs_points, f):
    """(s^, c^) of length 2n: s^ = (s_(n-2), .., s_0, n + 1 infinities), c^ = (f_(n-1), n + 1 zeros, f_1, .., f_(n-2))."""
    n = len(f)
    s = np.ascontiguousarray(srs_points, dtype=np.uint64).reshape(-1, 8)[:n - 1]
    s_hat = np.stack([s[n - 2 - i] for i in range(n - 1)] + [aff_infinity()] * (n + 1))
    c_hat = [f[n - 1]] + [0] * (n + 1) + [f[i] for i in range(1, n - 1)]
    assert s_hat.shape[0] == 2 * n and len(c_hat) == 2 * n
    return s_hat, c_hat


def open_all_embedding(oracle, srs_points, f):
    """The same proofs by the circulant route; also returns h (n points, h_(n-1) = infinity)."""
    n = len(f)
    lg = n.bit_length() - 1
    assert n >= 2 and 1 << lg == n
    s_hat, c_hat = embedding(srs_points, f)
    c_tr = fr_ntt(c_hat, lm.root(oracle, lg + 1))
    s_tr = g1_ntt(oracle, s_hat)
    prod = np.stack([oracle.g1_mul(p, k) for p, k in zip(s_tr, lm.ints_to_mont(oracle, c_tr))])
    h = g1_ntt(oracle, prod, inverse=True)[:n]
    return g1_ntt(oracle, h), h


def fr_fft(vals, w):
    """Radix-2 transform on Python integers, natural order in and out: out[k] = sum_j vals[j] w^(jk).  For the sizes fr_ntt is too slow at."""
    n = len(vals)
    if n == 1:
        return list(vals)
    even, odd = fr_fft(vals[0::2], w * w % R_MOD), fr_fft(vals[1::2], w * w % R_MOD)
    out = [0] * n
    t = 1
    for k in range(n // 2):
        u = t * odd[k] % R_MOD
        out[k] = (even[k] + u) % R_MOD
        out[k + n // 2] = (even[k] - u) % R_MOD
        t = t * w % R_MOD
    return out


def batch_inverse(vals):
    """1 / v for non-zero v mod r behind one modular inversion."""
    prefix, run = [], 1
    for v in vals:
        prefix.append(run)
        run = run * v % R_MOD
    inv = pow(run, R_MOD - 2, R_MOD)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * prefix[i] % R_MOD
        inv = inv * vals[i] % R_MOD
    return out


def closed_form_scalars(f, x, w):
    """(f(x) - f(w^m)) / (x - w^m) for m < n, plain integers; x must not lie on the domain.  For a powers string s_j = [x^j] G the proof
    at w^m is this scalar times G."""
    n = len(f)
    fx = 0
    for c in reversed(f):
        fx = (fx * x + c) % R_MOD
    values = fr_fft([c % R_MOD for c in f], w)
    dens, z = [], 1
    for _ in range(n):
        dens.append((x - z) % R_MOD)
        z = z * w % R_MOD
    assert all(dens)
    return [(fx - v) * d % R_MOD for v, d in zip(values, batch_inverse(dens))]
