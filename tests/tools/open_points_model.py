"""Integer models of csrc/open_points.hip and csrc/kzg_verify.hip, on Python integers mod r in standard form.

open_values restates the kernels step by step -- the weights u_i = w^-i / d_i, the two partial sums per inversion group, the hit index, the
value, the quotient values with the hit slot filled from S0 and S1 -- so that tests/test_open_points_cpu.py can hold the on-domain identity
    q_m = - w^-m sum_(i != m) (f_m - f_i) / d_i
to coefficient-form division.  kzg_closed_form and kzg_packed restate the reduction with every point written as its discrete logarithm to
the base G (the group is cyclic of order r, so the reduction is linear algebra on those logarithms)."""
import coarse_inputs as ci

R = ci.R_MOD
GROUP = 1024  # BARY_BLK: the points of one inversion group (csrc/bbg_internal.h)
NO_HIT = 0xFFFFFFFF


def root(log2n):
    return ci.root_of_unity(log2n)


def horner(coeffs, z):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % R
    return acc


def divide(coeffs, z):
    """(F(z), the coefficients of (F(X) - F(z)) / (X - z)), top coefficient zero: synthetic division."""
    n = len(coeffs)
    q = [0] * n
    acc = 0
    for i in range(n - 1, 0, -1):
        acc = (acc * z + coeffs[i]) % R
        q[i - 1] = acc
    return (acc * z + coeffs[0]) % R, q


def values(coeffs, log2n):
    """f_i = F(w^i), i < n."""
    w = root(log2n)
    return [horner(coeffs, pow(w, i, R)) for i in range(1 << log2n)]


def open_values(f, z, log2n):
    """(y, [q_i], hit) as k_op_weights, k_op_value and k_op_quotient compute them for the values f of one polynomial and its point z."""
    n = 1 << log2n
    assert len(f) == n
    w_inv = pow(root(log2n), -1, R)
    hit = NO_HIT
    u = [0] * n
    partials = []  # (S1, S0) per inversion group
    for base in range(0, n, GROUP):
        s1 = s0 = 0
        for i in range(base, min(base + GROUP, n)):
            wi = pow(w_inv, i, R)
            d = (z * wi - 1) % R
            if d == 0:
                hit = min(hit, i)
                u[i] = wi  # the weight slot of the hit holds w^-m (the inversion saw a one)
                continue
            inv = pow(d, -1, R)
            u[i] = wi * inv % R
            s1 = (s1 + f[i] * inv) % R
            s0 = (s0 + inv) % R
        partials.append((s1, s0))
    S1, S0 = sum(p[0] for p in partials) % R, sum(p[1] for p in partials) % R
    if hit != NO_HIT:
        y = f[hit] % R
        qm = pow(w_inv, hit, R) * (S1 - y * S0) % R
    else:
        y = (pow(z, n, R) - 1) * pow(n, -1, R) * S1 % R
        qm = None
    q = [(y - f[i]) * u[i] % R for i in range(n)]
    if hit != NO_HIT:
        assert q[hit] == 0
        q[hit] = qm
    return y, q, hit


def hit_identity(f, m, log2n):
    """q_m by the identity alone: - w^-m sum_(i != m) (f_m - f_i) / (w^(m - i) - 1)."""
    n = 1 << log2n
    w = root(log2n)
    acc = 0
    for i in range(n):
        if i != m:
            acc = (acc + (f[m] - f[i]) * pow(pow(w, (m - i) % n, R) - 1, -1, R)) % R
    return -pow(w, -m % n, R) * acc % R


# ---------------------------------------------------------------------------------------------- the verifier's reduction
def powers(rho, N):
    out, p = [], 1
    for _ in range(N):
        out.append(p)
        p = p * rho % R
    return out  # rho^0 = 1 also for rho = 0


def kzg_closed_form(c, z, y, w, rho):
    """(l, r) with L = [l] G and R = [r] G for commitments [c_i] G, points z_i, values y_i, proofs [w_i] G."""
    pw = powers(rho, len(c))
    l = sum(p * wi for p, wi in zip(pw, w)) % R
    r = sum(p * (ci_ - yi + zi * wi) for p, ci_, zi, yi, wi in zip(pw, c, z, y, w)) % R
    return l, r


def kzg_packed(c, z, y, w, rho):
    """The packed arrays of k_kv_prepare: points [C | pi | G] as logarithms, scalars [rho^i | rho^i z_i | s]."""
    pw = powers(rho, len(c))
    points = list(c) + list(w) + [1]
    scalars = pw + [p * zi % R for p, zi in zip(pw, z)] + [-sum(p * yi for p, yi in zip(pw, y)) % R]
    return points, scalars


def kzg_honest(x, polys, zs):
    """(c, y, w) of honest openings over the string [x^i] G: polys[i] (coefficients) opened at zs[i]."""
    c = [horner(f, x) for f in polys]
    y = [horner(f, zi) for f, zi in zip(polys, zs)]
    w = [(ci_ - yi) * pow(x - zi, -1, R) % R for ci_, yi, zi in zip(c, y, zs)]
    return c, y, w
