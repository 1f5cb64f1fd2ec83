"""Inputs and integer expectations shared by the GPU tests of bbg_open_points and bbg_kzg_verify (tests/test_gpu_open_points.py,
tests/test_gpu_kzg_verify.py, tests/test_gpu_open_points_stream.py).

The string is [x^i] G for a KNOWN x, so every expected point is one scalar multiplication of the integer model: the commitment of F is
[F(x)] G and the proof of its opening at z is [(F(x) - F(z)) / (x - z)] G.  Polynomials are chosen by their coefficients; their values come
from the oracle's transform; F(x) and F(z) from Horner on integers."""
import numpy as np

import open_points_model as om
import pairing_model as pm

R = om.R
X_INT = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % R
X_WORDS = pm.fr_words([X_INT])[0]


def rand_fr(rng):
    return int.from_bytes(rng.bytes(40), "little") % R


def g1_mul_g(s):
    """[s] G as an affine pair or None, in Jacobian coordinates with one inversion at the end (pm.g1_mul inverts at every step;
    tests/test_open_points_cpu.py holds this one to it)."""
    P = pm.P
    s %= R
    if s == 0:
        return None
    gx, gy = pm.G1
    X, Y, Z = gx, gy, 1
    for bit in bin(s)[3:]:
        # dbl-2009-l (a = 0)
        A, B = X * X % P, Y * Y % P
        C = B * B % P
        D = 2 * ((X + B) * (X + B) - A - C) % P
        E = 3 * A % P
        X3 = (E * E - 2 * D) % P
        Y3 = (E * (D - X3) - 8 * C) % P
        Z = 2 * Y * Z % P
        X, Y = X3, Y3
        if bit == "1":
            # madd: the sum cannot be the doubling or infinity for 1 < s < r on a curve of prime order r
            Z2 = Z * Z % P
            U2, S2 = gx * Z2 % P, gy * Z2 * Z % P
            H, Rr = (U2 - X) % P, (S2 - Y) % P
            H2 = H * H % P
            H3 = H * H2 % P
            V = X * H2 % P
            X3 = (Rr * Rr - H3 - 2 * V) % P
            Y = (Rr * (V - X3) - Y * H3) % P
            X, Z = X3, Z * H % P
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def g1(s):
    """[s] G as 8 canonical Montgomery words."""
    return pm.g1_words(g1_mul_g(s))


class Batch:
    """`count` polynomials of n = 2^log2n coefficients, one point each.  on_domain: {k: m} puts z_k = w^m; coeffs: {k: list} fixes
    polynomial k (shorter lists are padded with zeros).  Everything a test compares against is computed once, here."""

    def __init__(self, oracle, log2n, count, seed, on_domain=None, coeffs=None):
        rng = np.random.default_rng(seed)
        n = 1 << log2n
        self.log2n, self.n, self.count = log2n, n, count
        w = om.root(log2n)
        self.polys, self.z = [], []
        for k in range(count):
            f = (coeffs or {}).get(k)
            f = [rand_fr(rng) for _ in range(n)] if f is None else list(f) + [0] * (n - len(f))
            self.polys.append(f)
            m = (on_domain or {}).get(k)
            self.z.append(rand_fr(rng) if m is None else pow(w, m, R))
        self.evals = np.stack([oracle.canon(0, oracle.ntt(pm.fr_words(f), 0)) for f in self.polys])  # (count, n, 4)
        self.z_words = pm.fr_words(self.z)
        self.y = [om.horner(f, z) for f, z in zip(self.polys, self.z)]
        self.c = [om.horner(f, X_INT) for f in self.polys]
        self.w = [(c - y) * pow(X_INT - z, -1, R) % R for c, y, z in zip(self.c, self.y, self.z)]
        self.y_words = pm.fr_words(self.y)
        self.proofs = np.stack([g1(s) for s in self.w])
        self._commitments = None

    @property
    def commitments(self):
        if self._commitments is None:
            self._commitments = np.stack([g1(s) for s in self.c])
        return self._commitments


def lifted(words):
    """The second representative in [r, 2r) of canonical Fr words."""
    import coarse_inputs as ci
    return ci.add_int(words, R).reshape(np.shape(words))
