"""Big-integer model of the Lagrange-form operations (csrc/barycentric.hip): Montgomery words in, canonical Montgomery words out.

With n = 2^log2n, w = coarse_inputs.root_of_unity(log2n), f_i = F(w^i) and d_i = z w^-i - 1:
  evaluate            F(z)   = (z^n - 1)/n * sum_i f_i / d_i                 (z^n != 1)
  evaluate, shifted   F(z w) = (z^n - 1)/n * sum_i f_{(i+1) mod n} / d_i
  z = w^j             F(z) = f_j, F(z w) = f_{(j+1) mod n}
  opening             W(w^i) = w^-i (F(z) - f_i) / d_i,  W(X) = (F(X) - F(z)) / (X - z)   (z^n != 1)
  batch_invert        out_i = in_i^-1, zero (r itself included) stays zero
tests/test_barycentric_cpu.py proves these against the C oracle's coefficient route; tests/test_gpu_barycentric.py reuses the shared inputs
below, whose off-domain points are asserted to satisfy z^n != 1 on the CPU side."""
import numpy as np

import coarse_inputs as ci

R_MOD = ci.R_MOD

# ---- mirrored library constants (the GPU tests place their sizes and zeros around them)
E_BLK = 1024  # domain points one block handles: BARY_BLK = 256 * BARY_E, BARY_E = 4 (csrc/bbg_internal.h, "constexpr int BARY_E = BBG_BARY_E, BARY_BLK = 256 * BARY_E")
G = 1024      # inversion group length: one group per block, the same BARY_BLK (csrc/barycentric.hip block_invert)
LOG_E_BLK = 10

# ---- shared inputs: standard-form integers; every size either test file evaluates at
Z_INTS = (0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % R_MOD,
          0x2F0E1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221101 % R_MOD,
          0)
SIZES_CPU = (1, 2, 3, 6, 9)
SIZES_GPU = (1, 2, 6, LOG_E_BLK, LOG_E_BLK + 1, 16)
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R_MOD  # the commit test's SRS secret


def canon(oracle, words):
    """oracle.canon on Fr words, in the shape given ((4,) stays (4,))."""
    return oracle.canon(0, words).reshape(np.shape(words))


def mont_words(vals):
    """Standard-form integers -> (n, 4) canonical Montgomery words."""
    return ci.to_words([ci.to_mont(v % R_MOD, 0) for v in vals])


def _std(words):
    return [ci.from_mont(v % R_MOD, 0) for v in ci.to_ints(words)]


def off_domain(z, log2n):
    return pow(z % R_MOD, 1 << log2n, R_MOD) != 1


def batch_invert(words):
    return ci.to_words([ci.mont_inv(v, 0) for v in ci.to_ints(words)])


def _weights(z, log2n):
    """d_i = z w^-i - 1, i < n (standard form)."""
    n = 1 << log2n
    w_inv = pow(ci.root_of_unity(log2n), -1, R_MOD)
    out, x = [], 1
    for _ in range(n):
        out.append((z * x - 1) % R_MOD)
        x = x * w_inv % R_MOD
    return out


def evaluate_int(f, log2n, z, shifted=False):
    """f: n standard-form values; z standard form.  F(z), or F(z w) for shifted."""
    n = 1 << log2n
    assert len(f) == n
    d = _weights(z, log2n)
    sh = 1 if shifted else 0
    if 0 in d:
        return f[(d.index(0) + sh) % n]
    s = sum(f[(i + sh) % n] * pow(d[i], -1, R_MOD) for i in range(n)) % R_MOD
    return (pow(z, n, R_MOD) - 1) * pow(n, -1, R_MOD) * s % R_MOD


def evaluate(evals, log2n, z, shifted=False):
    return mont_words([evaluate_int(_std(evals), log2n, _std(z)[0], shifted)])[0]


def opening(evals, log2n, z):
    """(the n values of W on the domain, F(z)); z must be off the domain."""
    n = 1 << log2n
    f, zi = _std(evals), _std(z)[0]
    assert off_domain(zi, log2n)
    d = _weights(zi, log2n)
    fz = evaluate_int(f, log2n, zi)
    w_inv = pow(ci.root_of_unity(log2n), -1, R_MOD)
    out, x = [], 1
    for i in range(n):
        out.append(x * (fz - f[i]) * pow(d[i], -1, R_MOD) % R_MOD)
        x = x * w_inv % R_MOD
    return mont_words(out), mont_words([fz])[0]


def coarse_poly(seed, n):
    """n values over the whole input range [0, 2r) (coarse_inputs' catalogue spliced in)."""
    return ci.coarse_scalars(seed, n, 0)


def second_representative(words):
    """x + r for canonical x: the other representative below 2r."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    assert ci.below(w, R_MOD).all()
    return ci.add_int(w, R_MOD)
