"""Python-integer models behind the fixed-base tests (tests/test_fixed_base_cpu.py, tests/test_gpu_fixed_base.py):

* byte_digits      the digit decomposition k = sum_w d_w 2^(8w) csrc/fixed_base.hip walks (k_fb_mul adds T[w][d_w - 1] for d_w != 0);
* mix64            numpy restatement of the splitmix64 finaliser of csrc/msm.hip (the scalars of bbg_srs_synth_hashed);
* lagrange_closed_form   L_k(x) = w^k (x^n - 1) / (n (x - w^k)) for all k with ONE modular inversion: the discrete logarithms of
                   bbg_srs_lagrange's outputs when its input is the powers string [x^j] G.
"""
import numpy as np

import lagrange_model as lm

R_MOD = lm.R_MOD
WINDOWS = 32  # byte positions of a 256-bit scalar
MASK64 = (1 << 64) - 1


def byte_digits(k):
    """The 32 unsigned byte digits of a canonical k < r, least significant first."""
    assert 0 <= k < R_MOD
    return [(k >> (8 * w)) & 0xFF for w in range(WINDOWS)]


def digits_value(digits):
    return sum(d << (8 * w) for w, d in enumerate(digits))


def mix64(z):
    """splitmix64 finaliser on a numpy uint64 array (or scalar), wrapping like the device code."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def hashed_scalars(seed, n):
    """k_i = mix64(seed + i) | 1, i < n, as Python integers: P_i = k_i G is bbg_srs_synth_hashed(seed, n)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK64) + np.arange(n, dtype=np.uint64)
    return [int(v) for v in (mix64(z) | np.uint64(1))]


def batch_inverse(vals):
    """Inverses mod r of non-zero values behind one modular inversion (prefix products)."""
    prefix, acc = [], 1
    for v in vals:
        assert v % R_MOD != 0
        prefix.append(acc)
        acc = acc * v % R_MOD
    inv = pow(acc, R_MOD - 2, R_MOD)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * prefix[i] % R_MOD
        inv = inv * vals[i] % R_MOD
    return out


def lagrange_closed_form(oracle, x, log2n):
    """[L_k(x) mod r]_k for the domain of size n = 2^log2n: L_k(x) = w^k (x^n - 1) / (n (x - w^k)).  x must not be an n-th root of unity."""
    n = 1 << log2n
    w = lm.root(oracle, log2n)
    zx = (pow(x, n, R_MOD) - 1) % R_MOD
    assert zx != 0, "x^n = 1: x lies in the domain"
    wk, acc = [], 1
    for _ in range(n):
        wk.append(acc)
        acc = acc * w % R_MOD
    inv = batch_inverse([n * (x - v) % R_MOD for v in wk])
    return [v * zx % R_MOD * i % R_MOD for v, i in zip(wk, inv)]


def aff_infinity():
    """The affine encoding of the point at infinity include/bbg.h promises: bit 63 of x.data[3] set, every other bit zero."""
    p = np.zeros(8, dtype=np.uint64)
    p[3] = np.uint64(1 << 63)
    return p
