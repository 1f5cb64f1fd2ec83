"""Variable-base batch scalar multiplication and the SRS power update (bbg_g1_batch_mul, bbg_srs_scale_powers): what can be checked
without a GPU -- the ABI surface and the Python-integer model of the scalar recoding of csrc/var_base.hip.h
(tests/tools/var_base_model.py), pinned to the C oracle here.

Sign convention: the model (and the device code) writes k = k1 - k2 lambda (mod r) with k1 >= 0 and a SIGNED k2.  oracle.endo_split returns
the reference's halves, k = k1 - k2 lambda with both halves truncated to 128 bits; the two agree wherever the model's k2 is not negative,
which is every scalar of the GPU list but the one constructed to have k2 < 0 (about one scalar in 2^63 does; the reference's truncation
has no correct answer there, the model's sign does).

A half of 2^127 or more: half_bounds() proves there is none for this split (k1 < 0.977 * 2^127, |k2| < 0.941 * 2^127 for every canonical
k), so the GPU list cannot contain one; the list holds a first half close to its bound instead (top digit 7), and the recoding itself is
checked here up to 2^128 - 1."""
import os
import re

import numpy as np

import lagrange_model as lm
import var_base_model as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bbg_g1_batch_mul", "bbg_g1_batch_mul_device", "bbg_srs_scale_powers")
R = vb.R_MOD


def test_header_and_binding_declare_the_entry_points(pkg):
    header = open(os.path.join(ROOT, "include", "bbg.h")).read()
    declared = set(re.findall(r"\b(bbg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/bbg.h"
        assert sym in pkg.binding.EXPORTED_SYMBOLS, f"{sym} is missing from binding.EXPORTED_SYMBOLS"
    for method in ("g1_batch_mul", "g1_batch_mul_device"):
        assert callable(getattr(pkg.Bbg, method, None)), f"Bbg.{method} is missing"
    assert callable(getattr(pkg.binding.Srs, "scale_powers", None)), "Srs.scale_powers is missing"
    for name in ('"var_base_mul"', '"batch_mul_glv"', '"ecntt_mul"'):
        assert name in header, f"{name} is not listed in include/bbg.h"


def test_constants_against_the_oracle(oracle):
    """lambda and beta are the cube roots for which lambda (x, y) = (beta x, y), by oracle.g1_mul on G and on another point."""
    assert vb.constants_ok()
    G = lm.canon_points(oracle, oracle.g1_generator())[0]
    P = lm.canon_points(oracle, oracle.g1_mul(G, lm.ints_to_mont(oracle, [0xFEDCBA987654321])[0]))[0]
    lam = lm.ints_to_mont(oracle, [vb.LAMBDA])[0]
    for pt in (G, P):
        got = lm.canon_points(oracle, oracle.g1_mul(pt, lam))[0]
        x = lm.limbs_to_int(oracle.from_mont(1, pt[:4].reshape(1, 4))[0])
        bx = oracle.to_mont(1, lm.ints_to_limbs([vb.BETA * x % vb.Q_MOD]))[0]
        assert np.array_equal(got[:4], oracle.canon(1, bx.reshape(1, 4))[0]), "lambda P: x is not beta x_P"
        assert np.array_equal(got[4:], pt[4:]), "lambda P: y is not y_P"


def test_split_agrees_with_the_oracle(oracle):
    names, ks = vb.gpu_scalars()
    rng = np.random.default_rng(vb.SEED + 2)
    ks = ks + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(2000)]
    halves = oracle.endo_split(lm.ints_to_mont(oracle, ks))
    negative = 0
    for k, h in zip(ks, halves):
        k1, k2 = vb.split(k)
        if k2 < 0:
            negative += 1
            continue
        assert (int(h[0]) | int(h[1]) << 64, int(h[2]) | int(h[3]) << 64) == (k1, k2), f"k = {k:#x}: halves differ from oracle.endo_split"
    assert negative == 1  # the constructed one
    k1_max, k2_max = vb.half_bounds()
    assert k1_max < 1 << 127 and k2_max < 1 << 127  # no canonical scalar has a half of 2^127 or more
    assert max(max(vb.split(k)[0], abs(vb.split(k)[1])) for k in ks) < max(k1_max, k2_max)


def test_recoding_recombines():
    """Digits are odd, in range, select a table entry below 8, and the rounds + skews give back k mod r for the whole GPU list."""
    names, ks = vb.gpu_scalars()
    assert 290 <= len(ks) <= 300
    for name, k in zip(names, ks):
        assert vb.recombine(k) == k, f"{name}: the recoded halves do not recombine to k"
    # the recoding alone over the whole range of a 128-bit half, 2^127 and more included
    rng = np.random.default_rng(vb.SEED + 3)
    hs = [0, 1, 2, 15, 16, 17, (1 << 127) - 1, 1 << 127, (1 << 127) + 1, (1 << 128) - 2, (1 << 128) - 1]
    hs += [int.from_bytes(rng.bytes(16), "little") for _ in range(500)]
    for h in hs:
        digits, skew = vb.recode(h)
        assert len(digits) == vb.WINDOWS and skew == 1 - (h & 1) and vb.digits_value(digits) == h + skew
        assert digits[0] > 0 and all(0 <= vb.table_index(d) < 8 for d in digits)


def test_gpu_scalar_list_covers_the_branches():
    names, ks = vb.gpu_scalars()
    rep = vb.case_report(ks)
    assert vb.split(0) == (0, 0) and vb.split(1) == (1, 0)
    # a zero first half beside a non-zero second does not exist (case_report's docstring); 0 - 1 lambda = r - lambda is in the list all the
    # same and splits into two large halves
    assert not rep["zero_k1_only"] and min(vb.split(R - vb.LAMBDA)) > 1 << 120
    for case in ("zero_k1", "zero_k2", "zero_k2_only", "skew1_set", "skew1_clear", "skew2_set", "skew2_clear", "negative_k2"):
        assert rep[case], f"no scalar of the GPU list has {case}"
    assert rep["digits"] == set(range(-15, 16, 2))  # every digit value, both extremes +-15 and +-1 among them
    assert rep["top_digits"] == {1, 3, 5, 7}  # every top digit the bounds allow
    assert rep["max_half"] > 0x7C << 120  # a half close to the proven bound
    for name in ("0", "1", "2", "r - 1", "lambda", "lambda - 1", "lambda + 1", "r - lambda", "2^127 - 1", "2^127 + 1", "2^128", "nibbles 7", "nibbles 8", "nibbles f"):
        assert name in names


def test_scale_powers_closed_form(oracle):
    """[y^i] [x^i] G = [(x y)^i] G on the oracle, n = 8."""
    x, y = 0x1F0E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978, 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
    n = 8
    px = lm.canon_points(oracle, oracle.srs_powers(lm.ints_to_mont(oracle, [x])[0], n))
    pxy = lm.canon_points(oracle, oracle.srs_powers(lm.ints_to_mont(oracle, [x * y % R])[0], n))
    yi = lm.ints_to_mont(oracle, [pow(y, i, R) for i in range(n)])
    for i in range(n):
        assert np.array_equal(lm.canon_points(oracle, oracle.g1_mul(px[i], yi[i]))[0], pxy[i]), f"point {i}"
