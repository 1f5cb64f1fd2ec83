"""Fixed-base batch scalar multiplication and the powers-of-x SRS (bbg_g1_fixed_base_mul, bbg_srs_synth_powers): what can be checked
without a GPU -- the ABI surface, the digit model of csrc/fixed_base.hip, and the expected-value generators the GPU tests rely on
(tests/tools/fixed_base_model.py), each pinned to the C oracle here."""
import os
import re

import numpy as np

import fixed_base_model as fb
import lagrange_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bbg_g1_fixed_base_mul", "bbg_g1_fixed_base_mul_device", "bbg_srs_synth_powers")
X_FIXED = 0x1F0E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978  # a fixed 189-bit x


def test_header_and_binding_declare_the_entry_points(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bbg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bbg_[a-z0-9_]+)\s*\(", text))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/bbg.h"
        assert sym in pkg.binding.EXPORTED_SYMBOLS, f"{sym} is missing from binding.EXPORTED_SYMBOLS"
    for method in ("g1_fixed_base_mul", "g1_fixed_base_mul_device", "srs_synth_powers"):
        assert callable(getattr(pkg.Bbg, method, None)), f"Bbg.{method} is missing"
    header = open(os.path.join(ROOT, "include", "bbg.h")).read()
    assert '"fixed_base_table"' in header and '"fixed_base_mul"' in header  # the profile names


def test_digit_model():
    """k = sum_w d_w 2^(8w) with 32 byte digits; the kernel adds T[w][d_w - 1] exactly for the digits 1 .. 255."""
    rng = np.random.default_rng(0xF1BED)
    ks = [0, 1, 255, 256, 1 << 248, fb.R_MOD - 1, (1 << 253) + 12345]
    ks += [int.from_bytes(rng.bytes(32), "little") % fb.R_MOD for _ in range(200)]
    for k in ks:
        d = fb.byte_digits(k)
        assert len(d) == fb.WINDOWS and fb.digits_value(d) == k
        assert all(1 <= v <= 255 for v in d if v != 0) and all(0 <= v <= 255 for v in d)
        # the table index of the last window stays inside the 32 x 255 entries
        assert all(w * 255 + v - 1 < 32 * 255 for w, v in enumerate(d) if v)
    assert fb.byte_digits(0) == [0] * 32
    assert fb.byte_digits(1 << 248)[31] == 1
    assert fb.byte_digits(fb.R_MOD - 1)[31] == 0x30  # r < 2^254: the top digit never exceeds 0x30


def test_lagrange_closed_form_matches_the_model(oracle):
    """[L_k(x)] G from the closed form equals the oracle model's transform of the oracle's powers string, for every k."""
    G = oracle.g1_generator()
    x_mont = lm.ints_to_mont(oracle, [X_FIXED])[0]
    for lg in (1, 3, 5):
        n = 1 << lg
        powers = oracle.srs_powers(x_mont, n)
        want = lm.lagrange_srs(oracle, powers, lg)
        e = lm.ints_to_mont(oracle, fb.lagrange_closed_form(oracle, X_FIXED, lg))
        assert sum(fb.lagrange_closed_form(oracle, X_FIXED, lg)) % fb.R_MOD == 1  # partition of unity
        for k in range(n):
            got = lm.canon_points(oracle, oracle.g1_mul(G, e[k]))[0]
            assert np.array_equal(got, want[k]), f"2^{lg}: [L_{k}(x)] G differs from the model's LB[{k}]"


def test_powers_string_of_the_oracle(oracle):
    """oracle.srs_powers is [x^i] G by oracle.g1_mul: pins the reference of the GPU powers test to the one primitive the others use."""
    G = oracle.g1_generator()
    x_mont = lm.ints_to_mont(oracle, [X_FIXED])[0]
    pts = lm.canon_points(oracle, oracle.srs_powers(x_mont, 6))
    e = lm.ints_to_mont(oracle, [pow(X_FIXED, i, fb.R_MOD) for i in range(6)])
    for i in range(6):
        assert np.array_equal(pts[i], lm.canon_points(oracle, oracle.g1_mul(G, e[i]))[0])
    assert np.array_equal(pts[0], lm.canon_points(oracle, G)[0])


def test_mix64_matches_the_hashed_string(oracle):
    G = oracle.g1_generator()
    seed = 0xBB254
    ks = fb.hashed_scalars(seed, 8)
    want = lm.canon_points(oracle, oracle.srs_hashed(seed, 8))
    sc = lm.ints_to_mont(oracle, ks)
    for i in range(8):
        assert ks[i] & 1 and ks[i] < 1 << 64
        assert np.array_equal(lm.canon_points(oracle, oracle.g1_mul(G, sc[i]))[0], want[i]), f"point {i}"
    # wrap-around of seed + i like the device's 64-bit addition
    assert fb.hashed_scalars((1 << 64) - 2, 4)[2] == int(fb.mix64(np.uint64(0))) | 1


def test_infinity_encoding():
    p = fb.aff_infinity()
    assert int(p[3]) == 1 << 63 and not p[[0, 1, 2, 4, 5, 6, 7]].any()
