"""CPU tests of tests/tools/coarse_inputs.py, the helpers of the coarse-range GPU tests (tests/test_gpu_coarse_range.py): the edge
catalogue lies in [0, 2p), the big-integer references agree with the oracle, and the MSM digit patterns are exactly what a restatement
of recode_digits (msm_kernels.hip.h) makes of them."""
import numpy as np
import pytest

import coarse_inputs as ci


@pytest.mark.parametrize("which", [0, 1])
def test_catalogue_and_coarse_scalars_in_range(which):
    p = ci.MODULI[which]
    cat = ci.catalogue(which)
    assert all(0 <= v < 2 * p for v in cat)
    for v in (0, 1, p - 1, p, p + 1, 2 * p - 1, (1 << 252) - 1, 1 << 252, 1 << 253, ci.MONT_R % p, p + ci.MONT_R % p):
        assert v in cat
    top = max(v for v in cat if v % (1 << 232) == (1 << 232) - 1)
    assert top < 2 * p <= top + (1 << 232)
    vals = ci.coarse_ints(5, 4096, which)
    assert vals == ci.coarse_ints(5, 4096, which)  # deterministic
    assert all(0 <= v < 2 * p for v in vals)
    assert set(cat) <= set(vals)
    # spread over the whole range, not only its bottom sixth
    assert sum(v >= p for v in vals) > 1500 and sum(v >= (1 << 252) for v in vals) > 3000
    w = ci.coarse_scalars(5, 4096, which)
    assert ci.to_ints(w) == vals
    ci.assert_coarse(w, which)
    with pytest.raises(AssertionError):
        ci.assert_coarse(ci.to_words([2 * p]), which)
    with pytest.raises(AssertionError):  # differs from 2p only below the top word
        ci.assert_coarse(ci.to_words([2 * p + (1 << 64)]), which)
    ci.assert_canonical(ci.to_words([p - 1]), which)
    with pytest.raises(AssertionError):
        ci.assert_canonical(ci.to_words([p]), which)


def test_word_arithmetic():
    a = ci.coarse_ints(1, 500, 0)
    b = ci.coarse_ints(2, 500, 0)
    assert ci.to_ints(ci.add_words(ci.to_words(a), ci.to_words(b))) == [x + y for x, y in zip(a, b)]
    assert ci.to_ints(ci.add_int(ci.to_words(a), ci.R_MOD)) == [x + ci.R_MOD for x in a]
    with pytest.raises(AssertionError):
        ci.add_int(ci.to_words([(1 << 256) - 1]), 1)
    mask = ci.below(ci.to_words(a), ci.R_MOD)
    assert mask.tolist() == [x < ci.R_MOD for x in a]


def test_jacobian_range_check():
    q2 = 2 * ci.Q_MOD
    ok = ci.to_words([q2 - 1, 5, q2 - 1]).reshape(1, 12)
    ci.assert_coarse_jacobian(ok)
    bad = ok.copy()
    bad[0, 8:12] = ci.to_words([q2])[0]
    with pytest.raises(AssertionError):
        ci.assert_coarse_jacobian(bad)
    inf = bad.copy()
    inf[0, 3] |= np.uint64(1 << 63)  # the infinity bit: coordinates are not read
    ci.assert_coarse_jacobian(inf)


@pytest.mark.parametrize("which", [0, 1])
def test_big_integer_references_agree_with_the_oracle(oracle, which):
    vals = ci.catalogue(which)
    a_int = [x for x in vals for _ in vals]
    b_int = [y for _ in vals for y in vals]
    a, b = ci.to_words(a_int), ci.to_words(b_int)
    for fn, ref in ((oracle.fe_mul, ci.mont_mul), (oracle.fe_add, ci.mont_add), (oracle.fe_sub, ci.mont_sub)):
        assert ci.to_ints(oracle.canon(which, fn(which, a, b))) == [ref(x, y, which) for x, y in zip(a_int, b_int)]
    w = ci.to_words(vals)
    assert ci.to_ints(oracle.canon(which, oracle.from_mont(which, w))) == [ci.from_mont(v, which) for v in vals]
    assert ci.to_ints(oracle.canon(which, oracle.to_mont(which, w))) == [ci.to_mont(v, which) for v in vals]
    nz = [v for v in vals if v % ci.MODULI[which]]
    assert ci.to_ints(oracle.canon(which, oracle.fe_inv(which, ci.to_words(nz)))) == [ci.mont_inv(v, which) for v in nz]


@pytest.mark.parametrize("lg", [0, 1, 2, 3, 5])
def test_dft_and_horner_agree_with_the_oracle(oracle, lg):
    n = 1 << lg
    vals = ci.coarse_ints(40 + lg, n, 0)
    w = ci.to_words(vals)
    assert ci.to_ints(oracle.canon(0, oracle.root_of_unity(lg).reshape(1, 4)))[0] == ci.to_mont(ci.root_of_unity(lg), 0)
    for op in range(4):
        assert ci.to_ints(oracle.canon(0, oracle.ntt(w, op))) == ci.dft(vals, op), op
    z = ci.coarse_ints(99, 1, 0)[0]
    assert ci.to_ints(oracle.canon(0, oracle.poly_eval(w, ci.to_words([z])[0]).reshape(1, 4)))[0] == ci.horner(vals, z)


@pytest.mark.parametrize("c", ci.MSM_WINDOWS)
def test_window_layout_covers_255_bits(c):
    L = ci.MsmLayout(c)
    assert L.offset(L.windows) == 255
    assert all(L.offset(w + 1) - L.offset(w) == L.width(w) for w in range(L.windows))
    assert L.windows <= 32 and L.width(L.windows - 1) in (c, c - 1)
    if c == 8:  # msm_tiny.hip: 31 windows of 8 bits and a 7-bit top window, 128 buckets
        assert (L.windows, L.nwide) == (32, 31)


@pytest.mark.parametrize("c", ci.MSM_WINDOWS)
def test_digit_patterns_recode_to_their_digits(c):
    L = ci.MsmLayout(c)
    top = 1 << (c - 1)
    pats = ci.msm_digit_patterns(c)
    names = [p[0] for p in pats]
    assert len(set(names)) == len(names)
    for w in range(1, L.windows):
        assert f"ones_{L.offset(w)}" in names  # the carry chain through every window, up to the top one
    for name, k, digits in pats:
        assert 0 <= k < ci.R_MOD, name
        got, buckets = ci.recode_digits(k, c)
        assert got == digits, name
        assert ci.digits_value(got, c) == k, name
        assert all(0 <= b <= top for b in buckets), name
        for w, d in enumerate(got):
            h = 1 << (L.width(w) - 1)
            assert -h < d <= h, (name, w)
        assert got[-1] >= 0, name
    by = dict((p[0], p[2]) for p in pats)
    _, b = ci.recode_digits(dict((p[0], p[1]) for p in pats)["top_bucket_all"], c)
    assert b[:-1] == [top] * (L.windows - 1)  # every window but the top one in the lone extra sort partition
    assert all(d == -((1 << (L.width(w) - 1)) - 1) for w, d in enumerate(by["neg_carry_all"][:-1]))
    chain = by[f"ones_{L.offset(L.windows - 1)}"]
    assert chain == [-1] + [0] * (L.windows - 2) + [1]  # zero digits from carries all the way to the top window


def test_recode_restatement_on_random_scalars():
    rng = np.random.default_rng(3)
    for c in ci.MSM_WINDOWS:
        for _ in range(200):
            k = int.from_bytes(rng.bytes(32), "little") % ci.R_MOD
            digits, _ = ci.recode_digits(k, c)
            assert ci.digits_value(digits, c) == k
