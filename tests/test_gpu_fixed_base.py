"""bbg_g1_fixed_base_mul / bbg_g1_fixed_base_mul_device / bbg_srs_synth_powers on the MI355X (csrc/fixed_base.hip).

Every comparison is bit-exact on canonical Montgomery affine points.  Expected values come from the C oracle (g1_mul, srs_powers) or from
Python integers (tests/tools/fixed_base_model.py, pinned to the oracle in tests/test_fixed_base_cpu.py); where two independent paths of
the library are played against each other (the hashed generator, MSM + poly_evaluate, the Lagrange transform) the test says so.  The point
at infinity is expected in the encoding include/bbg.h promises, written out in fixed_base_model.aff_infinity().

Time limits: each test runs under a limit of its own, stated where it is used.  Nothing here had been measured when the limits were
written, so they are derived, not fitted: the library calls from the operation count of include/bbg.h (at most 32 mixed additions per
scalar, against the 64 doublings + ~32 additions per point of the hashed generator, which makes 2^20 points in well under a second) with a
generous allowance, the host side from the oracle calls and Python-integer loops a test makes."""
import contextlib
import ctypes
import time

import numpy as np
import pytest

import coarse_inputs as ci
import fixed_base_model as fb
import lagrange_model as lm

pytestmark = pytest.mark.gpu

SEED = 0xF1BED
R = fb.R_MOD
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R  # the structured string's x: a fixed full-width value


@contextlib.contextmanager
def time_limit(seconds, what):
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    print(f"{what}: {dt:.3f} s (limit {seconds:.1f} s)")
    assert dt <= seconds, f"{what} took {dt:.3f} s, limit {seconds:.1f} s"


def mont(vals):
    """Python integers -> canonical Montgomery Fr words (k R mod r), vectorised."""
    return ci.to_words([ci.to_mont(v % R, 0) for v in vals])


def oracle_mul(oracle, base, k_mont):
    return lm.canon_points(oracle, oracle.g1_mul(base, k_mont))[0]


def expected(oracle, base, k_mont_words, k_ints):
    """s * base by the oracle; the promised encoding of infinity where s = 0 mod r."""
    return np.stack([fb.aff_infinity() if k % R == 0 else oracle_mul(oracle, base, w) for w, k in zip(k_mont_words, k_ints)])


def device_mul(bbg, scalars, base=None):
    """The device entry point on buffers of its own."""
    n = scalars.shape[0]
    d_s, d_o = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64)
    try:
        bbg.dev_upload(d_s, scalars)
        bbg.g1_fixed_base_mul_device(d_s, n, d_o, base)
        return bbg.dev_download(d_o, (n, 8))
    finally:
        bbg.dev_free(d_s)
        bbg.dev_free(d_o)


@pytest.fixture(scope="module")
def warm(bbg, oracle):
    """One small call before anything is timed: code-object load, the generator's table and first-use allocations."""
    bbg.g1_fixed_base_mul(mont([1, 2, 3]))
    bbg.srs_synth_powers(mont([X_INT])[0], 3).free()


def parity_scalars():
    """(Montgomery words, integers): the edge values of the issue plus random full-width ones, about 300 in all."""
    rng = np.random.default_rng(SEED)
    ks = [0, 1, 2, 255, 256, R - 1]
    for w in (1, 2, 3, 4, 7, 8, 15, 16, 24, 30, 31):
        ks += [(1 << (8 * w)) - 1, (1 << (8 * w)) + 1]
    ks.append(int.from_bytes(b"\xff" * 31 + b"\x2f", "little"))  # every byte 0xff below the top one, < r
    assert ks[-1] < R
    ks += [int.from_bytes(rng.bytes(32), "little") % R for _ in range(260)]
    words = mont(ks)
    # non-canonical representatives: the Montgomery words of k plus r, for k = r (i.e. 0), r + 1 (i.e. 1) and 2r - 1 (i.e. r - 1)
    extra = [R, R + 1, 2 * R - 1]
    coarse = ci.add_int(mont(extra), R)
    assert ci.below(coarse, 2 * R).all() and not ci.below(coarse, R).any()
    return np.concatenate([words, coarse]), ks + extra


# 1 ------------------------------------------------------------------------------------------------ oracle parity, generator
def test_oracle_parity_generator(bbg, oracle, warm):
    words, ks = parity_scalars()
    assert 280 <= len(ks) <= 320
    G = oracle.g1_generator()
    want = expected(oracle, G, words, ks)
    with time_limit(5.0, f"fixed_base_mul, {len(ks)} scalars, host + device entry"):  # two sub-millisecond launches and copies
        got = bbg.g1_fixed_base_mul(words)
        got_dev = device_mul(bbg, words)
    bad = [i for i in range(len(ks)) if not np.array_equal(got[i], want[i])]
    assert not bad, f"scalars {[hex(ks[i]) for i in bad[:6]]} (indices {bad[:6]}) differ from the oracle"
    assert np.array_equal(got_dev, got), "device and host entry points disagree"
    assert sum(1 for k in ks if k % R == 0) == 2  # 0 and its representative r: both produced the infinity encoding above
    # n = 0 is legal
    assert bbg.g1_fixed_base_mul(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 8)
    assert bbg.lib.bbg_g1_fixed_base_mul(bbg.ctx, None, None, 0, None) == 0
    # null pointers with n > 0
    assert bbg.lib.bbg_g1_fixed_base_mul(bbg.ctx, None, None, 4, None) == -1
    assert bbg.lib.bbg_g1_fixed_base_mul_device(bbg.ctx, None, None, 4, None) == -1


# 2 ------------------------------------------------------------------------------------------------ other bases
def test_oracle_parity_other_bases(bbg, oracle, pkg, warm):
    G = oracle.g1_generator()
    B = lm.canon_points(oracle, oracle.g1_mul(G, mont([0xFEDCBA987654321])[0]))[0]
    B_coarse = B.copy()
    B_coarse[:4] = ci.add_int(B[:4].reshape(1, 4), ci.Q_MOD)[0]  # x + p: the same point, a coarse representative
    rng = np.random.default_rng(SEED + 2)
    ks = [0, 1, 2, 255, 256, R - 1, (1 << 248) + 1, (1 << 128) - 1] + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(56)]
    words = mont(ks)
    want_b = expected(oracle, B, words, ks)
    want_g = expected(oracle, G, words, ks)
    with time_limit(5.0, "three table rebuilds and four 64-scalar batches"):  # ~1 ms per table, sub-millisecond batches
        got_b = bbg.g1_fixed_base_mul(words, B)
        got_c = bbg.g1_fixed_base_mul(words, B_coarse)
        got_g = bbg.g1_fixed_base_mul(words)  # the one-slot table cache switches back
        got_gx = bbg.g1_fixed_base_mul(words, lm.canon_points(oracle, G)[0])  # the generator spelt out = the NULL base
    assert np.array_equal(got_b, want_b), "base B: differs from the oracle"
    assert np.array_equal(got_c, want_b), "base B with x + p: differs from the oracle"
    assert np.array_equal(got_g, want_g), "generator after another base: differs from the oracle"
    assert np.array_equal(got_gx, want_g)
    # an infinite base: every multiple is infinite
    got_inf = bbg.g1_fixed_base_mul(words[:5], fb.aff_infinity())
    assert all(np.array_equal(p, fb.aff_infinity()) for p in got_inf)
    assert np.array_equal(bbg.g1_fixed_base_mul(words), want_g)
    # off the curve
    off = B.copy()
    off[4] ^= np.uint64(1)
    assert not oracle.g1_on_curve(off)
    out = np.zeros((len(ks), 8), dtype=np.uint64)
    rc = bbg.lib.bbg_g1_fixed_base_mul(bbg.ctx, off.ctypes.data, words.ctypes.data, len(ks), out.ctypes.data)
    assert rc == -1 and b"curve" in bbg.lib.bbg_last_error() and not out.any()
    with pytest.raises(pkg.BbgError, match="curve"):
        device_mul(bbg, words, off)
    assert np.array_equal(bbg.g1_fixed_base_mul(words, B), want_b)  # the context still computes


# 3 ------------------------------------------------------------------------------------------------ powers string
def test_powers_string_against_the_oracle(bbg, oracle, pkg, warm):
    x_mont = mont([X_INT])[0]
    with time_limit(30.0, "oracle.srs_powers(x, 2^12 + 1)"):  # 4097 host scalar multiplications
        want = lm.canon_points(oracle, oracle.srs_powers(x_mont, (1 << 12) + 1))
    assert np.array_equal(want[0], lm.canon_points(oracle, oracle.g1_generator())[0])
    for n in (1, 2, 3, 257, (1 << 12) + 1):
        with time_limit(5.0, f"bbg_srs_synth_powers n = {n}"):  # microseconds of kernels + the window-table build of make_srs
            srs = bbg.srs_synth_powers(x_mont, n)
        try:
            assert srs.num_points == n
            got = srs.read()
        finally:
            srs.free()
        bad = [i for i in range(n) if not np.array_equal(got[i], want[i])]
        assert not bad, f"n = {n}: points {bad[:8]} differ from oracle.srs_powers"
    # a coarse representative of x gives the same string
    srs = bbg.srs_synth_powers(ci.add_int(x_mont.reshape(1, 4), R)[0], 257)
    try:
        assert np.array_equal(srs.read(), want[:257])
    finally:
        srs.free()
    # x = 0 in both representatives, n = 0, null pointers: BBG_E_INVALID, no handle, *out untouched
    live = bbg.memory_report()["live_srs"]
    sentinel = 0x5E17117E1
    for bad_x in (np.zeros(4, dtype=np.uint64), ci.to_words([R])[0]):
        h = ctypes.c_void_p(sentinel)
        assert bbg.lib.bbg_srs_synth_powers(bbg.ctx, bad_x.ctypes.data, 16, ctypes.byref(h)) == -1
        assert h.value == sentinel and bbg.lib.bbg_last_error()
        with pytest.raises(pkg.BbgError):
            bbg.srs_synth_powers(bad_x, 16)
    h = ctypes.c_void_p(sentinel)
    assert bbg.lib.bbg_srs_synth_powers(bbg.ctx, x_mont.ctypes.data, 0, ctypes.byref(h)) == -1 and h.value == sentinel
    assert bbg.lib.bbg_srs_synth_powers(bbg.ctx, None, 4, ctypes.byref(h)) == -1
    assert bbg.lib.bbg_srs_synth_powers(bbg.ctx, x_mont.ctypes.data, 4, None) == -1
    assert bbg.memory_report()["live_srs"] == live


# 4 ------------------------------------------------------------------------------------------------ hashed string reproduced
def test_hashed_string_reproduced(bbg, oracle, warm):
    """Two independent kernels of the library: k_srs_hashed (64-bit double-and-add, pinned to the oracle by existing tests) and the table."""
    n, seed = 1 << 16, 0xBB254 + 41
    scalars = mont(fb.hashed_scalars(seed, n))
    with time_limit(10.0, "hashed string 2^16 + fixed_base_mul 2^16"):  # both far below a second of kernels; 6 MB of copies
        srs = bbg.srs_synth_hashed(seed, n)
        want = srs.read()
        srs.free()
        got = bbg.g1_fixed_base_mul(scalars)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {n} points differ from bbg_srs_synth_hashed, first at {bad[:8]}"
    assert np.array_equal(got[:8], lm.canon_points(oracle, oracle.srs_hashed(seed, 8)))


# 5 ------------------------------------------------------------------------------------------------ commit equivalence
@pytest.mark.parametrize("n", [(1 << 13) + 1, 1 << 16, 1 << 20, (1 << 21) + 2])
def test_commit_equivalence(bbg, oracle, pkg, warm, n):
    """sum_i c_i [x^i] G = [c(x)] G: one wrong point among the n changes the left side.  MSM and poly_evaluate are oracle-tested elsewhere."""
    x_mont = mont([X_INT])[0]
    coeffs = pkg.synthetic_scalars(SEED + n, n)
    with time_limit(20.0, f"powers string + MSM + evaluation, n = {n}"):  # seconds at most: 2 M points, one MSM, one evaluation
        srs = bbg.srs_synth_powers(x_mont, n)
        try:
            assert srs.num_points == n
            lhs = bbg.g1_normalize(bbg.msm(srs, coeffs))[0]
            first, last = srs.read(0, 1)[0], srs.read(n - 1, 1)[0]
        finally:
            srs.free()
        value = bbg.poly_evaluate(coeffs, x_mont)
        rhs = bbg.g1_fixed_base_mul(value.reshape(1, 4))[0]
    assert np.array_equal(lhs, rhs), f"n = {n}: commitment over the powers string differs from [c(x)] G"
    assert np.array_equal(first, lm.canon_points(oracle, oracle.g1_generator())[0])
    assert np.array_equal(last, oracle_mul(oracle, oracle.g1_generator(), mont([pow(X_INT, n - 1, R)])[0]))


# 6 ------------------------------------------------------------------------------------------------ Lagrange closed form
@pytest.mark.parametrize("lg", [10, 16, 20])
def test_lagrange_closed_form(bbg, oracle, warm, lg):
    """Every output of bbg_srs_lagrange on the powers string is [L_k(x)] G, L_k(x) = w^k (x^n - 1) / (n (x - w^k)) in Python integers."""
    n = 1 << lg
    assert pow(X_INT, n, R) != 1
    with time_limit(60.0, f"closed form in Python integers, 2^{lg}"):  # ~10 big-integer products per k
        e_int = fb.lagrange_closed_form(oracle, X_INT, lg)
        e = mont(e_int)
    with time_limit(20.0, f"powers string, Lagrange transform, fixed_base_mul, 2^{lg}"):  # the transform: 0.45 s at 2^20 (its own test's figure)
        mono = bbg.srs_synth_powers(mont([X_INT])[0], n)
        try:
            lb = mono.lagrange(lg)
            got = lb.read()
            lb.free()
        finally:
            mono.free()
        want = bbg.g1_fixed_base_mul(e)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"2^{lg}: {bad.size} Lagrange points differ from [L_k(x)] G, first at {bad[:8]}"
    if lg == 10:
        rng = np.random.default_rng(SEED + 6)
        G = oracle.g1_generator()
        for k in [0, 1, n // 2, n - 1] + [int(v) for v in rng.integers(0, n, 28)]:
            assert np.array_equal(got[k], oracle_mul(oracle, G, e[k])), f"LB[{k}] != oracle.g1_mul(G, L_k(x))"


# 7 ------------------------------------------------------------------------------------------------ large batch
def test_large_batch_sampled_against_the_oracle(bbg, oracle, warm):
    n = (1 << 20) + 3
    scalars = ci.coarse_scalars(SEED + 7, n, 0)  # Montgomery words spread over the whole [0, 2r), edge values spliced in
    with time_limit(20.0, f"fixed_base_mul_device n = {n}"):
        got = device_mul(bbg, scalars)
    rng = np.random.default_rng(SEED + 7)
    idx = [0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, n - 5, n - 4, n - 3, n - 2, n - 1]  # first, last, borders of the threads' chunks
    idx += [int(v) for v in rng.integers(0, n, 256 - len(idx))]
    G = oracle.g1_generator()
    ks = [ci.from_mont(v, 0) for v in ci.to_ints(scalars[idx])]
    want = expected(oracle, G, scalars[idx], ks)
    bad = [i for j, i in enumerate(idx) if not np.array_equal(got[i], want[j])]
    assert not bad, f"indices {bad[:8]} differ from the oracle"
    infinite = (got[:, 3] >> np.uint64(63)) != 0
    assert np.array_equal(got[infinite], np.tile(fb.aff_infinity(), (int(infinite.sum()), 1)))
    finite = got[~infinite]
    ci.assert_canonical(finite[:, :4], 1, "x")
    ci.assert_canonical(finite[:, 4:], 1, "y")
    for i in idx[:64]:
        if not infinite[i]:
            assert oracle.g1_on_curve(got[i]), f"output {i} is not on the curve"


# 8 ------------------------------------------------------------------------------------------------ memory
def test_table_memory_is_reported_and_trimmed(bbg, oracle, warm):
    table_bytes = 32 * 255 * 64
    words = mont([3, R - 2, 0x123456789ABCDEF0123456789ABCDEF])
    before = bbg.g1_fixed_base_mul(words)
    assert bbg.memory_report()["scratch"] >= table_bytes
    released = bbg.memory_trim()
    assert released >= table_bytes
    assert bbg.memory_report()["scratch"] < table_bytes  # the trim drops every scratch buffer, the table among them
    with time_limit(5.0, "rebuild of the table after a trim"):
        after = bbg.g1_fixed_base_mul(words)
    assert np.array_equal(after, before)
    assert bbg.memory_report()["scratch"] >= table_bytes
    G = oracle.g1_generator()
    assert np.array_equal(after, expected(oracle, G, words, [3, R - 2, 0x123456789ABCDEF0123456789ABCDEF]))
