"""bbg_open_all on the MI355X: the opening proofs of one polynomial at all n points of its domain through a prepared handle
(csrc/open_all.hip, Feist-Khovratovich over the G1 transforms of csrc/ecntt.hip).

Every comparison is bit-exact on canonical Montgomery affine words.  Expected values come from the host model's DEFINITION route
(tests/tools/open_all_model.py: quotient coefficients, then oracle.msm_naive), from the closed form over a powers string through
bbg_g1_fixed_base_mul and oracle.g1_mul, or from the existing single-opening route bbg_kate_opening + bbg_msm.  Where all n proofs by the
model would take minutes (2^10: a million oracle multiplications) sixteen seeded indices are checked by it instead.

The SRS is freed between prepare and the first call in every test: the handle keeps nothing of it."""
import contextlib
import ctypes
import json
import os
import statistics
import time

import numpy as np
import pytest

import coarse_inputs as ci
import lagrange_model as lm
import open_all_model as oa

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = oa.R_MOD
SEED = 0xBB254 + 0x0A11
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R


@contextlib.contextmanager
def option(bbg, key, value, default):
    bbg.set_option(key, value)
    try:
        yield
    finally:
        bbg.set_option(key, default)


def mont(vals):
    return ci.to_words([ci.to_mont(v % R, 0) for v in vals])


def coefficients(seed, n):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]


def infinities(n):
    return np.tile(oa.aff_infinity(), (n, 1))


def check(got, want, what):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} proofs differ, first at {bad[:8]}"


def prepared(bbg, srs, lg):
    """The handle over `srs`, which is freed before the handle is used."""
    h = bbg.open_all_prepare(srs, lg)
    srs.free()
    return h


@pytest.fixture(scope="module")
def hashed(bbg):
    """{lg: (points, handle)} over hashed strings (no structure), made on first use and kept for the module."""
    made = {}

    def get(lg):
        if lg not in made:
            srs = bbg.srs_synth_hashed(SEED + lg, 1 << lg)
            pts = srs.read()
            made[lg] = (pts, prepared(bbg, srs, lg))
        return made[lg]
    yield get
    for _, h in made.values():
        h.free()


# 1 ------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("lg", [1, 2, 3, 6])
def test_against_the_model(bbg, oracle, hashed, lg):
    n = 1 << lg
    pts, h = hashed(lg)
    f = coefficients(SEED + 100 + lg, n)
    want = oa.open_all_definition(oracle, pts, f)
    words = mont(f)
    check(h.open(words), want, f"n = {n}, canonical coefficients")
    lifted = ci.add_int(words, R)
    assert ci.below(lifted, 2 * R).all() and not ci.below(lifted, R).any()
    check(h.open(lifted), want, f"n = {n}, coefficients in [r, 2r)")
    # the device entry, coefficients left untouched
    d_c, d_o = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64)
    try:
        bbg.dev_upload(d_c, lifted)
        h.open_device(d_c, d_o)
        check(bbg.dev_download(d_o, (n, 8)), want, f"n = {n}, device entry")
        assert np.array_equal(bbg.dev_download(d_c, (n, 4)), lifted), "the coefficients were written"
    finally:
        bbg.dev_free(d_c)
        bbg.dev_free(d_o)


# 2 ------------------------------------------------------------------------------------------------ closed form at size
@pytest.fixture(scope="module")
def closed_form(bbg):
    """{lg: (coefficient words, scalars k_m, [k_m] G by bbg_g1_fixed_base_mul)} over the powers string of X_INT, computed once."""
    made = {}

    def get(lg):
        if lg not in made:
            n = 1 << lg
            f = coefficients(SEED + 200 + lg, n)
            ks = oa.closed_form_scalars(f, X_INT, ci.root_of_unity(lg))
            made[lg] = (mont(f), ks, bbg.g1_fixed_base_mul(mont(ks)))
        return made[lg]
    return get


@pytest.mark.parametrize("lg,key,value,default", [(12, None, 0, 0), (16, None, 0, 0), (12, "batch_mul_lanes", 64, 1 << 17), (12, "ecntt_mul", 0, 1)])
def test_closed_form_over_a_powers_string(bbg, oracle, closed_form, lg, key, value, default):
    n = 1 << lg
    assert lm.root(oracle, lg) == ci.root_of_unity(lg)
    words, ks, want = closed_form(lg)
    with option(bbg, key, value, default) if key else contextlib.nullcontext():
        h = prepared(bbg, bbg.srs_synth_powers(mont([X_INT])[0], n), lg)
        try:
            got = h.open(words)
        finally:
            h.free()
    check(got, want, f"2^{lg}, {key} = {value}")
    if key is None:
        G = oracle.g1_generator()
        rng = np.random.default_rng(SEED + lg)
        for m in [0, n - 1] + [int(v) for v in rng.integers(0, n, 14)]:
            assert np.array_equal(got[m], oa.canon_points(oracle, oracle.g1_mul(G, mont([ks[m]])[0]))[0]), f"2^{lg}: proof {m} != [k_m] G"


# 3 ------------------------------------------------------------------------------------------------ the existing route
def test_agrees_with_kate_opening_and_msm(bbg, oracle):
    lg = 12
    n = 1 << lg
    srs = bbg.srs_synth_hashed(SEED + 300, n)
    try:
        h = bbg.open_all_prepare(srs, lg)
        try:
            words = mont(coefficients(SEED + 301, n))
            got = h.open(words)
        finally:
            h.free()
        w = ci.root_of_unity(lg)
        rng = np.random.default_rng(SEED + 302)
        for m in [0] + [int(v) for v in rng.integers(1, n, 7)]:
            quotient, _ = bbg.kate_opening(words, mont([pow(w, m, R)])[0])
            want = bbg.g1_normalize(bbg.msm(srs, quotient))[0]
            assert np.array_equal(got[m], want), f"proof {m} differs from kate_opening + msm"
    finally:
        srs.free()


# 4 ------------------------------------------------------------------------------------------------ edge polynomials
@pytest.mark.parametrize("lg", [3, 10])
def test_edge_polynomials(bbg, oracle, hashed, lg):
    n = 1 << lg
    pts, h = hashed(lg)
    zero = [0] * n
    check(h.open(mont(zero)), infinities(n), "f = 0")
    check(h.open(mont([12345] + zero[1:])), infinities(n), "f = a constant")
    check(h.open(mont(coefficients(SEED + 400, 1) + zero[1:])), infinities(n), "f_0 random, the rest zero")
    check(h.open(ci.to_words([R] * n)), infinities(n), "f = 0 written as r")
    check(h.open(mont([0, 1] + zero[2:])), np.tile(pts[0], (n, 1)), "f = X")
    top = zero[:n - 1] + [1]
    got = h.open(mont(top))
    if lg <= 3:
        check(got, oa.open_all_definition(oracle, pts, top), "f = X^(n-1)")
    else:
        rng = np.random.default_rng(SEED + 401)
        ms = [0, 1, n // 2, n - 1] + [int(v) for v in rng.integers(0, n, 12)]
        check(got[ms], oa.open_all_definition(oracle, pts, top, ms), "f = X^(n-1), sixteen indices")


# 5 ------------------------------------------------------------------------------------------------ handle behaviour
def test_handle_behaviour(bbg, oracle, hashed):
    lg = 6
    n = 1 << lg
    pts, h = hashed(lg)
    assert h.device_bytes() == 2 * n * 64 + 2 * n * 128 + n * 128 + 2 * n * 32
    f1, f2 = mont(coefficients(SEED + 500, n)), mont(coefficients(SEED + 501, n))
    with open(os.path.join(ROOT, "tests", "golden", "lagrange_srs.json")) as fh:
        fixture = json.load(fh)
    golden = np.frombuffer(bytes.fromhex(fixture["points"]["6"]), dtype=np.uint64).reshape(-1, 8)
    mono = bbg.srs_synth_hashed(fixture["srs_seed"], 1 << 12)
    try:
        def lagrange():
            lb = mono.lagrange(6)
            try:
                return lb.read()
            finally:
                lb.free()
        assert np.array_equal(lagrange(), golden)
        a1 = h.open(f1)
        assert np.array_equal(lagrange(), golden), "bbg_srs_lagrange changed after an open-all call on the same context"
    finally:
        mono.free()
    a2 = h.open(f2)
    assert not np.array_equal(a1, a2)
    check(h.open(f1), a1, "the first polynomial again through the same handle")
    fresh = []
    for f in (f1, f2):
        g = prepared(bbg, bbg.srs_register(pts), lg)
        try:
            fresh.append(g.open(f))
        finally:
            g.free()
    check(a1, fresh[0], "one handle, first polynomial, against a fresh handle")
    check(a2, fresh[1], "one handle, second polynomial, against a fresh handle")
    check(a1, oa.open_all_definition(oracle, pts, [ci.from_mont(v, 0) for v in ci.to_ints(f1)]), "first polynomial against the model")
    # the handle's memory is its own: a trim between two calls changes nothing, and does not count or release it
    bbg.memory_trim()
    assert h.device_bytes() == 576 * n
    check(h.open(f2), a2, "after bbg_memory_trim")


# 6 ------------------------------------------------------------------------------------------------ errors
def test_errors(bbg, pkg):
    srs = bbg.srs_synth_hashed(SEED + 600, 16)
    try:
        sentinel = 0x5E17117E1
        for lg in (0, 28, 5):  # out of range twice, then 32 > the 16 points the string holds
            out = ctypes.c_void_p(sentinel)
            assert bbg.lib.bbg_open_all_prepare(bbg.ctx, srs.handle, lg, ctypes.byref(out)) == -1 and bbg.lib.bbg_last_error()
            assert out.value == sentinel, "*out was written on the error path"
            with pytest.raises(pkg.BbgError):
                bbg.open_all_prepare(srs, lg)
        out = ctypes.c_void_p(sentinel)
        assert bbg.lib.bbg_open_all_prepare(bbg.ctx, None, 4, ctypes.byref(out)) == -1 and out.value == sentinel
        assert bbg.lib.bbg_open_all_prepare(bbg.ctx, srs.handle, 4, None) == -1
        assert bbg.lib.bbg_open_all_prepare(None, srs.handle, 4, ctypes.byref(out)) == -1 and out.value == sentinel
        h = bbg.open_all_prepare(srs, 4)  # n = num_points exactly is legal
        try:
            buf = np.zeros((16, 8), dtype=np.uint64)
            co = np.zeros((16, 4), dtype=np.uint64)
            assert bbg.lib.bbg_open_all(None, co.ctypes.data, buf.ctypes.data) == -1
            assert bbg.lib.bbg_open_all(h.handle, None, buf.ctypes.data) == -1
            assert bbg.lib.bbg_open_all(h.handle, co.ctypes.data, None) == -1
            assert bbg.lib.bbg_open_all_device(None, None, None) == -1 and bbg.lib.bbg_open_all_device(h.handle, None, None) == -1
            size = ctypes.c_size_t(7)
            assert bbg.lib.bbg_open_all_device_bytes(None, ctypes.byref(size)) == -1 and bbg.lib.bbg_open_all_device_bytes(h.handle, None) == -1
            assert size.value == 7 and not buf.any()
            with pytest.raises(ValueError):
                h.open(co[:8])
        finally:
            h.free()
        bbg.lib.bbg_open_all_free(None)  # legal, does nothing
    finally:
        srs.free()


# 7 ------------------------------------------------------------------------------------------------ one time bound
def test_time_bound_at_2_12(bbg):
    """A prepared call at 2^12 is the stages of srs.lagrange(13) and srs.lagrange(12) and the products of a 2^13-term batch multiplication,
    minus two normalisations, plus one 2^13 Fr NTT and three small kernels: it must take no more than 1.5 x the sum of those three existing
    entry points, medians of five runs each after a warm-up, same process.  At this size all of it is launch latency; the margin covers
    the Fr NTT and the small kernels."""
    lg = 12
    n = 1 << lg
    srs = bbg.srs_synth_hashed(SEED + 700, 2 * n)
    d_p = d_s = d_o = d_c = None
    h = None
    try:
        h = bbg.open_all_prepare(srs, lg)
        d_p, d_s, d_o, d_c = bbg.dev_alloc(2 * n * 64), bbg.dev_alloc(2 * n * 32), bbg.dev_alloc(2 * n * 64), bbg.dev_alloc(n * 32)
        scalars = mont(coefficients(SEED + 701, 2 * n))
        bbg.dev_upload(d_p, srs.read())
        bbg.dev_upload(d_s, scalars)
        bbg.dev_upload(d_c, scalars[:n])

        def lagrange(k):
            srs.lagrange(k).free()

        def batch_mul():
            bbg.g1_batch_mul_device(d_p, d_s, 2 * n, d_o)
            bbg.sync()

        def open_all():
            h.open_device(d_c, d_o)
            bbg.sync()

        def median(fn):
            fn()  # warm-up
            bbg.sync()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts)

        parts = [median(lambda: lagrange(13)), median(lambda: lagrange(12)), median(batch_mul)]
        mine = median(open_all)
        print(f"open_all 2^12: {mine * 1e3:.2f} ms; lagrange(13) + lagrange(12) + batch_mul(2^13) = "
              f"{parts[0] * 1e3:.2f} + {parts[1] * 1e3:.2f} + {parts[2] * 1e3:.2f} = {sum(parts) * 1e3:.2f} ms; bound {1.5 * sum(parts) * 1e3:.2f} ms")
        assert mine <= 1.5 * sum(parts), f"open_all at 2^12 took {mine * 1e3:.2f} ms, more than 1.5 x {sum(parts) * 1e3:.2f} ms"
    finally:
        if h is not None:
            h.free()
        for d in (d_p, d_s, d_o, d_c):
            if d is not None:
                bbg.dev_free(d)
        srs.free()
