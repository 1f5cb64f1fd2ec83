"""bbg_open_all on the MI355X: the opening proofs of one polynomial at all n points of its domain through a prepared handle
(csrc/open_all.hip, Feist-Khovratovich over the G1 transforms of csrc/ecntt.hip).

Every comparison is bit-exact on canonical Montgomery affine words.  Expected values come from the host model's DEFINITION route
(tests/tools/open_all_model.py: quotient coefficients, then oracle.msm_naive), from the closed form over a powers string through
bbg_g1_fixed_base_mul and oracle.g1_mul, or from the existing single-opening route bbg_kate_opening + bbg_msm.  Where all n proofs by the
model would take minutes (2^10: a million oracle multiplications) sixteen seeded indices are checked by it instead.

The SRS is freed between prepare and the first call in every test: the handle keeps nothing of it.

Designed inputs (sections 8 - 11, tests/tools/g1_design.py; tests/test_g1_design_cpu.py holds the designs to their claims).  Over a hashed or
a random powers string no entry of s_hat = NTT_G1,2n(s^) is infinite and no entry of c_hat = NTT_Fr,2n(c^) is zero, so these cases build
strings [a_j] G and coefficients whose transforms vanish at chosen indices, and want [k_m] G for the integers k_m = sum_j q^(m)_j a_j:
  8   infinite entries of the prepared string: k_open_batch_pointwise's aff_is_inf branch, k_ecntt_normalize<true>'s stored infinity, and
      xyzz_mul_glv returning early in some lanes of a wave -- both ends, a wave border, a later round of the lane-stride loop;
  9   zero entries of c_hat: the k = 0 path of xyzz_mul_glv among ordinary products, beside a finite and at an infinite s_hat entry;
  10  powers strings of x = 1, -1, w_n, w_n^3, w_n^-1, w_2n with f = 1 + X + .., 1 - X + .., random: equal and opposite points meet inside
      both sets of stages, which the pointwise products feed with non-normalised XYZZ (for f = 1 + X + .. and x on the domain all proofs
      but two cancel to infinity inside the forward stages);
  11  one handle through a random, a designed, the zero and the first polynomial again: nothing an early return leaves behind leaks."""
import contextlib
import ctypes
import json
import os
import statistics
import time

import numpy as np
import pytest

import coarse_inputs as ci
import g1_design as gd
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


# ------------------------------------------------------------------------------------------------ designed inputs (g1_design.py)
INF_AT = {2: {3}, 3: {0, 5, 15}, 6: {0, 1, 63, 64, 65, 127}, 8: {0, 1, 63, 64, 65, 130, 511}}  # where s_hat is the point at infinity
# where c_hat is zero: at an infinite s_hat entry, at its finite neighbour, at 0 and at 2n - 1; at 2^8 also past the first 64 lanes,
# at the infinite entry 130 and the finite 131
ZERO_AT = {3: {0, 5, 6, 15}, 6: {0, 1, 2, 127}, 8: {0, 1, 2, 130, 131, 511}}
LANES64 = ("batch_mul_lanes", 64, 1 << 17)
SERIAL = ("ecntt_mul", 0, 1)


def fixed(bbg, scalars):
    """[k] G for plain integers k by bbg_g1_fixed_base_mul; k = 0 comes back as the affine encoding of infinity."""
    out = bbg.g1_fixed_base_mul(mont(scalars))
    for i, k in enumerate(scalars):
        assert np.array_equal(out[i], oa.aff_infinity()) == (k % R == 0)
    return out


def optional(bbg, opt):
    return option(bbg, *opt) if opt else contextlib.nullcontext()


def sixteen(n, seed, must=()):
    ms = list(dict.fromkeys([0, n - 1] + list(must)))
    rng = np.random.default_rng(seed)
    while len(ms) < min(16, n):
        m = int(rng.integers(0, n))
        if m not in ms:
            ms.append(m)
    return ms


def by_generator(oracle, scalars):
    G = oracle.g1_generator()
    return oa.canon_points(oracle, np.stack([oracle.g1_mul(G, k) for k in mont(scalars)]))


@pytest.fixture(scope="module")
def designed_string(bbg):
    """lg -> (scalars a, points [a_j] G) of the string whose s_hat is infinite at exactly INF_AT[lg], made on first use."""
    made = {}

    def get(lg):
        if lg not in made:
            a, s_hat = gd.design_string(lg, INF_AT[lg], SEED + 800 + lg)
            assert {k for k, v in enumerate(s_hat) if v == 0} == INF_AT[lg]
            pts = fixed(bbg, a)
            # what prepare computes, through bbg_g1_ntt (the same load, stages and normalize<true>): [s_hat_k] G, infinite where designed
            check(bbg.g1_ntt(oa.embedding(pts, [0] * (1 << lg))[0]), fixed(bbg, s_hat), f"2^{lg}: NTT_G1,2n(s^) of the designed string")
            made[lg] = (a, pts)
        return made[lg]
    return get


# 8 ------------------------------------------------------------------------------------------------ infinite entries of s_hat
@pytest.mark.parametrize("lg,opt", [(2, None), (3, None), (6, None), (8, LANES64), (2, SERIAL)], ids=["4", "8", "64", "256-lanes64", "4-ecntt_mul0"])
def test_infinite_entries_of_the_prepared_string(bbg, oracle, designed_string, lg, opt):
    n = 1 << lg
    a, pts = designed_string(lg)
    f = coefficients(SEED + 810 + lg, n)
    ks = gd.proof_scalars(f, a)
    want = fixed(bbg, ks)
    with optional(bbg, opt):
        h = prepared(bbg, bbg.srs_register(pts), lg)
        try:
            got = h.open(mont(f))
        finally:
            h.free()
    check(got, want, f"n = {n}, {opt}: s_hat infinite at {sorted(INF_AT[lg])}")
    if n <= 8:
        check(want, oa.open_all_definition(oracle, pts, f), f"n = {n}: [k_m] G against the definition")
    else:
        ms = sixteen(n, SEED + 811)
        by_oracle = oa.open_all_definition(oracle, pts, f, ms) if n <= 64 else by_generator(oracle, [ks[m] for m in ms])
        check(want[ms], by_oracle, f"n = {n}: [k_m] G against the oracle at {ms}")


# 9 ------------------------------------------------------------------------------------------------ zero entries of c_hat
@pytest.mark.parametrize("string,lg,opt", [("hashed", 3, None), ("hashed", 6, None), ("hashed", 3, SERIAL),
                                           ("designed", 3, None), ("designed", 6, None), ("designed", 8, LANES64), ("designed", 3, SERIAL)],
                         ids=["hashed-8", "hashed-64", "hashed-8-ecntt_mul0", "designed-8", "designed-64", "designed-256-lanes64", "designed-8-ecntt_mul0"])
def test_zero_entries_of_the_transformed_coefficients(bbg, oracle, hashed, designed_string, string, lg, opt):
    n = 1 << lg
    f, c_hat = gd.design_coeffs(lg, ZERO_AT[lg], SEED + 820 + lg)
    assert {k for k, v in enumerate(c_hat) if v == 0} == ZERO_AT[lg]
    if string == "hashed":
        pts = hashed(lg)[0]
        want = None
    else:
        a, pts = designed_string(lg)
        assert ZERO_AT[lg] & INF_AT[lg] and ZERO_AT[lg] - INF_AT[lg]  # 0 x infinity, and 0 x a finite point
        want = fixed(bbg, gd.proof_scalars(f, a))
    with optional(bbg, opt):
        h = prepared(bbg, bbg.srs_register(pts), lg)
        try:
            got = h.open(mont(f))
        finally:
            h.free()
    what = f"n = {n}, {string} string, {opt}: c_hat zero at {sorted(ZERO_AT[lg])}"
    if want is not None:
        check(got, want, what)
    if n <= 8:
        check(got, oa.open_all_definition(oracle, pts, f), what + ", against the definition")
    elif n <= 64:
        ms = sixteen(n, SEED + 821)
        check(got[ms], oa.open_all_definition(oracle, pts, f, ms), what + f", against the definition at {ms}")


# 10 ----------------------------------------------------------------------------------------------- degenerate powers strings
def power_bases(lg):
    w = ci.root_of_unity(lg)
    return {"1": 1, "-1": R - 1, "w_n": w, "w_n^3": pow(w, 3, R), "w_n^-1": pow(w, R - 2, R), "w_2n": ci.root_of_unity(lg + 1)}


@pytest.mark.parametrize("lg,names,polys,opt", [(6, ("1", "-1", "w_n", "w_n^3", "w_n^-1", "w_2n"), ("ones", "alternating", "random"), None),
                                                (6, ("1", "-1", "w_n", "w_n^3", "w_n^-1", "w_2n"), ("ones", "alternating", "random"), SERIAL),
                                                (8, ("w_n^3",), ("ones",), LANES64)], ids=["64", "64-ecntt_mul0", "256-lanes64"])
def test_degenerate_powers_strings(bbg, lg, names, polys, opt):
    n = 1 << lg
    fs = {"ones": [1] * n, "alternating": [1, R - 1] * (n // 2), "random": coefficients(SEED + 830 + lg, n)}
    for name in names:
        x = power_bases(lg)[name]
        a = [pow(x, j, R) for j in range(n)]
        with optional(bbg, opt):
            h = prepared(bbg, bbg.srs_synth_powers(mont([x])[0], n), lg)
            try:
                got = {p: h.open(mont(fs[p])) for p in polys}
            finally:
                h.free()
        for p in polys:
            ks = gd.proof_scalars(fs[p], a)
            if p == "ones" and name in ("-1", "w_n", "w_n^3", "w_n^-1"):
                assert sum(1 for k in ks if k == 0) == n - 2  # all but the proofs at 1 and at x
            check(got[p], fixed(bbg, ks), f"2^{lg}, x = {name}, f = {p}, {opt}")


# 11 ----------------------------------------------------------------------------------------------- one handle, degenerate calls between
@pytest.mark.parametrize("opt", [None, SERIAL], ids=["default", "ecntt_mul0"])
def test_reuse_after_degenerate_calls(bbg, designed_string, opt):
    lg = 6
    n = 1 << lg
    a, pts = designed_string(lg)
    f1 = coefficients(SEED + 840, n)
    f2, _ = gd.design_coeffs(lg, ZERO_AT[lg], SEED + 841)
    with optional(bbg, opt):
        h = prepared(bbg, bbg.srs_register(pts), lg)
        try:
            first = h.open(mont(f1))
            check(first, fixed(bbg, gd.proof_scalars(f1, a)), f"{opt}: a random f")
            check(h.open(mont(f2)), fixed(bbg, gd.proof_scalars(f2, a)), f"{opt}: a designed f behind it")
            check(h.open(mont([0] * n)), infinities(n), f"{opt}: f = 0 behind that")
            check(h.open(mont(f1)), first, f"{opt}: the first f again")
        finally:
            h.free()
