"""bbg_fr_batch_invert_device, bbg_poly_evaluate_lagrange(_device), bbg_kate_opening_lagrange_device and bbg_prover_evaluate_lagrange on the
MI355X (csrc/barycentric.hip, host side in csrc/poly.hip and csrc/prover.hip).

Every comparison is bit-exact on canonical Montgomery words.  Expected values come from the C oracle's coefficient route (inverse NTT, then
Horner), which tests/test_barycentric_cpu.py ties to the formulas, and, GPU against GPU, from the library's own coefficient-form entry
points.  The off-domain points are barycentric_model.Z_INTS, asserted off every domain used here on the CPU side.

Time limits: derived as in tests/test_gpu_var_base.py, not fitted.  The largest call is about 2^16 x (4 + count) field products,
microseconds of arithmetic on a chip that sustains 10^11 products a second, so every library call gets the 5 s allowance those tests use,
first-use allocations and copies included."""
import contextlib
import ctypes
import time

import numpy as np
import pytest

import barycentric_model as bm
import coarse_inputs as ci

pytestmark = pytest.mark.gpu

R = bm.R_MOD
FFT, IFFT = 0, 1
G, E_BLK = bm.G, bm.E_BLK
CALL_LIMIT = 5.0
COUNTS = (1, 5, 32)
QP_W_1, QP_Z, QP_SIGMA_1, QP_Q_M, PP_QUOTIENT = 0, 4, 5, 14, 21  # enum bbg_quotient_poly / bbg_prover_poly (include/bbg.h)
E_INVALID = -1


@contextlib.contextmanager
def time_limit(what, seconds=CALL_LIMIT):
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    print(f"{what}: {dt:.3f} s (limit {seconds:.1f} s)")
    assert dt <= seconds, f"{what} took {dt:.3f} s, limit {seconds:.1f} s"


class Dev:
    """Device buffers of a test, freed together."""

    def __init__(self, bbg):
        self.bbg, self.ptrs = bbg, []

    def alloc(self, nbytes):
        p = self.bbg.dev_alloc(max(nbytes, 32))
        self.ptrs.append(p)
        return p

    def put(self, array):
        p = self.alloc(array.nbytes)
        if array.nbytes:
            self.bbg.dev_upload(p, array)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.bbg.sync()
        for p in self.ptrs:
            self.bbg.dev_free(p)


def shifted_pattern(count):
    return [1 if k % 3 == 1 else 0 for k in range(count)]


def times_root(oracle, z, lg):
    return bm.canon(oracle, oracle.fe_mul(0, np.reshape(z, (1, 4)), oracle.root_of_unity(lg).reshape(1, 4))[0])


@pytest.fixture(scope="module")
def warm(bbg):
    """One small call of each kind before anything is timed: code-object load and first-use allocations."""
    with Dev(bbg) as d:
        a = d.put(bm.mont_words([3, 5, 7, 9]))
        b = d.alloc(4 * 32)
        bbg.fr_batch_invert_device(a, b, 4)
        bbg.poly_evaluate_lagrange_device([a], 2, bm.mont_words([bm.Z_INTS[0]])[0])
        bbg.kate_opening_lagrange_device(a, b, 2, bm.mont_words([bm.Z_INTS[0]])[0])


_POLYS = {}


@pytest.fixture(scope="module")
def polys(pkg, oracle):
    """lg -> (32 value arrays, their coefficient forms by the oracle's inverse NTT), made once per size and left unchanged.  Polynomials 1
    and 4 hold values over the whole input range [0, 2r), polynomial 2 is a second representative throughout where that fits."""
    def get(lg):
        if lg not in _POLYS:
            n = 1 << lg
            vals = [pkg.synthetic_scalars(0xBA70 + 64 * lg + k, n) for k in range(32)]
            vals[1], vals[4] = bm.coarse_poly(0xBA60 + lg, n), bm.coarse_poly(0xBA61 + lg, n)
            vals[2] = ci.add_int(bm.canon(oracle, vals[2]), R)
            for v in vals:
                v.setflags(write=False)
            coeffs = [oracle.ntt(v, IFFT) for v in vals]
            _POLYS[lg] = (vals, coeffs)
        return _POLYS[lg]
    return get


def oracle_evals(oracle, coeffs, lg, z, shifted):
    zw = times_root(oracle, z, lg)
    return np.stack([bm.canon(oracle, oracle.poly_eval(c, zw if s else z)) for c, s in zip(coeffs, shifted)])


# 1 ------------------------------------------------------------------------------------------------ batch inversion
def invert_input(n):
    """Random values with the edge cases of the issue spliced in; returns the words."""
    vals = bm.coarse_poly(0xBA80 + n, n) if n else np.zeros((0, 4), dtype=np.uint64)
    vals = vals.copy()
    zeros = {0, n - 1}
    for b in range(G, n + G, G):  # both sides of every group border
        zeros |= {b - 1, b}
    zeros = sorted(i for i in zeros if 0 <= i < n)
    for k, i in enumerate(zeros):
        vals[i] = ci.to_words([R])[0] if k % 2 else 0  # zero, and r itself as a zero
    taken = set(zeros)
    spare = [i for i in range(min(n, 64)) if i not in taken]
    for i, v in zip(spare, (ci.to_mont(1, 0), ci.to_mont(R - 1, 0), ci.to_mont(1, 0) + R, 1, R - 1, R + 1, 2 * R - 1)):
        vals[i] = ci.to_words([v])[0]
    return vals


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, G - 1, G, G + 1, 256 * G + 1, (1 << 16) + 3])
def test_batch_invert(bbg, oracle, warm, n):
    vals = invert_input(n)
    live = np.array([v % R != 0 for v in ci.to_ints(vals)], dtype=bool)
    assert n < 2 or not live.all()
    want = bm.canon(oracle, oracle.fe_inv(0, vals)) if n else vals
    want[~live] = 0
    for case, data, expect in (("mixed", vals, want), ("all zero", np.zeros_like(vals), np.zeros_like(vals))):
        with Dev(bbg) as d:
            a, b = d.put(data), d.alloc(n * 32)
            with time_limit(f"batch_invert n={n} {case}"):
                bbg.fr_batch_invert_device(a, b, n)      # out of place
                out = bbg.dev_download(b, (n, 4)) if n else data
                bbg.fr_batch_invert_device(a, a, n)      # in place
                inplace = bbg.dev_download(a, (n, 4)) if n else data
            assert np.array_equal(out, expect), f"n={n} {case}: out of place"
            assert np.array_equal(inplace, expect), f"n={n} {case}: in place"


def test_batch_invert_refuses_partial_overlap_and_null(bbg, warm):
    n = G + 5
    data = bm.mont_words(range(1, 2 * n + 1))  # room for both ranges of every refused call
    with Dev(bbg) as d:
        a = d.put(data)
        for off in (32, (n - 2) * 32):          # all but one element shared, and exactly one
            assert bbg.lib.bbg_fr_batch_invert_device(bbg.ctx, ctypes.c_void_p(a), ctypes.c_void_p(a + off), n - 1) == E_INVALID
            assert bbg.lib.bbg_fr_batch_invert_device(bbg.ctx, ctypes.c_void_p(a + off), ctypes.c_void_p(a), n - 1) == E_INVALID
        assert bbg.lib.bbg_fr_batch_invert_device(bbg.ctx, None, ctypes.c_void_p(a), 4) == E_INVALID
        assert bbg.lib.bbg_fr_batch_invert_device(bbg.ctx, ctypes.c_void_p(a), None, 4) == E_INVALID
        assert np.array_equal(bbg.dev_download(a, data.shape), data), "a refused call wrote"


# 2 ------------------------------------------------------------------------------------------------ evaluation
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("lg", bm.SIZES_GPU)
def test_evaluate_against_the_oracle(bbg, oracle, polys, warm, lg, count):
    vals, coeffs = polys(lg)
    zs = bm.mont_words(bm.Z_INTS)  # two random points and z = 0
    with Dev(bbg) as d:
        ptrs = [d.put(v) for v in vals[:count]]
        patterns = [shifted_pattern(count)] + ([None, [1]] if count == 1 else [])
        for sh in patterns:
            flags = sh if sh is not None else [0] * count
            for zi, z in enumerate(zs):
                want = oracle_evals(oracle, coeffs[:count], lg, z, flags)
                with time_limit(f"evaluate_lagrange 2^{lg} x {count}"):
                    got = bbg.poly_evaluate_lagrange_device(ptrs, lg, z, sh)
                assert np.array_equal(got, want), f"2^{lg} count {count} shifted {sh} z#{zi}"
                if zi == 0:  # the other representative of the same point: the same output
                    again = bbg.poly_evaluate_lagrange_device(ptrs, lg, bm.second_representative(z)[0], sh)
                    assert np.array_equal(again, want), f"2^{lg} count {count}: z + r"
    if count == 1:
        with time_limit(f"evaluate_lagrange (host buffer) 2^{lg}"):
            got = bbg.poly_evaluate_lagrange(vals[1], zs[0])
        assert np.array_equal(got, oracle_evals(oracle, coeffs[1:2], lg, zs[0], [0])[0])


@pytest.mark.parametrize("lg", bm.SIZES_GPU)
def test_evaluate_against_the_coefficient_entry_points(bbg, oracle, polys, warm, lg):
    """GPU against GPU: bbg_ntt_device(IFFT) + bbg_poly_evaluate_device at z and at z w."""
    vals, _ = polys(lg)
    n, count = 1 << lg, 32
    z = bm.mont_words(bm.Z_INTS[1:2])[0]
    zw = times_root(oracle, z, lg)
    assert np.array_equal(zw, bm.canon(oracle, oracle.fe_mul(0, z.reshape(1, 4), bbg.fr_root_pow(lg, 1).reshape(1, 4))[0]))
    sh = shifted_pattern(count)
    with Dev(bbg) as d:
        ptrs = [d.put(v) for v in vals]
        got = bbg.poly_evaluate_lagrange_device(ptrs, lg, z, sh)
        work = d.alloc(n * 32)
        for k in range(count):
            bbg.dev_upload(work, vals[k])
            bbg.ntt_device(work, lg, IFFT)
            want = bm.canon(oracle, bbg.poly_evaluate_device(work, n, zw if sh[k] else z))
            assert np.array_equal(got[k], want), f"2^{lg}: polynomial {k}"


@pytest.mark.parametrize("lg", bm.SIZES_GPU)
def test_evaluate_on_the_domain_and_flag_reset(bbg, oracle, polys, warm, lg):
    vals, coeffs = polys(lg)
    n, count = 1 << lg, 5
    canon = [bm.canon(oracle, v) for v in vals[:count]]
    sh = shifted_pattern(count)
    z_off = bm.mont_words(bm.Z_INTS[:1])[0]
    want_off = oracle_evals(oracle, coeffs[:count], lg, z_off, sh)
    last_block = (n - 1) // E_BLK * E_BLK + min(n - 1, 77) % n  # an index inside the last block (the only one up to 2^10)
    with Dev(bbg) as d:
        ptrs = [d.put(v) for v in vals[:count]]
        for j in sorted({0, 1, n - 1, last_block % n}):
            z = bbg.fr_root_pow(lg, j)
            for rep in (z, bm.second_representative(bm.canon(oracle, z))[0]):
                got = bbg.poly_evaluate_lagrange_device(ptrs, lg, rep, sh)
                want = np.stack([canon[k][(j + sh[k]) % n] for k in range(count)])
                assert np.array_equal(got, want), f"2^{lg}: z = w^{j}"
            assert np.array_equal(bbg.poly_evaluate_lagrange_device(ptrs, lg, z_off, sh), want_off), f"2^{lg}: off-domain call after z = w^{j}"


def test_evaluate_refuses_bad_arguments(bbg, warm):
    lib = bbg.lib
    with Dev(bbg) as d:
        a = d.put(bm.mont_words(range(1, 5)))
        arr = (ctypes.c_void_p * 33)(*[ctypes.c_void_p(a)] * 33)
        z = bm.mont_words([7])[0]
        sentinel = np.full((33, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        out = sentinel.copy()
        call = lambda arr_, cnt, lg, zp, op: lib.bbg_poly_evaluate_lagrange_device(bbg.ctx, arr_, None, cnt, lg, zp, op)  # noqa: E731
        assert call(arr, 0, 2, z.ctypes.data, out.ctypes.data) == E_INVALID
        assert call(arr, 33, 2, z.ctypes.data, out.ctypes.data) == E_INVALID
        assert call(arr, 1, 0, z.ctypes.data, out.ctypes.data) == E_INVALID
        assert call(arr, 1, 29, z.ctypes.data, out.ctypes.data) == E_INVALID
        assert call(None, 1, 2, z.ctypes.data, out.ctypes.data) == E_INVALID
        assert call(arr, 1, 2, None, out.ctypes.data) == E_INVALID
        assert call(arr, 1, 2, z.ctypes.data, None) == E_INVALID
        arr[1] = None
        assert call(arr, 2, 2, z.ctypes.data, out.ctypes.data) == E_INVALID
        assert np.array_equal(out, sentinel), "a refused call wrote"
        assert lib.bbg_poly_evaluate_lagrange(bbg.ctx, None, 2, z.ctypes.data, out.ctypes.data) == E_INVALID
        assert lib.bbg_poly_evaluate_lagrange(bbg.ctx, sentinel.ctypes.data, 0, z.ctypes.data, out.ctypes.data) == E_INVALID


# 3 ------------------------------------------------------------------------------------------------ opening
@pytest.mark.parametrize("lg", bm.SIZES_GPU)
def test_opening_against_the_coefficient_entry_point(bbg, oracle, polys, warm, lg):
    vals, coeffs = polys(lg)
    n = 1 << lg
    for k, zi in ((1, 0), (0, 1), (4, 2)):  # coarse values at a random point, plain ones at another, coarse ones at z = 0
        z = bm.mont_words(bm.Z_INTS[zi:zi + 1])[0]
        with Dev(bbg) as d:
            ev, dest, co, ref = d.put(vals[k]), d.alloc(n * 32), d.put(vals[k]), d.alloc(n * 32)
            with time_limit(f"kate_opening_lagrange 2^{lg}"):
                f = bbg.kate_opening_lagrange_device(ev, dest, lg, z)
            w_vals = bbg.dev_download(dest, (n, 4))
            assert ci.below(w_vals, R).all(), "the quotient's values are canonical"
            assert np.array_equal(f, bm.canon(oracle, oracle.poly_eval(coeffs[k], z))), f"2^{lg}: F(z)"
            bbg.ntt_device(dest, lg, IFFT)
            bbg.ntt_device(co, lg, IFFT)
            f_ref = bbg.kate_opening_device(co, ref, n, z)
            got, want = bm.canon(oracle, bbg.dev_download(dest, (n, 4))), bm.canon(oracle, bbg.dev_download(ref, (n, 4)))
            assert not got[n - 1].any() and not want[n - 1].any(), "W has degree n - 2"
            assert np.array_equal(got, want), f"2^{lg}: iNTT of the values of W != the coefficient-form quotient"
            assert np.array_equal(f, bm.canon(oracle, f_ref))
            if lg <= 6:  # and the big-integer model itself, where it is cheap
                mw, mf = bm.opening(vals[k], lg, z)
                assert np.array_equal(w_vals, mw) and np.array_equal(f, mf)


def test_opening_refuses_domain_points_and_overlap(bbg, oracle, polys, warm):
    for lg in (6, bm.LOG_E_BLK + 1):
        vals, _ = polys(lg)
        n = 1 << lg
        pattern = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        f = np.full(4, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        with Dev(bbg) as d:
            ev, dest = d.put(np.concatenate([vals[0], vals[0]])), d.put(pattern)
            call = lambda e, t, zp: bbg.lib.bbg_kate_opening_lagrange_device(bbg.ctx, ctypes.c_void_p(e), ctypes.c_void_p(t), lg, zp, f.ctypes.data)  # noqa: E731
            z3 = bbg.fr_root_pow(lg, 3)
            for z in (z3, bm.second_representative(bm.canon(oracle, z3))[0], bbg.fr_root_pow(lg, 0)):
                assert call(ev, dest, z.ctypes.data) == E_INVALID
                assert b"domain" in bbg.lib.bbg_last_error()
            bbg.sync()
            assert np.array_equal(bbg.dev_download(dest, (n, 4)), pattern), "a refused opening wrote to dest"
            z = bm.mont_words(bm.Z_INTS[:1])[0]
            for t in (ev, ev + 32, ev + (n - 1) * 32):
                assert call(ev + 0, t, z.ctypes.data) == E_INVALID
            assert call(ev + 32, ev, z.ctypes.data) == E_INVALID
            assert call(ev, dest, None) == E_INVALID and call(0, dest, z.ctypes.data) == E_INVALID and call(ev, 0, z.ctypes.data) == E_INVALID
            bbg.sync()
            assert np.array_equal(bbg.dev_download(ev, (2 * n, 4)), np.concatenate([vals[0], vals[0]]))
            assert np.array_equal(f, np.full(4, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)), "a refused call wrote f_out"


# 4 ------------------------------------------------------------------------------------------------ commit equivalence
def test_commit_in_the_lagrange_base_equals_the_monomial_commit(bbg, oracle, polys, warm):
    lg, n = 10, 1 << 10
    vals, coeffs = polys(lg)
    z = bm.mont_words(bm.Z_INTS[:1])[0]
    srs = bbg.srs_synth_powers(bm.mont_words([bm.X_INT])[0], n)
    lag = srs.lagrange(lg)
    try:
        with Dev(bbg) as d:
            ev, dest = d.put(vals[1]), d.alloc(n * 32)
            bbg.kate_opening_lagrange_device(ev, dest, lg, z)
            w_vals = bbg.dev_download(dest, (n, 4))
            bbg.ntt_device(dest, lg, IFFT)
            w_coeffs = bbg.dev_download(dest, (n, 4))
        commits = bbg.g1_normalize(np.stack([bbg.msm(lag, w_vals), bbg.msm(srs, w_coeffs), bbg.msm(lag, vals[1]), bbg.msm(srs, coeffs[1])]))
        assert np.array_equal(commits[0], commits[1]), "commitment to W: Lagrange base != monomial base"
        assert np.array_equal(commits[2], commits[3]), "commitment to F: Lagrange base != monomial base"
        assert not np.array_equal(commits[0], commits[2])
    finally:
        lag.free()
        srs.free()


# 5 ------------------------------------------------------------------------------------------------ resident prover
def make_prover(pkg, bbg, srs, lg, width):
    lib, n = bbg.lib, 1 << lg
    gens = np.stack([bbg.field_op(0, 5, np.array([[k, 0, 0, 0]], dtype=np.uint64))[0] for k in (5, 5, 6, 7)])
    h = ctypes.c_void_p()
    assert lib.bbg_prover_create(bbg.ctx, srs.handle, lg, width, gens.ctypes.data, ctypes.byref(h)) == 0, lib.bbg_last_error()
    for pid in range(5, 20):
        if width == 3 and pid == 8:  # sigma_4
            continue
        assert lib.bbg_prover_set_key_poly(h, pid, 0, pkg.synthetic_scalars(500 + pid, n).ctypes.data) == 0
    assert lib.bbg_prover_finalize_key(h) == 0, lib.bbg_last_error()
    return h


def rounds_1_3_4(pkg, bbg, h, n, width):
    """As tests/test_gpu_parity.py::_prover_rounds_1_to_4: synthetic wires and challenges; the commitments W_i, Z, T_i as canonical affine points."""
    lib = bbg.lib
    wires = [pkg.synthetic_scalars(600 + k, n) for k in range(4)]
    wp = (ctypes.c_void_p * 4)(*[w.ctypes.data for w in wires])
    ch = pkg.synthetic_scalars(700, 8)
    com = np.zeros((2 * width + 1, 12), dtype=np.uint64)
    assert lib.bbg_prover_round1(h, wp, com.ctypes.data) == 0, lib.bbg_last_error()
    assert lib.bbg_prover_round3(h, ch[0].ctypes.data, ch[1].ctypes.data, ch[2:5].ctypes.data, com[width:].ctypes.data) == 0, lib.bbg_last_error()
    assert lib.bbg_prover_round4(h, ch[5].ctypes.data, ch[6].ctypes.data, com[width + 1:].ctypes.data) == 0, lib.bbg_last_error()
    return bbg.g1_normalize(com)


@pytest.mark.parametrize("lg,width", [(10, 4), (6, 3)])
def test_prover_evaluates_its_lagrange_arrays(pkg, bbg, oracle, warm, lg, width):
    lib, n = bbg.lib, 1 << lg
    srs = bbg.srs_synth_hashed(5, n + 1)
    h = make_prover(pkg, bbg, srs, lg, width)
    fresh = make_prover(pkg, bbg, srs, lg, width)
    try:
        zeta = bm.mont_words(bm.Z_INTS[:1])[0]
        ids = [QP_W_1 + k for k in range(width)] + [QP_SIGMA_1 + k for k in range(width)]
        sh = [k % 2 for k in range(len(ids))]
        idv, shv = (ctypes.c_int * len(ids))(*ids), (ctypes.c_int * len(ids))(*sh)
        sentinel = np.full((len(ids), 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        got = sentinel.copy()
        ev = lambda handle, cnt, idp: lib.bbg_prover_evaluate_lagrange(handle, cnt, idp, shv, zeta.ctypes.data, got.ctypes.data)  # noqa: E731
        assert ev(h, len(ids), idv) == E_INVALID and b"round 1" in lib.bbg_last_error()  # before round 1
        first = rounds_1_3_4(pkg, bbg, h, n, width)
        for bad in (QP_Q_M, QP_Z, PP_QUOTIENT, 99, -1) + ((QP_W_1 + 3, QP_SIGMA_1 + 3) if width == 3 else ()):
            assert ev(h, 1, (ctypes.c_int * 1)(bad)) == E_INVALID, bad
        assert lib.bbg_prover_evaluate_lagrange(h, 0, idv, shv, zeta.ctypes.data, got.ctypes.data) == E_INVALID
        assert lib.bbg_prover_evaluate_lagrange(h, 33, idv, shv, zeta.ctypes.data, got.ctypes.data) == E_INVALID
        assert lib.bbg_prover_evaluate_lagrange(h, 1, None, shv, zeta.ctypes.data, got.ctypes.data) == E_INVALID
        assert np.array_equal(got, sentinel), "a refused call wrote"
        with time_limit(f"prover_evaluate_lagrange 2^{lg} width {width}"):
            assert ev(h, len(ids), idv) == 0, lib.bbg_last_error()
        want = np.zeros_like(got)
        assert lib.bbg_prover_evaluate(h, len(ids), idv, shv, zeta.ctypes.data, want.ctypes.data) == 0, lib.bbg_last_error()
        assert np.array_equal(got, bm.canon(oracle, want)), "Lagrange-form evaluations differ from the coefficient-form ones"
        assert ci.below(got, R).all()
        # also exactly at a domain point: the stored values
        j = 5
        zj = bbg.fr_root_pow(lg, j)
        assert lib.bbg_prover_evaluate_lagrange(h, len(ids), idv, None, zj.ctypes.data, got.ctypes.data) == 0
        row = np.zeros((n, 4), dtype=np.uint64)
        for k, pid in enumerate(ids):
            assert lib.bbg_prover_read_poly(h, pid, 1, row.ctypes.data, n) == 0
            assert np.array_equal(got[k], bm.canon(oracle, row[j]))
        # nothing was disturbed: the proof goes on, and a second proof on the handle equals a fresh handle's
        second = rounds_1_3_4(pkg, bbg, h, n, width)
        other = rounds_1_3_4(pkg, bbg, fresh, n, width)
        assert np.array_equal(first, other) and np.array_equal(second, other)
    finally:
        lib.bbg_prover_destroy(h)
        lib.bbg_prover_destroy(fresh)
        srs.free()


def test_scratch_is_accounted_and_trimmed(pkg, warm):
    """The partial sums live in the evaluation scratch: counted under `scratch`, released by bbg_memory_trim, no growth on a repeat."""
    ctx = pkg.Bbg(0)
    try:
        lg, n = 11, 1 << 11
        vals = pkg.synthetic_scalars(0xBA90, n)
        z = bm.mont_words(bm.Z_INTS[:1])[0]
        a = ctx.dev_alloc(n * 32)
        ctx.dev_upload(a, vals)
        before = ctx.memory_report()["scratch"]
        first = ctx.poly_evaluate_lagrange_device([a] * 32, lg, z)
        grown = ctx.memory_report()["scratch"]
        assert grown > before
        ctx.profile_enable(True)
        again = ctx.poly_evaluate_lagrange_device([a] * 32, lg, z)
        ctx.fr_batch_invert_device(a, a, n)
        ctx.sync()
        assert ctx.profile_get("barycentric")[1] == 1 and ctx.profile_get("fr_batch_invert")[1] == 1
        ctx.profile_enable(False)
        assert ctx.memory_report()["scratch"] == grown and np.array_equal(first, again)
        assert len({r.tobytes() for r in first}) == 1
        ctx.dev_free(a)
        ctx.memory_trim()
        assert ctx.memory_report()["scratch"] == 0
    finally:
        ctx.close()
