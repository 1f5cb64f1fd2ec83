"""bbg_srs_lagrange on the MI355X: the Lagrange-base form of a reference string (an inverse NTT over G1, csrc/ecntt.hip).

Every point comparison is on canonical values below p.  Expected values come from the reference's own transform_srs (the fixture
tests/golden/lagrange_srs.json), from the oracle model of tests/tools/lagrange_model.py, or from identities the transform must satisfy.

Time limits: TIME_LIMIT_S[log2n] bounds one bbg_srs_lagrange call (window tables included) at three times the time measured on an
MI355X, written beside each entry; the call is timed after it returns, so a slow run fails instead of passing unnoticed.  2^20 appears in
two tests only (commit equivalence and closed form), each making the transform once."""
import contextlib
import ctypes
import hashlib
import json
import os
import subprocess
import time

import numpy as np
import pytest

import lagrange_model as lm
from test_lagrange_srs_cpu import edge_family_expected

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRS_SEED = 0xBB254
# seconds allowed = 3 x measured (measured value in the comment); sizes not listed take the next larger entry
TIME_LIMIT_S = {
    6: 3 * 0.023,    # measured 0.023 s at 2^6 (0.007 s at 2^1): launch latency of log2n stages + window tables
    10: 3 * 0.037,   # measured 0.037 s
    12: 3 * 0.044,   # measured 0.044 s (41.6 ms of it in the stages: one wave per butterfly group cannot fill the chip)
    16: 3 * 0.054,   # measured 0.054 s (2^13: 0.045 s, 2^14: 0.047 s, 2^15: 0.050 s)
    18: 3 * 0.108,   # measured 0.108 s
    20: 3 * 0.446,   # measured 0.446 s (stages 424 ms, normalisation 0.7 ms, the rest window tables)
}


@contextlib.contextmanager
def time_limit(lg, what):
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    limit = TIME_LIMIT_S[min(k for k in TIME_LIMIT_S if k >= lg)]
    print(f"{what} 2^{lg}: {dt:.3f} s (limit {limit:.2f} s)")
    assert dt <= limit, f"{what} at 2^{lg} took {dt:.3f} s, limit {limit:.2f} s"


def lagrange(srs, lg):
    with time_limit(lg, "bbg_srs_lagrange"):
        return srs.lagrange(lg)


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "lagrange_srs.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def warm(bbg):
    """One small transform before anything is timed: code-object load and first-use allocations are not the transform's time."""
    s = bbg.srs_synth_hashed(SRS_SEED, 4)
    s.lagrange(2).free()
    s.free()


def affine(oracle, jac):
    return lm.canon_points(oracle, oracle.jac_to_affine(jac))[0]


def sha(points):
    return hashlib.sha256(np.ascontiguousarray(points, dtype=np.uint64).tobytes()).hexdigest()


def is_canonical(oracle, pts):
    return np.array_equal(lm.canon_points(oracle, pts), np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 8))


# 1 ------------------------------------------------------------------------------------------------ reference parity
def test_reference_parity(bbg, oracle, fixture, warm):
    assert fixture["srs"] == "hashed" and fixture["srs_seed"] == SRS_SEED
    srs = bbg.srs_synth_hashed(SRS_SEED, 1 << 12)
    try:
        for lg in range(1, 7):
            lb = lagrange(srs, lg)
            got = lb.read()
            lb.free()
            want = np.frombuffer(bytes.fromhex(fixture["points"][str(lg)]), dtype=np.uint64).reshape(-1, 8)
            assert got.shape == want.shape and is_canonical(oracle, got)
            bad = [k for k in range(1 << lg) if not np.array_equal(got[k], want[k])]
            assert not bad, f"2^{lg}: points {bad[:8]} differ from the reference's transform_srs"
        for lg in (8, 10, 12):
            lb = lagrange(srs, lg)
            got = lb.read()
            lb.free()
            assert is_canonical(oracle, got)
            assert sha(got) == fixture["sha256"][str(lg)], f"2^{lg}: digest differs from the reference's transform_srs"
    finally:
        srs.free()


# 2 ------------------------------------------------------------------------------------------------ commit equivalence
@pytest.mark.parametrize("lg", [8, 13, 14, 18, 20])
def test_commit_equivalence(bbg, oracle, pkg, warm, lg):
    """The reference's own test at scale (lagrange_base.test.cpp): msm(coefficients, monomial) == msm(fft(coefficients), Lagrange)."""
    n = 1 << lg
    mono = bbg.srs_synth_hashed(SRS_SEED + lg, n)
    lb = None
    try:
        lb = lagrange(mono, lg)
        assert lb.num_points == n
        top = np.zeros((n, 4), dtype=np.uint64)
        top[n - 1] = lm.ints_to_mont(oracle, [1])[0]  # X^(n-1)
        for name, coeffs in (("random", pkg.synthetic_scalars(SRS_SEED + 100 + lg, n)), ("X^(n-1)", top)):
            evals = bbg.ntt(coeffs.copy(), pkg.binding.FFT)
            want = affine(oracle, bbg.msm(mono, coeffs))
            got = affine(oracle, bbg.msm(lb, evals))
            assert np.array_equal(got, want), f"2^{lg}, {name} polynomial: commitment from evaluations differs"
        # X^(n-1) commits to M_{n-1} itself
        assert np.array_equal(want, mono.read(n - 1, 1)[0])
    finally:
        if lb is not None:
            lb.free()
        mono.free()


# 3 ------------------------------------------------------------------------------------------------ partition of unity
@pytest.mark.parametrize("lg", [3, 10, 15])
def test_partition_of_unity(bbg, oracle, warm, lg):
    """sum_k L_k = 1: the MSM of all-ones over the Lagrange SRS is M_0."""
    n = 1 << lg
    mono = bbg.srs_synth_hashed(SRS_SEED + 7, n)
    lb = lagrange(mono, lg)
    try:
        ones = np.tile(lm.ints_to_mont(oracle, [1]), (n, 1))
        assert np.array_equal(affine(oracle, bbg.msm(lb, ones)), mono.read(0, 1)[0])
    finally:
        lb.free()
        mono.free()


# 4 ------------------------------------------------------------------------------------------------ closed form
@pytest.mark.parametrize("lg", [16, 20])
def test_closed_form_linear_srs(bbg, oracle, warm, lg):
    """M_j = (a + j s) G has known discrete logs d_j; LB[k] = e_k G with e = iNTT(d) by the oracle's scalar transform."""
    n = 1 << lg
    a, s = 0x1D2C3B4A5F6E7, 0x9E3779B97F4A7C15
    mono = bbg.srs_synth_linear(a, s, n)
    lb = lagrange(mono, lg)
    try:
        d = lm.ints_to_mont(oracle, [a + j * s for j in range(n)])
        e = oracle.canon(0, oracle.ntt(d, 1))  # op 1 = ifft
        rng = np.random.default_rng(SRS_SEED + lg)
        ks = [0, 1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1] + [int(k) for k in rng.integers(0, n, 56)]
        G = oracle.g1_generator()
        for k in ks:
            want = lm.canon_points(oracle, oracle.g1_mul(G, e[k]))[0]
            assert np.array_equal(lb.read(k, 1)[0], want), f"2^{lg}: LB[{k}] != e_k G"
    finally:
        lb.free()
        mono.free()


# 5 ------------------------------------------------------------------------------------------------ group-law edges
@pytest.mark.parametrize("lg", [2, 6, 10])
def test_group_law_edges_finite_outputs(bbg, oracle, warm, lg):
    """M_j = P (j < n-1), M_{n-1} = R: the butterflies meet P + P, P - P and infinite operands, every output is finite."""
    n = 1 << lg
    G = oracle.g1_generator()
    P = oracle.g1_mul(G, lm.ints_to_mont(oracle, [0x1F2E3D4C5B6A7988])[0])
    R = oracle.g1_mul(G, lm.ints_to_mont(oracle, [0x0123456789ABCDEF1])[0])
    pts = lm.canon_points(oracle, np.stack([P] * (n - 1) + [R]))
    mono = bbg.srs_register(pts)
    lb = lagrange(mono, lg)
    try:
        got = lb.read()
        if lg <= 6:
            want = lm.lagrange_srs(oracle, pts, lg)  # the model itself
        else:
            want = edge_family_expected(oracle, P, R, lg, range(n))  # the closed form (checked against the model on the CPU side)
        bad = [k for k in range(n) if not np.array_equal(got[k], want[k])]
        assert not bad, f"2^{lg}: points {bad[:8]} differ"
    finally:
        lb.free()
        mono.free()


# 6 ------------------------------------------------------------------------------------------------ infinite outputs
@pytest.mark.parametrize("family", ["constant", "single_frequency"])
def test_infinite_output_is_an_error(bbg, oracle, pkg, warm, family):
    lg, m = 5, 11
    n = 1 << lg
    G = oracle.g1_generator()
    if family == "constant":  # every LB[k != 0] is the point at infinity
        pts = np.stack([G] * n)
    else:  # M_j = [w^(m j)] G: only LB[m] is finite
        w = lm.root(oracle, lg)
        pts = np.stack([oracle.g1_mul(G, lm.ints_to_mont(oracle, [pow(w, m * j, lm.R_MOD)])[0]) for j in range(n)])
    mono = bbg.srs_register(lm.canon_points(oracle, pts))
    try:
        sentinel = 0x5E17117E1
        out = ctypes.c_void_p(sentinel)
        rc = bbg.lib.bbg_srs_lagrange(bbg.ctx, mono.handle, lg, ctypes.byref(out))
        assert rc != 0
        assert "infinity" in bbg.lib.bbg_last_error().decode()
        assert out.value == sentinel, "*out was written on the error path"
        with pytest.raises(pkg.BbgError, match="infinity"):
            mono.lagrange(lg)
        # the context still computes: an MSM over the same handle against the oracle
        scalars = pkg.synthetic_scalars(SRS_SEED + 66, n)
        assert np.array_equal(affine(oracle, bbg.msm(mono, scalars)), lm.canon_points(oracle, oracle.msm_naive(scalars, mono.read()))[0])
    finally:
        mono.free()


# 7 ------------------------------------------------------------------------------------------------ an ordinary SRS
def test_result_is_an_ordinary_srs(bbg, oracle, pkg, fixture, warm, tmp_path):
    lg = 10
    n = 1 << lg
    mono = bbg.srs_synth_hashed(SRS_SEED, 2 * n)
    with pytest.raises(pkg.BbgError):
        mono.lagrange(lg + 2)  # more points than the source holds
    with pytest.raises(pkg.BbgError):
        mono.lagrange(0)
    with pytest.raises(pkg.BbgError):
        mono.lagrange(29)
    h = ctypes.c_void_p()
    assert bbg.lib.bbg_srs_lagrange(bbg.ctx, None, lg, ctypes.byref(h)) == -1 and bbg.lib.bbg_srs_lagrange(bbg.ctx, mono.handle, lg, None) == -1
    lb = lagrange(mono, lg)
    mono.free()  # the result has its own lifetime
    try:
        pts = lb.read()
        assert lb.num_points == n and sha(pts) == fixture["sha256"][str(lg)]
        assert np.array_equal(lb.read(5, 3), pts[5:8])
        lb.write_transcript(tmp_path)
        back = bbg.srs_load_transcript(str(tmp_path), n)
        try:
            # a transcript's reader supplies point 0 = G itself (srs/io.cpp:137): points 1 .. n-1 are the file's
            assert np.array_equal(back.read()[1:], pts[1:])
        finally:
            back.free()
        scalars = pkg.synthetic_scalars(SRS_SEED + 77, n)
        assert np.array_equal(affine(oracle, bbg.msm(lb, scalars)), lm.canon_points(oracle, oracle.pippenger(scalars, pts))[0])
    finally:
        lb.free()


# 8 ------------------------------------------------------------------------------------------------ drop-in
def test_lagrange_check_binary():
    """oracle/_ref/lagrange_check: barretenberg's own TUs (lagrange_base.cpp among them) + the shim, transform_srs wrapped at link time
    onto bbg_srs_lagrange; the wrapped call (GPU) against the reference's CPU body, and the reference's own commitment test."""
    exe = os.path.join(ROOT, "oracle", "_ref", "lagrange_check")
    if not os.path.exists(exe):
        pytest.skip("prebuilt oracle/_ref/lagrange_check not shipped")
    flags = open("/proc/cpuinfo").read()
    if not all(f in flags for f in (" adx", " bmi2", " avx2")):
        pytest.skip("host CPU lacks the ISA the reference build uses")
    r = subprocess.run(["timeout", "-k", "10", "300", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0 and "lagrange_check PASS" in out, out
