"""bbg_g1_batch_mul / bbg_g1_batch_mul_device / bbg_srs_scale_powers and the option "ecntt_mul" on the MI355X (csrc/var_base.hip,
csrc/var_base.hip.h).

Every comparison is bit-exact on canonical Montgomery affine words.  Expected values come from the C oracle (g1_mul), from
bbg_g1_fixed_base_mul / bbg_srs_synth_powers (oracle-tested in tests/test_gpu_fixed_base.py), or from playing the two values of an option
against each other where the issue asks for that.  The scalar list and its branch coverage are tests/tools/var_base_model.py's, proven on
the CPU side (tests/test_var_base_cpu.py).

Time limits: derived, not fitted -- nothing had been measured when they were written.  A windowed multiplication is about 128 doublings +
74 additions, some 2 500 field products; the bit-serial one twice that.  2^16 of them are 1.6 * 10^8 products, a millisecond-scale
kernel on a chip that sustains 10^11 products a second, so every library call here is far below a second and gets the 5 s allowance the
fixed-base tests use for calls of that size (first-use allocations and copies included); 20 s where an SRS of 2^16 points is built, read
back and compared as well."""
import contextlib
import ctypes
import time

import numpy as np
import pytest

import coarse_inputs as ci
import fixed_base_model as fb
import lagrange_model as lm
import var_base_model as vb

pytestmark = pytest.mark.gpu

R = vb.R_MOD
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
Y_INT = 0x3243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C8 % R
S_INT = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % R  # a full-width scalar for the one-scalar form
CHUNK = 4  # points per lane behind one inversion (VB_CH, csrc/var_base.hip)


@contextlib.contextmanager
def time_limit(seconds, what):
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    print(f"{what}: {dt:.3f} s (limit {seconds:.1f} s)")
    assert dt <= seconds, f"{what} took {dt:.3f} s, limit {seconds:.1f} s"


@contextlib.contextmanager
def option(bbg, key, value, default):
    bbg.set_option(key, value)
    try:
        yield
    finally:
        bbg.set_option(key, default)


def mont(vals):
    return ci.to_words([ci.to_mont(v % R, 0) for v in vals])


def device_mul(bbg, points, scalars, one_scalar=False, in_place=False):
    n = points.shape[0]
    d_p, d_s = bbg.dev_alloc(max(n, 1) * 64), bbg.dev_alloc(max(scalars.shape[0], 1) * 32)
    d_o = d_p if in_place else bbg.dev_alloc(max(n, 1) * 64)
    try:
        bbg.dev_upload(d_p, points)
        bbg.dev_upload(d_s, scalars)
        bbg.g1_batch_mul_device(d_p, d_s, n, d_o, one_scalar)
        return bbg.dev_download(d_o, (n, 8))
    finally:
        bbg.dev_free(d_p)
        bbg.dev_free(d_s)
        if not in_place:
            bbg.dev_free(d_o)


@pytest.fixture(scope="module")
def warm(bbg, oracle):
    """One small call of each kind before anything is timed: code-object load and first-use allocations."""
    G = lm.canon_points(oracle, oracle.g1_generator())
    bbg.g1_batch_mul(G, mont([3]))
    s = bbg.srs_synth_powers(mont([X_INT])[0], 3)
    s.scale_powers(mont([Y_INT])[0]).free()
    s.free()


@pytest.fixture(scope="module")
def pairs(oracle):
    """About 300 (point, scalar) pairs and their products by oracle.g1_mul, computed once and left unchanged."""
    names, ks = vb.gpu_scalars()
    words = mont(ks)
    extra = [R, R + 1, 2 * R - 1]  # non-canonical representatives: the Montgomery words of k plus r
    coarse = ci.add_int(mont(extra), R)
    assert ci.below(coarse, 2 * R).all() and not ci.below(coarse, R).any()
    words, ks = np.concatenate([words, coarse]), ks + extra
    G = lm.canon_points(oracle, oracle.g1_generator())[0]
    rng = np.random.default_rng(vb.SEED + 4)
    mult = [2, 3, 15, 16, 17, R - 1, vb.LAMBDA, R - vb.LAMBDA] + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(12)]
    base = [G] + [lm.canon_points(oracle, oracle.g1_mul(G, w))[0] for w in mont(mult)]
    assert len({p.tobytes() for p in base}) == 21
    pool, canon = [], []
    for p in base:
        px, py = p.copy(), p.copy()
        px[:4] = ci.add_int(p[:4].reshape(1, 4), ci.Q_MOD)[0]  # x + p
        py[4:] = ci.add_int(p[4:].reshape(1, 4), ci.Q_MOD)[0]  # y + p
        pool += [p, px, py]
        canon += [p, p, p]
    pool.append(fb.aff_infinity())
    canon.append(None)
    n = len(ks)
    assert 295 <= n <= 305
    # scalar i meets pool entry 7 i mod 64 (7 is coprime to the pool's 64 entries: the edge scalars at the head of the list meet G, coarse
    # and infinite points alike)
    assert len(pool) == 64
    idx = [(7 * i) % 64 for i in range(n)]
    points = np.stack([pool[j] for j in idx])
    want = np.stack([fb.aff_infinity() if canon[j] is None or k % R == 0 else lm.canon_points(oracle, oracle.g1_mul(canon[j], w))[0]
                     for j, w, k in zip(idx, words, ks)])
    return points, words, want


# 1 ------------------------------------------------------------------------------------------------ oracle parity
def test_oracle_parity(bbg, pairs, warm):
    points, words, want = pairs
    got = {}
    with time_limit(5.0, f"batch_mul, {len(words)} pairs, host + device entry, both values of batch_mul_glv"):
        for glv in (1, 0):
            with option(bbg, "batch_mul_glv", glv, 1):
                got[glv, "host"] = bbg.g1_batch_mul(points, words)
                got[glv, "device"] = device_mul(bbg, points, words)
    for key, res in got.items():
        bad = [i for i in range(len(words)) if not np.array_equal(res[i], want[i])]
        assert not bad, f"batch_mul_glv = {key[0]}, {key[1]} entry: pairs {bad[:8]} differ from oracle.g1_mul"
    inf = sum(1 for p in want if np.array_equal(p, fb.aff_infinity()))
    assert inf >= 6  # k = 0, its representative r, and the infinite point of the pool


# 2 ------------------------------------------------------------------------------------------------ launch-shape edges
@pytest.mark.parametrize("lanes,glv", [(1 << 17, 1), (64, 1), (64, 0)])
def test_launch_shape_edges(bbg, pairs, warm, lanes, glv):
    """n around the wave (64 lanes), the inversion chunk (4 points) and the slab (lanes x 4 points; 64 lanes = 256 points, so that a lane
    takes a second and a third chunk -- under both values of batch_mul_glv: the bit-serial kernel walks the chunks with the same stride).
    The largest size also goes through the device entry.  Expected: the parity test's oracle values, cycled."""
    points, words, want = pairs
    m = len(words)
    slab = 64 * CHUNK
    sizes = [1, CHUNK - 1, CHUNK, CHUNK + 1, 63, 64, 65, slab - 1, slab, slab + 1, 2 * slab + 1]
    with option(bbg, "batch_mul_lanes", lanes, 1 << 17), option(bbg, "batch_mul_glv", glv, 1):
        with time_limit(5.0, f"{len(sizes)} small batches, {lanes} lanes, batch_mul_glv = {glv}"):
            for n in sizes:
                sel = [i % m for i in range(n)]
                got = bbg.g1_batch_mul(points[sel], words[sel])
                bad = [i for i in range(n) if not np.array_equal(got[i], want[sel[i]])]
                assert not bad, f"n = {n}, {lanes} lanes, batch_mul_glv = {glv}: outputs {bad[:8]} differ"
            assert np.array_equal(device_mul(bbg, points[sel], words[sel]), got), "device entry differs at the largest size"


# 3 ------------------------------------------------------------------------------------------------ one scalar
def test_one_scalar_over_a_powers_string(bbg, oracle, warm):
    n = 1 << 16
    with time_limit(20.0, "powers string 2^16, one-scalar batch_mul, fixed_base_mul of s x^i"):
        srs = bbg.srs_synth_powers(mont([X_INT])[0], n)
        try:
            pts = srs.read()
        finally:
            srs.free()
        exps, acc = [], S_INT
        for _ in range(n):
            exps.append(acc)
            acc = acc * X_INT % R
        want = bbg.g1_fixed_base_mul(mont(exps))
        got = bbg.g1_batch_mul(pts, mont([S_INT]), one_scalar=True)
        got_dev = device_mul(bbg, pts, mont([S_INT]), one_scalar=True)
        zero = bbg.g1_batch_mul(pts, mont([0]), one_scalar=True)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {n} points differ from [s x^i] G, first at {bad[:8]}"
    assert np.array_equal(got_dev, got)
    assert np.array_equal(zero, np.tile(fb.aff_infinity(), (n, 1))), "s = 0 must give infinity everywhere"
    G = oracle.g1_generator()
    for i in (0, 1, n - 1):
        assert np.array_equal(got[i], lm.canon_points(oracle, oracle.g1_mul(G, mont([exps[i]])[0]))[0])


# 4 ------------------------------------------------------------------------------------------------ scale_powers
def test_srs_scale_powers(bbg, pkg, warm):
    n = (1 << 12) + 3
    x, y = mont([X_INT])[0], mont([Y_INT])[0]
    y_inv = mont([pow(Y_INT, R - 2, R)])[0]
    with time_limit(20.0, "three strings of 2^12 + 3 points and two updates"):
        src = bbg.srs_synth_powers(x, n)
        want = bbg.srs_synth_powers(mont([X_INT * Y_INT % R])[0], n)
        scaled = back = None
        try:
            before = src.read()
            scaled = src.scale_powers(y)
            assert scaled.num_points == n
            got = scaled.read()
            bad = np.flatnonzero((got != want.read()).any(axis=1))
            assert bad.size == 0, f"{bad.size} points differ from the string of x y, first at {bad[:8]}"
            back = scaled.scale_powers(ci.add_int(y_inv.reshape(1, 4), R)[0])  # a coarse representative of 1 / y
            assert np.array_equal(back.read(), before), "scaling by y and by 1 / y does not give the string back"
            assert np.array_equal(src.read(), before), "the source SRS changed"
            # y = 0 in both representatives, null pointers: BBG_E_INVALID, no handle, *out untouched
            live = bbg.memory_report()["live_srs"]
            sentinel = 0x5E17117E1
            for bad_y in (np.zeros(4, dtype=np.uint64), ci.to_words([R])[0]):
                h = ctypes.c_void_p(sentinel)
                assert bbg.lib.bbg_srs_scale_powers(bbg.ctx, src.handle, bad_y.ctypes.data, ctypes.byref(h)) == -1
                assert h.value == sentinel and bbg.lib.bbg_last_error()
                with pytest.raises(pkg.BbgError):
                    src.scale_powers(bad_y)
            h = ctypes.c_void_p(sentinel)
            assert bbg.lib.bbg_srs_scale_powers(bbg.ctx, None, y.ctypes.data, ctypes.byref(h)) == -1 and h.value == sentinel
            assert bbg.lib.bbg_srs_scale_powers(bbg.ctx, src.handle, None, ctypes.byref(h)) == -1 and h.value == sentinel
            assert bbg.lib.bbg_srs_scale_powers(bbg.ctx, src.handle, y.ctypes.data, None) == -1
            assert bbg.memory_report()["live_srs"] == live
            assert np.array_equal(src.read(), before)
        finally:
            for s in (src, want, scaled, back):
                if s is not None:
                    s.free()


# 5 ------------------------------------------------------------------------------------------------ contract
def test_contract(bbg, pairs, warm):
    points, words, want = pairs
    n = len(words)
    # n = 0 is legal and does nothing
    assert bbg.g1_batch_mul(np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)).shape == (0, 8)
    assert bbg.lib.bbg_g1_batch_mul(bbg.ctx, None, None, 0, 0, None) == 0
    assert bbg.lib.bbg_g1_batch_mul_device(bbg.ctx, None, None, 0, 0, None) == 0
    # null pointers with n > 0
    out = np.zeros((n, 8), dtype=np.uint64)
    for args in ((None, words.ctypes.data, n, 0, out.ctypes.data), (points.ctypes.data, None, n, 0, out.ctypes.data),
                 (points.ctypes.data, words.ctypes.data, n, 0, None)):
        assert bbg.lib.bbg_g1_batch_mul(bbg.ctx, *args) == -1 and bbg.lib.bbg_last_error()
    assert bbg.lib.bbg_g1_batch_mul_device(bbg.ctx, None, None, 4, 0, None) == -1
    assert not out.any()
    with time_limit(5.0, "in-place and overlapping device calls, trim, rebuild"):
        # the output may BE the points ...
        assert np.array_equal(device_mul(bbg, points, words, in_place=True), want), "in-place multiplication differs"
        # ... and may not overlap them in any other way
        d_p, d_s = bbg.dev_alloc((n + 1) * 64), bbg.dev_alloc(n * 32)
        try:
            bbg.dev_upload(d_p, np.concatenate([points, points[:1]]))
            bbg.dev_upload(d_s, words)
            for d_o in (d_p + 64, d_p + 64 * (n - 1)):
                rc = bbg.lib.bbg_g1_batch_mul_device(bbg.ctx, ctypes.c_void_p(d_p), ctypes.c_void_p(d_s), n, 0, ctypes.c_void_p(d_o))
                assert rc == -1 and b"overlap" in bbg.lib.bbg_last_error()
            assert np.array_equal(bbg.dev_download(d_p, (n, 8)), points), "a refused call wrote to the points"
            # ... nor the scalars at all: lane t reads scalar 4t + 1 after it has written slot 4t
            d_big = bbg.dev_alloc(n * 96)
            try:
                for d_sc, d_o, one in ((d_big, d_big, 0), (d_big + 64 * n - 32, d_big, 0), (d_big + 32, d_big + 32 * n - 32, 0), (d_big + 64, d_big, 1)):
                    rc = bbg.lib.bbg_g1_batch_mul_device(bbg.ctx, ctypes.c_void_p(d_p), ctypes.c_void_p(d_sc), n, one, ctypes.c_void_p(d_o))
                    assert rc == -1 and b"scalars" in bbg.lib.bbg_last_error()
                # adjacent, not overlapping: scalars right behind the output, and one scalar right in front of it
                bbg.dev_upload(d_big + 64 * n, words)
                bbg.g1_batch_mul_device(d_p, d_big + 64 * n, n, d_big)
                assert np.array_equal(bbg.dev_download(d_big, (n, 8)), want)
            finally:
                bbg.dev_free(d_big)
        finally:
            bbg.dev_free(d_p)
            bbg.dev_free(d_s)
        # the lanes' tables are scratch: reported, trimmed, rebuilt
        lanes = -(-(-(-n // CHUNK)) // 64) * 64
        table_bytes = lanes * 1024
        assert bbg.memory_report()["scratch"] >= table_bytes
        assert bbg.memory_trim() >= table_bytes
        assert bbg.memory_report()["scratch"] < table_bytes
        assert np.array_equal(bbg.g1_batch_mul(points, words), want)
        assert bbg.memory_report()["scratch"] >= table_bytes


# 6 ------------------------------------------------------------------------------------------------ ecntt_mul
def test_lagrange_ecntt_mul_is_bit_identical(bbg, oracle, warm):
    lg = 10
    n = 1 << lg
    G = oracle.g1_generator()
    P = oracle.g1_mul(G, lm.ints_to_mont(oracle, [0x1F2E3D4C5B6A7988])[0])
    Q = oracle.g1_mul(G, lm.ints_to_mont(oracle, [0x0123456789ABCDEF1])[0])
    # M_j = P (j < n - 1), M_(n-1) = Q: the butterflies meet P + P, P - P and infinite operands, every output is finite
    edge = bbg.srs_register(lm.canon_points(oracle, np.stack([P] * (n - 1) + [Q])))
    hashed = bbg.srs_synth_hashed(0xBB254 + 77, n)
    try:
        with time_limit(5.0, "four Lagrange transforms at 2^10"):  # 0.04 s each with the bit-serial stages (tests/test_gpu_lagrange_srs.py)
            for name, srs in (("group-law edges", edge), ("hashed string", hashed)):
                res = []
                for v in (0, 1):
                    with option(bbg, "ecntt_mul", v, 1):
                        lb = srs.lagrange(lg)
                        res.append(lb.read())
                        lb.free()
                assert np.array_equal(res[0], res[1]), f"{name}: ecntt_mul = 1 differs from ecntt_mul = 0"
                assert not (res[0][:, 3] >> np.uint64(63)).any()
    finally:
        edge.free()
        hashed.free()
