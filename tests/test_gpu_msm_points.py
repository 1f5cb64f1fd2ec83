"""bbg_g1_msm / bbg_g1_msm_device on the MI355X: the table-free MSM over the caller's own points (csrc/msm_points.hip).

Every comparison is bit for bit on the 8 words of the one canonical affine output.  Expected values come by two independent routes:
oracle.msm_naive over up to 2^10 arbitrary points (the hashed string, whose discrete logarithms nobody knows), and the closed form
[sum s_i a_i mod r] G over designed points P_i = [a_i] G made by bbg_g1_fixed_base_mul[_device], which tests/test_gpu_fixed_base.py holds
to the oracle.  The scalar lists and the edges they hold are tests/tools/msm_points_model.py's, proven in tests/test_msm_points_cpu.py; the
sizes around the chunk and the segment come from bbg_g1_msm_plan, never from copied constants.

Time limits: derived, not fitted -- nothing had been measured when they were written, as in tests/test_gpu_var_base.py.  A term costs
2 windows(c) mixed additions, 20 at c = 13, some 200 field products; the largest call here, 2^21 + 1 terms, is 4 * 10^8 products beside
its sort, a kernel time of milliseconds on a chip that sustains 10^11 products a second.  The fixed tail (the reduction and the combine
chain of about 128 doublings on one lane) is a few hundred sequential group operations, below a millisecond.  So every library call
here is far below a second and gets the 5 s allowance the variable-base tests use for calls of that size, first-use allocations and
copies included."""
import contextlib
import ctypes
import time

import numpy as np
import pytest

import coarse_inputs as ci
import fixed_base_model as fb
import lagrange_model as lm
import msm_points_model as mp
import var_base_model as vb
from stream_order import SRS_SEED, env, to_device, unsynchronised, words as snap_words  # noqa: F401 (env: a fixture)

pytestmark = pytest.mark.gpu

R, Q = vb.R_MOD, vb.Q_MOD
S_INT = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % R  # full-width scalars for the long buckets
T_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
WIDTHS = list(range(mp.C_MIN, mp.C_MAX + 1))
EDGE_WIDTHS = [mp.C_MIN, mp.C_MAX, 0]  # the smallest, the largest, automatic
INF = fb.aff_infinity()


@contextlib.contextmanager
def time_limit(seconds, what):
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    print(f"{what}: {dt:.3f} s (limit {seconds:.1f} s)")
    assert dt <= seconds, f"{what} took {dt:.3f} s, limit {seconds:.1f} s"


def mont(vals):
    """Montgomery words of integers in [0, 2r): the representative k of [0, r), or the words of k - r plus r for k in [r, 2r)"""
    vals = list(vals)
    out = ci.to_words([ci.to_mont(v % R, 0) for v in vals])
    high = [i for i, v in enumerate(vals) if v >= R]
    if high:
        out[high] = ci.add_int(out[high], R)
    return out


def closed_form(bbg, value):
    return bbg.g1_fixed_base_mul(mont([value % R]))[0]


def same(got, want, what):
    assert np.array_equal(np.asarray(got), np.asarray(want)), f"{what}: {[hex(int(x)) for x in got]} is not {[hex(int(x)) for x in want]}"


def device_msm(bbg, points, scalars, window_bits=0):
    n = points.shape[0]
    d_p, d_s, d_o = bbg.dev_alloc(max(n, 1) * 64), bbg.dev_alloc(max(n, 1) * 32), bbg.dev_alloc(64)
    try:
        if n:
            bbg.dev_upload(d_p, points)
            bbg.dev_upload(d_s, scalars)
        bbg.g1_msm_device(d_p, d_s, n, d_o, window_bits)
        return bbg.dev_download(d_o, (8,))
    finally:
        for d in (d_p, d_s, d_o):
            bbg.dev_free(d)


def negated(points):
    out = points.copy()
    out[:, 4:] = ci.to_words([Q - y for y in ci.to_ints(points[:, 4:])])
    return out


@pytest.fixture(scope="module")
def warm(bbg):
    """One small call of each kind before anything is timed: code-object load and first-use allocations."""
    bbg.g1_msm(bbg.g1_fixed_base_mul(mont([3, 5])), mont([7, 11]))


@pytest.fixture(scope="module")
def arbitrary(oracle):
    """2^10 points of the hashed string, canonical, computed once and left unchanged"""
    pts = lm.canon_points(oracle, oracle.srs_hashed(SRS_SEED, 1 << 10))
    pts.setflags(write=False)
    return pts


@pytest.fixture(scope="module")
def designed(bbg):
    """300 designed points P_i = [a_i] G and their a_i"""
    rng = np.random.default_rng(vb.SEED + 60)
    a = [1, 2, R - 1] + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(297)]
    pts = bbg.g1_fixed_base_mul(mont(a))
    pts.setflags(write=False)
    return a, pts


def naive(oracle, ks, points):
    if len(ks) == 0:
        return INF
    return lm.canon_points(oracle, oracle.msm_naive(mont([k % R for k in ks]), points).reshape(1, 8))[0]


# 1 ------------------------------------------------------------------------------------------------ sizes at automatic width
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1000])
def test_sizes_at_automatic_width(bbg, oracle, arbitrary, warm, n):
    c = mp.plan(n)[0]
    ks = (mp.designed_scalars(c) * 4)[:n]
    want = naive(oracle, ks, arbitrary[:n])
    with time_limit(5.0, f"n = {n}, automatic width {c}, host and device entry"):
        got = bbg.g1_msm(arbitrary[:n], mont(ks))
        got_dev = device_msm(bbg, arbitrary[:n], mont(ks))
    same(got, want, f"n = {n}, host entry, against oracle.msm_naive")
    same(got_dev, want, f"n = {n}, device entry, against oracle.msm_naive")


# 2 ------------------------------------------------------------------------------------------------ every width, designed scalars
@pytest.mark.parametrize("c", WIDTHS)
def test_every_width_over_its_designed_scalars(bbg, oracle, arbitrary, designed, warm, c):
    ks = mp.designed_scalars(c)
    a, pts = designed
    n = len(ks)
    assert n == 300 and bbg.g1_msm_plan(n, c)[0] == c
    words = mont(ks)
    want_naive = naive(oracle, ks, arbitrary[:n])
    with time_limit(5.0, f"width {c}, two MSMs of 300 terms and one fixed-base product"):
        got_arbitrary = bbg.g1_msm(arbitrary[:n], words, c)
        got_designed = bbg.g1_msm(pts, words, c)
        want_closed = closed_form(bbg, sum(k * x for k, x in zip(ks, a)))
    same(got_arbitrary, want_naive, f"width {c}, arbitrary points, against oracle.msm_naive")
    same(got_designed, want_closed, f"width {c}, designed points, against the closed form")


# 3 ------------------------------------------------------------------------------------------------ degenerate points and scalars
@pytest.mark.parametrize("wb", EDGE_WIDTHS)
def test_degenerate_inputs(bbg, designed, warm, wb):
    a, pts = designed
    n = 200
    ks = mp.designed_scalars(mp.plan(n, wb)[0])[:n]
    words = mont(ks)
    with time_limit(5.0, f"window_bits = {wb}: eight degenerate MSMs of {n} terms"):
        # all points equal, distinct scalars
        got = bbg.g1_msm(np.tile(pts[3], (n, 1)), words, wb)
        same(got, closed_form(bbg, a[3] * sum(ks)), "all points equal")
        # pairs P, -P under the same scalar: infinity in the documented encoding
        pairs = np.empty((n, 8), dtype=np.uint64)
        pairs[0::2], pairs[1::2] = pts[:n // 2], negated(pts[:n // 2])
        pair_ks = [k for k in ks[:n // 2] for _ in (0, 1)]
        same(bbg.g1_msm(pairs, mont(pair_ks), wb), INF, "pairs P, -P")
        # inputs at infinity in several positions, and all infinite
        holes = [0, 1, 63, 64, 65, 100, n - 1]
        with_inf = pts[:n].copy()
        with_inf[holes] = INF
        same(bbg.g1_msm(with_inf, words, wb), closed_form(bbg, sum(k * x for i, (k, x) in enumerate(zip(ks, a)) if i not in holes)), "infinite inputs")
        same(bbg.g1_msm(np.tile(INF, (n, 1)), words, wb), INF, "all inputs infinite")
        # scalars all 0 (both representatives)
        same(bbg.g1_msm(pts[:n], mont([0] * n), wb), INF, "all scalars 0")
        same(bbg.g1_msm(pts[:n], mont([R] * n), wb), INF, "all scalars r")
        # coordinates lifted into [p, 2p), scalars lifted into [r, 2r)
        want = closed_form(bbg, sum(k * x for k, x in zip(ks, a)))
        lifted = pts[:n].copy()
        lifted[0::2, :4] = ci.add_int(lifted[0::2, :4], Q)
        lifted[1::3, 4:] = ci.add_int(lifted[1::3, 4:], Q)
        same(bbg.g1_msm(lifted, words, wb), want, "coordinates in [p, 2p)")
        high = mont([k % R + R for k in ks])
        assert not ci.below(high, R).any() and ci.below(high, 2 * R).all()
        same(bbg.g1_msm(pts[:n], high, wb), want, "scalars in [r, 2r)")


# 4 ------------------------------------------------------------------------------------------------ long buckets
@pytest.mark.parametrize("wb", [0, 14, mp.C_MAX])
def test_long_buckets_are_cut_into_segments(bbg, warm, wb):
    """All scalars equal put every term of a window into ONE bucket: 5 segment_entries + 7 entries, six segments summed apart and merged.
    Automatic width at this size sums a segment with a wave, widths 14 and 16 with a lane (another segment_entries, from the plan)."""
    seg = bbg.g1_msm_plan(0, wb)[3]
    n = 5 * seg + 7
    c, _, chunk, seg_n = bbg.g1_msm_plan(n, wb)
    if seg_n != seg:  # the automatic width moved with n
        n = 5 * seg_n + 7
        assert bbg.g1_msm_plan(n, wb)[3] == seg_n
    assert n <= chunk
    a = [0x1F2E3D4C5B6A7988 + 0x9E3779B97F4A7C15 * i for i in range(n)]
    with time_limit(5.0, f"window_bits = {wb} (width {c}): {n} designed points, two MSMs"):
        pts = bbg.g1_fixed_base_mul(mont(a))
        one = bbg.g1_msm(pts, np.tile(mont([S_INT]), (n, 1)), wb)
        two = bbg.g1_msm(pts, np.tile(mont([S_INT, T_INT]), (n // 2 + 1, 1))[:n], wb)
        want_one = closed_form(bbg, S_INT * sum(a))
        want_two = closed_form(bbg, S_INT * sum(a[0::2]) + T_INT * sum(a[1::2]))
    same(one, want_one, f"{n} equal scalars")
    same(two, want_two, f"{n} scalars of two interleaved values")


# 5, 6 --------------------------------------------------------------------------------------------- chunks and scale
def plain_sums(oracle, mont_words):
    """(sum k_i, sum i k_i) over the plain values k_i of Montgomery words, exact: 16-bit pieces summed in uint64"""
    w = oracle.from_mont(0, mont_words)
    idx = np.arange(w.shape[0], dtype=np.uint64)
    s0 = s1 = 0
    for limb in range(4):
        for piece in range(4):
            v = (w[:, limb] >> np.uint64(16 * piece)) & np.uint64(0xFFFF)
            s0 += int(v.sum()) << (64 * limb + 16 * piece)
            s1 += int((v * idx).sum()) << (64 * limb + 16 * piece)
    return s0, s1


def linear_case(bbg, pkg, oracle, n, wb, what):
    """P_i = [A + i B] G generated on the device, full-width scalars k_i: the result must be [A sum k_i + B sum i k_i] G"""
    A, B = 0x0123456789ABCDEF, 0x00000000FEDCBA98
    assert A + n * B < 1 << 63
    plain = np.zeros((n, 4), dtype=np.uint64)
    plain[:, 0] = np.uint64(A) + np.uint64(B) * np.arange(n, dtype=np.uint64)
    ks = pkg.synthetic_scalars(0xBB254 + 61, n)
    s0, s1 = plain_sums(oracle, ks)
    d_a, d_p, d_s, d_o = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64), bbg.dev_alloc(n * 32), bbg.dev_alloc(64)
    try:
        bbg.dev_upload(d_a, oracle.to_mont(0, plain))
        bbg.dev_upload(d_s, ks)
        with time_limit(5.0, f"{what}: {n} fixed-base products and one MSM"):
            bbg.g1_fixed_base_mul_device(d_a, n, d_p)
            bbg.g1_msm_device(d_p, d_s, n, d_o, wb)
            got = bbg.dev_download(d_o, (8,))
        same(got, closed_form(bbg, A * s0 + B * s1), what)
    finally:
        for d in (d_a, d_p, d_s, d_o):
            bbg.dev_free(d)


def test_plain_sums_helper(oracle, pkg):
    ks = pkg.synthetic_scalars(5, 100)
    vals = ci.to_ints(oracle.from_mont(0, ks))
    assert plain_sums(oracle, ks) == (sum(vals), sum(i * v for i, v in enumerate(vals)))


@pytest.mark.parametrize("which", ["chunk + 3", "2 chunk + 1"])
def test_chunks(bbg, pkg, oracle, warm, which):
    """The automatic width's chunk is 2^20 terms, not above 2^22, so the automatic width it is (the smallest chunk of all belongs to
    width 2, 983040 terms of 128 entries each)."""
    chunk = bbg.g1_msm_plan(1 << 21)[2]
    assert chunk <= 1 << 22
    n = chunk + 3 if which == "chunk + 3" else 2 * chunk + 1
    assert bbg.g1_msm_plan(n)[2] == chunk
    linear_case(bbg, pkg, oracle, n, 0, f"n = {which} = {n}, automatic width")


@pytest.mark.parametrize("lg", [16, 20])
def test_scale(bbg, pkg, oracle, warm, lg):
    linear_case(bbg, pkg, oracle, 1 << lg, 0, f"n = 2^{lg}, automatic width")


# 7 ------------------------------------------------------------------------------------------------ device entry contract
def test_device_entry_contract(bbg, designed, warm):
    a, pts = designed
    n = 300
    ks = mp.designed_scalars(13)
    words = mont(ks)
    want = closed_form(bbg, sum(k * x for k, x in zip(ks, a)))
    guard = np.full(24, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    lib, vp = bbg.lib, ctypes.c_void_p
    d_p, d_s, d_g = bbg.dev_alloc(n * 64), bbg.dev_alloc(n * 32), bbg.dev_alloc(192)
    try:
        bbg.dev_upload(d_p, pts)
        bbg.dev_upload(d_s, words)
        bbg.dev_upload(d_g, guard)
        d_o = d_g + 64
        with time_limit(5.0, "refusals, four device calls, a trim"):
            # every refusal leaves the output untouched
            refused = [
                (vp(d_p), vp(d_s), n, 0, vp(d_p)), (vp(d_p), vp(d_s), n, 0, vp(d_p + 64 * (n - 1))), (vp(d_p), vp(d_s), n, 0, vp(d_p + 32)),  # over the points
                (vp(d_p), vp(d_s), n, 0, vp(d_s)), (vp(d_p), vp(d_s), n, 0, vp(d_s + 32 * (n - 1) - 32)),                                    # over the scalars
                (None, vp(d_s), n, 0, vp(d_o)), (vp(d_p), None, n, 0, vp(d_o)), (vp(d_p), vp(d_s), n, 0, None), (None, None, 0, 0, None),      # null pointers
                (vp(d_p), vp(d_s), n, 1, vp(d_o)), (vp(d_p), vp(d_s), n, mp.C_MAX + 1, vp(d_o)), (vp(d_p), vp(d_s), n, -3, vp(d_o)),          # width out of range
                (vp(d_p), vp(d_s), mp.MAX_N + 1, 0, vp(d_o)),                                                                              # n above the maximum
            ]
            for args in refused:
                assert lib.bbg_g1_msm_device(bbg.ctx, *args) == -1 and lib.bbg_last_error(), f"{args} was not refused"
            assert np.array_equal(bbg.dev_download(d_g, (24,)), guard), "a refused call wrote"
            assert np.array_equal(bbg.dev_download(d_p, (n, 8)), pts) and np.array_equal(bbg.dev_download(d_s, (n, 4)), words)
            # a call: guard words on both sides intact, inputs unchanged
            bbg.g1_msm_device(d_p, d_s, n, d_o)
            after = bbg.dev_download(d_g, (24,))
            same(after[8:16], want, "device entry")
            assert np.array_equal(after[:8], guard[:8]) and np.array_equal(after[16:], guard[16:]), "the call wrote beside its output"
            assert np.array_equal(bbg.dev_download(d_p, (n, 8)), pts) and np.array_equal(bbg.dev_download(d_s, (n, 4)), words), "the call changed an input"
            # the working memory is scratch: reported, trimmed, grown again
            held = bbg.memory_report()["scratch"]
            assert bbg.memory_trim() > 0 and bbg.memory_report()["scratch"] < held
            bbg.dev_upload(d_g, guard)
            bbg.g1_msm_device(d_p, d_s, n, d_o)
            same(bbg.dev_download(d_g, (24,))[8:16], want, "device entry after bbg_memory_trim")
            # two calls back to back, another n and another width, one synchronisation at the end
            d_o2 = bbg.dev_alloc(64)
            try:
                bbg.g1_msm_device(d_p, d_s, n, d_o, 16)
                bbg.g1_msm_device(d_p, d_s, 77, d_o2, 5)
                bbg.sync()
                same(bbg.dev_download(d_o, (8,)), want, "first of two calls")
                same(bbg.dev_download(d_o2, (8,)), closed_form(bbg, sum(k * x for k, x in zip(ks[:77], a[:77]))), "second of two calls")
            finally:
                bbg.dev_free(d_o2)
        # the host entry's refusals
        out = np.zeros(8, dtype=np.uint64)
        for args in ((None, words.ctypes.data, n, 0, out.ctypes.data), (pts.ctypes.data, None, n, 0, out.ctypes.data), (pts.ctypes.data, words.ctypes.data, n, 0, None),
                     (pts.ctypes.data, words.ctypes.data, n, 17, out.ctypes.data), (pts.ctypes.data, words.ctypes.data, mp.MAX_N + 1, 0, out.ctypes.data)):
            assert lib.bbg_g1_msm(bbg.ctx, *args) == -1 and lib.bbg_last_error()
        assert not out.any()
        assert lib.bbg_g1_msm(bbg.ctx, None, None, 0, 0, out.ctypes.data) == 0 and np.array_equal(out, INF), "n = 0 must write infinity"
    finally:
        for d in (d_p, d_s, d_g):
            bbg.dev_free(d)


# 8 ------------------------------------------------------------------------------------------------ stream order
def test_stream_order_on_a_callers_stream(env, oracle):
    """In the manner of tests/test_gpu_stream_order_device.py: the call on a caller's own non-blocking stream, its inputs zeroed on the
    stream right behind it, the result read through a snapshot taken on the stream, one synchronisation of the stream at the end."""
    n = 1000
    arbitrary = lm.canon_points(oracle, env.pts[:n])
    ks = (mp.designed_scalars(mp.plan(n)[0]) * 4)[:n]
    want = naive(oracle, ks, arbitrary)

    def body(inputs, outs):
        env.ctx.g1_msm_device(inputs[0].data_ptr(), inputs[1].data_ptr(), n, outs[0].data_ptr())
        for t in inputs:
            t.zero_()
        return [outs[0].clone()] + [t.clone() for t in inputs]

    snap, zeroed_p, zeroed_s = unsynchronised(env, [to_device(env, np.array(arbitrary[:n])), to_device(env, mont(ks))], [64], body)
    assert not zeroed_p.any() and not zeroed_s.any(), "an input was not overwritten"
    same(snap_words(snap, 8)[0], want, "g1_msm_device, inputs zeroed behind the call")


# 9 ------------------------------------------------------------------------------------------------ the registered MSM
@pytest.mark.parametrize("lg", [12, 14])
def test_agrees_with_the_registered_msm(bbg, pkg, warm, lg):
    n = 1 << lg
    srs = bbg.srs_synth_hashed(0xBB254 + 62, n)
    try:
        pts = srs.read()
        ks = pkg.synthetic_scalars(0xBB254 + 63, n)
        with time_limit(5.0, f"2^{lg}: the registered MSM and the table-free one"):
            want = bbg.g1_normalize(bbg.msm(srs, ks).reshape(1, 12))[0]
            got = bbg.g1_msm(pts, ks)
        same(got, want, f"2^{lg}: bbg_g1_msm against bbg_msm + bbg_g1_normalize")
    finally:
        srs.free()
