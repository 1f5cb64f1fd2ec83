"""bbg_g1_ntt / bbg_g1_ntt_device on the MI355X: the NTT over G1 in both directions on plain arrays of points, points at infinity among
the inputs and the outputs (csrc/ecntt.hip).

Every comparison is bit-exact on canonical Montgomery affine words.  Expected values come from the oracle model
(tests/tools/open_all_model.py g1_ntt: one oracle.msm_naive per output), from bbg_srs_lagrange (reference parity in
tests/test_gpu_lagrange_srs.py) or from identities of the transform.  Oracle transforms are computed once per module and left unchanged.

The three settings every case at 2^6 runs under: the defaults, "ecntt_mul" = 0 (bit-serial stages) and "batch_mul_lanes" = 64, with which
the GLV stage kernel's lane-stride loop goes round more than once from 2^8 on -- so those cases include 2^8."""
import contextlib
import ctypes

import numpy as np
import pytest

import coarse_inputs as ci
import lagrange_model as lm
import open_all_model as oa

pytestmark = pytest.mark.gpu

SEED = 0xBB254 + 0x611
SETTINGS = {"default": {}, "ecntt_mul0": {"ecntt_mul": (0, 1)}, "lanes64": {"batch_mul_lanes": (64, 1 << 17)}}
INF_AT = (0, 5, 6, 31, 63)  # infinite inputs of the 2^6 case: both ends, neighbours, one butterfly partner of another


@contextlib.contextmanager
def settings(bbg, name):
    opts = SETTINGS[name]
    for key, (value, _) in opts.items():
        bbg.set_option(key, value)
    try:
        yield
    finally:
        for key, (_, default) in opts.items():
            bbg.set_option(key, default)


def lift(points):
    """The same points with x lifted into [p, 2p) on even rows and y on odd rows; infinite points stay as they are."""
    out = np.ascontiguousarray(points, dtype=np.uint64).copy()
    for i in range(out.shape[0]):
        if oa.is_infinity(out[i]):
            continue
        c = 0 if i % 2 == 0 else 4
        out[i, c:c + 4] = ci.add_int(out[i, c:c + 4].reshape(1, 4), ci.Q_MOD)[0]
        assert not ci.below(out[i, c:c + 4], ci.Q_MOD).any() and ci.below(out[i, c:c + 4], 2 * ci.Q_MOD).all()
    return out


def infinities(n):
    return np.tile(oa.aff_infinity(), (n, 1))


def device_ntt(bbg, points, inverse=False, in_place=False):
    n = points.shape[0]
    lg = n.bit_length() - 1
    d_p = bbg.dev_alloc(n * 64)
    d_o = d_p if in_place else bbg.dev_alloc(n * 64)
    try:
        bbg.dev_upload(d_p, points)
        bbg.g1_ntt_device(d_p, lg, d_o, inverse)
        out = bbg.dev_download(d_o, (n, 8))
        if not in_place:
            assert np.array_equal(bbg.dev_download(d_p, (n, 8)), points), "the input array was written"
        return out
    finally:
        bbg.dev_free(d_p)
        if not in_place:
            bbg.dev_free(d_o)


@pytest.fixture(scope="module")
def cases(oracle):
    """{name: (input points, forward transform by the oracle)}: hashed points at 2^1, 2^2, 2^3, 2^6; the 2^6 points with infinities at
    INF_AT; eight finite points among 2^8."""
    out = {}
    for lg in (1, 2, 3, 6):
        pts = oa.canon_points(oracle, oracle.srs_hashed(SEED + lg, 1 << lg))
        out[f"hashed{lg}"] = (pts, oa.g1_ntt(oracle, pts))
    holes = out["hashed6"][0].copy()
    holes[list(INF_AT)] = oa.aff_infinity()
    out["holes6"] = (holes, oa.g1_ntt(oracle, holes))
    sparse = infinities(256)
    sparse[[0, 1, 64, 127, 128, 200, 254, 255]] = out["hashed3"][0]
    out["sparse8"] = (sparse, oa.g1_ntt(oracle, sparse))
    return out


def check(got, want, what):
    bad = [k for k in range(want.shape[0]) if not np.array_equal(got[k], want[k])]
    assert not bad, f"{what}: outputs {bad[:8]} differ"


# 1 ------------------------------------------------------------------------------------------------ forward against the oracle
@pytest.mark.parametrize("lg", [1, 2, 3, 6])
def test_forward_against_the_oracle(bbg, cases, lg):
    pts, want = cases[f"hashed{lg}"]
    check(bbg.g1_ntt(pts), want, f"2^{lg}, host entry")
    check(device_ntt(bbg, pts), want, f"2^{lg}, device entry")
    check(bbg.g1_ntt(lift(pts)), want, f"2^{lg}, coordinates in [p, 2p)")


@pytest.mark.parametrize("setting", ["ecntt_mul0", "lanes64"])
def test_forward_against_the_oracle_under_options(bbg, cases, setting):
    with settings(bbg, setting):
        for name in ("hashed6", "holes6", "sparse8"):
            pts, want = cases[name]
            check(bbg.g1_ntt(pts), want, f"{name}, {setting}")
            check(bbg.g1_ntt(lift(pts)), want, f"{name}, {setting}, coordinates in [p, 2p)")


# 2 ------------------------------------------------------------------------------------------------ inverse against bbg_srs_lagrange
@pytest.mark.parametrize("setting,lgs", [("default", (6, 10)), ("ecntt_mul0", (6, 8)), ("lanes64", (6, 8))])
def test_inverse_is_the_lagrange_transform(bbg, setting, lgs):
    with settings(bbg, setting):
        for lg in lgs:
            srs = bbg.srs_synth_hashed(SEED + 100 + lg, 1 << lg)
            try:
                pts = srs.read()
                lb = srs.lagrange(lg)
                want = lb.read()
                lb.free()
            finally:
                srs.free()
            check(bbg.g1_ntt(pts, inverse=True), want, f"2^{lg}, {setting}")
            check(device_ntt(bbg, pts, inverse=True, in_place=True), want, f"2^{lg}, {setting}, device entry in place")


# 3 ------------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize("setting,lgs", [("default", (10, 12)), ("ecntt_mul0", (6,)), ("lanes64", (6, 8))])
def test_round_trips(bbg, oracle, setting, lgs):
    with settings(bbg, setting):
        for lg in lgs:
            n = 1 << lg
            srs = bbg.srs_synth_hashed(SEED + 200 + lg, n)
            try:
                pts = srs.read()
            finally:
                srs.free()
            pts[[1, n // 2, n - 1]] = oa.aff_infinity()
            for first in (False, True):  # inverse o forward, then forward o inverse
                mid = device_ntt(bbg, pts, inverse=first)
                assert not np.array_equal(mid, pts)
                check(device_ntt(bbg, mid, inverse=not first), pts, f"2^{lg}, {setting}, out of place, inverse first = {first}")
                d = bbg.dev_alloc(n * 64)
                try:
                    bbg.dev_upload(d, pts)
                    bbg.g1_ntt_device(d, lg, d, first)
                    bbg.g1_ntt_device(d, lg, d, not first)
                    check(bbg.dev_download(d, (n, 8)), pts, f"2^{lg}, {setting}, in place, inverse first = {first}")
                finally:
                    bbg.dev_free(d)


# 4 ------------------------------------------------------------------------------------------------ infinities
@pytest.mark.parametrize("setting,lgs", [("default", (1, 6)), ("ecntt_mul0", (6,)), ("lanes64", (6, 8))])
def test_infinite_inputs_and_outputs(bbg, oracle, cases, setting, lgs):
    P = cases["hashed3"][0][5]
    with settings(bbg, setting):
        for lg in lgs:
            n = 1 << lg
            # all inputs equal: out[0] = n P, every other output is the point at infinity, written as data
            nP = oa.canon_points(oracle, oracle.g1_mul(P, lm.ints_to_mont(oracle, [n])[0]))[0]
            got = bbg.g1_ntt(np.tile(P, (n, 1)))
            assert np.array_equal(got[0], nP), f"2^{lg}, {setting}: out[0] != n P"
            check(got[1:], infinities(n - 1), f"2^{lg}, {setting}, equal inputs")
            # the inverse of that gives the equal inputs back; the forward transform of P at index 0 alone is P everywhere
            check(bbg.g1_ntt(got, inverse=True), np.tile(P, (n, 1)), f"2^{lg}, {setting}, inverse of (n P, inf, ..)")
            delta = infinities(n)
            delta[0] = P
            check(bbg.g1_ntt(delta), np.tile(P, (n, 1)), f"2^{lg}, {setting}, forward of (P, inf, ..)")
            # nothing but infinity
            for inverse in (False, True):
                check(bbg.g1_ntt(infinities(n), inverse=inverse), infinities(n), f"2^{lg}, {setting}, all-infinite inputs")
        if setting == "default":
            pts, want = cases["holes6"]
            check(bbg.g1_ntt(pts), want, "2^6 with infinite inputs")
            check(device_ntt(bbg, pts, in_place=True), want, "2^6 with infinite inputs, in place")
            pts, want = cases["sparse8"]
            check(bbg.g1_ntt(pts), want, "2^8 with eight finite inputs")


# 5 ------------------------------------------------------------------------------------------------ errors
def test_errors(bbg, pkg, cases):
    pts = cases["hashed3"][0]
    out = np.zeros_like(pts)
    for lg in (0, 29):
        assert bbg.lib.bbg_g1_ntt(bbg.ctx, pts.ctypes.data, lg, 0, out.ctypes.data) == -1 and b"log2n" in bbg.lib.bbg_last_error()
    assert bbg.lib.bbg_g1_ntt(bbg.ctx, None, 3, 0, out.ctypes.data) == -1
    assert bbg.lib.bbg_g1_ntt(bbg.ctx, pts.ctypes.data, 3, 0, None) == -1
    assert not out.any()
    d = bbg.dev_alloc(8 * 64)
    try:
        bbg.dev_upload(d, pts)
        for lg in (0, 29):
            assert bbg.lib.bbg_g1_ntt_device(bbg.ctx, ctypes.c_void_p(d), lg, 1, ctypes.c_void_p(d)) == -1
        assert bbg.lib.bbg_g1_ntt_device(bbg.ctx, None, 3, 0, ctypes.c_void_p(d)) == -1
        assert bbg.lib.bbg_g1_ntt_device(bbg.ctx, ctypes.c_void_p(d), 3, 0, None) == -1
        assert np.array_equal(bbg.dev_download(d, (8, 8)), pts), "a refused call wrote to the points"
    finally:
        bbg.dev_free(d)
    with pytest.raises(ValueError):
        bbg.g1_ntt(pts[:3])
    with pytest.raises(pkg.BbgError):
        bbg.g1_ntt(pts[:1])
    # the working set is scratch: reported, trimmed, grown again
    n = 1 << 10
    srs = bbg.srs_synth_hashed(SEED + 300, n)
    try:
        big = srs.read()
    finally:
        srs.free()
    first = bbg.g1_ntt(big)
    assert bbg.memory_report()["scratch"] >= n * 128
    assert bbg.memory_trim() >= n * 128
    assert np.array_equal(bbg.g1_ntt(big), first)
