"""bbg_g1_ntt / bbg_g1_ntt_device on the MI355X: the NTT over G1 in both directions on plain arrays of points, points at infinity among
the inputs and the outputs (csrc/ecntt.hip).

Every comparison is bit-exact on canonical Montgomery affine words.  Expected values come from the oracle model
(tests/tools/open_all_model.py g1_ntt: one oracle.msm_naive per output), from bbg_srs_lagrange (reference parity in
tests/test_gpu_lagrange_srs.py) or from identities of the transform.  Oracle transforms are computed once per module and left unchanged.

The three settings every case at 2^6 runs under: the defaults, "ecntt_mul" = 0 (bit-serial stages) and "batch_mul_lanes" = 64, with which
the GLV stage kernel's lane-stride loop goes round more than once from 2^8 on -- so those cases include 2^8.

Designed inputs (section 6, tests/tools/g1_design.py): points [a_j] G whose scalars solve a linear system mod r, so that EVERY stage of the
transform, in both directions, has a butterfly with A = t (the doubling branch of xyzz_add) and one with A = -t (result at infinity) --
from stage 1 on under a twiddle other than 1 and between non-normalised XYZZ operands, in the inverse's last stage behind n^-1, at 2^8
under 64 lanes beyond the first round of the lane-stride loop.  Hashed inputs never give a stage kernel either.  The want is [y_k] G for
the integers y_k of the design's model, made by bbg_g1_fixed_base_mul and held to the oracle; tests/test_g1_design_cpu.py asserts that
the designs meet the coincidences they claim."""
import contextlib
import ctypes

import numpy as np
import pytest

import coarse_inputs as ci
import g1_design as gd
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


# 6 ------------------------------------------------------------------------------------------------ designed discrete logarithms
def mont(vals):
    return ci.to_words([ci.to_mont(v % ci.R_MOD, 0) for v in vals])


@pytest.fixture(scope="module")
def designed(bbg, oracle):
    """(lg, inverse) -> (points [a_j] G, want [y_k] G) of g1_design.design_ntt, both by bbg_g1_fixed_base_mul (another kernel, with an oracle
    parity test of its own), made on first use.  The want is held to the oracle: in full by the model's transform of the points up to
    2^6; at 2^8 by oracle.g1_mul at sixteen indices, the infinite outputs and their butterfly partners among them."""
    made = {}

    def get(lg, inverse):
        if (lg, inverse) not in made:
            n = 1 << lg
            a, y, report = gd.design_ntt(lg, inverse, SEED + 600 + lg)
            assert sorted(report) == list(range(lg)) and all(eq >= 1 and op >= 1 for eq, op, _ in report.values()), report
            pts, want = bbg.g1_fixed_base_mul(mont(a)), bbg.g1_fixed_base_mul(mont(y))
            infinite = [k for k in range(n) if y[k] == 0]
            assert len(infinite) == 2  # the last stage's A = t and A = -t
            for k in range(n):
                assert np.array_equal(want[k], oa.aff_infinity()) == (k in infinite), f"[y_{k}] G: infinity in the wrong place"
            if lg <= 6:
                check(want, oa.g1_ntt(oracle, pts, inverse=inverse), f"2^{lg}, inverse = {inverse}: [y_k] G against the oracle's transform")
            else:
                ks = infinite + [k ^ (n // 2) for k in infinite]
                rng = np.random.default_rng(SEED + 601)
                while len(ks) < 16:
                    k = int(rng.integers(0, n))
                    if k not in ks:
                        ks.append(k)
                G = oracle.g1_generator()
                by_oracle = oa.canon_points(oracle, np.stack([oracle.g1_mul(G, s) for s in mont([y[k] for k in ks])]))
                check(want[ks], by_oracle, f"2^{lg}, inverse = {inverse}: [y_k] G against oracle.g1_mul at {ks}")
            made[(lg, inverse)] = (pts, want)
        return made[(lg, inverse)]
    return get


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("setting,lgs", [("default", (3, 6)), ("ecntt_mul0", (3, 6)), ("lanes64", (3, 6, 8))], ids=["default", "ecntt_mul0", "lanes64"])
def test_designed_coincidences_in_every_stage(bbg, designed, setting, lgs, inverse):
    with settings(bbg, setting):
        for lg in lgs:
            pts, want = designed(lg, inverse)
            what = f"designed 2^{lg}, {setting}, inverse = {inverse}"
            check(bbg.g1_ntt(pts, inverse=inverse), want, f"{what}, host entry")
            check(device_ntt(bbg, pts, inverse=inverse), want, f"{what}, device entry")  # and the input unchanged
            check(device_ntt(bbg, pts, inverse=inverse, in_place=True), want, f"{what}, device entry in place")
            # back again, the two infinite outputs among the inputs as data
            check(bbg.g1_ntt(want, inverse=not inverse), pts, f"{what}, round trip")


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_designed_coincidences_with_lifted_coordinates(bbg, designed, inverse):
    pts, want = designed(6, inverse)
    check(bbg.g1_ntt(lift(pts), inverse=inverse), want, f"designed 2^6, inverse = {inverse}, coordinates in [p, 2p)")
    check(bbg.g1_ntt(lift(want), inverse=not inverse), pts, f"designed 2^6, inverse = {inverse}, round trip from coordinates in [p, 2p)")
