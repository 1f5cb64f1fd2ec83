"""CPU tests of tests/tools/msm_closed_forms.py and tests/tools/msm_options.py, which tests/test_gpu_msm_scale.py relies on: every closed
form equals oracle.msm_naive (the complete group law, term by term) at small n and rejects the near misses a broken kernel would make; the
launch-shape restatement agrees with bbg_msm_plan's recorded answers and pins the cases the GPU module documents; the options' defaults
table matches the library's initialisers."""
import os
import re

import numpy as np
import pytest

import msm_closed_forms as cf
import msm_options as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bases(oracle):
    return {lg: oracle.srs_hashed(0xC105ED + lg, 1 << lg) for lg in (10, 11, 12)}


def _same(oracle, got, want):
    """got: closed form (affine or None); want: oracle affine output."""
    if cf.is_inf(want):
        return got is None
    return got is not None and np.array_equal(got, want)


@pytest.mark.parametrize("lg", [10, 11, 12])
def test_closed_forms_equal_the_naive_msm(oracle, pkg, bases, lg):
    for fam in cf.FAMILIES:
        pts = cf.srs_points(oracle, cf.SRS_KIND[fam], bases[lg])
        case = cf.family_case(oracle, pkg, fam, pts, bases[lg], seed=700 + lg)
        assert case.scalars.shape == (1 << lg, 4) and case.scalars.dtype == np.uint64, fam
        assert _same(oracle, case.want, oracle.msm_naive(case.scalars, pts)), (fam, lg)
        if fam == "B_cancel":
            assert case.want is None
        else:
            assert case.want is not None, fam


def test_closed_forms_reject_near_misses(oracle, pkg, bases):
    """The result of an MSM that lost a term, misread a scalar, took a pair's sign wrong or counted a doubled point once differs from
    every family's closed form."""
    base = bases[11]
    n = base.shape[0]
    one = cf.mont_words([1])[0]
    for fam in cf.FAMILIES:
        pts = cf.srs_points(oracle, cf.SRS_KIND[fam], base)
        case = cf.family_case(oracle, pkg, fam, pts, base, seed=811)
        sc = case.scalars
        nz = np.flatnonzero(sc.any(axis=1) & ((pts[:, 3] >> np.uint64(63)) == 0))
        i = int(nz[len(nz) // 2])
        misses = {}
        keep = np.ones(n, dtype=bool)
        keep[i] = False
        misses["term dropped"] = (sc[keep], pts[keep])
        changed = sc.copy()
        changed[i] = oracle.fe_add(0, sc[i:i + 1], one.reshape(1, 4))[0]
        misses["scalar changed"] = (changed, pts)
        if cf.SRS_KIND[fam] == "pairs":
            flipped = pts.copy()
            flipped[i ^ 1] = pts[i & ~1]  # the pair's -P read as P
            misses["pair sign flipped"] = (sc, flipped)
        if cf.SRS_KIND[fam] in ("twice", "equal"):
            once = sc.copy()
            once[i ^ 1] = 0  # the second copy of a doubled point not counted
            misses["doubled point counted once"] = (once, pts)
        for what, (s_, p_) in misses.items():
            assert not _same(oracle, case.want, oracle.msm_naive(s_, p_)), (fam, what)


def test_mont_sum_and_digit_edges():
    vals = [0, 1, 5, cf.R_MOD - 1, 1 << 200]
    assert cf.mont_sum(cf.mont_words(vals)) == sum(vals) % cf.R_MOD
    many = cf.mont_words([cf.R_MOD - 1]) .repeat(1 << 22, axis=0)  # 2^22 words near 2^254: the sum must not wrap
    assert cf.mont_sum(many) == ((cf.R_MOD - 1) << 22) % cf.R_MOD
    ks, words = cf.digit_edge_scalars()
    assert len(ks) == words.shape[0] and len(ks) > 100
    assert [cf.plain(w) for w in words] == [k % cf.R_MOD for k in ks]


def test_window_restatement_matches_the_plan():
    """msm_auto_window and the window count agree with the bbg_msm_plan answers test_msm_batch_error_paths_and_plan asserts."""
    plan = {1 << 12: (8, 32), 1 << 13: (8, 32), 1 << 14: (13, 20), 1 << 18: (16, 16), 1 << 20: (19, 14), 1 << 21: (20, 13), 1 << 24: (22, 12)}
    for n, (c, w) in plan.items():
        assert (cf.msm_auto_window(n), cf.msm_windows(cf.msm_auto_window(n))) == (c, w), n
    assert cf.msm_windows(17) == 15 and cf.msm_auto_window(1 << 22) == 20


def test_scale_cases_as_documented():
    """The (n, msm_acc_waves) cases of tests/test_gpu_msm_scale.py reach what their table says: seg <= 8, seg above the accumulation
    queue's 64 slots, and both one-lane combine kernels at one n."""
    for (lg, waves), (seg, combine) in cf.SCALE_CASES.items():
        s = cf.msm_shape(1 << lg, waves=waves)
        assert (s["seg"], s["combine"]) == (seg, combine), (lg, waves, s)
    assert cf.msm_shape(1 << 16)["seg"] == 8 and cf.msm_shape(1 << 16)["combine"] == "k_combine_lanes"
    assert cf.msm_shape(1 << 22)["count"] == "k_sortA_count<STRIDE>" and cf.msm_shape(1 << 20)["count"] == "k_sortA_count"
    for lg in (18, 20):
        kernels = {cf.SCALE_CASES[k][1] for k in cf.SCALE_CASES if k[0] == lg}
        assert kernels == {"k_combine", "k_combine_lanes"}, lg
    assert min(v[0] for v in cf.SCALE_CASES.values()) <= 8 and max(v[0] for v in cf.SCALE_CASES.values()) > 64


def test_option_defaults_match_the_library():
    """msm_options.DEFAULTS against the initialisers of struct bbg_ctx (bbg_internal.h)."""
    with open(os.path.join(ROOT, "aztec-2.0_amd", "csrc", "bbg_internal.h")) as f:
        text = f.read()
    for key, (field, value) in mo.DEFAULTS.items():
        m = re.search(r"^\s*(?:bool|int)\s+" + field + r"\s*=\s*(true|false|-?\d+)\s*;", text, re.M)
        assert m, field
        lib = {"true": 1, "false": 0}.get(m.group(1))
        assert (int(m.group(1)) if lib is None else lib) == value, (key, field, m.group(1))
    with open(os.path.join(ROOT, "aztec-2.0_amd", "csrc", "bbg_capi.hip")) as f:
        capi = f.read()
    for key in mo.DEFAULTS:
        assert f'"{key}"' in capi, key


def test_msm_options_sets_and_restores():
    class Ctx:
        def __init__(self):
            self.calls = []

        def set_option(self, k, v):
            self.calls.append((k, v))

    ctx = Ctx()
    with pytest.raises(RuntimeError):
        with mo.msm_options(ctx, msm_reduce_quad=15, msm_acc_waves=3):
            assert ("msm_reduce_quad", 15) in ctx.calls and ("msm_acc_waves", 3) in ctx.calls
            assert ("msm_window", 0) in ctx.calls and not any(k == "msm_reduce_priority" for k, _ in ctx.calls)
            ctx.calls.clear()
            raise RuntimeError
    assert sorted(ctx.calls) == sorted((k, mo.default(k)) for k in mo.DEFAULTS if k != "msm_reduce_priority")
    with pytest.raises(AssertionError):
        with mo.msm_options(ctx, msm_reduce_quadd=15):
            pass
