"""k_accumulate29 after its mixed addition moved P, R and X3 into the products before them (csrc/curve29.hip.h): MSMs at 2^16, 2^20 and
2^22 terms under the library defaults and with msm_acc_waves 1 and 8 (other lane segments: other run lengths and drain patterns), each
against the oracle or a closed form of tests/tools/msm_closed_forms.py.

Inputs, beside random scalars over hashed points:
  * all-negative digits: 64 scalar classes whose every digit below the top window is negative (random in [-(2^(w-1) - 1), -1]; the top
    digit must be >= 0), by residue class of the index -- every addition of every run takes the p - y path;
  * P / -P pairs with equal scalars (all cancel) and with every other pair equal (families B_cancel, B_mixed): runs that meet
    P = -acc end with ZZ = 0 (mod p) and go through k_redo;
  * y next to p: the 32 hashed points whose stored y word (y * 2^256 mod p, what the kernel splits into limbs) is largest and the 32 whose
    word is smallest (p - y next to p under a negative digit), repeated over the whole point array -- 2^-16 .. 2^-20 below p is what a search
    over the hashed points reaches -- against all-negative and random scalar classes.
At 2^16 the default path is the four-lane kernel, so every case there also runs with msm_accumulate_quad 0, which is k_accumulate29."""
import numpy as np
import pytest
import torch

import coarse_inputs as ci
import msm_closed_forms as cf
from msm_options import msm_options

pytestmark = pytest.mark.gpu

SEED = 0xACC29
CLASSES = 64
SIZES = (16, 20, 22)


def _configs(lg):
    out = [("defaults", {}), ("acc_waves_1", {"msm_acc_waves": 1}), ("acc_waves_8", {"msm_acc_waves": 8})]
    if lg <= 16:
        out += [(name + "_one_lane", dict(opts, msm_accumulate_quad=0)) for name, opts in list(out)]
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).reshape(-1).copy()).cuda()


def _run_and_check(oracle, bbg, srs, scalars, want, lg, what):
    n = 1 << lg
    d = _dev(scalars)
    out = torch.zeros(12, dtype=torch.int64, device="cuda")
    for name, opts in _configs(lg):
        with msm_options(bbg, **opts):
            bbg.msm_device(srs, d.data_ptr(), n, out.data_ptr())
            jac = out.cpu().numpy().view(np.uint64).reshape(12).copy()
        ci.assert_coarse_jacobian(jac, str((what, lg, name)))
        got = None if int(jac[3]) >> 63 else oracle.jac_to_affine(jac)
        if want is None:
            assert got is None, (what, lg, name)
        else:
            assert got is not None and np.array_equal(got, want), (what, lg, name)


def _negative_digit_values(c, count, seed):
    """Plain scalars whose recoded digits are all negative below the top window (top digit 1)."""
    L = ci.MsmLayout(c)
    rng = np.random.default_rng(seed)
    vals = []
    for _ in range(count):
        digits = [-int(rng.integers(1, 1 << (L.width(w) - 1))) for w in range(L.windows - 1)] + [1]
        k = ci.digits_value(digits, c)
        assert 0 < k < ci.R_MOD and ci.recode_digits(k, c)[0] == digits
        vals.append(k)
    return vals


class Inputs:
    def __init__(self, bbg, oracle):
        self.bbg, self.oracle = bbg, oracle
        self.srs, self.base = {}, {}

    def hashed(self, lg):
        if (lg, "hashed") not in self.srs:
            s = self.bbg.srs_synth_hashed(SEED + lg, 1 << lg)
            self.srs[lg, "hashed"] = s
            self.base[lg] = s.read()
        return self.srs[lg, "hashed"]

    def get(self, lg, kind):
        self.hashed(lg)
        if (lg, kind) not in self.srs:
            base = self.base[lg]
            if kind == "y_edges":
                order = np.lexsort((base[:, 4], base[:, 5], base[:, 6], base[:, 7]))  # by the stored y word
                pick = np.concatenate([order[:32], order[-32:]])
                pts = base[pick][np.arange(base.shape[0]) % 64]
            else:
                pts = cf.srs_points(self.oracle, kind, base)
            self.srs[lg, kind] = self.bbg.srs_register(pts)
        return self.srs[lg, kind]

    def free(self):
        for s in self.srs.values():
            s.free()


@pytest.fixture(scope="module")
def inputs(bbg, oracle):
    s = Inputs(bbg, oracle)
    yield s
    s.free()


@pytest.mark.parametrize("lg", SIZES)
def test_random_scalars_against_the_oracle(oracle, pkg, bbg, inputs, lg):
    n = 1 << lg
    srs = inputs.hashed(lg)
    if lg <= 20:
        sc = pkg.synthetic_scalars(SEED + 3 * lg, n)
        want = cf.as_result(oracle.pippenger(sc, inputs.base[lg]))
    else:  # one pippenger at 2^22 costs more than the rest of the module: 2^12 random scalars at random indices (family F) and 3 classes (E)
        case = cf.family_case(oracle, pkg, "E", inputs.base[lg], inputs.base[lg], seed=SEED + lg)
        _run_and_check(oracle, bbg, srs, case.scalars, case.want, lg, "E")
        case = cf.family_case(oracle, pkg, "F", inputs.base[lg], inputs.base[lg], seed=SEED + lg)
        sc, want = case.scalars, case.want
    _run_and_check(oracle, bbg, srs, sc, want, lg, "random")


@pytest.mark.parametrize("lg", SIZES)
def test_all_negative_digits(oracle, bbg, inputs, lg):
    n = 1 << lg
    c = cf.msm_auto_window(n)
    vals = _negative_digit_values(c, CLASSES, SEED + lg)
    cls = np.arange(n) % CLASSES
    srs = inputs.hashed(lg)
    want = cf.class_form(oracle, inputs.base[lg], vals, cls)
    _run_and_check(oracle, bbg, srs, cf.mont_words(vals)[cls], want, lg, "all-negative digits")


# (B_mixed's expectation is a pippenger over n / 2 points: at 2^22 B_cancel alone covers k_redo)
@pytest.mark.parametrize("lg,fam", [(16, "B_cancel"), (16, "B_mixed"), (20, "B_cancel"), (20, "B_mixed"), (22, "B_cancel")])
def test_opposite_pairs_through_redo(oracle, pkg, bbg, inputs, lg, fam):
    srs = inputs.get(lg, "pairs")
    pts = srs.read()
    case = cf.family_case(oracle, pkg, fam, pts, inputs.base[lg], seed=SEED + 5 * lg)
    _run_and_check(oracle, bbg, srs, case.scalars, case.want, lg, fam)


@pytest.mark.parametrize("lg", SIZES)
def test_y_next_to_p(oracle, pkg, bbg, inputs, lg):
    n = 1 << lg
    c = cf.msm_auto_window(n)
    srs = inputs.get(lg, "y_edges")
    pts = srs.read()
    ys = ci.to_ints(pts[:64, 4:8])
    assert max(ys) > ci.Q_MOD - (ci.Q_MOD >> (lg - 6)) and min(ys) < (ci.Q_MOD >> (lg - 6))
    # 64 distinct points x 65 scalar classes: every point meets every class (65 is coprime to 64); half the classes all-negative
    vals = _negative_digit_values(c, 33, SEED + 7 * lg)
    vals += [cf.plain(w) for w in pkg.synthetic_scalars(SEED + 9 * lg, 32)]
    cls = np.arange(n) % 65
    want = cf.class_form(oracle, pts, vals, cls)
    _run_and_check(oracle, bbg, srs, cf.mont_words(vals)[cls], want, lg, "y next to p")
