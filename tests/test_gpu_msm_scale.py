"""Large MSMs on degenerate and skewed inputs, at the sizes where the bucket MSM changes shape.

Above 2^16 terms the accumulation's lane segments grow (seg 16 at 2^18, 56 at 2^20, 70 at 2^22: longer than the 64 slots of
k_accumulate29's parked-run queue), the one-lane combine switches from k_combine_lanes to k_combine, the second sort level takes 1024-thread
blocks and above 2^21 the counting pass strides.  The special cases of the accumulation -- runs that meet P = +-acc and end up in k_redo,
buckets that hold every entry of a window and go to k_combine_long, windows left empty by short scalars -- were only tested at n <= 2^16.

Every input family of tests/tools/msm_closed_forms.py runs at 2^18 and 2^20 (those whose expectation costs at most one pippenger also at 2^22) under the library defaults,
msm_reduce_quad 15, the 32-bit-limb accumulation, the asynchronous reduce with shapes changing between calls and msm_acc_waves values that
move seg and the combine kernel (msm_closed_forms.SCALE_CASES); every result equals the family's closed form.  Also: a batch of four
sets over one SRS with all-equal, P / -P and hashed regions through msm_batch and msm_batch_device, summed by g1_sum_device; and
msm_reduce_priority 0 on a fresh context.  Options are set through tests/tools/msm_options.py and always restored to the library defaults.
"""
import numpy as np
import pytest
import torch

import coarse_inputs as ci
import msm_closed_forms as cf
from msm_options import msm_options

pytestmark = pytest.mark.gpu

FAMILIES = {18: cf.FAMILIES, 20: cf.FAMILIES, 22: ("A", "AD", "D", "E", "F", "G8", "H", "I")}
SEED = 0x5CA1E


def _configs(lg):
    """(name, options) of one (family, size) case."""
    out = [("defaults", {}), ("reduce_quad_15", {"msm_reduce_quad": 15}), ("limbs32", {"msm_limbs29": 0})]
    out += [(f"acc_waves_{w}", {"msm_acc_waves": w}) for (l, w) in cf.SCALE_CASES if l == lg and w]
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).reshape(-1).copy()).cuda()


def _read(out, k=1):
    return out.cpu().numpy().view(np.uint64).reshape(k, 12).copy()


def _check(oracle, jac, want, what):
    ci.assert_coarse_jacobian(jac, str(what))
    got = None if int(jac[3]) >> 63 else oracle.jac_to_affine(jac)
    if want is None:
        assert got is None, what
    else:
        assert got is not None and np.array_equal(got, want), what


class Scale:
    """SRSs per (size, kind) and cases per (size, family), made on first use and kept for the module."""

    def __init__(self, bbg, oracle, pkg):
        self.bbg, self.oracle, self.pkg = bbg, oracle, pkg
        self.srs, self.base, self.cases = {}, {}, {}

    def get_srs(self, lg, kind):
        if (lg, "hashed") not in self.srs:
            s = self.bbg.srs_synth_hashed(SEED + lg, 1 << lg)
            self.srs[lg, "hashed"] = s
            self.base[lg] = s.read()
        if (lg, kind) not in self.srs:
            self.srs[lg, kind] = self.bbg.srs_register(cf.srs_points(self.oracle, kind, self.base[lg]))
        s = self.srs[lg, kind]
        n = 1 << lg
        assert s.num_points == n and self.bbg.msm_plan(n, s) == (cf.msm_auto_window(n), cf.msm_windows(cf.msm_auto_window(n)))
        return s

    def get_case(self, lg, fam):
        if (lg, fam) not in self.cases:
            kind = cf.SRS_KIND[fam]
            srs = self.get_srs(lg, kind)
            pts = self.base[lg] if kind == "hashed" else srs.read()
            case = cf.family_case(self.oracle, self.pkg, fam, pts, self.base[lg], seed=SEED + 17 * lg + cf.FAMILIES.index(fam))
            self.cases[lg, fam] = (srs, case, _dev(case.scalars))
        return self.cases[lg, fam]

    def free(self):
        for s in self.srs.values():
            s.free()


@pytest.fixture(scope="module")
def scale(bbg, oracle, pkg):
    s = Scale(bbg, oracle, pkg)
    yield s
    s.free()


@pytest.mark.parametrize("lg,fam", [(lg, f) for lg, fams in FAMILIES.items() for f in fams])
def test_msm_family_at_scale(oracle, bbg, scale, lg, fam):
    n = 1 << lg
    srs, case, d = scale.get_case(lg, fam)
    out = torch.zeros(3 * 12, dtype=torch.int64, device="cuda")
    for name, opts in _configs(lg):
        shape = cf.msm_shape(n, waves=opts.get("msm_acc_waves", 0))
        with msm_options(bbg, **opts):
            bbg.msm_device(srs, d.data_ptr(), n, out.data_ptr())
            _check(oracle, _read(out[:12])[0], case.want, (fam, lg, name, shape["seg"], shape["combine"]))
    # asynchronous reduce phases with the layout changing between calls: n terms, n / 2 + 1 terms (another width), n terms again
    half = n // 2 + 1
    with msm_options(bbg):
        bbg.msm_device(srs, d.data_ptr(), half, out.data_ptr() + 96)
        want_half = _read(out[12:24])[0]
        ci.assert_coarse_jacobian(want_half)
    out.zero_()
    with msm_options(bbg, msm_async_reduce=1):
        bbg.msm_device(srs, d.data_ptr(), n, out.data_ptr())
        bbg.msm_device(srs, d.data_ptr(), half, out.data_ptr() + 96)
        bbg.msm_device(srs, d.data_ptr(), n, out.data_ptr() + 192)
        bbg.join()
        bbg.sync()
        got = _read(out, 3)
    _check(oracle, got[0], case.want, (fam, lg, "async", 0))
    _check(oracle, got[2], case.want, (fam, lg, "async", 2))
    _check(oracle, got[1], None if int(want_half[3]) >> 63 else oracle.jac_to_affine(want_half), (fam, lg, "async half"))


def _regions_srs(oracle, base):
    """n points: [0, n/4) all equal to base[0], [n/4, n/2) P / -P pairs, [n/2, n) hashed."""
    n = base.shape[0]
    q = n // 4
    pts = np.array(base, copy=True)
    pts[:q] = base[0]
    pts[q:2 * q] = cf.srs_points(oracle, "pairs", base[q:2 * q])
    return pts


def _batch_sets(oracle, pkg, pts):
    """[(scalars, from)] of the four sets over _regions_srs points, and their expectations."""
    n = pts.shape[0]
    q = n // 4
    s0 = pkg.synthetic_scalars(SEED + 1, n - 1)
    s0[q:2 * q - 1:4] = s0[q - 1:2 * q - 2:4]  # pair region (points q .. 2q - 1 = scalars q - 1 .. 2q - 2): every other pair cancels
    s1 = np.repeat(pkg.synthetic_scalars(SEED + 2, 1), n, axis=0)
    f2 = 4097
    s2 = np.zeros((n - f2, 4), dtype=np.uint64)
    idx = np.sort(np.random.default_rng(SEED).choice(n - f2, size=cf.SPARSE_TERMS, replace=False))
    s2[idx] = pkg.synthetic_scalars(SEED + 3, idx.shape[0])
    s3 = np.zeros((0, 4), dtype=np.uint64)
    sets = [(s0, 1), (s1, 0), (s2, f2), (s3, 123)]
    # expectations: set 0 by region, set 1 = s * (q P + sum of the hashed region), set 2 = pippenger of its 2^12 terms, set 3 = infinity
    p = pts[0]
    pr = pts[q:2 * q]
    w0 = cf.mul(oracle, p, cf.mont_sum(s0[:q - 1]))
    w0 = cf.add(oracle, w0, cf.as_result(oracle.pippenger(oracle.fe_sub(0, s0[q - 1:2 * q - 1:2], s0[q:2 * q:2]), pr[0::2])))
    w0 = cf.add(oracle, w0, cf.as_result(oracle.pippenger(s0[2 * q - 1:], pts[2 * q:])))
    w1 = cf.mul(oracle, cf.add(oracle, cf.mul(oracle, p, q), cf.point_sum(oracle, pts[2 * q:])), cf.plain(s1[0]))
    w2 = cf.as_result(oracle.pippenger(s2[idx], pts[f2 + idx]))
    return sets, [w0, w1, w2, None]


def test_msm_batch_regions_2_20(oracle, pkg, bbg, scale):
    """Four sets over one 2^20-point SRS with an all-equal region (every addition a doubling: k_redo), a P / -P region (half the pairs with
    equal scalars) and a hashed region.  The sets differ in `from` and length: n - 1 random scalars from 1, n equal scalars from 0 (one
    bucket per window and set holds n entries), 2^12 nonzero scalars from 4097 and an empty set.  Redo's global bucket numbers (set x
    2^(C-1) + bucket) must land in the right set at seg > 8.  Through msm_batch and msm_batch_device, under the defaults, the asynchronous
    reduce and msm_acc_waves 3; the four results summed on the device by g1_sum_device."""
    lg = 20
    n = 1 << lg
    scale.get_srs(lg, "hashed")
    base = scale.base[lg]
    pts = _regions_srs(oracle, base)
    srs = bbg.srs_register(pts)
    try:
        sets, want = _batch_sets(oracle, pkg, pts)
        total = None
        for w in want:
            total = cf.add(oracle, total, w)
        d_sc = [_dev(s) if s.shape[0] else None for s, _ in sets]
        ptrs = [t.data_ptr() if t is not None else 0 for t in d_sc]
        ns = [s.shape[0] for s, _ in sets]
        starts = [f for _, f in sets]
        shape = cf.msm_shape(n, sets=4, total_n=sum(ns))
        for name, opts in (("defaults", {}), ("async", {"msm_async_reduce": 1}), ("acc_waves_3", {"msm_acc_waves": 3})):
            with msm_options(bbg, **opts):
                got = bbg.msm_batch(srs, [s for s, _ in sets], starts)
                for k in range(4):
                    _check(oracle, got[k], want[k], ("msm_batch", name, k, shape["seg"]))
                out = torch.zeros(5 * 12, dtype=torch.int64, device="cuda")
                bbg.msm_batch_device(srs, ptrs, ns, out.data_ptr(), starts)
                bbg.join()
                bbg.g1_sum_device(out.data_ptr(), 4, out.data_ptr() + 4 * 96)
                res = _read(out, 5)
                for k in range(4):
                    _check(oracle, res[k], want[k], ("msm_batch_device", name, k))
                _check(oracle, res[4], total, ("g1_sum_device", name))
    finally:
        srs.free()


def test_msm_reduce_priority_on_a_fresh_context(oracle, pkg, bbg, scale):
    """msm_reduce_priority = 0 applies when the reduce streams are created: set on a fresh context before its first asynchronous MSM.
    Three back-to-back asynchronous MSMs at 2^20 (degenerate, digit-edge and short scalars) give the same points as on the shared context
    (the same affine words: the sort's scatter is ordered by atomics, so the Jacobian representatives of two runs may differ)."""
    lg = 20
    n = 1 << lg
    fams = ("A", "H", "G64")
    want = []
    with msm_options(bbg, msm_async_reduce=1):
        for fam in fams:
            srs, case, _ = scale.get_case(lg, fam)
            want.append(bbg.msm(srs, case.scalars))
            _check(oracle, want[-1], case.want, (fam, "shared context"))
    ctx = pkg.Bbg(0)
    try:
        ctx.set_option("msm_reduce_priority", 0)
        ctx.set_option("msm_async_reduce", 1)
        for fam, w in zip(fams, want):
            _, case, _ = scale.get_case(lg, fam)
            srs = ctx.srs_register(cf.srs_points(oracle, cf.SRS_KIND[fam], scale.base[lg]))
            try:
                assert ctx.msm_plan(n, srs) == (19, 14)
                got = ctx.msm(srs, case.scalars)
                _check(oracle, got, case.want, (fam, "fresh context"))
                assert np.array_equal(oracle.jac_to_affine(got), oracle.jac_to_affine(w)), fam
            finally:
                srs.free()
    finally:
        ctx.close()
