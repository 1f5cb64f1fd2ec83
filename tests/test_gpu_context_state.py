"""GPU tests of a context's own state: every device buffer it owns is counted by bbg_memory_report, released by bbg_memory_trim and
rebuilt by the next call with bit-identical results; and bbg_set_option accepts, refuses and applies its 29 keys as documented
(include/bbg.h).  Each test runs on a fresh context of its own, so nothing here depends on what the session's shared context holds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SRS_SEED, SRS_N = 0xC0DE, 1 << 14


def run_every_owner(pkg, bbg, srs, oracle):
    """One call per buffer owner of a context; returns the outputs by name.  An MSM returns a Jacobian REPRESENTATIVE of its result, which
    was measured to differ between two identical calls on one context with nothing in between (the same point both times): the output
    compared is the point, in canonical affine form, as everywhere else in the suite."""
    out = {}
    out["ntt"] = bbg.ntt(pkg.synthetic_scalars(901, 1 << 12))  # two passes: the ping-pong buffer exists
    out["msm_tiny"] = oracle.jac_to_affine(bbg.msm(srs, pkg.synthetic_scalars(902, 1 << 10)))  # the small-circuit arena
    out["msm"] = oracle.jac_to_affine(bbg.msm(srs, pkg.synthetic_scalars(903, 1 << 14)))  # the main arena
    out["poly_evaluate"] = bbg.poly_evaluate(pkg.synthetic_scalars(904, 1 << 10), pkg.synthetic_scalars(905, 1)[0])
    # the permutation grand product at 2^10 on the inputs of test_gpu_parity.py::test_permutation_grand_product_vs_oracle
    log2n, n = 10, 1 << 10
    ch = pkg.synthetic_scalars(820, 5)
    bufs = [bbg.dev_alloc(n * 32) for _ in range(9)]
    try:
        for k in range(4):
            bbg.dev_upload(bufs[k], pkg.synthetic_scalars(800 + k, n))
            bbg.dev_upload(bufs[4 + k], pkg.synthetic_scalars(810 + k, n))
        bbg.dev_upload(bufs[8], np.zeros((n, 4), dtype=np.uint64))
        bbg.permutation_grand_product_device(bufs[:4], bufs[4:8], log2n, ch[0], ch[1], ch[2:5], bufs[8])
        out["grand_product"] = bbg.dev_download(bufs[8], (n, 4))
    finally:
        for b in bufs:
            bbg.dev_free(b)
    points = srs.read(0, 8)
    out["fixed_base_mul"] = bbg.g1_fixed_base_mul(pkg.synthetic_scalars(906, 5))
    out["batch_mul"] = bbg.g1_batch_mul(points[:5], pkg.synthetic_scalars(907, 5))
    out["g1_ntt"] = bbg.g1_ntt(points)
    return out


def test_every_owner_is_counted_trimmed_and_rebuilt(pkg, oracle):
    bbg = pkg.Bbg(0)
    try:
        srs = bbg.srs_synth_hashed(SRS_SEED, SRS_N)
        first = run_every_owner(pkg, bbg, srs, oracle)
        rep = bbg.memory_report()
        print("memory_report after the calls:", rep)
        assert rep["scratch"] > 0 and rep["msm_arena"] > 0 and rep["ntt_tables"] > 0, rep
        parts = ("srs_points", "srs_tables", "ntt_tables", "msm_arena", "scratch", "prover_keys")
        assert rep["total"] == sum(rep[k] for k in parts), rep
        srs.free()
        before = bbg.memory_report()
        released = bbg.memory_trim(tables=True)
        after = bbg.memory_report()
        print("memory_report after the trim:", after)
        assert released == before["total"] - after["total"], (released, before, after)
        assert after["scratch"] == 0 and after["msm_arena"] == 0 and after["ntt_tables"] == 0 and after["ntt_domains"] == 0, after
        srs = bbg.srs_synth_hashed(SRS_SEED, SRS_N)
        second = run_every_owner(pkg, bbg, srs, oracle)
        srs.free()
        assert sorted(first) == sorted(second)
        for name in first:
            assert np.array_equal(first[name], second[name]), name
    finally:
        bbg.close()


# key -> (lowest accepted, highest accepted, library default); the keys bbg_set_option checks against a range (include/bbg.h)
RANGES = {
    "msm_upload_pieces": (1, 4, 1),
    "batch_mul_glv": (0, 1, 1),
    "ecntt_mul": (0, 1, 1),
    "quotient_setup_plan": (0, 1, 1),
    "poly_limbs29": (0, 1, 1),
    "prover_fused_divide": (0, 1, 1),
    "prover_msm_batch": (0, 8, 4),  # BBG_MSM_BATCH_MAX = 8
    "prover_early_cosets": (-1, 1, -1),
    "ntt_limbs29": (-1, 1, -1),
    "ntt_lds_planes": (0, 2, 0),
    "ntt_tile_log": (9, 12, 10),
    "ntt_kernel": (1, 2, 2),
    "ntt_big_tile": (0, 3, 1),
    "ntt_max_logr8": (6, 11, 10),
    "ntt_max_logr": (4, 10, 7),
}
# the remaining defaults this test touches
OTHER_DEFAULTS = {"msm_sort": 1, "msm_window": 0, "batch_mul_lanes": 1 << 17, "msm_reduce_priority": 1, "msm_async_reduce": 0}


def test_options_are_accepted_refused_and_applied(pkg, oracle):
    bbg = pkg.Bbg(0)
    coeffs = pkg.synthetic_scalars(911, 1 << 10)
    want = oracle.canon(0, coeffs)

    def still_works():
        back = bbg.ntt(bbg.ntt(coeffs, pkg.binding.FFT), pkg.binding.IFFT)
        assert np.array_equal(oracle.canon(0, back), want)

    def refused(key, value):
        with pytest.raises(pkg.BbgError):
            bbg.set_option(key, value)
        still_works()

    try:
        still_works()
        refused("no_such_option", 1)
        for key, (lo, hi, default) in RANGES.items():
            refused(key, lo - 1)
            refused(key, hi + 1)
            bbg.set_option(key, lo)
            bbg.set_option(key, hi)
            still_works()
            bbg.set_option(key, default)
        # msm_sort: 0 and 1, but 0 only where the library was built with the rocPRIM sort path beside the partition sort
        refused("msm_sort", -1)
        refused("msm_sort", 2)
        bbg.set_option("msm_sort", 1)
        try:
            bbg.set_option("msm_sort", 0)
        except pkg.BbgError as e:
            assert "ROCPRIM_SORT" in str(e)
        bbg.set_option("msm_sort", OTHER_DEFAULTS["msm_sort"])

        # a window width is 0 or a compiled one
        bbg.set_option("msm_window", 16)
        refused("msm_window", 15)
        bbg.set_option("msm_window", OTHER_DEFAULTS["msm_window"])

        # lanes: a multiple of 64 in 64 .. 2^20
        srs = bbg.srs_synth_hashed(SRS_SEED, SRS_N)
        points, scalars = srs.read(0, 5), pkg.synthetic_scalars(907, 5)
        default_out = bbg.g1_batch_mul(points, scalars)
        for bad in (96, 63, 0, (1 << 20) + 1, (1 << 20) + 64):
            refused("batch_mul_lanes", bad)
        for good in (64, 1 << 20, 128):
            bbg.set_option("batch_mul_lanes", good)
        assert np.array_equal(bbg.g1_batch_mul(points, scalars), default_out)
        bbg.set_option("batch_mul_lanes", OTHER_DEFAULTS["batch_mul_lanes"])

        # a plan option drops the cached domains, a launch-time choice between kernels does not
        still_works()
        domains = bbg.memory_report()["ntt_domains"]
        assert domains > 0
        bbg.set_option("ntt_lds_planes", 2)
        assert bbg.memory_report()["ntt_domains"] == domains
        bbg.set_option("ntt_lds_planes", RANGES["ntt_lds_planes"][2])
        bbg.set_option("ntt_tile_log", 9)
        assert bbg.memory_report()["ntt_domains"] == 0
        bbg.set_option("ntt_tile_log", RANGES["ntt_tile_log"][2])
        still_works()

        # the reduce streams are torn down and come back with the next MSM
        msm_scalars = pkg.synthetic_scalars(903, 1 << 14)
        msm_before = oracle.jac_to_affine(bbg.msm(srs, msm_scalars))
        bbg.set_option("msm_reduce_priority", 0)
        bbg.set_option("msm_reduce_priority", OTHER_DEFAULTS["msm_reduce_priority"])
        bbg.set_option("msm_async_reduce", 1)
        msm_after = bbg.msm(srs, msm_scalars)
        bbg.join()
        msm_after = oracle.jac_to_affine(msm_after)  # the same point: the Jacobian representative is not fixed (run_every_owner)
        assert np.array_equal(msm_after, msm_before)
        bbg.set_option("msm_async_reduce", OTHER_DEFAULTS["msm_async_reduce"])
        srs.free()
    finally:
        bbg.close()
