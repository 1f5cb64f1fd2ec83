"""The host-side dispatch of the Fr NTT (csrc/ntt.hip): which pass kernel a transform runs on, and the batched core against the one-by-one one.

1. bbg_ntt_plan against the rule as include/bbg.h words it (options ntt_kernel, ntt_limbs29, ntt_lds_planes), written out here as a table and
   not taken from the library.  bbg_ntt_plan builds no tables, so the sweep costs nothing on the device.
2. The batched core (grid.y = transforms) is reachable only through the resident prover, under option prover_ntt_batch: rounds 1 and 3 with
   the option off and on, under each of the three radix-8 kernel families, give bit-identical wires in every form, and those equal the
   oracle's transforms of the Lagrange form read from the same handle.

Every comparison is bit-exact on canonical Montgomery words."""
import ctypes
import itertools

import numpy as np
import pytest

from test_gpu_barycentric import make_prover

pytestmark = pytest.mark.gpu

IFFT, COSET_FFT = 1, 2
FORM_COEFF, FORM_LAGRANGE, FORM_COSET = 0, 1, 2  # enum bbg_poly_form (include/bbg.h)
QP_W_1 = 0
NTT_DEFAULTS = {"ntt_kernel": 2, "ntt_limbs29": -1, "ntt_lds_planes": 0}
KERNEL_NAMES = {0: "k_ntt_pass", 8: "k_ntt_pass8", 81: "k_ntt_pass8s", 29: "k_ntt_pass29"}


def documented_kernel(lg, kernel, limbs29, planes):
    """include/bbg.h on bbg_ntt_plan and on the three options, nothing else."""
    if kernel == 1 or lg < 11:
        return 0
    if limbs29 == 1 or (limbs29 == -1 and lg >= 18):
        return 29
    if planes == 1 or (planes == 0 and lg >= 22):
        return 81
    return 8


def restore_ntt_options(ctx):
    for key, value in NTT_DEFAULTS.items():
        ctx.set_option(key, value)


def test_ntt_plan_reports_the_documented_rule(pkg):
    ctx = pkg.Bbg(0)  # a fresh context has no built domain: every plan is computed, none remembered
    try:
        for kernel, limbs29, planes in itertools.product((1, 2), (-1, 0, 1), (0, 1, 2)):
            ctx.set_option("ntt_kernel", kernel)
            ctx.set_option("ntt_limbs29", limbs29)
            ctx.set_option("ntt_lds_planes", planes)
            for lg in (10, 11, 12, 17, 18, 21, 22):
                plan = ctx.ntt_plan(lg)
                where = (lg, kernel, limbs29, planes, plan)
                assert plan["kernel"] == KERNEL_NAMES[documented_kernel(lg, kernel, limbs29, planes)], where
                assert len(plan["log_radix"]) == plan["passes"] and sum(plan["log_radix"]) == lg, where
        restore_ntt_options(ctx)
        for lg in (10, 11, 12, 17, 18, 21, 22):
            plan = ctx.ntt_plan(lg)
            assert (plan["tile_log"] == 12) == (lg == 21), (lg, plan)  # the 4096-element tile: 2^21 alone under defaults
    finally:
        restore_ntt_options(ctx)
        ctx.close()


def read_wires(bbg, h, n, width):
    """(form -> (width, len, 4) raw words) of the wires as the handle holds them."""
    out = {}
    for form, length in ((FORM_LAGRANGE, n), (FORM_COEFF, n), (FORM_COSET, 4 * n)):
        rows = np.zeros((width, length, 4), dtype=np.uint64)
        for k in range(width):
            assert bbg.lib.bbg_prover_read_poly(h, QP_W_1 + k, form, rows[k].ctypes.data, length) == 0, bbg.lib.bbg_last_error()
        out[form] = rows
    return out


@pytest.mark.parametrize("lg,width", [(10, 3), (10, 4), (12, 3), (12, 4)])
def test_batched_and_single_transforms_agree_under_every_family(pkg, bbg, oracle, lg, width):
    """lg = 10: the wires' iFFT at 2^10 runs below the batched path, their coset forms at 2^12 through the fused batched load; lg = 12: a
    two-pass batched iFFT at 2^12 and coset forms at 2^14.  Widths 3 and 4 are the batch counts the prover uses."""
    lib, n = bbg.lib, 1 << lg
    srs = bbg.srs_synth_hashed(5, n + 1)
    wires = [pkg.synthetic_scalars(600 + k, n) for k in range(4)]  # as test_gpu_barycentric.rounds_1_3_4
    wp = (ctypes.c_void_p * 4)(*[w.ctypes.data for w in wires])
    ch = pkg.synthetic_scalars(700, 8)
    first = want = None
    try:
        for planes, batch in itertools.product((2, 1, 29), (0, 1)):  # the families as tests/test_gpu_parity.py::test_ntt_pass8_plans selects them
            bbg.set_option("ntt_lds_planes", planes if planes != 29 else 0)
            bbg.set_option("ntt_limbs29", 1 if planes == 29 else 0)
            bbg.set_option("prover_ntt_batch", batch)
            h = make_prover(pkg, bbg, srs, lg, width)
            try:
                com = np.zeros((width + 1, 12), dtype=np.uint64)
                assert lib.bbg_prover_round1(h, wp, com.ctypes.data) == 0, lib.bbg_last_error()
                assert lib.bbg_prover_round3(h, ch[0].ctypes.data, ch[1].ctypes.data, ch[2:5].ctypes.data, com[width:].ctypes.data) == 0, lib.bbg_last_error()
                got = {form: oracle.canon(0, rows.reshape(-1, 4)).reshape(rows.shape) for form, rows in read_wires(bbg, h, n, width).items()}
                got["round1"] = bbg.g1_normalize(com[:width])
            finally:
                lib.bbg_prover_destroy(h)
            if first is None:
                first = got
                coeffs = [oracle.ntt(got[FORM_LAGRANGE][k], IFFT) for k in range(width)]
                extended = [np.concatenate([c, np.zeros((3 * n, 4), dtype=np.uint64)]) for c in coeffs]
                want = {FORM_COEFF: np.stack(coeffs), FORM_COSET: np.stack([oracle.ntt(e, COSET_FFT, n) for e in extended])}
            for form in (FORM_COEFF, FORM_COSET):
                assert np.array_equal(got[form], want[form]), (planes, batch, form)
            for key in first:
                assert np.array_equal(got[key], first[key]), (planes, batch, key)
    finally:
        bbg.set_option("ntt_lds_planes", 0)
        bbg.set_option("ntt_limbs29", -1)
        bbg.set_option("prover_ntt_batch", 1)
        srs.free()
