"""GPU tests of the kernel variants the prover switches to at large sizes (run with -m gpu on an MI355X).

Several kernels change shape with the circuit: the grand product's k_gp_terms<W, E> takes E = 4 rows per thread from 2^18 rows
(gp_rows_per_thread), its k_gp_blocks gives each thread per = ceil(B / 256) > 1 block totals once there are more than 256 blocks (2^17
rows, and 2^19 up), and the 29-bit permutation widget k_quotient29_permutation<W, CH> takes CH = PERM_CH = 4 points per thread, stepping
w^256, from 2^20 points (quotient.hip launch_widget).  Apart from one 2^20-gate TurboPLONK proof, the rest of the suite runs these kernels
well below the switches, and their width-3 variants not at all.  Here each runs on both sides of its switch against the oracle, with its
raw outputs checked below 2p: the grand product in full against oracle.permutation_z up to 2^18 rows and through the O(n) recurrence of
tests/tools/size_switch_checks.py at every size; the width-4 and width-3 permutation widgets against oracle.quotient_widget on 2^19 ..
2^21 points.  The width-3 grand product (StandardPLONK) has no entry point of its own, so whole proofs on either side of the switches
must reproduce the reference CPU proof byte for byte."""
import functools
import os

import numpy as np
import pytest

import coarse_inputs as ci
import size_switch_checks as sc
from test_gpu_parity import _gpu_grand_product, _powers_srs, _run_gpu_widgets

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- permutation grand product
def _grand_product_case(pkg, oracle, bbg, wires, sigmas, ch, closing=False, full=False, what=""):
    log2n = wires.shape[1].bit_length() - 1
    z = _gpu_grand_product(pkg, bbg, wires, sigmas, log2n, ch[0], ch[1], ch[2:5])
    ci.assert_coarse(z, 0, what)
    N, D = sc.row_terms(oracle, wires, sigmas, ch[0], ch[1], ch[2:5], 4)
    sc.check_grand_product(oracle, z, N, D, closing=closing, what=what)
    if full:  # the oracle's serial restatement: ~4 s at 2^18 rows, too slow above
        assert np.array_equal(oracle.canon(0, z), oracle.permutation_z(wires, sigmas, ch[0], ch[1], ch[2:5])), what


@pytest.mark.parametrize("log2n", [16, 17, 18, 19, 20, 22])
def test_grand_product_across_the_row_and_block_switches(pkg, oracle, bbg, log2n):
    """Width 4 on random inputs.  2^16: E = 1, per = 1; 2^17: E = 1, per = 2; 2^18: E = 4, per = 1; 2^19: per = 2; 2^20: per = 4;
    2^22: per = 16."""
    n = 1 << log2n
    wires = np.stack([pkg.synthetic_scalars(0x5A00 + 16 * log2n + k, n) for k in range(4)])
    sigmas = np.stack([pkg.synthetic_scalars(0x5A08 + 16 * log2n + k, n) for k in range(4)])
    ch = pkg.synthetic_scalars(0x5B00 + log2n, 5)
    _grand_product_case(pkg, oracle, bbg, wires, sigmas, ch, full=log2n <= 18, what=("random", log2n))


@pytest.mark.parametrize("log2n", [18, 20])
def test_grand_product_coarse_inputs_across_the_switches(pkg, oracle, bbg, log2n):
    """Every wire and sigma value handed over as x + p (the top of [0, 2p)), the challenges too."""
    n = 1 << log2n
    wires = np.stack([pkg.synthetic_scalars(0x5C00 + 16 * log2n + k, n) for k in range(4)])
    sigmas = np.stack([pkg.synthetic_scalars(0x5C08 + 16 * log2n + k, n) for k in range(4)])
    ch = pkg.synthetic_scalars(0x5D00 + log2n, 5)
    z = _gpu_grand_product(pkg, bbg, sc.plus_p(wires), sc.plus_p(sigmas), log2n, sc.plus_p(ch[0]), sc.plus_p(ch[1]), sc.plus_p(ch[2:5]))
    ci.assert_coarse(z, 0, ("coarse", log2n))
    N, D = sc.row_terms(oracle, wires, sigmas, ch[0], ch[1], ch[2:5], 4)
    sc.check_grand_product(oracle, z, N, D, what=("coarse", log2n))
    if log2n <= 18:
        assert np.array_equal(oracle.canon(0, z), oracle.permutation_z(wires, sigmas, ch[0], ch[1], ch[2:5]))


def test_grand_product_of_a_closing_permutation_2_20(pkg, oracle, bbg):
    """sigma a random copy permutation of the identity tags K_k w^j, wires constant on its cycles: prod_j N_j / D_j = 1 over all
    2^20 rows, so the last row closes as well -- z[n-1] N_{n-1} = D_{n-1} ties together every block total k_gp_blocks scans."""
    ch = pkg.synthetic_scalars(0x5E00, 5)
    wires, sigmas = sc.closing_inputs(oracle, 20, ch[2:5], 4, seed=0x5E01)
    _grand_product_case(pkg, oracle, bbg, wires, sigmas, ch, closing=True, what="closing 2^20")


# ---------------------------------------------------------------------------------------------- permutation widgets
@functools.lru_cache(maxsize=1)
def _widget_polys(pkg, log2_large):
    m = 1 << log2_large
    return tuple(pkg.synthetic_scalars(0x5F00 + 32 * log2_large + k, m) for k in range(21))


def _widgets_vs_oracle(pkg, oracle, bbg, log2_large, widgets, coarse=False):
    """The widgets in order on the device (alpha_base chained) and in the oracle: alpha_base and the whole quotient after each, raw
    words below 2p."""
    m = 1 << log2_large
    polys = _widget_polys(pkg, log2_large)
    ch9 = pkg.synthetic_scalars(0x6000 + log2_large, 9)
    gpu_polys = [sc.plus_p(p) for p in polys] if coarse else list(polys)
    quot = np.zeros((m, 4), dtype=np.uint64)
    alpha_base = ch9[0].copy()
    for widget, (alpha_out, q) in zip(widgets, _run_gpu_widgets(pkg, bbg, gpu_polys, log2_large, ch9, ch9[0], widgets)):
        what = (widget, log2_large, coarse)
        ch = ch9.copy()
        ch[0] = alpha_base
        alpha_base = oracle.quotient_widget(widget, polys, log2_large, ch, quot)
        ci.assert_coarse(q, 0, what)
        assert np.array_equal(oracle.canon(0, alpha_out.reshape(1, 4))[0], alpha_base), what
        assert np.array_equal(oracle.canon(0, q), oracle.canon(0, quot)), what


@pytest.mark.parametrize("log2_large", [19, 21, 20])  # 20 last: the next tests reuse its inputs
def test_permutation_widgets_across_the_ch_switch(pkg, oracle, bbg, log2_large):
    """Widget 0 (width 4, TurboPLONK) and widget 5 (width 3, StandardPLONK and MiMC), each ASSIGNING the quotient: one point per thread
    at 2^19, PERM_CH = 4 points per thread from 2^20."""
    _widgets_vs_oracle(pkg, oracle, bbg, log2_large, (0, 5))


def test_permutation_widgets_coarse_inputs_2_20(pkg, oracle, bbg):
    _widgets_vs_oracle(pkg, oracle, bbg, 20, (0, 5), coarse=True)


def test_turbo_widget_chain_2_20(pkg, oracle, bbg):
    """The TurboPLONK widgets in round 4's order (permutation, arithmetic, fixed base, range, logic) over 2^20 points, each against the
    oracle.  One widget per call: the fused arithmetic + range + logic pass of a prover chain (option quotient_fuse) runs at this size in
    the 2^20-gate proof of tests/test_gpu_parity.py."""
    _widgets_vs_oracle(pkg, oracle, bbg, 20, (0, 1, 2, 3, 4))


# ---------------------------------------------------------------------------------------------- division by Z*_H
def test_divide_by_pseudo_vanishing_at_the_round4_shape(pkg, oracle, bbg):
    """Round 4 of a 2^18-gate proof: 2^20 coset values divided by Z*_H of the 2^18 domain (the goldens stop at 2^16), on random and on
    coarse values."""
    import torch
    e = pkg.synthetic_scalars(0x6100, 1 << 20)
    want = oracle.divide_by_pseudo_vanishing(e, 18)
    for vals in (e, sc.plus_p(e)):
        d = torch.from_numpy(np.ascontiguousarray(vals).view(np.int64).reshape(-1).copy()).cuda()
        bbg.divide_by_pseudo_vanishing_device(d.data_ptr(), 18, 20, 4)
        bbg.sync()
        got = d.cpu().numpy().view(np.uint64).reshape(-1, 4)
        ci.assert_coarse(got, 0, "dpv")
        assert np.array_equal(oracle.canon(0, got), oracle.canon(0, want))
        host = bbg.divide_by_pseudo_vanishing(vals, 18, 4)
        ci.assert_coarse(host, 0, "dpv host")
        assert np.array_equal(oracle.canon(0, host), oracle.canon(0, want))


# ---------------------------------------------------------------------------------------------- whole proofs straddling the switches
@functools.lru_cache(maxsize=1)
def _srs(oracle, count):  # ~7 s at 2^18 + 1 points: shared by both 2^18 proofs
    return _powers_srs(oracle, count)


@pytest.mark.parametrize("flavour,log2n", [(1, 18), (4, 18), (0, 17)])
def test_resident_proof_at_the_switches(pkg, oracle, bbg, flavour, log2n):
    """The resident prover against the reference CPU prover on recorded blinding, byte for byte, and the verifier accepts.
    StandardPLONK at 2^18 rows (flavour 1; 4 = its unrolled prover) runs k_gp_terms<3, 4> and k_quotient29_permutation<3, 4>, which
    nothing else reaches, and the automatic early coset forms.  TurboPLONK at 2^17 rows is the last size below the switches: k_gp_blocks
    with per = 2, the wires' batched coset extension at its largest shape (4n = 2^19) and round 1's grouped commitments."""
    from oracle.oracle import RefProver, prover_available, PROVER_GPU_SO
    if not prover_available() or not os.path.exists(PROVER_GPU_SO):
        pytest.skip("oracle/_ref/libbbprover_gpu.so absent on this machine")
    n = 1 << log2n
    x, pts = _srs(oracle, n + 1)
    gates = n - 64
    A = RefProver(gates, 31 + flavour, pts, x, flavour=flavour)
    assert A.n == n
    proof_cpu, blind = A.prove_recording()
    assert A.verify() == 1
    A.free()
    B = RefProver(gates, 31 + flavour, pts, x, gpu_linked=True, flavour=flavour)
    assert B.n == n
    assert B.resident_check_key() == 0
    proof_gpu, _ = B.prove_resident(blind)
    assert B.verify() == 1
    assert proof_gpu == proof_cpu, f"resident proof differs from the reference CPU proof (flavour {flavour}, n = 2^{log2n})"
    proof_fresh, _ = B.prove_resident()  # fresh randomness over the same key: a different, valid proof
    assert B.verify() == 1 and proof_fresh != proof_cpu
    B.free()
