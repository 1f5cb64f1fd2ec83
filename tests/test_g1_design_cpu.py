"""CPU side of the designed inputs for bbg_g1_ntt / bbg_open_all (tests/tools/g1_design.py): the designs reach what they claim to reach,
and their integer models agree with the oracle's group operations.  No GPU.

tests/test_gpu_g1_ntt.py and tests/test_gpu_open_all.py compare the kernels with [y] G for integers y computed by g1_design.  A GPU test
whose inputs silently stopped meeting a branch would still pass; these assertions are what keeps them on the branches."""
import numpy as np
import pytest

import coarse_inputs as ci
import g1_design as gd
import lagrange_model as lm
import open_all_model as oa

R = oa.R_MOD
SEED = 0xBB254 + 0xD51
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
STRING_SETS = {2: {3}, 3: {0, 5, 15}, 6: {0, 1, 63, 64, 65, 127}, 8: {0, 1, 63, 64, 65, 130, 511}}  # the sets tests/test_gpu_open_all.py runs


def lifted(oracle, scalars):
    """[k] G for plain integers k, canonical; k = 0 is the point at infinity."""
    G = oracle.g1_generator()
    return oa.canon_points(oracle, np.stack([oracle.g1_mul(G, k) for k in lm.ints_to_mont(oracle, scalars)]))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("lg", [3, 6, 8])
def test_every_stage_meets_both_coincidences(lg, inverse):
    n = 1 << lg
    a, y, report = gd.design_ntt(lg, inverse, SEED + lg)
    chosen = gd.chosen_butterflies(lg, SEED + lg)
    assert sorted(report) == list(range(lg))
    _, pairs = gd.dit_model(a, lg, inverse)
    for s in range(lg):
        equal, opposite, twiddled = report[s]
        assert equal >= 1 and opposite >= 1, f"2^{lg}, stage {s}: {report[s]}"
        # the chosen butterflies are where the model meets them, between finite operands
        (A, t), (B, u) = pairs[s][chosen[s][0]], pairs[s][chosen[s][1]]
        assert A and A == t and B and (B + u) % R == 0
        if s == 0:
            assert twiddled == 0  # every twiddle of stage 0 is 1
        elif lg == 3 and s == 1:
            assert twiddled >= 1  # g1_design.chosen_butterflies: two are not to be had at 2^3
        else:
            assert twiddled >= 2, f"2^{lg}, stage {s}: a coincidence under the twiddle 1 only"
            assert all(b & ((1 << s) - 1) for b in chosen[s])
        if lg == 8:
            assert max(chosen[s]) >= 64, "no chosen butterfly beyond the first round of 64 lanes"
    if lg >= 4:
        picks = [b for s in range(lg) for b in chosen[s]]
        assert len(set(picks)) == len(picks)
    # A = t in the last stage is an output at infinity at i + n/2, A = -t one at i; no other output is infinite
    last = chosen[lg - 1]
    assert sorted(k for k in range(n) if y[k] == 0) == sorted([last[0] + n // 2, last[1]])
    assert all(a) and len(set(a)) == n - 1  # the one repeat is stage 0's A = t


def test_dit_model_is_the_transform(oracle):
    lg, n = 3, 8
    w = ci.root_of_unity(lg)
    assert w == lm.root(oracle, lg)
    vals = [int.from_bytes(np.random.default_rng(SEED).bytes(32), "little") % R for _ in range(n)]
    for inverse in (False, True):
        for src in (vals, gd.design_ntt(lg, inverse, SEED + lg)[0]):
            out, _ = gd.dit_model(src, lg, inverse)
            base, scale = (pow(w, R - 2, R), pow(n, R - 2, R)) if inverse else (w, 1)
            assert out == [scale * v % R for v in oa.fr_ntt(src, base)]
            assert np.array_equal(lifted(oracle, out), oa.g1_ntt(oracle, lifted(oracle, src), inverse=inverse))
    minus, plus = gd.stage_functionals(lg, False)
    _, pairs = gd.dit_model(vals, lg, False)
    for s in range(lg):
        for b, (A, t) in enumerate(pairs[s]):
            assert sum(c * v for c, v in zip(minus[s][b], vals)) % R == (A - t) % R
            assert sum(c * v for c, v in zip(plus[s][b], vals)) % R == (A + t) % R


@pytest.mark.parametrize("lg", sorted(STRING_SETS))
def test_designed_zeros_are_where_they_were_asked_for(lg):
    n = 1 << lg
    inf_at = STRING_SETS[lg]
    a, s_hat = gd.design_string(lg, inf_at, SEED + 10 + lg)
    assert len(a) == n and all(a) and len(set(a)) == n
    assert s_hat == gd.string_transform(a) and len(s_hat) == 2 * n
    assert {k for k in range(2 * n) if s_hat[k] == 0} == inf_at
    if lg <= 3:  # the fast transform against the plain sum
        assert s_hat == oa.fr_ntt([a[n - 2 - i] for i in range(n - 1)] + [0] * (n + 1), ci.root_of_unity(lg + 1))
    if lg < 3:
        return
    k = min(inf_at - {0})
    zero_at = {k, k + 1, 0, 2 * n - 1} | ({130} if lg == 8 else set())
    f, c_hat = gd.design_coeffs(lg, zero_at, SEED + 20 + lg)
    assert len(f) == n and len(c_hat) == 2 * n
    assert {k for k in range(2 * n) if c_hat[k] == 0} == zero_at
    # c_hat is the transform of open_all_model's own embedding, and f_0 is free
    c = oa.embedding(np.zeros((n - 1, 8), dtype=np.uint64), f)[1]
    assert c_hat == oa.fr_fft(c, ci.root_of_unity(lg + 1))
    assert gd.coeff_transform([(f[0] + 1) % R] + f[1:]) == c_hat


def test_proof_scalars_match_the_closed_form():
    lg, n = 6, 64
    rng = np.random.default_rng(SEED + 30)
    f = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]
    a = [pow(X_INT, j, R) for j in range(n)]
    assert gd.proof_scalars(f, a) == oa.closed_form_scalars(f, X_INT, ci.root_of_unity(lg))


def test_proof_scalars_match_the_definition(oracle):
    lg, n = 3, 8
    a, _ = gd.design_string(lg, STRING_SETS[lg], SEED + 10 + lg)
    f, _ = gd.design_coeffs(lg, {5, 6, 0, 15}, SEED + 20 + lg)
    assert np.array_equal(lifted(oracle, gd.proof_scalars(f, a)), oa.open_all_definition(oracle, lifted(oracle, a), f))


def test_all_ones_over_a_string_of_domain_powers():
    """f = 1 + X + .. + X^(n-1) vanishes on the domain except at 1, so over s_j = [x^j] G with x = w^a, a != 0, every proof but those at
    1 and at x is the point at infinity -- while h is not: the forward stages cancel it."""
    lg, n = 4, 16
    w = ci.root_of_unity(lg)
    for e in (1, 3, n - 1, n // 2):
        x = pow(w, e, R)
        ks = gd.proof_scalars([1] * n, [pow(x, j, R) for j in range(n)])
        assert [m for m in range(n) if ks[m]] == sorted({0, e})
    assert all(gd.proof_scalars([1] * n, [1] * n))  # x = 1: f(1) = n, no proof vanishes
