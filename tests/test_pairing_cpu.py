"""The integer model of the BN254 pairing (tests/tools/pairing_model.py) that tests/test_gpu_pairing.py holds the device to, checked on its
own: bilinearity, the constants it derives, the generated header, the final exponentiation's program, and the reference's own
known-answer test.  No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest

import pairing_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REF", "/root/reference")  # the reference tree, where oracle/Makefile looks for it
KAT = os.path.join(REF, "barretenberg", "src", "aztec", "ecc", "curves", "bn254", "pairing.test.cpp")


def generator_module():
    spec = importlib.util.spec_from_file_location("gen_pairing_consts", os.path.join(ROOT, "scripts", "gen_pairing_consts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def g():
    return pm.reduced_ate_pairing(pm.G1, pm.G2)


def random_f12(seed):
    rng = np.random.default_rng(seed)
    v = [int.from_bytes(rng.bytes(40), "little") % pm.P for _ in range(12)]
    two = [(v[2 * i], v[2 * i + 1]) for i in range(6)]
    return (tuple(two[:3]), tuple(two[3:]))


def test_parameters_and_generator():
    assert pm.P % 4 == 3 and pm.P % 6 == 1 and pow(pm.Z, 1, 2) == 1
    assert pm.g2_on_twist(pm.G2) and pm.g2_mul(pm.G2, pm.R) is None and pm.g2_mul(pm.G2, pm.R - 1) == pm.g2_neg(pm.G2)
    assert pm.g1_mul(pm.G1, pm.R) is None
    assert pm.f2_mul(pm.TWIST_B, pm.XI) == (3, 0)
    assert 2 * pm.TWO_INV % pm.P == 1
    # the loop digits are a signed-digit form of 6 z + 2 below its leading bit, the other table the bits of z
    value = 1
    for d in pm.LOOP_BITS:
        value = 2 * value + {0: 0, 1: 1, 3: -1}[d]
    assert value == 6 * pm.Z + 2
    assert int("1" + "".join(map(str, pm.NEG_Z_LOOP_BITS)), 2) == pm.Z


def test_bilinear_and_non_degenerate(g):
    assert g != pm.F12_ONE and pm.f12_pow(g, pm.R) == pm.F12_ONE
    for a, b in ((1, 2), (3, 5), (0x1234567, pm.R - 7), (pm.R - 1, pm.R - 1)):
        assert pm.reduced_ate_pairing(pm.g1_mul(pm.G1, a), pm.g2_mul(pm.G2, b)) == pm.f12_pow(g, a * b % pm.R), (a, b)
    table = pm.PowerTable(g)
    for e in (0, 1, 15, 16, pm.R - 1, 0xDEADBEEF << 200):
        assert table.pow(e) == pm.f12_pow(g, e)


def test_batch_miller_loop_is_the_product_of_the_single_ones(g):
    qs = [pm.g2_mul(pm.G2, b) for b in (1, 7, 11)]
    ps = [pm.g1_mul(pm.G1, a) for a in (5, 3, pm.R - 2)]
    tables = [pm.precompute_miller_lines(q) for q in qs]
    batch = pm.miller_loop_batch(ps, tables)
    single = pm.F12_ONE
    for p, t in zip(ps, tables):
        single = pm.f12_mul(single, pm.miller_loop(p, t))
    assert batch == single
    assert pm.final_exponentiation(batch) == pm.f12_pow(g, (5 * 1 + 3 * 7 - 2 * 11) % pm.R)
    # a pair at infinity is the factor one; every pair at infinity is one
    assert pm.reduced_ate_pairing_batch_precomputed([ps[0], None, ps[2]], tables) == pm.f12_pow(g, (5 - 22) % pm.R)
    assert pm.reduced_ate_pairing_batch_precomputed([None] * 3, tables) == pm.F12_ONE


def test_frobenius_constants_against_exponentiation():
    x = random_f12(1)
    for k in (1, 2, 3):
        assert pm.f12_frobenius(x, k) == pm.f12_pow(x, pm.P**k), k
        assert pm.f6_frobenius(x[0], k) == pm.f12_pow((x[0], pm.F6_ZERO), pm.P**k)[0], k
    gen = generator_module()
    flat = lambda a: [c for six in a for c in six]  # noqa: E731
    for k, row in zip((1, 2, 3), gen.frobenius_table()):
        want = flat(pm.f12_frobenius(x, k))
        m = pm.f2_conj if k & 1 else (lambda c: c)
        assert [m(flat(x)[0])] + [pm.f2_mul(c, m(part)) for c, part in zip(row, flat(x)[1:])] == want, k
    # pi on the twist is multiplication by p there
    q = pm.g2_mul(pm.G2, 12345)
    assert pm.mul_by_q(q) == pm.g2_mul(q, pm.P % pm.R)


def test_tower_inverses_and_sparse_product():
    x, y = random_f12(2), random_f12(3)
    assert pm.f12_mul(x, pm.f12_inv(x)) == pm.F12_ONE
    assert pm.f6_mul(x[0], pm.f6_inv(x[0])) == pm.F6_ONE
    assert pm.f12_sqr(x) == pm.f12_mul(x, x)
    assert pm.f12_mul(pm.f12_mul(x, y), pm.f12_inv(y)) == x
    # w^2 = v, v^3 = xi
    w = (pm.F6_ZERO, pm.F6_ONE)
    v = ((pm.F2_ZERO, pm.F2_ONE, pm.F2_ZERO), pm.F6_ZERO)
    assert pm.f12_sqr(w) == v and pm.f12_mul(pm.f12_sqr(v), v) == ((pm.XI, pm.F2_ZERO, pm.F2_ZERO), pm.F6_ZERO)
    a = pm.f2_sqrt(pm.f2_sqr((5, 7)))
    assert a in ((5, 7), pm.f2_neg((5, 7)))


def test_cyclotomic_square_on_the_subgroup():
    x = pm.final_exponentiation_easy_part(random_f12(4))
    assert pm.f12_mul(x, pm.f12_conj(x)) == pm.F12_ONE, "the easy part lands in the cyclotomic subgroup: the conjugate is the inverse"
    assert pm.f12_cyclotomic_sqr(x) == pm.f12_sqr(x)
    assert pm.f12_cyclotomic_sqr(random_f12(5)) != pm.f12_sqr(random_f12(5)), "outside the subgroup the two differ: the test above says something"


def test_final_exponentiation_program(g):
    gen = generator_module()
    prog = gen.final_exponentiation_program()
    assert len(prog) == 295 and prog[-1] == 0
    f = pm.miller_loop(pm.g1_mul(pm.G1, 77), pm.precompute_miller_lines(pm.g2_mul(pm.G2, 5)))
    assert gen.run_program(prog, f) == pm.final_exponentiation(f) == pm.f12_pow(g, 385)
    # the whole exponent: (p^12 - 1) / r up to a factor prime to r
    x = random_f12(6)
    assert pm.f12_pow(pm.final_exponentiation(x), pm.R) == pm.F12_ONE


def test_generated_pairing_constants_are_in_sync():
    """csrc/pairing_consts.hip.h is generated (scripts/gen_pairing_consts.py): the committed header must be what the generator renders."""
    gen = generator_module()
    assert gen.render() == open(gen.PATH).read()


def test_lines_and_serialisation():
    lines = pm.precompute_miller_lines(pm.G2)
    words = pm.lines_words(lines)
    assert words.shape == (pm.LINES_BYTES // 8,) and words.dtype == np.uint64
    assert pm.fq_ints(words[:8].reshape(2, 4)) == list(lines[0][0])
    q = pm.g2_mul(pm.G2, 99)
    assert pm.g2_from_words(pm.g2_words(q)) == q and pm.g2_from_words(pm.g2_words(None)) is None
    x = random_f12(7)
    assert pm.f12_from_words(pm.f12_words(x)) == x
    assert pm.g1_from_words(pm.g1_words((1, 2))) == (1, 2)


def test_point_outside_the_subgroup():
    q = pm.g2_point_outside_subgroup()
    assert pm.g2_on_twist(q) and pm.g2_mul(q, pm.R) is not None
    assert pm.g2_mul(q, pm.R * (2 * pm.P - pm.R)) is None, "the twist has r (2p - r) points"


def parse_uint256(text):
    """Every uint256_t(a, b, c, d) of the text as an integer, limbs least significant first."""
    out = []
    for m in re.finditer(r"uint256_t\(\s*(0x[0-9a-fA-F]+)\s*,\s*(0x[0-9a-fA-F]+)\s*,\s*(0x[0-9a-fA-F]+)\s*,\s*(0x[0-9a-fA-F]+)\s*\)", text):
        out.append(sum(int(m.group(i + 1), 16) << (64 * i) for i in range(4)))
    return out


def test_reference_known_answer():
    """The reference's own known-answer test (ecc/curves/bn254/pairing.test.cpp, reduced_ate_pairing_check_against_constants): P, Q and the
    expected fq12 are read out of that file at run time and the model's reduced_ate_pairing is held to them."""
    if not os.path.exists(KAT):
        pytest.skip("the reference tree is not here")
    text = open(KAT).read()
    body = text[text.index("reduced_ate_pairing_check_against_constants"):text.index("reduced_ate_pairing_consistency_check")]
    v = parse_uint256(body)
    assert len(v) == 2 + 4 + 12
    p, q = (v[0], v[1]), ((v[2], v[3]), (v[4], v[5]))
    e = v[6:]
    expected = (tuple((e[2 * i], e[2 * i + 1]) for i in range(3)), tuple((e[2 * i], e[2 * i + 1]) for i in range(3, 6)))
    assert (p[1] * p[1] - p[0]**3 - 3) % pm.P == 0 and pm.g2_on_twist(q)
    assert pm.reduced_ate_pairing(p, q) == expected
