"""The vectors and expectations of the pairing-arithmetic conformance test (tests/tools/tower_vectors.py), checked without a GPU.

tests/test_gpu_tower.py holds every device function of csrc/fq_tower.hip.h, fq12_wave.hip.h and g2.hip.h to the integer models on raw
operands.  That comparison is only worth what its vectors are worth, so here:
  * every operand row is inside the tower's contract [0, 2p] and every expected row is a residue below p;
  * every operand position of every op meets every value of the corner set; the random group has both halves of the range;
  * every designed vector meets the condition its name states, recomputed here with plain integers;
  * the comparison itself (tower_vectors.check) accepts what the model gives, in either representative, and refuses a row off by one;
  * the op table restates the kernels' X-macro table, every __device__ function of the three headers has an op or a listed reason, and the
    entry points are in the header and the binding.
"""
import os
import re

import pytest

import pairing_model as pm
import pairing_wave_model as pwm
import tower_vectors as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aztec-2.0_amd", "csrc")
P = pm.P
OPS = sorted(tv.OPS)
ids = lambda op: "%d-%s" % (op, tv.OPS[op].name)  # noqa: E731


def _named(op, prefix):
    b = tv.build(op)
    found = [(n, v, e) for n, v, e in zip(b.names, b.operands, b.expected) if n.startswith(prefix)]
    assert found, "%s has no vector named %s*" % (tv.OPS[op].name, prefix)
    return found


def _plain(v):
    return [tv.plain(r) for r in v]


def _mont_mul(a, b):
    """What fe_mul leaves for raw a, b <= 2p: (a b + m p) / 2^256 with m = -a b / p mod 2^256 (no final subtraction)."""
    t = a * b
    m = (-t * pow(P, -1, 1 << 256)) % (1 << 256)
    assert (t + m * P) % (1 << 256) == 0
    r = (t + m * P) >> 256
    assert r < 2 * P and (r << 256) % P == t % P
    return r


# ------------------------------------------------------------------------------------------------ every op
@pytest.mark.parametrize("op", OPS, ids=ids)
def test_rows_are_in_range_and_corners_reach_every_position(op):
    o, b = tv.OPS[op], tv.build(op)
    assert 80 <= len(b.names) <= 1500 and len(set(b.names)) == len(b.names)
    seen = [set() for _ in range(o.nin)]
    for v, e in zip(b.operands, b.expected):
        assert len(v) == o.nin and len(e) == (5 if o.kinds[0] == "point" else o.nout)
        assert all(0 <= r <= 2 * P for r in v), "an operand row outside [0, 2p]"
        assert all(0 <= r < P for r in e), "an expected row that is no canonical residue"
        for pos, r in enumerate(v):
            seen[pos].add(r)
    for pos in range(o.nin):
        assert set(tv.CORNERS) <= seen[pos], (o.name, pos)
    assert tv.CORNERS == [0, 1, (1 << 256) % P, P - 1, P, P + 1, 2 * P - 1, 2 * P]
    for c in tv.CORNERS:  # all coefficients equal to the same corner
        assert [c] * o.nin in b.operands
    rnd = _named(op, "random:")
    assert len(rnd) == 64
    assert all(r < P for _, v, _ in rnd[:32] for r in v) and all(P <= r < 2 * P for _, v, _ in rnd[32:] for r in v)
    if op in tv.UNARY_F2:
        assert {tuple(v) for v in b.operands} >= {(x, y) for x in tv.CORNERS for y in tv.CORNERS}
    if op in tv.BINARY_F2:
        assert tv.REDUCED == [0, P - 1, P, 2 * P - 1, 2 * P]
        have = {tuple(v) for v in b.operands}
        assert all((w, x, y, z) in have for w in tv.REDUCED for x in tv.REDUCED for y in tv.REDUCED for z in tv.REDUCED)


def test_unary_and_binary_fq2_ops_are_the_ones_with_two_and_four_rows():
    for op, o in tv.OPS.items():
        if op < 13:
            assert (op in tv.UNARY_F2) == (o.nin == 2) and (op in tv.BINARY_F2) == (o.nin == 4), o.name
    assert 34 in tv.BINARY_F2


@pytest.mark.parametrize("op", OPS, ids=ids)
def test_the_comparison_accepts_the_model_and_refuses_a_row_off_by_one(op):
    """tower_vectors.check on a device that is the model: the expected residues as they are, and lifted by p; then one row off by one."""
    o, b = tv.OPS[op], tv.build(op)
    for i in range(0, len(b.names), 7):
        v, e = b.operands[i], b.expected[i]
        if o.kinds[0] == "point":
            z = (5, 7)
            q = None if e[0] else ((tv.plain(e[1]), tv.plain(e[2])), (tv.plain(e[3]), tv.plain(e[4])))
            good = [tv.raw(c) for c in (tv.jac(q, z) if q else [3, 4, 5, 6, 0, 0])]
            lifted = [g + P for g in good]
            bad = [good[0] + 1] + good[1:] if q else good[:4] + [1, 0]
        else:
            good = [v[k] if kind == "same" else r for k, (r, kind) in enumerate(zip(e, o.kinds))]
            lifted = [g + P if kind == "res" else g for g, kind in zip(good, o.kinds)]
            bad = good[:-1] + [good[-1] ^ 1]
        assert tv.check(op, v, e, good) is None, b.names[i]
        assert tv.check(op, v, e, lifted) is None, b.names[i]
        assert tv.check(op, v, e, bad), b.names[i]
        if "res" in o.kinds:
            k = o.kinds.index("res")
            assert "above 2p" in tv.check(op, v, e, good[:k] + [good[k] + 2 * P + (0 if good[k] else P)] + good[k + 1:])


# ------------------------------------------------------------------------------------------------ the designed vectors
def test_f2_mul_vectors_wrap_the_karatsuba_sum_and_borrow():
    for tag, total in (("2p", 2 * P), ("2p+1", 2 * P + 1)):
        for side, off in (("a", 0), ("b", 2)):
            for _, v, _ in _named(5, "designed:sum_%s:%s" % (tag, side)):
                assert v[off] + v[off + 1] == total
    for _, v, _ in _named(5, "designed:t0_lt_t1"):
        assert _mont_mul(v[0], v[2]) < _mont_mul(v[1], v[3])  # fe_sub(t0, t1) borrows
    eq = _named(5, "designed:t0_eq_t1")
    for _, v, e in eq:
        t0, t1 = _mont_mul(v[0], v[2]), _mont_mul(v[1], v[3])
        assert t0 % P == t1 % P and e[0] == 0 and e[1] != 0
    assert any(_mont_mul(v[0], v[2]) != _mont_mul(v[1], v[3]) for _, v, _ in eq) or len(eq) >= 8
    assert tv.mont_mul_raw(2 * P, 2 * P) == _mont_mul(2 * P, 2 * P) < 2 * P


def test_f2_sqr_vectors_have_equal_and_opposite_halves():
    for _, v, e in _named(6, "designed:c0_eq_c1"):
        assert (v[0] - v[1]) % P == 0 and v[0] % P and e[0] == 0
    for _, v, e in _named(6, "designed:c0_eq_neg_c1"):
        assert (v[0] + v[1]) % P == 0 and v[0] % P and e[0] == 0 and e[1] != 0
    assert any(v[0] != v[1] for _, v, _ in _named(6, "designed:c0_eq_c1")) and any(v[0] == v[1] for _, v, _ in _named(6, "designed:c0_eq_c1"))
    assert any(v[0] + v[1] == 2 * P for _, v, _ in _named(6, "designed:c0_eq_neg_c1"))


def _tower_mul(op, a, b):
    if op == 9:
        return list(pm.f2_mul(tv.F2(a), tv.F2(b)))
    if op == 26:
        return tv.flat6(pm.f6_mul(tv.F6(a), tv.F6(b)))
    if op == 33:
        return tv.flat12(pm.f12_mul(tv.F12(a), tv.F12(b)))
    return pwm.to_w(pm.f12_mul(pwm.from_w(a), pwm.from_w(b)))


@pytest.mark.parametrize("op", [9, 26, 33, 57], ids=ids)
def test_inversion_vectors(op):
    n = tv.OPS[op].nin
    zeros = _named(op, "designed:zero:")
    for _, v, e in zeros:
        assert all(r in (0, P, 2 * P) for r in v) and e == [0] * n
    assert len(zeros) >= (9 if n == 2 else 30)
    for pos in range(n):
        assert {v[pos] for _, v, _ in zeros} == {0, P, 2 * P}
    if n == 2:
        assert len({tuple(v) for _, v, _ in zeros}) == 9
    one = [1] + [0] * (n - 1)
    for which, first in (("one", lambda k: k == 1), ("minus_one", lambda k: k == P - 1), ("fq", lambda k: k not in (0, 1, P - 1))):
        units = _named(op, "designed:unit:%s" % which)
        assert len(units) == 2
        for name, v, e in units:
            a = _plain(v)
            assert first(a[0]) and not any(a[1:])
            assert all(r >= P for r in v) == name.endswith(":lifted")
            assert _tower_mul(op, a, _plain(e)) == one
    b = tv.build(op)
    for v, e in list(zip(b.operands, b.expected))[::5]:  # and in general: the product with the input is one, or both are zero
        a = _plain(v)
        assert _tower_mul(op, a, _plain(e)) == (one if any(a) else [0] * n)


def test_f2_is_zero_and_f2_eq_vectors():
    true = _named(11, "designed:true")
    assert {tuple(v) for _, v, _ in true} == {(x, y) for x in (0, P, 2 * P) for y in (0, P, 2 * P)} and all(e == [1] for _, _, e in true)
    false = _named(11, "designed:false")
    assert all(e == [0] for _, _, e in false)
    for miss in (1, tv.RM, tv.RM + 1):
        for z in (0, P, 2 * P):
            assert [miss, z] in [v for _, v, _ in false] and [z, miss] in [v for _, v, _ in false]
    eq = _named(12, "designed:true")
    for _, v, e in eq:
        assert (v[0] - v[2]) % P == 0 and (v[1] - v[3]) % P == 0 and e == [1]
    assert {(v[0] >= P, v[1] >= P, v[2] >= P, v[3] >= P) for _, v, _ in eq if v[0] % P} == {(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)}
    assert {tuple(v) for _, v, _ in _named(12, "designed:true:zero")} == {(a, b, c, d) for a in tv.ZEROS for b in tv.ZEROS for c in tv.ZEROS for d in tv.ZEROS}
    ne = _named(12, "designed:false")
    assert {n.split("coefficient")[1][0] for n, _, _ in ne} == set("0123")
    for name, v, e in ne:
        k = int(name.split("coefficient")[1][0])
        d = [(v[0] - v[2]) % P, (v[1] - v[3]) % P]
        assert e == [0] and d[k & 1] in (1, P - 1) and d[1 - (k & 1)] == 0


@pytest.mark.parametrize("op", [40, 59], ids=ids)
def test_is_one_vectors(op):
    true = _named(op, "designed:true")
    for _, v, e in true:
        assert v[0] in (tv.RM, tv.RM + P) and all(r in (0, P, 2 * P) for r in v[1:]) and e[-1] == 1
    assert {v[0] for _, v, _ in true} == {tv.RM, tv.RM + P}
    for pos in range(1, 12):
        assert {v[pos] for _, v, _ in true} == {0, P, 2 * P}
    false = {n: (v, e) for n, v, e in _named(op, "designed:false")}
    assert all(e[-1] == 0 for _, e in false.values())
    for k in range(1, 12):
        v, _ = false["designed:false:coefficient%d=1" % k]
        assert v == [tv.RM] + [1 if i == k else 0 for i in range(1, 12)]
    assert false["designed:false:word1_for_R"][0] == [1] + [0] * 11
    assert false["designed:false:R+1"][0] == [tv.RM + 1] + [0] * 11
    only_last = [v for n, (v, _) in false.items() if ":only_last=" in n]
    last = [v for n, (v, _) in false.items() if ":last=" in n]
    assert only_last and all(not any(v[:11]) and v[11] % P for v in only_last)
    assert last and all(v[:11] == [tv.RM] + [0] * 10 and v[11] % P for v in last)
    if op == 59:  # the twelve canonical rows are the value in the reference's layout
        b = tv.build(op)
        for v, e in list(zip(b.operands, b.expected))[::9]:
            assert tv.F12(_plain(e[:12])) == pwm.from_w(_plain(v))


def test_cyclotomic_vectors_are_in_the_subgroup_where_both_squarings_agree():
    found = _named(35, "designed:cyclotomic")
    assert len(found) >= 5
    for name, v, e in found:
        a = tv.F12(_plain(v))
        assert pm.f12_mul(a, pm.f12_conj(a)) == pm.F12_ONE                                       # unitary: what the easy part leaves
        assert pm.f12_mul(pm.f12_frobenius(pm.f12_frobenius(a, 2), 2), a) == pm.f12_frobenius(a, 2)      # order divides p^4 - p^2 + 1
        assert tv.F12(_plain(e)) == pm.f12_cyclotomic_sqr(a) == pm.f12_sqr(a)
        if name.endswith(":lifted"):
            assert all(P <= r < 2 * P for r in v)
    assert sum(n.endswith(":lifted") for n, _, _ in found) == 1
    rnd = _named(35, "random:")  # off the subgroup the two differ: the expectation there is the device's algorithm, not the plain square
    assert any(tv.F12(_plain(e)) != pm.f12_sqr(tv.F12(_plain(v))) for _, v, e in rnd[:4])


@pytest.mark.parametrize("op", [36, 37, 38, 54, 55, 56], ids=ids)
def test_frobenius_vectors_have_one_non_zero_component_each(op):
    seen = set()
    for _, v, e in _named(op, "designed:single"):
        a = _plain(v)
        six = tv.F12(a) if op < 50 else pwm.from_w(a)
        live = [c for c, two in enumerate(six[0] + six[1]) if two != pm.F2_ZERO]
        assert len(live) == 1
        seen.add((live[0], six[live[0] // 3][live[0] % 3][0] != 0, six[live[0] // 3][live[0] % 3][1] != 0))
        out = tv.F12(_plain(e)) if op < 50 else pwm.from_w(_plain(e))
        assert [c for c, two in enumerate(out[0] + out[1]) if two != pm.F2_ZERO] == live  # Frobenius keeps the component
    assert seen == {(c, x, y) for c in range(6) for x, y in ((True, True), (True, False), (False, True))}


@pytest.mark.parametrize("op", [39, 52], ids=ids)
def test_sparse_product_vectors(op):
    for zi, zn in enumerate(("o", "vw", "vv")):
        reps = set()
        for name, v, _ in _named(op, "designed:line:%s=" % zn):
            assert v[12 + 2 * zi] % P == 0 and v[13 + 2 * zi] % P == 0
            reps.add(v[12 + 2 * zi])
            if ":rest=" not in name:
                assert all(r % P for k, r in enumerate(v[12:]) if k // 2 != zi)
        assert reps == {0, P, 2 * P}
        assert {n.split(":rest=")[1] for n, _, _ in _named(op, "designed:line:%s=2p:rest=" % zn)} == set(tv.CORNER_NAMES)
    ones = _named(op, "designed:acc_one")
    for _, v, e in ones:
        assert _plain(v[:12]) == [1] + [0] * 11
        line = _plain(v[12:])
        want = ((tv.F2(line, 0), pm.F2_ZERO, tv.F2(line, 4)), (pm.F2_ZERO, tv.F2(line, 2), pm.F2_ZERO))   # one times the line is the line
        assert (tv.F12(_plain(e)) if op == 39 else pwm.from_w(_plain(e))) == want
    assert {v[0] for _, v, _ in ones} == {tv.RM, tv.RM + P}
    assert {n.split("line=")[1] for n, _, _ in ones if "line=" in n} == set(tv.CORNER_NAMES)


@pytest.mark.parametrize("op", [50, 51], ids=ids)
def test_w_basis_product_vectors_cover_every_pair_and_the_wrap(op):
    pairs = {}
    for name, v, e in _named(op, "designed:pair"):
        a, b = v[:12], v[12:]
        i = [k for k in range(6) if a[2 * k] or a[2 * k + 1]]
        j = [k for k in range(6) if b[2 * k] or b[2 * k + 1]]
        assert len(i) == 1 and len(j) == 1
        i, j = i[0], j[0]
        assert a[2 * i] == a[2 * i + 1] == b[2 * j] == b[2 * j + 1] and a[2 * i] in (tv.RM, 2 * P - 1)
        pairs.setdefault((i, j), set()).add(a[2 * i])
        # the product lands on w^((i + j) mod 6), times xi where i + j >= 6
        x = tv.plain(a[2 * i])
        term = pm.f2_mul((x, x), (x, x))
        if i + j >= 6:
            term = pm.f2_mul_xi(term)
        want = [0] * 12
        want[2 * ((i + j) % 6)], want[2 * ((i + j) % 6) + 1] = term
        assert _plain(e) == want
    assert set(pairs) == {(i, j) for i in range(6) for j in range(6)} and all(s == {tv.RM, 2 * P - 1} for s in pairs.values())
    assert sum(i + j == 6 for i, j in pairs) == 5 and sum(i + j >= 6 for i, j in pairs) == 15


def test_g2_on_twist_vectors():
    named = {n: (v, e) for n, v, e in _named(60, "designed:")}
    v, e = named["designed:true:generator"]
    assert (tv.F2(_plain(v)), tv.F2(_plain(v), 2)) == pm.G2 and e == [1]
    v, e = named["designed:true:multiple:lifted"]
    q = (tv.F2(_plain(v)), tv.F2(_plain(v), 2))
    assert all(P <= r < 2 * P for r in v) and q != pm.G2 and pm.g2_on_twist(q) and pm.g2_mul(q, pm.R) is None and e == [1]
    v, e = named["designed:true:outside_subgroup"]
    q = (tv.F2(_plain(v)), tv.F2(_plain(v), 2))
    assert pm.g2_on_twist(q) and pm.g2_mul(q, pm.R) is not None and e == [1]
    false = [(n, v, e) for n, (v, e) in named.items() if ":false:" in n]
    assert {n.split(":")[3][:4] for n, _, _ in false} == {"x.c0", "x.c1", "y.c0", "y.c1"}
    for tag, q in (("generator", pm.G2), ("multiple", tv.g2_points()[1])):
        rows = tv._aff_rows(q)
        mine = [(n, v, e) for n, v, e in false if ":%s:" % tag in n]
        assert len(mine) == 8
        for _, v, e in mine:
            assert e == [0] and sorted((a - b) % P for a, b in zip(v, rows))[:3] == [0, 0, 0] and sum((a - b) % P in (1, P - 1) for a, b in zip(v, rows)) == 1


def _point(e):
    return None if e[0] else ((tv.plain(e[1]), tv.plain(e[2])), (tv.plain(e[3]), tv.plain(e[4])))


def test_g2_madd_vectors_reach_every_exceptional_branch():
    inf = _named(62, "designed:p_infinite")
    assert {(v[4], v[5]) for _, v, _ in inf} == {(x, y) for x in tv.ZEROS for y in tv.ZEROS}
    for _, v, e in inf:
        assert _point(e) == (tv.F2(_plain(v), 6), tv.F2(_plain(v), 8))
    for branch, sign in (("p_eq_q", 1), ("p_eq_minus_q", -1)):
        for tag in ("generator", "multiple"):
            lifted = set()
            found = _named(62, "designed:%s:%s" % (branch, tag))
            for _, v, e in found:
                a = _plain(v)
                q = (tv.F2(a, 6), tv.F2(a, 8))
                p = tv.jac_affine(a[:6])
                assert tv.F2(a, 4) not in (pm.F2_ONE, pm.F2_ZERO)
                assert p == (q if sign == 1 else pm.g2_neg(q)) and pm.g2_on_twist(q)
                assert _point(e) == (pm.g2_add(q, q) if sign == 1 else None) and (sign == -1 or _point(e) is not None)
                lifted |= {k for k in range(6) if P <= v[k] <= 2 * P}
            assert lifted == set(range(6))
            assert any(all(r < P for r in v[:6]) for _, v, _ in found) and any(all(r >= P for r in v[6:]) for _, v, _ in found)
    for _, v, e in _named(62, "designed:generic"):
        a = _plain(v)
        p, q = tv.jac_affine(a[:6]), (tv.F2(a, 6), tv.F2(a, 8))
        assert p[0] != q[0] and pm.g2_on_twist(p) and pm.g2_on_twist(q) and _point(e) == pm.g2_add(p, q) and pm.g2_on_twist(_point(e))


def test_g2_dbl_vectors():
    inf = _named(61, "designed:infinity")
    assert {(v[4], v[5]) for _, v, _ in inf} == {(x, y) for x in tv.ZEROS for y in tv.ZEROS} and all(e[0] == 1 for _, _, e in inf)
    gen = _named(61, "designed:generic")
    assert any(tv.F2(_plain(v), 4) != pm.F2_ONE for _, v, _ in gen)
    for _, v, e in gen:
        p = tv.jac_affine(_plain(v))
        assert pm.g2_on_twist(p) and _point(e) == pm.g2_add(p, p) and _point(e) is not None


@pytest.mark.parametrize("op", [63, 64, 65], ids=ids)
def test_line_and_mul_by_q_vectors(op):
    found = _named(op, "designed:")
    g, other = tv.g2_points()[0], tv.g2_points()[2]
    assert g == pm.G2 and other != g
    assert len(found) == (4 if op == 65 else 12)
    assert sum(n.endswith(":lifted") for n, _, _ in found) == len(found) // 2
    for name, v, e in found:
        assert all(P <= r < 2 * P for r in v) == name.endswith(":lifted")
    if op == 65:
        for tag, q in (("generator", g), ("other", other)):
            for _, v, e in _named(op, "designed:%s" % tag):
                assert (tv.F2(_plain(v)), tv.F2(_plain(v), 2)) == q and (tv.F2(_plain(e)), tv.F2(_plain(e), 2)) == pm.mul_by_q(q)
        return
    for tag, q in (("generator", g), ("other", other)):   # the first three doubling / addition steps of precompute_miller_lines(q)
        lines = pm.precompute_miller_lines(q)
        kinds = []   # per line: is it an addition step
        for bit in pm.LOOP_BITS:
            kinds += [False] + ([True] if bit else [])
        mine = [k for k, add in enumerate(kinds) if add == (op == 64)][:3]
        for step, k in enumerate(mine):
            for _, v, e in _named(op, "designed:step:%s:%d" % (tag, step)):
                assert tv.flat6(lines[k]) == _plain(e[6:])
        first = _plain(_named(op, "designed:step:%s:0" % tag)[0][1])
        if op == 63:
            assert first == [*q[0], *q[1], 1, 0]
        else:
            assert (tv.F2(first), tv.F2(first, 2)) in (q, pm.g2_neg(q))


# ------------------------------------------------------------------------------------------------ the sources and the harness agree
def test_op_table_restates_the_kernels_table():
    """BBG_TOWER_OPS of csrc/tower_check.hip against the Python table (the GPU module asks bbg_tower_op_shape as well)"""
    src = open(os.path.join(CSRC, "tower_check.hip")).read()
    ops = {int(m.group(1)): (int(m.group(2)), int(m.group(3)), m.group(4), m.group(5))
           for m in re.finditer(r"^\s*X\((\d+), (\d+), (\d+), (TW_\w+)\)\s*/\* ([^ :]+)", src, re.M)}
    assert len(ops) == len(re.findall(r"^\s*X\(\d+,", src, re.M)), "a row of the table this scan does not read"
    mine = {op: (o.nin, o.nout, "TW_WAVE" if op in tv.WAVE_OPS else "TW_LANE", o.name) for op, o in tv.OPS.items()}
    assert ops == mine
    assert "namespace {" in src and "switch (op)" in src.split("int tower_op_shape")[1]


def _device_functions(header):
    text = open(os.path.join(CSRC, header)).read()
    text = re.sub(r"//[^\n]*", "", text)
    return re.findall(r"__device__\s+(?:__forceinline__\s+)?[\w:<>]+\s+(\w+)\s*\(", text)


def test_every_device_function_has_an_op():
    """A device function added to one of the three headers needs an op in BBG_TOWER_OPS / tower_vectors.OPS (or a reason in EXEMPT)."""
    named = {re.split(r"[<(]", o.name)[0] for o in tv.OPS.values()} | {"f12_store_lanes"}
    assert "f12_load_lanes" in named
    total = 0
    for header in ("fq_tower.hip.h", "fq12_wave.hip.h", "g2.hip.h"):
        found = _device_functions(header)
        assert len(found) >= 8, "the scan found too little in %s" % header
        assert len(found) == re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, header)).read()).count("__device__"), "a __device__ function this scan does not read in %s" % header
        total += len(found)
        for name in found:
            assert name in named or name in tv.EXEMPT, "%s (%s) has no op in tower_vectors.OPS / BBG_TOWER_OPS and no reason in tower_vectors.EXEMPT" % (name, header)
    assert total >= 60
    listed = set()
    for header in ("fq_tower.hip.h", "fq12_wave.hip.h", "g2.hip.h"):
        listed |= set(_device_functions(header))
    assert named <= listed, "an op names a function that is in none of the headers: %s" % sorted(named - listed)
    assert set(tv.EXEMPT) <= listed and not (set(tv.EXEMPT) & named)
    allowed = re.compile(r"f\d+_(zero|one)|f2_load|f2_store|(fq|f2)_(load|store)_lanes|w12_ref_component|w12_line_power|f12_frob_part|f2_3t_(minus|plus)_2z|line_store|g2_aff_\w+")
    assert all(allowed.fullmatch(n) for n in tv.EXEMPT), "the list of exempt helpers is short and explicit: constants, copies, index arithmetic, steps of a function with an op"


def test_g2_header_is_what_pairing_and_the_check_kernels_include():
    pairing = open(os.path.join(CSRC, "pairing.hip")).read()
    assert '#include "g2.hip.h"' in pairing and "struct G2Jac" not in pairing and "g2_madd(const" not in pairing
    check = open(os.path.join(CSRC, "tower_check.hip")).read()
    assert '#include "g2.hip.h"' in check and '#include "fq12_wave.hip.h"' in check
    for name in _device_functions("fq_tower.hip.h") + _device_functions("fq12_wave.hip.h") + _device_functions("g2.hip.h"):
        assert not re.search(r"__device__[^;{]*\b%s\s*\(" % name, check), "tower_check.hip re-implements %s" % name


def test_entry_points_are_in_the_header_and_the_binding(pkg):
    header = open(os.path.join(ROOT, "include", "bbg.h")).read()
    assert "int bbg_tower_op(bbg_ctx* ctx, int op, const uint32_t* in, size_t n, uint32_t* out);" in header
    assert "int bbg_tower_op_shape(int op, int* operands, int* results);" in header
    assert "bbg_tower_op" in pkg.binding.EXPORTED_SYMBOLS and "bbg_tower_op_shape" in pkg.binding.EXPORTED_SYMBOLS
    assert callable(pkg.binding.Bbg.tower_op) and callable(pkg.binding.Bbg.tower_op_shape)
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "tower_check.o" in makefile.split("OBJS")[1].split("\n")[0]
