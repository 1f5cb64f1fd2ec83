"""The cases of tests/tools/g1_sum_cases.py held to a second route on the CPU, and to the properties their designs claim.

Second route: the closed form [sum k_i] G (one oracle.g1_mul on the generator) against oracle.g1_sum over the very Jacobian words the GPU
tests hand to the library -- left-to-right Jacobian additions in C, another order and another coordinate system than k_g1_sum's.
Design properties: `replay` walks the reduction order of k_g1_sum on the integers and lists every addition of two finite operands; each
family is asserted to meet (or, for `generic`, to avoid) equal and opposite operands where its name says so."""
import numpy as np
import pytest

import coarse_inputs as ci
import fixed_base_model as fb
import g1_sum_cases as gc

R, Q = gc.R, gc.Q


def steps_of(name):
    total, steps = gc.replay(gc.spec(name).eff)
    assert total == gc.spec(name).total
    return [(where, gc.kind(a, b)) for where, a, b in steps]


def test_the_case_list_covers_the_sizes_and_families():
    assert len(set(gc.NAMES)) == len(gc.NAMES)
    assert {n for f, n in gc.FAMILIES if f == "generic"} == {0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000}
    families = {f for f, _ in gc.FAMILIES}
    for f in families - {"generic"}:
        sizes = {n for g, n in gc.FAMILIES if g == f}
        need = {2, 4, 16, 256, 257, 600}
        if f.startswith("serial_"):
            need = {257, 600}            # n > 256 by definition
        elif f.startswith("level2_"):
            need -= {2}                  # a tree of two levels has four slots
        elif f.endswith("_free"):
            need = {4, 16, 256, 257, 600, 3, 15, 255}  # at n = 2 the free pair is the only one; n = w - 1: one unpaired point
        assert need <= sizes, (f, sizes)
    assert {"all_equal", "level1_equal", "level1_opposite", "level1_equal_free", "level1_opposite_free", "level2_equal", "level2_opposite",
            "serial_equal", "serial_opposite", "lifted_twin"} | {"inf_" + p for p in gc.INF_PATTERNS} <= families
    assert {n for _, n in gc.FAMILIES if n in gc.DEVICE_SIZES} == {0, 1, 257, 600}


def test_tree_width_and_replay_on_small_inputs():
    assert [gc.tree_width(n) for n in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 128, 129, 256, 257, 1000)] == [1, 1, 2, 4, 4, 8, 8, 16, 16, 32, 128, 256, 256,
                                                                                                      256, 256]
    assert gc.replay([]) == (0, [])
    assert gc.replay([7]) == (7, [])
    assert gc.replay([7, 7]) == (14, [(("tree", 1), 7, 7)])
    # n = 3: width 4, (0, 2) meet at level 1, slot 3 is absent, then (0 + 2, 1) at level 2
    assert gc.replay([1, 2, 3]) == (6, [(("tree", 1), 1, 3), (("tree", 2), 4, 2)])
    # n = 258: threads 0 and 1 take one serial step each; level 1 pairs t with t + 128
    ks = list(range(1, 259))
    total, steps = gc.replay(ks)
    assert total == sum(ks) and steps[:2] == [(("serial", 1), 1, 257), (("serial", 1), 2, 258)]
    assert steps[2] == (("tree", 1), 258, 129) and len(steps) == 2 + 255
    assert gc.replay([5, 0, R - 5, 0])[1] == [(("tree", 1), 5, R - 5)]  # infinity operands are not compared


@pytest.mark.parametrize("name", gc.NAMES)
def test_case_by_the_oracle_sum_and_its_design(oracle, name):
    c = gc.case(oracle, name)
    s = c.spec
    assert c.jac.shape == (c.n, 12) and c.want.shape == (8,)
    # the words: finite entries have the flag clear and every coordinate below 2 q, canonical unless lifted
    for i in range(c.n):
        if i in s.flags:
            assert int(c.jac[i, 3]) >> 63 == 1
            continue
        X, Y, Z = ci.to_ints(c.jac[i].reshape(3, 4))
        for co, v in enumerate((X, Y, Z)):
            assert (Q <= v < 2 * Q) if s.lifts.get(i) == co else v < Q, (name, i, co)
    # second route
    assert np.array_equal(oracle.g1_sum(c.jac), c.want), name
    if s.total == 0:
        assert np.array_equal(c.want, fb.aff_infinity())
    else:
        ci.assert_canonical(c.want.reshape(2, 4), 1, name)
    if c.n == 1:
        assert np.array_equal(oracle.jac_to_affine(c.jac[0]), c.want)
    # the design
    family = name.rsplit("-", 1)[0]
    steps = steps_of(name)
    where = lambda w: [kd for at, kd in steps if at == w]  # noqa: E731
    serial = [kd for at, kd in steps if at[0] == "serial"]
    sign = "equal" if "equal" in family else "opposite"
    if family == "generic":
        assert s.total != 0 or c.n == 0
        assert len(set(s.ks)) == c.n and all(kd == "generic" for _, kd in steps), name
        assert len(steps) == max(c.n - 1, 0)  # every addition is between finite operands
    elif family == "all_equal":
        assert len(set(s.ks)) == 1 and len(set(s.lams)) == c.n and s.total == c.n * s.ks[0] % R
        assert where(("tree", 1)) and set(where(("tree", 1))) == ({"equal"} if c.n <= 256 or c.n == 512 else {"equal", "generic"})
        if c.n & (c.n - 1) == 0:
            assert all(kd == "equal" for _, kd in steps) and len(steps) == c.n - 1, name
        if c.n > 256:
            assert set(where(("serial", 1))) == {"equal"}
    elif family.startswith("level1_"):
        free = family.endswith("_free")
        w = gc.tree_width(c.n)
        pairs = sum(1 for t in range(w // 2) if t + w // 2 < c.n)
        loose = 1 if free and c.n >= w else 0  # at n = w - 1 the free slot's partner is absent: no comparison at all
        got = where(("tree", 1))
        assert len(got) == pairs and got.count(sign) == pairs - loose and got.count("generic") == loose, name
        assert all(kd == "generic" for kd in serial)
        if c.n <= 256:
            assert all(s.lams[t] != s.lams[t + w // 2] for t in range(w // 2) if t + w // 2 < c.n)
        assert (s.total == 0) == (sign == "opposite" and not free and pairs == w // 2), name
        if free:
            assert s.total != 0
    elif family.startswith("level2_"):
        w = gc.tree_width(c.n)
        assert len(set(s.ks)) == c.n and len({min(k, R - k) for k in s.ks}) == c.n
        assert all(kd == "generic" for kd in serial + where(("tree", 1))) and len(where(("tree", 1))) == w // 2
        assert where(("tree", 2)) == [sign] * (w // 4), name
        assert (s.total == 0) == (sign == "opposite")
    elif family.startswith("serial_"):
        assert c.n > 256 and set(where(("serial", 1))) == {sign} and len(where(("serial", 1))) == min(c.n, 512) - 256
        assert all(s.lams[i] != s.lams[i - 256] for i in range(256, c.n))
        assert (s.total == 0) == (sign == "opposite" and c.n == 512)
    elif family == "lifted_twin":
        w = gc.tree_width(c.n)
        at = ("serial", 1) if c.n > 256 else ("tree", 1)
        twins = [(i - 256, i) for i in range(256, min(c.n, 512))] if c.n > 256 else [(t, t + w // 2) for t in range(w // 2) if t + w // 2 < c.n]
        assert where(at) == ["equal"] * len(twins) and twins
        for a, b in twins:
            assert s.ks[a] == s.ks[b] and s.lams[a] == s.lams[b] and (a in s.lifts) != (b in s.lifts)
            # the same element: the words differ in exactly the lifted coordinate, by q
            lifted, plain = (a, b) if a in s.lifts else (b, a)
            co = s.lifts[lifted]
            diff = [x - y for x, y in zip(ci.to_ints(c.jac[lifted].reshape(3, 4)), ci.to_ints(c.jac[plain].reshape(3, 4)))]
            assert diff == [Q if v == co else 0 for v in range(3)]
        if len(twins) >= 6:
            assert {s.lifts[i] for i in s.lifts} == {0, 1, 2}
            assert any(a in s.lifts for a, _ in twins) and any(b in s.lifts for _, b in twins)
    else:
        assert family.startswith("inf_")
        pattern = family[4:]
        count = {"all": c.n, "every_other": (c.n + 1) // 2, "every_other_dirty": (c.n + 1) // 2, "only_first": 1, "all_but_last": c.n - 1}.get(pattern)
        if count is None:
            h = gc.tree_width(c.n) // 2
            count = sum(1 for i in range(c.n) if (i % 256 < h) == (pattern == "lower_half"))
            assert 0 < count < c.n
        assert len(s.flags) == count and set(s.flags.values()) == {pattern.endswith("_dirty")}
        assert (s.total == 0) == (count == c.n)
        assert all(kd == "generic" for _, kd in steps)
        for i, dirty in s.flags.items():
            rest = np.delete(c.jac[i], 3)
            assert rest.any() == dirty and (int(c.jac[i, 3]) != 1 << 63) == dirty


@pytest.mark.parametrize("n", gc.NORMALIZE_SIZES)
def test_normalize_case_entry_by_entry(oracle, n):
    jac, want, kinds = gc.normalize_case(oracle, n)
    assert jac.shape == (n, 12) and want.shape == (n, 8) and len(kinds) == n
    if n >= 24:
        assert set(kinds) == {"rescaled", "plain", "lifted", "flagged"}
    one = ci.to_mont(1, 1)
    for i in range(n):
        assert np.array_equal(oracle.jac_to_affine(jac[i]), want[i]), (n, i)
        X, Y, Z = ci.to_ints(jac[i].reshape(3, 4))
        if kinds[i] == "flagged":
            assert X >> 255 == 1 and np.array_equal(want[i], fb.aff_infinity())
        else:
            assert X >> 255 == 0 and (Z % Q == one) == (kinds[i] == "plain")
            assert (max(X, Y, Z) >= Q) == (kinds[i] == "lifted")
            ci.assert_canonical(want[i].reshape(2, 4), 1)
