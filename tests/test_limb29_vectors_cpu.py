"""The vectors and expected rows of the limb-arithmetic conformance test (tests/tools/limb29_vectors.py), checked without a GPU.

tests/test_gpu_limb29.py holds the device primitives of csrc/field29.hip.h, field29c.hip.h, curve29.hip.h, ntt29.hip.h and w29.hip.h to the
integer models on raw lazily reduced operands.  That comparison is only worth what its reference and its vectors are worth, so here:
  * every vector of every op passes through its model without a model assertion firing (it is inside the op's contract), and through the
    model the suite already had for that field, with the same rows;
  * every expected row satisfies the op's residue identity and value bound computed with plain % arithmetic on the operands' values;
  * the vectors reach the corners the models exist to protect: column sums with bit 63 set, limbs with bit 31 set, the first and the last
    reachable row of every table and both sides of the boundaries between rows;
  * every f29_sub / f29_neg / n29_bfly template argument list in the sources has an op.
"""
import glob
import math
import os
import re

import pytest

import acc29_model as accm
import limb29_vectors as lv

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aztec-2.0_amd", "csrc")
CASES = lv.cases()


@pytest.mark.parametrize("case", CASES, ids=lv.case_id)
def test_vectors_are_in_contract_and_expected_rows_hold_in_plain_arithmetic(case):
    which, op = case
    b = lv.build(which, op)  # a model assertion (overflow, negative limb, stated bound) fails here
    o, f = lv.OPS[op], lv.FIELDS[which]
    assert 50 <= len(b.operands) <= 4000, "a few thousand vectors at most"
    for v, r in zip(b.operands, b.expected):
        assert len(v) == o.nin and len(r) == o.nout
        o.check(f, v, r)  # residue identity and value bound, not through the model


def test_every_listed_primitive_has_an_op():
    names = " ".join(o.name for o in lv.OPS.values())
    for want in ("f29_from_fe<P,0>", "f29_from_fe<P,5>", "f29_carry", "f29_norm", "f29_to_fe", "f29_div32_to_fe", "f29_add", "w29::up",
                 "f29_mul", "f29_sqr", "f29_mul_sub2", "f29_mul_ilp", "fe_mul29", "fe_mul29_ilp", "f29_mul2", "f29_sqr2", "f29_mul_sub2_mul",
                 "f29_mul2_z", "f29_mul2_add", "f29_sqr_add_mul", "f29_mul_sub2_mul_z", "f29_sqr_z", "aff29_from_table(+)",
                 "aff29_from_table(-)", "xyzz29_from_affine", "xyzz29_madd", "xyzz29_finish", "ntt29_reduce", "n29_step8<0,true>",
                 "n29_step8<0,false>", "n29_step8<1,true>", "n29_step8<1,false>", "n29_step4<0>", "n29_step4<1>", "n29_step2", "n29_step8_raw<0>",
                 "n29_step8_raw<1>", "n29_finish", "n29_finish_mul", "f29_mulc", "w29::dot"):
        assert want in names, want
    for op in (0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23):
        assert lv.OPS[op].fields == (lv.FR, lv.FQ), "representation and products: both fields"


# ---- the corners
@pytest.mark.parametrize("case", [c for c in CASES if lv.OPS[c[1]].flags.get("bit63")], ids=lv.case_id)
def test_plain_products_reach_a_column_sum_with_bit_63_set(case):
    """f29_mul's contract (bitlen(a limbs) + bitlen(b limbs) <= 60) admits 9 * 2^60 + 9 * 2^58 in a column: above 2^63.  A signed shift or
    a signed comparison of a column shows only there."""
    b = lv.build(*case)
    assert (1 << 63) <= b.max_column < (1 << 64), math.log2(b.max_column)


# The accumulation's jobs keep every column below acc29_model.COLUMN_LIMIT = 2^63.  Largest column the vectors reach (Fq, measured from the
# models when this test was written), beside acc29_model.madd_bounds()'s figure with ALL limbs of every operand at their maximum at once (which
# no input reaches):
#     the single products (U2 / S2 / PP / PPP / Q / ZZ3 / ZZZ3 / X3 shapes)   bound 3172127054898649539 = 2^61.460
#     Y3 = R T + (64p - Y1) PPP                                                 bound 9038679483197574338 = 2^62.971
ACC_JOB_REACHED = {
    19: 2754427852840501248,  # f29_mul2_z          2^61.256
    20: 2754427852840501248,  # f29_mul2_add        2^61.256
    21: 2786216077787398144,  # f29_sqr_add_mul     2^61.273
    22: 8412156076249579520,  # f29_mul_sub2_mul_z  2^62.867
    23: 2801363737024397312,  # f29_sqr_z           2^61.281
    33: 4965790360455348224,  # xyzz29_madd         2^62.107 (its Y3, from the extreme-limb accumulators)
}


@pytest.mark.parametrize("op", sorted(ACC_JOB_REACHED))
def test_accumulation_jobs_reach_their_recorded_columns_below_the_limit(op):
    assert lv.OPS[op].flags.get("acc_job")
    bounds = accm.madd_bounds()
    single = max(v for k, v in bounds.items() if not k.startswith("Y3"))
    assert single == 3172127054898649539 and bounds["Y3 = R T + (64p - Y1) PPP"] == 9038679483197574338
    b = lv.build(lv.FQ, op)
    assert b.max_column == ACC_JOB_REACHED[op], (op, b.max_column)
    assert b.max_column < (bounds["Y3 = R T + (64p - Y1) PPP"] if op in (22, 33) else single) < accm.COLUMN_LIMIT
    if lv.FR in lv.OPS[op].fields:
        assert lv.build(lv.FR, op).max_column < accm.COLUMN_LIMIT


@pytest.mark.parametrize("case", [c for c in CASES if lv.OPS[c[1]].flags.get("bit31")], ids=lv.case_id)
def test_operand_limbs_with_bit_31_set(case):
    """the minuends of the subtractions and the addends of the ADD jobs may have bit 31 set (the f29_neg<12, 31> addend is below 2^31 + 2^29)"""
    b = lv.build(*case)
    for idx in lv.OPS[case[1]].flags["bit31"]:
        assert any(max(v[idx]) >= (1 << 31) for v in b.operands), idx
    if case[1] in (20, 21):  # the largest addend limb the contract allows: 2^31 + 2^29 - 1 - (a limb of 12p)
        top = max(max(v[idx][:8]) for v in b.operands for idx in lv.OPS[case[1]].flags["bit31"])
        assert (1 << 31) + (1 << 28) <= top < (1 << 31) + (1 << 29)


@pytest.mark.parametrize("case", [c for c in CASES if lv.OPS[c[1]].flags.get("out31")], ids=lv.case_id)
def test_subtractions_leave_limbs_with_bit_31_set(case):
    """a + spread - b may fill all 32 bits of a limb; f29_neg<M, 31> alone reaches 2^31 (an E = 31 subtrahend itself stays below 2^31)"""
    b = lv.build(*case)
    assert any(max(r[-1][:8]) >= (1 << 31) for r in b.expected)
    if lv.OPS[case[1]].name.startswith("f29_sub"):
        # the largest minuend limb against a zero subtrahend limb: 2^32 - 1 - 2^29 + (a limb of M p) - 2^(E - 29)
        assert max(max(r[0][:8]) for r in b.expected) >= (1 << 32) - (1 << 29) - 4


@pytest.mark.parametrize("case", [c for c in CASES if lv.OPS[c[1]].flags.get("table")], ids=lv.case_id)
def test_table_ops_select_the_first_and_last_row_and_both_sides_of_a_boundary(case):
    """f29_div32_to_fe / xyzz29_finish: all 32 five-bit digits.  ntt29_reduce: row max(q - 1, 0) for a value below 32p: rows 0 .. 30 (row
    31 belongs to no value inside the contract).  n29_finish: row q for a value up to 31p: rows 0 .. 30, and 31 only for 31p itself."""
    b = lv.build(*case)
    last = lv.OPS[case[1]].flags["table"] - 1
    assert b.rows >= set(range(last + 1)), sorted(b.rows)
    assert max(b.rows) in (last, last + 1) and max(b.rows) <= 31


def test_reduce_and_finish_vectors_sit_on_both_sides_of_every_top_limb_boundary():
    import test_ntt29_model as nttm
    for op in (40, 41):
        tops = {nttm.carry(v[0])[8] for v in lv.build(lv.FR, op).operands}
        for q in range(1, 31):
            c8 = -(-(q << 32) // nttm.INV_TOP)
            assert (c8 * nttm.INV_TOP) >> 32 == q and ((c8 - 1) * nttm.INV_TOP) >> 32 == q - 1
            assert c8 in tops and c8 - 1 in tops, (op, q)


# ---- the sources and the harness agree
def _template_lists(name):
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip*"))):
        for line in open(path):
            code = line.split("//")[0]
            for m in re.finditer(r"\b%s<([^<>()]*)>\s*\(" % name, code):
                out.setdefault(m.group(1).strip(), []).append(os.path.basename(path))
    return out


@pytest.mark.parametrize("name", ["f29_sub", "f29_neg", "n29_bfly"])
def test_every_instantiated_pair_has_an_op(name):
    found = _template_lists(name)
    assert found, "no use of %s found: the scan is broken" % name
    for args, where in found.items():
        if re.fullmatch(r"\d+(\s*,\s*\d+)?", args):
            nums = [int(x) for x in args.split(",")]
            pair = (nums[0], nums[1] if len(nums) > 1 else 30)  # E defaults to 30
            assert pair in lv.PAIRS, "%s<%s> (%s) has no op in limb29_vectors.PAIRS / BBG_L29_PAIRS" % (name, args, where[0])
        else:
            assert args in lv.TEMPLATE_EXPRESSIONS, "%s<%s> (%s): list the pairs this expression takes in TEMPLATE_EXPRESSIONS" % (name, args, where[0])
    for pairs in lv.TEMPLATE_EXPRESSIONS.values():
        assert set(pairs) <= set(lv.PAIRS)


def test_op_table_restates_the_kernels_table():
    """BBG_L29_OPS / BBG_L29_PAIRS of csrc/limb29_check.hip against the Python table (the GPU module asks bbg_limb29_op_shape as well)"""
    src = open(os.path.join(CSRC, "limb29_check.hip")).read()
    field_sets = {"L29_BOTH": (lv.FR, lv.FQ), "L29_FR": (lv.FR,), "L29_FQ": (lv.FQ,)}
    ops = {int(m.group(1)): (int(m.group(2)), int(m.group(3)), field_sets[m.group(4)])
           for m in re.finditer(r"^\s*X\((\d+), (\d+), (\d+), (L29_\w+)\)", src, re.M)}
    mine = {op: (o.nin, o.nout, o.fields) for op, o in lv.OPS.items() if op < 100}
    assert ops == mine
    pairs = [(int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^\s*X\((\d+), (\d+), (\d+)\)", src, re.M)]
    assert pairs == lv.PAIRS
    for i in range(len(lv.PAIRS)):
        assert (lv.OPS[100 + i].nin, lv.OPS[100 + i].nout, lv.OPS[200 + i].nin, lv.OPS[300 + i].nin, lv.OPS[300 + i].nout) == (2, 1, 1, 2, 2)
