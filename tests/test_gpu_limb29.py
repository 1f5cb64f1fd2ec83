"""The device code of the 29-bit-limb arithmetic against its integer models, on the same raw operands (bbg_limb29_op).

The hot path runs on lazily reduced 9 x 29-bit limbs whose correctness rests on contracts written in comments.  The integer models
(tests/test_limb29_model.py, test_ntt29_model.py, test_w29_model.py, tests/tools/acc29_model.py) prove that a RESTATEMENT of each operation
never overflows inside its contract; the end-to-end GPU tests feed the kernels canonical inputs and cannot steer a register inside a kernel to
the edge of a contract.  Here each device primitive -- the product's own function from the product's own header, one kernel per op in
csrc/limb29_check.hip -- runs on the vectors of tests/tools/limb29_vectors.py: the corners of its contract (limbs with bit 31 set, column sums
with bit 63 set, accumulators with every limb at 2^29 + 7, top limbs at the value bound, both sides of every row boundary of the table-driven
reductions) and random fill.  tests/test_limb29_vectors_cpu.py shows, without a GPU, that those vectors are inside the contracts and reach
the corners.

Each case asserts, in this order:
  1. residue and bound: val(result) satisfies the op's identity mod p and its stated output bound, from plain modular arithmetic on the
     operands.  A failure here is wrong device arithmetic for an in-contract operand.
  2. exact limbs: all nine words equal the model's, the unmasked top limb included (for the pair ops: both results equal the single-product
     models).  A failure here with 1 passing means the model is not the algorithm the device runs.
"""
import ctypes

import numpy as np
import pytest

import limb29_vectors as lv

pytestmark = pytest.mark.gpu


def _hex(rows):
    return "[" + ", ".join("(" + " ".join("%08x" % w for w in r) + ")" for r in rows) + "]"


def _report(b, what, i, got):
    return ("%s (which %d, op %d): %s at vector %d of %d\n  operands %s\n  device   %s\n  model    %s"
            % (b.name, b.which, b.op, what, i, len(b.operands), _hex(b.operands[i]), _hex(got), _hex(b.expected[i])))


@pytest.mark.parametrize("case", lv.cases(), ids=lv.case_id)
def test_device_primitive_against_its_model(bbg, case):
    which, op = case
    o, f = lv.OPS[op], lv.FIELDS[which]
    assert bbg.limb29_op_shape(which, op) == (o.nin, o.nout), "the Python op table and the kernels' table disagree"
    b = lv.build(which, op)
    got = bbg.limb29_op(which, op, np.array(b.operands, dtype=np.uint32)).tolist()
    assert len(got) == len(b.operands)
    # 1. residue and bound, by plain modular arithmetic on the operands
    for i, (v, r) in enumerate(zip(b.operands, got)):
        try:
            o.check(f, v, r)
        except AssertionError as e:
            pytest.fail(_report(b, "residue identity / output bound violated (%s)" % (e.args[0] if e.args else "check"), i, r))
    # 2. the model's exact limbs
    for i, r in enumerate(got):
        if r != b.expected[i]:
            pytest.fail(_report(b, "limbs differ from the model's (the residue and bound hold)", i, r))


def test_error_paths_leave_the_output_untouched(bbg):
    lib, ctx = bbg.lib, bbg.ctx
    invalid = -1  # BBG_E_INVALID
    operands, results = ctypes.c_int(77), ctypes.c_int(77)
    rows = np.array(lv.build(lv.FQ, 10).operands[:4], dtype=np.uint32)
    sentinel = 0xA5A5A5A5
    out = np.full((4, 1, 9), sentinel, dtype=np.uint32)
    unknown = [(lv.FQ, 9), (lv.FQ, 99), (lv.FQ, 100 + len(lv.PAIRS)), (lv.FQ, 400), (lv.FQ, -1), (lv.FQ, 1 << 30),  # unknown ops
               (2, 10), (-1, 10),                                                                                    # unknown which
               (lv.FQ, 40), (lv.FQ, 300), (lv.FR, 33)]                                                                # an op of the other field only
    for which, op in unknown:
        assert lib.bbg_limb29_op_shape(which, op, ctypes.byref(operands), ctypes.byref(results)) == invalid, (which, op)
        assert (operands.value, results.value) == (77, 77)
        assert lib.bbg_limb29_op(ctx, which, op, rows.ctypes.data, 4, out.ctypes.data) == invalid, (which, op)
        assert lib.bbg_limb29_op(ctx, which, op, rows.ctypes.data, 0, out.ctypes.data) == invalid, (which, op)
        with pytest.raises(Exception):
            bbg.limb29_op(which, op, rows)
    assert lib.bbg_limb29_op_shape(lv.FQ, 10, None, ctypes.byref(results)) == invalid
    # null pointers
    assert lib.bbg_limb29_op(ctx, lv.FQ, 10, None, 4, out.ctypes.data) == invalid
    assert lib.bbg_limb29_op(ctx, lv.FQ, 10, rows.ctypes.data, 4, None) == invalid
    assert lib.bbg_limb29_op(None, lv.FQ, 10, rows.ctypes.data, 4, out.ctypes.data) == invalid
    # n = 0 is fine, with or without pointers
    assert lib.bbg_limb29_op(ctx, lv.FQ, 10, None, 0, None) == 0
    assert lib.bbg_limb29_op(ctx, lv.FQ, 10, rows.ctypes.data, 0, out.ctypes.data) == 0
    # n = 2^20 + 1 (the buffers really are that long: a missing check must not read past them)
    n = (1 << 20) + 1
    big_in = np.zeros((n, 1, 9), dtype=np.uint32)
    big_out = np.full((n, 1, 9), sentinel, dtype=np.uint32)
    assert lib.bbg_limb29_op(ctx, lv.FQ, 2, big_in.ctypes.data, n, big_out.ctypes.data) == invalid
    assert (big_out == sentinel).all()
    # nothing above wrote the output; the context still works
    assert (out == sentinel).all()
    got = bbg.limb29_op(lv.FQ, 10, rows)
    assert got.tolist() == lv.build(lv.FQ, 10).expected[:4]
