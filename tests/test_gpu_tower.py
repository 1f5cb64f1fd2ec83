"""The device code of the pairing arithmetic against the integer models, function by function, on raw operands (bbg_tower_op).

The pairing tests (test_gpu_pairing.py, test_gpu_pairing_wave.py, the cell and KZG verification tests) compare end results of honest inputs,
where every intermediate coefficient is a generic 254-bit residue.  The tower's contract -- every coefficient coarsely reduced in the CLOSED
interval [0, 2p], fe_neg mapping 0 to 2p -- is met at its edges by almost no such input.  Here each device function of csrc/fq_tower.hip.h,
fq12_wave.hip.h and g2.hip.h (the product's own function, one kernel per op in csrc/tower_check.hip, operands loaded raw) runs on the vectors
of tests/tools/tower_vectors.py: the corner set {0, 1, R, p - 1, p, p + 1, 2p - 1, 2p} at every coefficient, vectors designed for the
conditions a generic input does not meet, and random fill in both halves of the range.  tests/test_tower_vectors_cpu.py shows, without a
GPU, that those vectors are what they claim.  The models (tests/tools/pairing_model.py, pairing_wave_model.py) are the reference for every
value; nothing expected comes from a device.

Each case makes ONE bbg_tower_op call over all vectors of its op and asserts, per vector:
  * every raw result row is at most 2p (the range contract);
  * every result row's residue is the model's; rows documented as canonical (f2_canon, f12_store, the words of w12_store_is_one, the stored
    lines) are the model's words exactly; booleans are exact; the lane-interleaved round trip returns the operand's raw words;
  * for g2_dbl / g2_madd the Jacobian result, normalised with the model (z = 0 is infinity), is the model's affine sum.
"""
import ctypes

import numpy as np
import pytest

import tower_vectors as tv

pytestmark = pytest.mark.gpu


def _words(rows):
    return np.array(tv.rows_to_words(rows), dtype=np.uint32)


def _ints(rows):
    return [tv.words_to_int(r) for r in rows]


def _hex(vals):
    return "[" + ", ".join("%#x" % v for v in vals) + "]"


@pytest.mark.parametrize("op", sorted(tv.OPS), ids=lambda op: "%d-%s" % (op, tv.OPS[op].name))
def test_device_function_against_the_model(bbg, op):
    o = tv.OPS[op]
    assert bbg.tower_op_shape(op) == (o.nin, o.nout), "the Python op table and the kernels' table disagree"
    b = tv.build(op)
    got = bbg.tower_op(op, _words(b.operands)).tolist()
    assert len(got) == len(b.operands)
    for i, rows in enumerate(got):
        vals = _ints(rows)  # a boolean row (word 0 is 0 or 1, the other words 0) is the integer 0 or 1
        what = tv.check(op, b.operands[i], b.expected[i], vals)
        if what:
            pytest.fail("%s (op %d), vector %d of %d '%s': %s\n  operands %s\n  device   %s\n  model    %s"
                        % (o.name, op, i, len(got), b.names[i], what, _hex(b.operands[i]), _hex(vals), _hex(b.expected[i])))


def test_refusals_leave_the_output_untouched(bbg):
    lib, ctx = bbg.lib, bbg.ctx
    invalid = -1  # BBG_E_INVALID
    b = tv.build(5)  # f2_mul
    rows = _words(b.operands[:4])
    sentinel = 0xA5A5A5A5
    out = np.full((4, 2, 8), sentinel, dtype=np.uint32)
    operands, results = ctypes.c_int(77), ctypes.c_int(77)
    for op in (14, 19, 27, 43, 49, 66, 100, -1, 1 << 30):
        assert op not in tv.OPS
        assert lib.bbg_tower_op_shape(op, ctypes.byref(operands), ctypes.byref(results)) == invalid, op
        assert (operands.value, results.value) == (77, 77)
        assert lib.bbg_tower_op(ctx, op, rows.ctypes.data, 4, out.ctypes.data) == invalid, op
        assert lib.bbg_last_error().decode() == "bbg_tower_op: unknown op"
        assert lib.bbg_tower_op(ctx, op, rows.ctypes.data, 0, out.ctypes.data) == invalid, op
        with pytest.raises(Exception):
            bbg.tower_op(op, rows)
    assert lib.bbg_tower_op_shape(5, None, ctypes.byref(results)) == invalid and results.value == 77
    # null pointers
    assert lib.bbg_tower_op(ctx, 5, None, 4, out.ctypes.data) == invalid
    assert lib.bbg_last_error().decode() == "bbg_tower_op: null argument"
    assert lib.bbg_tower_op(ctx, 5, rows.ctypes.data, 4, None) == invalid
    assert lib.bbg_tower_op(None, 5, rows.ctypes.data, 4, out.ctypes.data) == invalid
    # n = 0 is legal, with or without pointers
    assert lib.bbg_tower_op(ctx, 5, None, 0, None) == 0
    assert lib.bbg_tower_op(ctx, 5, rows.ctypes.data, 0, out.ctypes.data) == 0
    # n = 2^16 + 1 (the buffers really are that long: a missing check must not read past them)
    n = (1 << 16) + 1
    big_in = np.zeros((n, 1, 8), dtype=np.uint32)
    big_out = np.full((n, 1, 8), sentinel, dtype=np.uint32)
    assert lib.bbg_tower_op(ctx, 13, big_in.ctypes.data, n, big_out.ctypes.data) == invalid
    assert lib.bbg_last_error().decode() == "bbg_tower_op: n > 2^16"
    assert (big_out == sentinel).all()
    # nothing above wrote the output; a legal call right after gives the right answer
    assert (out == sentinel).all()
    got = bbg.tower_op(5, rows).tolist()
    for i, r in enumerate(got):
        assert tv.check(5, b.operands[i], b.expected[i], _ints(r)) is None
    # the largest legal n (fq_canon of zero is zero)
    assert not bbg.tower_op(13, big_in[:1 << 16]).any()
