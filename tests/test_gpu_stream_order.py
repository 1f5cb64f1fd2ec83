"""Stream ordering of the *_device entry points on a caller's own non-blocking stream (include/bbg.h: "enqueues on the context stream and
returns"; with msm_async_reduce = 1 an MSM's result is complete for a stream-ordered consumer after bbg_join / bbg_join_lag).

Every case follows the consumer pattern of a framework that shares its stream with the library through bbg_set_stream:
  1. the result tensor is filled with a poison pattern (every byte 0x5A) on the stream,
  2. the library call or calls are queued,
  3. bbg_join / bbg_join_lag where the case says so,
  4. `snap = out.clone()` on the stream -- a device-to-device copy that nothing but the stream orders,
  5. the stream is synchronised and the SNAPSHOT is compared on the host.
Between 2 and 5 there is no bbg_sync, no torch.cuda.synchronize, no host-pointer entry point and no option that synchronises the device:
a wait the library failed to queue shows as poison (or a partial result) in the snapshot.  The one option set inside such a section is
"msm_window" in the five-MSM case, which only assigns a field of the context (bbg_set_option in csrc/bbg_capi.hip); every other option is
set before and restored after.

Each unsynchronised section runs twice: a first pass into scratch buffers, then a full host synchronisation, then the pass that is checked.
The first pass is not a retry.  It takes the first-use work out of the checked pass -- window tables, the scratch arena and its growth
(DevBuf::ensure synchronises the device before it frees), NTT tables -- because a host synchronisation inside the section would hide a
missing device-side wait.

Expected values come from the C oracle on the same inputs (pippenger, msm_naive, g1_sum, g1_mul, ntt, poly_binop), compared bit for bit
as canonical Montgomery affine points / canonical field elements.  No result of the library is used as an expectation.

Nothing here asserts the negative ("without a join the snapshot is stale"): that is a race, not a property.

The helpers of a section (`env`, `options`, `unsynchronised`, ..) live in tests/tools/stream_order.py and serve this file and its second
half, tests/test_gpu_stream_order_device.py ("device:" below; A / B / C n are the sections of that file, B = the inputs zeroed on the stream
right behind the call).  Every *_device function declared in include/bbg.h, and the case that covers it:

  bbg_msm_device                         sections 1 - 5, 7, 8 here; device: C 2 (beside a reduction that shares the arena)
  bbg_msm_batch_device                   sections 5, 6
  bbg_g1_sum_device                      section 7
  bbg_ntt_device                         section 9; device: C 1 (the filler in front of the pinned-array calls)
  bbg_poly_op_device                     section 9
  bbg_g1_fixed_base_mul_device           section 9; device: C 3 (the one table slot rebuilt twice)
  bbg_g1_batch_mul_device                section 9; device: C 4
  bbg_g1_ntt_device                      device: A 1 (both directions, ecntt_mul 1 and 0), B 1, C 4
  bbg_open_all_device                    device: A 2 (every point, 2^8), A 3 / B 3 (cells, (10, 4)), C 4, C 5 (behind a stream switch)
  bbg_open_all_batch_device              device: A 4 / B 4 (chunks of 2, 2, 1 over one workspace; one chunk of 3)
  bbg_cells_values_device                device: A 5
  bbg_cells_recover_device               device: A 6 / B 6, C 1
  bbg_cells_verify_reduce_device         device: A 7 / B 7 (msm_async_reduce 0 and 1), C 1, C 2
  bbg_fr_batch_invert_device             device: A 8
  bbg_kate_opening_device                device: A 9 (synchronises for F(z); the quotient array is snapshotted on the stream)
  bbg_kate_opening_lagrange_device       device: A 9 (the same)
  bbg_poly_linear_combination_device     device: A 10 (poly_limbs29 1 and 0)
  bbg_permutation_grand_product_device   device: A 11
  bbg_quotient_widget_device             device: A 12 (alpha_base_out = NULL: with it the call synchronises)
  bbg_divide_by_pseudo_vanishing_device  device: A 13
  bbg_cross_dft_device                   device: A 14
  bbg_scale_powers_device                device: A 15
  bbg_coset_fft_split_device             device: A 16
  bbg_poly_evaluate_device               none: its only output is a host value, returned after the call's own synchronisation
  bbg_poly_evaluate_lagrange_device      none: the same
  bbg_srs_register_device                none: it queues the table build on the context stream and synchronises it before it returns its
                                         only output, the handle
  bbg_multi_ntt_device                   none, for another reason than the three above: it runs on the streams of the group's own contexts
                                         and its contract is completion after bbg_multi_sync, not the order of a caller's stream.
                                         tests/test_gpu_multi_group.py::test_multi_sync_alone_completes_a_resident_call shows that with this
                                         file's discipline (snapshots on fresh streams behind bbg_multi_sync, nothing else synchronised); its
                                         back-to-back sections queue group calls with no synchronisation between them"""
import numpy as np
import pytest

import lagrange_model as lm
from stream_order import N16, N_TINY, SEED_K, affine, env, options, poisoned, to_device, unsynchronised, words  # noqa: F401 (env: a fixture)

pytestmark = pytest.mark.gpu

SEED_A, SEED_B, SEED_C, SEED_T, SEED_U = 0x57A0, 0x57A1, 0x57A2, 0x57A3, 0x57A4


def scalars(env, seed, n):
    return env.pkg.synthetic_scalars(seed, n)


def want_msm(env, seed, n, start=0, naive=False):
    """The oracle's MSM of synthetic_scalars(seed, n) over points [start, start + n): computed once per module, never changed."""
    key = (seed, n, start, naive)
    if key not in env.want:
        fn = env.oracle.msm_naive if naive else env.oracle.pippenger
        r = fn(scalars(env, seed, n), env.pts[start:start + n])
        r.setflags(write=False)
        env.want[key] = r
    return env.want[key]


def msm(env, d_scalars, n, out, start=0, scalar_offset=0, out_offset=0):
    env.ctx.msm_device(env.srs, d_scalars.data_ptr() + 32 * scalar_offset, n, out.data_ptr() + 96 * out_offset, start)


# 1 ---------------------------------------------------------------------------------------------------------- join, single MSM
@pytest.mark.parametrize("n,window", [(N16, 20), (N16, 22), (N16, 0), (N_TINY, 0)])
def test_join_orders_one_msm(env, n, window):
    """msm_async_reduce = 1: msm_device, join(), snapshot.  Windows 20 / 22 reduce 2^19 / 2^21 buckets on the auxiliary stream -- far longer
    than queuing a clone takes --, width 0 is the automatic one (16 bits at 2^16 terms, the 8-bit path at 4096)."""
    seed = SEED_T if n == N_TINY else SEED_A
    d_a = to_device(env, scalars(env, seed, n))

    def body(inputs, outs):
        msm(env, inputs[0], n, outs[0])
        env.ctx.join()
        return [outs[0].clone()]

    with options(env, msm_async_reduce=1, msm_window=window):
        snap, = unsynchronised(env, [d_a], [96], body)
    assert np.array_equal(affine(env, snap)[0], want_msm(env, seed, n)), (n, window)


# 2 ---------------------------------------------------------------------------------------------------------- two reductions outstanding
@pytest.mark.parametrize("window", [20, 22])
def test_join_orders_two_outstanding_reductions(env, window):
    """Two MSMs of the same n and window (no re-layout, no slot reuse: neither call waits for anything by itself) leave exactly MSM_SLOTS
    reductions in flight; one join() must cover both."""
    d_a, d_b = to_device(env, scalars(env, SEED_A, N16)), to_device(env, scalars(env, SEED_B, N16))

    def body(inputs, outs):
        msm(env, inputs[0], N16, outs[0])
        msm(env, inputs[1], N16, outs[1])
        env.ctx.join()
        return [outs[0].clone(), outs[1].clone()]

    with options(env, msm_async_reduce=1, msm_window=window):
        snap_a, snap_b = unsynchronised(env, [d_a, d_b], [96, 96], body)
    assert np.array_equal(affine(env, snap_a)[0], want_msm(env, SEED_A, N16)), window
    assert np.array_equal(affine(env, snap_b)[0], want_msm(env, SEED_B, N16)), window


# 3 ---------------------------------------------------------------------------------------------------------- join_lag
def test_join_lag_one_waits_for_the_older_reduction(env):
    """A, B, join(1): A's result is complete for the stream, B's may still be reducing; join(): B's is complete too.  The reduce slots go
    round robin over a counter that synchronous MSMs advance as well, so the sequence runs twice: as it comes, and with one synchronous
    MSM in front of A, which puts A into the other slot.  What this pins: join(1) queues a wait that covers A (a join(1) that queues none
    fails here in either parity).  What it cannot pin is WHICH slot the wait names: B's reduction starts after A's and normally ends
    after it, so a wait on B's slot would give a right snapshot of A too, and telling the two apart would mean asserting a race."""
    ctx = env.ctx
    d_a, d_b = to_device(env, scalars(env, SEED_A, N16)), to_device(env, scalars(env, SEED_B, N16))
    sync_out = []

    def body(inputs, outs):
        msm(env, inputs[0], N16, outs[0])
        msm(env, inputs[1], N16, outs[1])
        ctx.join(1)
        snap_a = outs[0].clone()
        ctx.join()
        return [snap_a, outs[1].clone()]

    def synchronous_msm_first():
        # outside the unsynchronised section: the option synchronises the device, and so does the bbg_sync behind the call
        ctx.set_option("msm_async_reduce", 0)
        try:
            out = poisoned(env, 96)
            msm(env, d_a, N16, out)
            ctx.sync()
            sync_out.append(out.cpu().numpy())
        finally:
            ctx.set_option("msm_async_reduce", 1)

    with options(env, msm_async_reduce=1, msm_window=22):
        for between in (None, synchronous_msm_first):
            snap_a, snap_b = unsynchronised(env, [d_a, d_b], [96, 96], body, between=between)
            tag = "synchronous MSM first" if between else "as it comes"
            assert np.array_equal(affine(env, snap_a)[0], want_msm(env, SEED_A, N16)), f"A after join(1), {tag}"
            assert np.array_equal(affine(env, snap_b)[0], want_msm(env, SEED_B, N16)), f"B after join(), {tag}"
    assert len(sync_out) == 1 and np.array_equal(affine(env, sync_out[0])[0], want_msm(env, SEED_A, N16))


@pytest.mark.parametrize("lag", [2, 5])
def test_join_lag_beyond_the_slots_waits_for_nothing_and_succeeds(env, lag):
    """At most MSM_SLOTS = 2 reductions are ever outstanding, so a lag of 2 or more leaves all of them outstanding: BBG_OK, and the
    results are complete after the join() that follows."""
    ctx = env.ctx
    d_a, d_b = to_device(env, scalars(env, SEED_A, N16)), to_device(env, scalars(env, SEED_B, N16))
    rcs = []

    def body(inputs, outs):
        msm(env, inputs[0], N16, outs[0])
        msm(env, inputs[1], N16, outs[1])
        rcs.append(ctx.lib.bbg_join_lag(ctx.ctx, lag))
        ctx.join()
        return [outs[0].clone(), outs[1].clone()]

    with options(env, msm_async_reduce=1, msm_window=20):
        snap_a, snap_b = unsynchronised(env, [d_a, d_b], [96, 96], body)
    assert rcs == [0, 0]
    assert np.array_equal(affine(env, snap_a)[0], want_msm(env, SEED_A, N16))
    assert np.array_equal(affine(env, snap_b)[0], want_msm(env, SEED_B, N16))


# 4 ---------------------------------------------------------------------------------------------------------- five back to back
def test_five_msms_of_alternating_shapes_behind_one_join(env):
    """2^16 at window 20, 4096 (8-bit path), 2^16 at window 16, 1000 (8-bit path), 2^16 at window 22 into five buffers, one join(), five
    snapshots: slot reuse (the third, fourth and fifth call each reuse a slot) and re-layout of the arena with no host synchronisation.
    "msm_window" is set between the calls; it assigns a field and synchronises nothing."""
    ctx = env.ctx
    plan = [(N16, 20, SEED_A), (N_TINY, 0, SEED_T), (N16, 16, SEED_B), (1000, 0, SEED_K), (N16, 22, SEED_C)]
    masters = [to_device(env, scalars(env, seed, n)) for n, _, seed in plan]

    def body(inputs, outs):
        for (n, window, _), d, o in zip(plan, inputs, outs):
            ctx.set_option("msm_window", window)
            msm(env, d, n, o)
        ctx.join()
        return [o.clone() for o in outs]

    with options(env, msm_async_reduce=1, msm_window=0):
        snaps = unsynchronised(env, masters, [96] * 5, body)
    for k, ((n, window, seed), snap) in enumerate(zip(plan, snaps)):
        assert np.array_equal(affine(env, snap)[0], want_msm(env, seed, n, naive=(n == 1000))), (k, n, window)


# 5 ---------------------------------------------------------------------------------------------------------- inputs in stream order
@pytest.mark.parametrize("async_reduce", [0, 1])
@pytest.mark.parametrize("n", [N16, N_TINY])
def test_scalars_are_consumed_in_stream_order(env, n, async_reduce):
    """A caller may overwrite d_scalars on the same stream as soon as msm_device has returned: the result is the ORIGINAL scalars' MSM."""
    seed = SEED_T if n == N_TINY else SEED_A
    d_a = to_device(env, scalars(env, seed, n))

    def body(inputs, outs):
        msm(env, inputs[0], n, outs[0])
        inputs[0].zero_()
        env.ctx.join()
        return [outs[0].clone(), inputs[0].clone()]

    with options(env, msm_async_reduce=async_reduce):
        snap, zeroed = unsynchronised(env, [d_a], [96], body)
    assert not zeroed.any()  # the overwrite did happen
    assert np.array_equal(affine(env, snap)[0], want_msm(env, seed, n)), (n, async_reduce)


def batch_sets(env, count):
    """(seed, n, start) of a batch's MSMs, of unequal length; the device scalars and the oracle's results."""
    sets = [(SEED_A, N16, 0), (SEED_U, 40001, 100), (SEED_T, N_TINY, 0), (SEED_B, N16, 0)][:count]
    masters = [to_device(env, scalars(env, seed, n)) for seed, n, _ in sets]
    want = [want_msm(env, seed, n, start) for seed, n, start in sets]
    return sets, masters, want


@pytest.mark.parametrize("async_reduce", [0, 1])
def test_batch_scalars_are_consumed_in_stream_order(env, async_reduce):
    """The same for msm_batch_device with three sets of unequal length: every set is overwritten behind the call."""
    sets, masters, want = batch_sets(env, 3)

    def body(inputs, outs):
        env.ctx.msm_batch_device(env.srs, [d.data_ptr() for d in inputs], [n for _, n, _ in sets], outs[0].data_ptr(), [st for _, _, st in sets])
        for d in inputs:
            d.zero_()
        env.ctx.join()
        return [outs[0].clone()]

    with options(env, msm_async_reduce=async_reduce):
        snap, = unsynchronised(env, masters, [3 * 96], body)
    got = affine(env, snap)
    for k in range(3):
        assert np.array_equal(got[k], want[k]), (k, sets[k], async_reduce)


# 6 ---------------------------------------------------------------------------------------------------------- batch under async reduce
def test_join_orders_a_batch_of_four(env):
    """msm_batch_device under msm_async_reduce = 1 at window 20 (4 x 2^19 buckets to reduce): join(), one snapshot of all 4 x 96 bytes."""
    sets, masters, want = batch_sets(env, 4)

    def body(inputs, outs):
        env.ctx.msm_batch_device(env.srs, [d.data_ptr() for d in inputs], [n for _, n, _ in sets], outs[0].data_ptr(), [st for _, _, st in sets])
        env.ctx.join()
        return [outs[0].clone()]

    with options(env, msm_async_reduce=1, msm_window=20):
        snap, = unsynchronised(env, masters, [4 * 96], body)
    got = affine(env, snap)
    for k in range(4):
        assert np.array_equal(got[k], want[k]), (k, sets[k])


# 7 ---------------------------------------------------------------------------------------------------------- multi-GPU combine pattern
def test_join_orders_partials_in_front_of_g1_sum(env):
    """What csrc/multi.hip does on context 0: asynchronous MSMs over point-range thirds of one scalar vector into one 3 x 96-byte buffer,
    join(), g1_sum_device over the buffer.  The sum is the oracle's whole MSM, and so is the oracle's own sum of the snapshotted partials."""
    third = 21845
    n = 3 * third
    d_a = to_device(env, scalars(env, SEED_A, n))

    def body(inputs, outs):
        for k in range(3):
            msm(env, inputs[0], third, outs[0], start=k * third, scalar_offset=k * third, out_offset=k)
        env.ctx.join()
        env.ctx.g1_sum_device(outs[0].data_ptr(), 3, outs[1].data_ptr())
        return [outs[0].clone(), outs[1].clone()]

    with options(env, msm_async_reduce=1, msm_window=20):
        parts, total = unsynchronised(env, [d_a], [3 * 96, 96], body)
    whole = want_msm(env, SEED_A, n)
    assert np.array_equal(affine(env, total)[0], whole)
    assert np.array_equal(lm.canon_points(env.oracle, env.oracle.g1_sum(words(parts, 12)))[0], whole)


# 8 ---------------------------------------------------------------------------------------------------------- stream switch
def test_join_carries_the_wait_to_a_new_stream(env):
    """bbg_set_stream synchronises the OLD stream only -- the reduction queued on an auxiliary stream is still in flight --, so the join
    behind the switch must make the NEW stream wait for it."""
    torch, ctx = env.torch, env.ctx
    s2 = torch.cuda.Stream()
    d_a = to_device(env, scalars(env, SEED_A, N16))

    def body(inputs, outs):
        msm(env, inputs[0], N16, outs[0])
        ctx.set_stream(s2.cuda_stream)
        ctx.join()
        # outs[0] belongs to `s` for torch's caching allocator and no record_stream tells it about s2: reading it on s2 is safe only because
        # the tensor outlives s2.synchronize() (unsynchronised() keeps `outs` until its snapshots are on the host) -- keep that order
        with torch.cuda.stream(s2):
            return [outs[0].clone()]

    def back_to_the_first_stream():  # behind the first pass and its synchronisation: the checked pass starts on `s` again
        ctx.set_stream(env.s.cuda_stream)

    with options(env, msm_async_reduce=1, msm_window=22):
        try:
            snap, = unsynchronised(env, [d_a], [96], body, between=back_to_the_first_stream, final_stream=s2)
        finally:
            ctx.set_stream(env.s.cuda_stream)
    assert np.array_equal(affine(env, snap)[0], want_msm(env, SEED_A, N16))


# 9 ---------------------------------------------------------------------------------------------------------- single-stream entry points
@pytest.mark.parametrize("lg", [12, 17])
def test_ntt_device_on_the_callers_stream(env, lg):
    """One call, one snapshot, no sync(): the only place these entry points run on a stream other than torch's current one."""
    c = scalars(env, 0x9100 + lg, 1 << lg)
    d_c = to_device(env, c)

    def body(inputs, outs):
        env.ctx.ntt_device(inputs[0].data_ptr(), lg, env.pkg.binding.FFT)
        return [inputs[0].clone()]

    snap, = unsynchronised(env, [d_c], [], body)
    assert np.array_equal(env.oracle.canon(0, words(snap, 4)), env.oracle.ntt(c, 0)), lg


def test_poly_op_device_on_the_callers_stream(env):
    n = 70001
    a, b = scalars(env, 0x9200, n), scalars(env, 0x9201, n)
    masters = [to_device(env, a), to_device(env, b)]
    for op in (0, 1, 2):
        def body(inputs, outs, op=op):
            env.ctx.poly_op_device(op, inputs[0].data_ptr(), inputs[1].data_ptr(), outs[0].data_ptr(), n)
            return [outs[0].clone()]

        snap, = unsynchronised(env, masters, [32 * n], body)
        assert np.array_equal(env.oracle.canon(0, words(snap, 4)), env.oracle.canon(0, env.oracle.poly_binop(op, a, b))), op


def test_fixed_base_mul_device_on_the_callers_stream(env):
    n = 300
    k = scalars(env, 0x9300, n)
    d_k = to_device(env, k)

    def body(inputs, outs):
        env.ctx.g1_fixed_base_mul_device(inputs[0].data_ptr(), n, outs[0].data_ptr())
        return [outs[0].clone()]

    snap, = unsynchronised(env, [d_k], [64 * n], body)
    g = env.oracle.g1_generator()
    want = lm.canon_points(env.oracle, np.stack([env.oracle.g1_mul(g, w) for w in k]))
    bad = np.flatnonzero((words(snap, 8) != want).any(axis=1))
    assert bad.size == 0, f"products {bad[:6]} differ from the oracle"


def test_batch_mul_device_on_the_callers_stream(env):
    n = 300
    k = scalars(env, 0x9400, n)
    p = env.pts[1000:1000 + n]
    masters = [to_device(env, p), to_device(env, k)]

    def body(inputs, outs):
        env.ctx.g1_batch_mul_device(inputs[0].data_ptr(), inputs[1].data_ptr(), n, outs[0].data_ptr())
        return [outs[0].clone()]

    snap, = unsynchronised(env, masters, [64 * n], body)
    want = lm.canon_points(env.oracle, np.stack([env.oracle.g1_mul(pt, w) for pt, w in zip(p, k)]))
    bad = np.flatnonzero((words(snap, 8) != want).any(axis=1))
    assert bad.size == 0, f"products {bad[:6]} differ from the oracle"
