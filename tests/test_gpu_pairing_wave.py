"""The wave-cooperative pairing product on the MI355X (bbg_pairing_product_wave*, csrc/pairing_wave.hip): one wave per product, the contract
of bbg_pairing_product.

Every comparison is bit-exact on canonical Montgomery words.  Fixtures as in tests/test_gpu_pairing.py: P_ij = [a_ij] G by
bbg_g1_fixed_base_mul, Q_j = [B[j]] G2 by bbg_g2_mul, so product i is g^(sum_j a_ij B[j] mod r) with g = e(G, G2) -- the closed form.  Each
product is also held to the lane form (bbg_pairing_product) on the same input, and three of them to the integer model of the reference's
reduced_ate_pairing_batch_precomputed and to the model of the kernel's own dataflow (tests/tools/pairing_wave_model.py)."""
import numpy as np
import pytest

import coarse_inputs as ci
import pairing_model as pm
import pairing_wave_model as wm
from stream_order import Env, to_device, unsynchronised

pytestmark = pytest.mark.gpu

R, P = pm.R, pm.P
SEED = 0xBB254 + 0x3A7E
GUARD = 0xA5A5A5A5A5A5A5A5
B = [0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % R, 3, R - 5, 0x0123456789ABCDEF << 130,
     0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R, 1, 0xFFFFFFFFFFFFFFFF, R - 1]  # Q_j = [B[j]] G2


@pytest.fixture(scope="module")
def world(bbg):
    """g = e(G, G2) and its power table, computed once and shared; Q_j by the device; line handles and model lines made on first use."""
    w = Env()
    w.g = pm.reduced_ate_pairing(pm.G1, pm.G2)
    w.table = pm.PowerTable(w.g)
    w.q_words = bbg.g2_mul(pm.fr_words(B))
    w.q = [pm.g2_mul(pm.G2, b) for b in B]
    handles, model_lines = {}, {}

    def lines(pairs):
        if pairs not in handles:
            handles[pairs] = bbg.g2_lines_prepare(w.q_words[:pairs])
        return handles[pairs]

    def lines_of(j):
        if j not in model_lines:
            model_lines[j] = pm.precompute_miller_lines(w.q[j])
        return model_lines[j]
    w.lines, w.lines_of = lines, lines_of
    yield w
    for h in handles.values():
        h.free()


def g1_points(bbg, scalars):
    return bbg.g1_fixed_base_mul(pm.fr_words(scalars))


def lifted(points):
    """Both coordinates of every finite point moved into [p, 2p)."""
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8).copy()
    finite = (p[:, 3] >> np.uint64(63)) == 0
    p[finite] = ci.add_int(p[finite].reshape(-1, 4), P).reshape(-1, 8)
    return p


# 1 ------------------------------------------------------------------------------------------------ values
# count 257 and 1030: more blocks than the chip has CUs (256) and SIMDs (1024), so blocks queue behind one another.  The kernel has one
# product per block, so there is no packing factor whose neighbours would need sizes of their own.
@pytest.mark.parametrize("count,pairs", [(c, p) for c in (1, 2, 5) for p in (1, 2, 3, 8)] + [(257, 2), (1030, 2)])
def test_values(bbg, world, count, pairs):
    rng = np.random.default_rng(SEED + 1000 * count + pairs)
    a = [[int.from_bytes(rng.bytes(40), "little") % R for _ in range(pairs)] for _ in range(count)]
    pts = g1_points(bbg, [x for row in a for x in row]).reshape(count, pairs, 8)
    pts[1::2] = lifted(pts[1::2]).reshape(-1, pairs, 8)  # every second product with its coordinates in [p, 2p)
    values, status = bbg.pairing_product_wave(world.lines(pairs), pts.reshape(-1, 8))
    assert not status.any(), "a random product is not one"
    want = np.stack([pm.f12_words(world.table.pow(sum(x * b for x, b in zip(row, B)) % R)) for row in a])
    bad = np.flatnonzero((values != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {count} products differ from g^(sum a b), first at {bad[:8]}"
    lane_values, lane_status = bbg.pairing_product(world.lines(pairs), pts.reshape(-1, 8))
    assert np.array_equal(values, lane_values) and np.array_equal(status, lane_status), "the wave form differs from the lane form"
    for i in sorted({0, count // 2, count - 1}):
        points = [pm.g1_mul(pm.G1, x) for x in a[i]]
        tables = [world.lines_of(j) for j in range(pairs)]
        assert np.array_equal(values[i], pm.f12_words(pm.reduced_ate_pairing_batch_precomputed(points, tables))), f"product {i} differs from the full model"
        assert np.array_equal(values[i], pm.f12_words(wm.pairing_product(points, tables)[0])), f"product {i} differs from the model of the kernel's dataflow"


# 2 ------------------------------------------------------------------------------------------------ status
def test_status_words(bbg, pkg, world):
    a, b = 0x1234567890ABCDEF1234567890ABCDEF % R, B[0]
    q = world.q_words[0]
    h = bbg.g2_lines_prepare(np.stack([q, q]))
    try:
        pa, pna, pna1 = g1_points(bbg, [a, R - a, R - a + 1])
        inf = pm.G1_INFINITY_WORDS
        products = [(pa, pna), (pa, pna1), (inf, pa), (inf, inf), (pna, pa)]  # one by design, one off, a pair at infinity, all at infinity, swapped
        expo = [0, b, a * b % R, 0, 0]
        pts = np.stack([p for pair in products for p in pair])
        values, status = bbg.pairing_product_wave(h, pts)
        assert list(status) == [1, 0, 0, 1, 1]
        assert np.array_equal(values, np.stack([pm.f12_words(world.table.pow(e)) for e in expo]))
        assert np.array_equal(values[3], pm.f12_words(pm.F12_ONE)), "every pair at infinity: the Fq12 one"
        none, only_status = bbg.pairing_product_wave(h, pts, want_values=False)
        assert none is None and list(only_status) == [1, 0, 0, 1, 1]
        # an off-curve point in product 2: status 2 there, every other product as before; the host form says BBG_E_INVALID
        bad = pts.copy()
        bad[5, 4:] = ci.add_int(bad[5, 4:], 1)[0]  # y + 1
        d_in, d_out, d_st = bbg.dev_alloc(bad.nbytes), bbg.dev_alloc(5 * 384), bbg.dev_alloc(5 * 4)
        try:
            bbg.dev_upload(d_in, bad)
            bbg.pairing_product_wave_device(h, d_in, 5, d_out, d_st)
            got_st = bbg.dev_download(d_st, (5,), dtype=np.uint32)
            got = bbg.dev_download(d_out, (5, 48))
            assert list(got_st) == [1, 0, 2, 1, 1]
            keep = [0, 1, 3, 4]
            assert np.array_equal(got[keep], values[keep]), "the other products are not affected"
            bbg.dev_upload(d_in, pts)  # the honest batch right after it
            bbg.pairing_product_wave_device(h, d_in, 5, d_out, d_st)
            assert list(bbg.dev_download(d_st, (5,), dtype=np.uint32)) == [1, 0, 0, 1, 1] and np.array_equal(bbg.dev_download(d_out, (5, 48)), values)
        finally:
            for d in (d_in, d_out, d_st):
                bbg.dev_free(d)
        st = np.zeros(5, dtype=np.uint32)
        vals = np.zeros((5, 48), dtype=np.uint64)
        assert bbg.lib.bbg_pairing_product_wave(bbg.ctx, h.handle, bad.ctypes.data, 5, vals.ctypes.data, st.ctypes.data) == -1
        assert b"bbg_pairing_product_wave" in bbg.lib.bbg_last_error() and b"not on the curve" in bbg.lib.bbg_last_error()
        assert list(st) == [1, 0, 2, 1, 1], "the host form reports which product it was"
        assert np.array_equal(vals[keep], values[keep]), "and has written the values"
        with pytest.raises(pkg.BbgError):
            bbg.pairing_product_wave(h, bad)
    finally:
        h.free()


# 3 ------------------------------------------------------------------------------------------------ argument errors, no working memory
def test_argument_errors(bbg, world):
    import torch
    pairs, count = 2, 3
    h = world.lines(pairs)
    pts = g1_points(bbg, [1, 2, 3, 4, 5, 6])
    d_in, d_out = bbg.dev_alloc(pts.nbytes), bbg.dev_alloc(count * 388 + 64)
    d_st = d_out + count * 384
    guard = np.full((count * 388 + 64) // 4, 0xA5A5A5A5, dtype=np.uint32)
    lib = bbg.lib

    def call(hh=h.handle, di=d_in, n=count, do=d_out, ds=d_st, null_ctx=False):
        return lib.bbg_pairing_product_wave_device(None if null_ctx else bbg.ctx, hh, di, n, do, ds)

    try:
        bbg.dev_upload(d_in, pts)
        bbg.dev_upload(d_out, guard)
        errors = {"null context": dict(null_ctx=True), "null handle": dict(hh=None), "null points": dict(di=None), "both outputs null": dict(do=None, ds=None),
                  "count = 0": dict(n=0), "count above 2^24": dict(n=(1 << 24) + 1), "the values on the last point": dict(do=d_in + pts.nbytes - 64),
                  "the status on the first point": dict(ds=d_in + 60), "the status inside the values": dict(ds=d_out + 380),
                  "the values on the status": dict(do=d_st - 380)}
        for what, kw in errors.items():
            assert call(**kw) == -1 and lib.bbg_last_error(), what
        host_v, host_s = np.full((count, 48), GUARD, dtype=np.uint64), np.full(count, 0xA5A5A5A5, dtype=np.uint32)
        for kw in (dict(hh=None), dict(pp=None), dict(n=0), dict(n=(1 << 24) + 1), dict(v=None, s=None)):
            args = dict(hh=h.handle, pp=pts.ctypes.data, n=count, v=host_v.ctypes.data, s=host_s.ctypes.data)
            args.update(kw)
            assert lib.bbg_pairing_product_wave(bbg.ctx, args["hh"], args["pp"], args["n"], args["v"], args["s"]) == -1
        assert lib.bbg_pairing_product_wave(None, h.handle, pts.ctypes.data, count, host_v.ctypes.data, host_s.ctypes.data) == -1
        assert (host_v == GUARD).all() and (host_s == 0xA5A5A5A5).all()
        if torch.cuda.device_count() > 1:  # a handle made on another device
            other = type(bbg)(1)
            try:
                h1 = other.g2_lines_prepare(world.q_words[:pairs])
                assert call(hh=h1.handle) == -1 and b"another device" in lib.bbg_last_error()
                h1.free()
            finally:
                other.close()
        bbg.sync()
        assert np.array_equal(bbg.dev_download(d_out, guard.shape, dtype=np.uint32), guard), "an argument error wrote an output"
        assert np.array_equal(bbg.dev_download(d_in, pts.shape), pts), "an argument error wrote the input"
        # the neighbours are legal: the status right behind the values, one output alone
        assert call() == 0 and call(do=None) == 0 and call(ds=None) == 0
        got = bbg.dev_download(d_out, guard.shape, dtype=np.uint32)
        want = np.stack([pm.f12_words(world.table.pow((a * B[0] + b * B[1]) % R)) for a, b in ((1, 2), (3, 4), (5, 6))])
        assert np.array_equal(got[:count * 96].view(np.uint64).reshape(count, 48), want) and not got[count * 96:count * 97].any()
        assert (got[count * 97:] == 0xA5A5A5A5).all(), "the words behind the status"
    finally:
        bbg.dev_free(d_in)
        bbg.dev_free(d_out)


def test_no_working_memory(pkg, world):
    """A fresh context: the device form grows no buffer of the context."""
    ctx = pkg.Bbg(0)
    h = None
    try:
        h = ctx.g2_lines_prepare(world.q_words[:2])
        pts = ctx.g1_fixed_base_mul(pm.fr_words([1, 2, 3, 4]))
        d_in, d_out, d_st = ctx.dev_alloc(pts.nbytes), ctx.dev_alloc(2 * 384), ctx.dev_alloc(8)
        try:
            ctx.dev_upload(d_in, pts)
            ctx.sync()
            before = ctx.memory_report()["scratch"]
            ctx.pairing_product_wave_device(h, d_in, 2, d_out, d_st)
            ctx.sync()
            assert ctx.memory_report()["scratch"] == before, "the wave form took working memory"
            want = np.stack([pm.f12_words(world.table.pow((a * B[0] + b * B[1]) % R)) for a, b in ((1, 2), (3, 4))])
            assert np.array_equal(ctx.dev_download(d_out, (2, 48)), want) and not ctx.dev_download(d_st, (2,), dtype=np.uint32).any()
        finally:
            for d in (d_in, d_out, d_st):
                ctx.dev_free(d)
    finally:
        if h is not None:
            h.free()
        ctx.close()


# 4 ------------------------------------------------------------------------------------------------ the device form on the caller's stream
def test_device_form_is_ordered_on_the_callers_stream(pkg, world):
    """Under the discipline of tests/test_gpu_stream_order.py: a context of its own on a non-blocking stream, two passes, the input zeroed on
    the stream right behind the call, the snapshot taken on the stream, one synchronisation of that stream."""
    import torch
    env = Env()
    env.torch, env.ctx, env.s = torch, pkg.Bbg(0), torch.cuda.Stream()
    assert env.s.cuda_stream != 0
    env.ctx.set_stream(env.s.cuda_stream)
    pairs, count = 2, 70
    rng = np.random.default_rng(SEED + 6)
    a = [[int.from_bytes(rng.bytes(40), "little") % R for _ in range(pairs)] for _ in range(count)]
    h = env.ctx.g2_lines_prepare(world.q_words[:pairs])
    try:
        pts = env.ctx.g1_fixed_base_mul(pm.fr_words([x for row in a for x in row]))
        master = to_device(env, pts)
        env.ctx.sync()

        def body(inputs, outs):
            env.ctx.pairing_product_wave_device(h, inputs[0].data_ptr(), count, outs[0].data_ptr(), outs[1].data_ptr())
            inputs[0].zero_()
            return [outs[0].clone(), outs[1].clone(), inputs[0].clone()]
        values, status, zeroed = unsynchronised(env, [master], [count * 384, count * 4], body)
        assert not zeroed.any(), "the input was not overwritten"
        want = np.stack([pm.f12_words(world.table.pow(sum(x * b for x, b in zip(row, B)) % R)) for row in a])
        assert np.array_equal(np.ascontiguousarray(values).view(np.uint64).reshape(count, 48), want), "the values of the ORIGINAL input"
        assert not np.ascontiguousarray(status).view(np.uint32).any()
    finally:
        env.ctx.sync()
        h.free()
        env.ctx.close()
