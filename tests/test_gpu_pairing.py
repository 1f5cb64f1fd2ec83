"""G2 and batched pairing product checks on the MI355X (bbg_g2_mul, bbg_g2_lines_*, bbg_pairing_product*, csrc/pairing.hip).

Every comparison is bit-exact on canonical Montgomery words against the integer model (tests/tools/pairing_model.py, itself held to the
reference's known-answer test by tests/test_pairing_cpu.py).  Inputs are designed so that expectations are cheap: P_ij = [a_ij] G made by
bbg_g1_fixed_base_mul, Q_j = [b_j] G2 made by bbg_g2_mul, so that product i is g^(sum_j a_ij b_j mod r) with g = e(G, G2): one model
pairing once, then one exponentiation per product.  The last test is the one the feature exists for: cell proofs made, reduced and then
CHECKED by the library alone, against [x^l]_2."""
import ctypes

import numpy as np
import pytest

import coarse_inputs as ci
import pairing_model as pm
from stream_order import Env, to_device, unsynchronised

pytestmark = pytest.mark.gpu

R, P = pm.R, pm.P
SEED = 0xBB254 + 0x9A121
GUARD = 0xA5A5A5A5A5A5A5A5
B = [0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % R, 3, R - 5, 0x0123456789ABCDEF << 130,
     0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R, 1, 0xFFFFFFFFFFFFFFFF, R - 1]  # Q_j = [B[j]] G2
X_INT = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % R


@pytest.fixture(scope="module")
def world(bbg):
    """g = e(G, G2) and its power table; Q_j by the device, held to the model once; line handles per pair count, made on first use."""
    w = Env()
    w.g = pm.reduced_ate_pairing(pm.G1, pm.G2)
    w.table = pm.PowerTable(w.g)
    w.q_words = bbg.g2_mul(pm.fr_words(B))
    w.q = [pm.g2_mul(pm.G2, b) for b in B]
    assert np.array_equal(w.q_words, np.stack([pm.g2_words(q) for q in w.q])), "bbg_g2_mul differs from the model on the test's own G2 points"
    w.model_lines = {}
    handles = {}

    def lines(pairs):
        if pairs not in handles:
            handles[pairs] = bbg.g2_lines_prepare(w.q_words[:pairs])
        return handles[pairs]

    def model_lines(j):
        if j not in w.model_lines:
            w.model_lines[j] = pm.precompute_miller_lines(w.q[j])
        return w.model_lines[j]
    w.lines, w.lines_of = lines, model_lines
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


def negated(point):
    """-P of one affine point in Montgomery words; infinity stays."""
    p = pm.g1_from_words(point)
    return pm.g1_words(None if p is None else (p[0], -p[1] % P))


# 1 ------------------------------------------------------------------------------------------------ bbg_g2_mul
def test_g2_mul_edges(bbg, pkg):
    scalars = [0, 1, 2, R - 1, 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, 1 << 253]
    want = np.stack([pm.g2_words(pm.g2_mul(pm.G2, s)) for s in scalars])
    assert np.array_equal(bbg.g2_mul(pm.fr_words(scalars)), want), "canonical scalars on the generator"
    assert np.array_equal(want[0], pm.G2_INFINITY_WORDS) and np.array_equal(want[1], pm.g2_words(pm.G2))
    # the representatives in [r, 2r): r itself (0 + r), r + 1, and the rest lifted
    lift = pm.fr_words(scalars, lift=1)
    assert ci.below(lift, 2 * R).all() and not ci.below(lift, R).any()
    assert np.array_equal(bbg.g2_mul(lift), want), "scalars in [r, 2r)"
    # another base, also with coordinates in [p, 2p); an infinite base
    base = pm.g2_mul(pm.G2, 0xC0FFEE)
    want = np.stack([pm.g2_words(pm.g2_mul(base, s)) for s in scalars])
    assert np.array_equal(bbg.g2_mul(pm.fr_words(scalars), pm.g2_words(base)), want), "a base other than the generator"
    assert np.array_equal(bbg.g2_mul(lift, ci.add_int(pm.g2_words(base).reshape(4, 4), P).reshape(16)), want), "its coordinates in [p, 2p)"
    assert np.array_equal(bbg.g2_mul(pm.fr_words([5]), pm.G2_INFINITY_WORDS)[0], pm.G2_INFINITY_WORDS), "an infinite base"
    # a point of the twist outside the subgroup is a legal base: [r] Q is finite there
    outside = pm.g2_point_outside_subgroup()
    assert np.array_equal(bbg.g2_mul(pm.fr_words([7]), pm.g2_words(outside))[0], pm.g2_words(pm.g2_mul(outside, 7)))
    # off the twist: refused, out untouched (n = 0 included); n above 2^16
    bad = pm.g2_words((base[0], pm.f2_add(base[1], (1, 0))))
    out = np.full((2, 16), GUARD, dtype=np.uint64)
    sc = pm.fr_words([1, 2])
    assert bbg.lib.bbg_g2_mul(bbg.ctx, bad.ctypes.data, sc.ctypes.data, 2, out.ctypes.data) == -1 and b"twist" in bbg.lib.bbg_last_error()
    assert bbg.lib.bbg_g2_mul(bbg.ctx, bad.ctypes.data, None, 0, None) == -1
    assert bbg.lib.bbg_g2_mul(bbg.ctx, None, sc.ctypes.data, (1 << 16) + 1, out.ctypes.data) == -1
    assert bbg.lib.bbg_g2_mul(bbg.ctx, None, None, 2, out.ctypes.data) == -1 and bbg.lib.bbg_g2_mul(bbg.ctx, None, sc.ctypes.data, 2, None) == -1
    assert (out == GUARD).all()
    assert bbg.lib.bbg_g2_mul(bbg.ctx, None, None, 0, None) == 0, "n = 0 is legal"


# 2 ------------------------------------------------------------------------------------------------ the lines
def test_lines_read_is_the_model(bbg, world):
    other = pm.g2_mul(pm.G2, B[0])
    h = bbg.g2_lines_prepare(np.stack([pm.g2_words(pm.G2), ci.add_int(pm.g2_words(other).reshape(4, 4), P).reshape(16)]))
    try:
        assert h.pairs == 2
        assert np.array_equal(h.read(0), pm.lines_words(pm.precompute_miller_lines(pm.G2))), "the lines of the generator"
        assert np.array_equal(h.read(1), pm.lines_words(pm.precompute_miller_lines(other))), "the lines of another point, given in [p, 2p)"
        out = np.full(2088, GUARD, dtype=np.uint64)
        assert bbg.lib.bbg_g2_lines_read(h.handle, 2, out.ctypes.data) == -1 and (out == GUARD).all()
    finally:
        h.free()


def test_prepare_refuses_bad_points(bbg):
    good = pm.g2_words(pm.G2)
    off = pm.g2_words((pm.G2[0], pm.f2_add(pm.G2[1], (0, 1))))
    outside = pm.g2_point_outside_subgroup()
    assert pm.g2_on_twist(outside) and pm.g2_mul(outside, R) is not None
    sentinel = 0x1234
    for what, bad, needle in (("infinity", pm.G2_INFINITY_WORDS, b"infinity"), ("off the twist", off, b"twist"),
                              ("outside the subgroup", pm.g2_words(outside), b"subgroup")):
        for pts in (np.stack([bad]), np.stack([good, bad]), np.stack([bad, good, good])):
            h = ctypes.c_void_p(sentinel)
            assert bbg.lib.bbg_g2_lines_prepare(bbg.ctx, pts.ctypes.data, pts.shape[0], ctypes.byref(h)) == -1, what
            assert needle in bbg.lib.bbg_last_error() and h.value == sentinel, what
    h = ctypes.c_void_p(sentinel)
    nine = np.stack([good] * 9)
    for pts, pairs in ((nine, 0), (nine, 9), (None, 1)):
        assert bbg.lib.bbg_g2_lines_prepare(bbg.ctx, None if pts is None else pts.ctypes.data, pairs, ctypes.byref(h)) == -1 and h.value == sentinel
    assert bbg.lib.bbg_g2_lines_prepare(bbg.ctx, nine.ctypes.data, 1, None) == -1
    assert bbg.lib.bbg_g2_lines_pairs(None, None) == -1


# 3 ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("pairs", [1, 2, 3, 8])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_values(bbg, world, count, pairs):
    rng = np.random.default_rng(SEED + 1000 * count + pairs)
    a = [[int.from_bytes(rng.bytes(40), "little") % R for _ in range(pairs)] for _ in range(count)]
    pts = g1_points(bbg, [x for row in a for x in row]).reshape(count, pairs, 8)
    pts[1::2] = lifted(pts[1::2]).reshape(-1, pairs, 8)  # every second product with its coordinates in [p, 2p)
    values, status = bbg.pairing_product(world.lines(pairs), pts.reshape(-1, 8))
    assert not status.any(), "a random product is not one"
    want = np.stack([pm.f12_words(world.table.pow(sum(x * b for x, b in zip(row, B)) % R)) for row in a])
    bad = np.flatnonzero((values != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {count} products differ from g^(sum a b), first at {bad[:8]}"
    for i in sorted({0, count // 2, count - 1}):
        model = pm.reduced_ate_pairing_batch_precomputed([pm.g1_mul(pm.G1, x) for x in a[i]], [world.lines_of(j) for j in range(pairs)])
        assert np.array_equal(values[i], pm.f12_words(model)), f"product {i} differs from the full model"


# 4 ------------------------------------------------------------------------------------------------ status
def test_status_words(bbg, pkg, world):
    a, b = 0x1234567890ABCDEF1234567890ABCDEF % R, B[0]
    q = world.q_words[0]
    h = bbg.g2_lines_prepare(np.stack([q, q]))
    try:
        pa, pna, pna1 = g1_points(bbg, [a, R - a, R - a + 1])
        inf = pm.G1_INFINITY_WORDS
        products = [(pa, pna), (pa, pna1), (inf, pa), (inf, inf), (pna, pa)]
        expo = [0, b, a * b % R, 0, 0]
        pts = np.stack([p for pair in products for p in pair])
        values, status = bbg.pairing_product(h, pts)
        assert list(status) == [1, 0, 0, 1, 1]
        assert np.array_equal(values, np.stack([pm.f12_words(world.table.pow(e)) for e in expo]))
        assert np.array_equal(values[3], pm.f12_words(pm.F12_ONE)), "every pair at infinity: the Fq12 one"
        _, only_status = bbg.pairing_product(h, pts, want_values=False)
        assert list(only_status) == [1, 0, 0, 1, 1]
        # an off-curve point in product 2: status 2 there, every other product as before; the host form says BBG_E_INVALID
        bad = pts.copy()
        bad[5, 4:] = ci.add_int(bad[5, 4:], 1)[0]  # y + 1
        d_in, d_out, d_st = bbg.dev_alloc(bad.nbytes), bbg.dev_alloc(5 * 384), bbg.dev_alloc(5 * 4)
        try:
            bbg.dev_upload(d_in, bad)
            bbg.pairing_product_device(h, d_in, 5, d_out, d_st)
            got_st = bbg.dev_download(d_st, (5,), dtype=np.uint32)
            got = bbg.dev_download(d_out, (5, 48))
            assert list(got_st) == [1, 0, 2, 1, 1]
            keep = [0, 1, 3, 4]
            assert np.array_equal(got[keep], values[keep]), "the other products are not affected"
            # the honest batch right after it
            bbg.dev_upload(d_in, pts)
            bbg.pairing_product_device(h, d_in, 5, d_out, d_st)
            assert list(bbg.dev_download(d_st, (5,), dtype=np.uint32)) == [1, 0, 0, 1, 1] and np.array_equal(bbg.dev_download(d_out, (5, 48)), values)
        finally:
            for d in (d_in, d_out, d_st):
                bbg.dev_free(d)
        st = np.zeros(5, dtype=np.uint32)
        assert bbg.lib.bbg_pairing_product(bbg.ctx, h.handle, bad.ctypes.data, 5, None, st.ctypes.data) == -1 and b"not on the curve" in bbg.lib.bbg_last_error()
        assert list(st) == [1, 0, 2, 1, 1], "the host form reports which product it was"
        with pytest.raises(pkg.BbgError):
            bbg.pairing_product(h, bad)
    finally:
        h.free()


# 5 ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(bbg, world):
    import torch
    pairs, count = 2, 3
    h = world.lines(pairs)
    pts = g1_points(bbg, [1, 2, 3, 4, 5, 6])
    d_in, d_out = bbg.dev_alloc(pts.nbytes), bbg.dev_alloc(count * 388 + 64)
    d_st = d_out + count * 384
    guard = np.full((count * 388 + 64) // 4, 0xA5A5A5A5, dtype=np.uint32)
    lib = bbg.lib

    def call(ctx=None, hh=h.handle, di=d_in, n=count, do=d_out, ds=d_st, null_ctx=False):
        return lib.bbg_pairing_product_device(None if null_ctx else bbg.ctx, hh, di, n, do, ds)

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
            assert lib.bbg_pairing_product(bbg.ctx, args["hh"], args["pp"], args["n"], args["v"], args["s"]) == -1
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
        # the neighbours are legal: the status right behind the values, one output alone, the working memory back after a trim
        before = bbg.memory_report()["scratch"]
        assert call() == 0 and call(do=None) == 0 and call(ds=None) == 0
        assert bbg.memory_report()["scratch"] >= before and bbg.memory_trim() > 0
        assert call() == 0
        got = bbg.dev_download(d_out, guard.shape, dtype=np.uint32)
        want = np.stack([pm.f12_words(world.table.pow((a * B[0] + b * B[1]) % R)) for a, b in ((1, 2), (3, 4), (5, 6))])
        assert np.array_equal(got[:count * 96].view(np.uint64).reshape(count, 48), want) and not got[count * 96:count * 97].any()
        assert (got[count * 97:] == 0xA5A5A5A5).all(), "the words behind the status"
    finally:
        bbg.dev_free(d_in)
        bbg.dev_free(d_out)


# 6 ------------------------------------------------------------------------------------------------ the device form on the caller's stream
def test_device_form_is_ordered_on_the_callers_stream(pkg, world):
    """Under the discipline of tests/test_gpu_stream_order.py: a context of its own on a non-blocking stream, two passes, the input zeroed on
    the stream right behind the call, the snapshot taken on the stream, one synchronisation of that stream."""
    import torch
    env = Env()
    env.torch, env.ctx, env.s = torch, pkg.Bbg(0), torch.cuda.Stream()
    assert env.s.cuda_stream != 0
    env.ctx.set_stream(env.s.cuda_stream)
    pairs, count = 2, 130
    rng = np.random.default_rng(SEED + 6)
    a = [[int.from_bytes(rng.bytes(40), "little") % R for _ in range(pairs)] for _ in range(count)]
    h = env.ctx.g2_lines_prepare(world.q_words[:pairs])
    try:
        pts = env.ctx.g1_fixed_base_mul(pm.fr_words([x for row in a for x in row]))
        master = to_device(env, pts)
        env.ctx.sync()

        def body(inputs, outs):
            env.ctx.pairing_product_device(h, inputs[0].data_ptr(), count, outs[0].data_ptr(), outs[1].data_ptr())
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


# 7 ------------------------------------------------------------------------------------------------ end to end: cell proofs made, reduced AND checked here
@pytest.mark.parametrize("lg,lc", [(6, 2), (8, 4)])
def test_cell_proofs_end_to_end(bbg, world, lg, lc):
    n, l, r = 1 << lg, 1 << lc, 1 << (lg - lc)
    rng = np.random.default_rng(SEED + 16 * lg + lc)
    srs = bbg.srs_synth_powers(pm.fr_words([X_INT])[0], n)
    opener = bbg.open_all_prepare(srs, lg, lc)
    lines = bbg.g2_lines_prepare(np.stack([bbg.g2_mul(pm.fr_words([pow(X_INT, l, R)]))[0], pm.g2_words(pm.G2)]))
    rho = pm.fr_words([int.from_bytes(rng.bytes(40), "little") % R])[0]

    def verdict(commitments, cids, mids, values, proofs):
        L, R_ = bbg.cells_verify_reduce(srs, lg, lc, commitments, cids, mids, values, proofs, rho)
        _, status = bbg.pairing_product(lines, np.stack([L, negated(R_)]), want_values=False)
        return int(status[0]), L, R_

    def batch(polys):
        words = [pm.fr_words(f) for f in polys]
        proofs = np.stack([opener.open(w) for w in words])                                   # (polys, r, 8)
        commitments = bbg.g1_normalize(np.stack([bbg.msm(srs, w) for w in words]))           # (polys, 8)
        values = np.stack([bbg.cells_values(w, lg, lc).reshape(r, l, 4) for w in words])     # (polys, r, l, 4)
        cells = [(c, m) for m in range(r) for c in range(len(polys))]
        cids, mids = [c for c, _ in cells], [m for _, m in cells]
        return commitments, cids, mids, np.stack([values[c, m] for c, m in cells]), np.stack([proofs[c, m] for c, m in cells])

    try:
        polys = [[int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)] for _ in range(2)]
        com, cids, mids, values, proofs = batch(polys)
        ok, L, R_ = verdict(com, cids, mids, values.reshape(-1, 4), proofs)
        assert ok == 1 and int(L[3]) >> 63 == 0, "the honest batch"
        v2 = values.copy()
        v2[3, l - 1] = pm.fr_words([12345])[0]
        assert verdict(com, cids, mids, v2.reshape(-1, 4), proofs)[0] == 0, "one value changed"
        p2 = proofs.copy()
        p2[[0, 1]] = p2[[1, 0]]
        assert verdict(com, cids, mids, values.reshape(-1, 4), p2)[0] == 0, "two proofs swapped"
        m2 = list(mids)
        m2[2] = (m2[2] + 1) % r
        assert verdict(com, cids, m2, values.reshape(-1, 4), proofs)[0] == 0, "a wrong cell id"
        # every polynomial of degree below l: no proof is finite, L = R = infinity, and the check holds
        low = [[int.from_bytes(rng.bytes(40), "little") % R for _ in range(l)] + [0] * (n - l) for _ in range(2)]
        com, cids, mids, values, proofs = batch(low)
        ok, L, R_ = verdict(com, cids, mids, values.reshape(-1, 4), proofs)
        assert int(L[3]) >> 63 and int(R_[3]) >> 63 and ok == 1, "degree below l"
    finally:
        lines.free()
        opener.free()
        srs.free()
