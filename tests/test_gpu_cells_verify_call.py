"""The verdict on a batch of cell proofs in one call on the MI355X (bbg_cells_verify*, csrc/cells_verify.hip): the reduction, the packed
pair [L, -R], the wave pairing at count 1 and the status word, queued with no host round trip.

Batches are built as in tests/test_gpu_pairing.py::test_cell_proofs_end_to_end -- a powers string, two polynomials, every cell of both,
proofs by bbg_open_all, commitments by bbg_msm -- and every status is also held to the verdict of the two-step route the call replaces:
bbg_cells_verify_reduce, the negation of R on the host, bbg_pairing_product (the lane form)."""
import ctypes

import numpy as np
import pytest

import coarse_inputs as ci
import pairing_model as pm
from stream_order import Env, to_device, unsynchronised

pytestmark = pytest.mark.gpu

R, P = pm.R, pm.P
SEED = 0xBB254 + 0xCE115
X_INT = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % R
GUARD32 = 0xA5A5A5A5
SHAPES = [(6, 2), (8, 4), (5, 0)]


def negated(point):
    """-P of one affine point in Montgomery words; infinity stays."""
    p = pm.g1_from_words(point)
    return pm.g1_words(None if p is None else (p[0], -p[1] % P))


def g2_pair(ctx, l):
    """The words of ([x^l]_2, [1]_2)."""
    return np.stack([ctx.g2_mul(pm.fr_words([pow(X_INT, l, R)]))[0], pm.g2_words(pm.G2)])


class Case:
    """One shape: the string, the line handles, an honest batch and one of degree below l, made once and shared by the tests of the shape."""

    def __init__(self, bbg, lg, lc):
        self.bbg, self.lg, self.lc = bbg, lg, lc
        self.n, self.l, self.r = 1 << lg, 1 << lc, 1 << (lg - lc)
        rng = np.random.default_rng(SEED + 16 * lg + lc)
        self.srs = bbg.srs_synth_powers(pm.fr_words([X_INT])[0], self.n)
        self.opener = bbg.open_all_prepare(self.srs, lg, lc)
        self.lines = bbg.g2_lines_prepare(g2_pair(bbg, self.l))
        self.rho = pm.fr_words([int.from_bytes(rng.bytes(40), "little") % R])[0]
        self.honest = self.batch([[int.from_bytes(rng.bytes(40), "little") % R for _ in range(self.n)] for _ in range(2)])
        self.low = self.batch([[int.from_bytes(rng.bytes(40), "little") % R for _ in range(self.l)] + [0] * (self.n - self.l) for _ in range(2)])

    def batch(self, polys):
        """(commitments, commitment ids, cell ids, values (K l, 4), proofs (K, 8)): every cell of every polynomial, cell-major."""
        bbg, lg, lc, r, l = self.bbg, self.lg, self.lc, self.r, self.l
        words = [pm.fr_words(f) for f in polys]
        proofs = np.stack([self.opener.open(w) for w in words])
        commitments = bbg.g1_normalize(np.stack([bbg.msm(self.srs, w) for w in words]))
        values = np.stack([(bbg.cells_values(w, lg, lc) if lc else bbg.ntt(w)).reshape(r, l, 4) for w in words])
        cells = [(c, m) for m in range(r) for c in range(len(polys))]
        cids, mids = [c for c, _ in cells], [m for _, m in cells]
        return commitments, cids, mids, np.stack([values[c, m] for c, m in cells]).reshape(-1, 4), np.stack([proofs[c, m] for c, m in cells])

    def one_call(self, b):
        return self.bbg.cells_verify(self.srs, self.lines, self.lg, self.lc, b[0], b[1], b[2], b[3], b[4], self.rho)

    def two_step(self, b):
        L, R_ = self.bbg.cells_verify_reduce(self.srs, self.lg, self.lc, b[0], b[1], b[2], b[3], b[4], self.rho)
        _, status = self.bbg.pairing_product(self.lines, np.stack([L, negated(R_)]), want_values=False)
        return int(status[0]), L, R_

    def free(self):
        self.lines.free()
        self.opener.free()
        self.srs.free()


@pytest.fixture(scope="module")
def cases(bbg):
    """shape -> its Case, made on first use."""
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Case(bbg, *shape)
        return made[shape]
    yield get
    for c in made.values():
        c.free()


@pytest.fixture(params=SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def case(cases, request):
    return cases(request.param)


@pytest.fixture
def first(cases):
    """The tests that do not depend on the shape run on the first one."""
    return cases(SHAPES[0])


def changed(b, **kw):
    names = ["com", "cids", "mids", "values", "proofs"]
    return tuple(kw.get(k, v) for k, v in zip(names, b))


# 1 ------------------------------------------------------------------------------------------------ the verdicts
def test_verdicts(case):
    b = case.honest
    l, r = case.l, case.r
    assert case.one_call(b) == 1 and case.two_step(b)[0] == 1, "the honest batch"
    v2 = b[3].copy()
    v2[3 * l + l - 1] = pm.fr_words([12345])[0]
    p2 = b[4].copy()
    p2[[0, 1]] = p2[[1, 0]]
    m2 = list(b[2])
    m2[2] = (m2[2] + 1) % r
    for what, wrong in (("one value changed", changed(b, values=v2)), ("two proofs swapped", changed(b, proofs=p2)), ("a wrong cell id", changed(b, mids=m2))):
        assert case.one_call(wrong) == 0, what
        assert case.two_step(wrong)[0] == 0, what + ": the two-step route"
    # every polynomial of degree below l: no proof is finite, L = R = infinity, and the check holds
    ok, L, R_ = case.two_step(case.low)
    assert int(L[3]) >> 63 and int(R_[3]) >> 63 and ok == 1
    assert case.one_call(case.low) == 1, "degree below l"
    assert case.one_call(b) == 1, "the honest batch again, behind the others"


def test_device_form_and_the_off_curve_status(case, pkg):
    bbg = case.bbg
    com, cids, mids, values, proofs = case.honest
    bad = proofs.copy()
    bad[1, 4:] = ci.add_int(bad[1, 4:], 1)[0]  # y + 1
    d_com, d_val, d_prf, d_st = bbg.dev_alloc(com.nbytes), bbg.dev_alloc(values.nbytes), bbg.dev_alloc(proofs.nbytes), bbg.dev_alloc(12)
    try:
        bbg.dev_upload(d_com, com)
        bbg.dev_upload(d_val, values)
        bbg.dev_upload(d_st, np.full(3, GUARD32, dtype=np.uint32))
        for prf, want in ((proofs, 1), (bad, 2), (proofs, 1)):
            bbg.dev_upload(d_prf, prf)
            bbg.cells_verify_device(case.srs, case.lines, case.lg, case.lc, d_com, com.shape[0], cids, mids, d_val, d_prf, case.rho, d_st + 4)
            assert list(bbg.dev_download(d_st, (3,), dtype=np.uint32)) == [GUARD32, want, GUARD32]
    finally:
        for d in (d_com, d_val, d_prf, d_st):
            bbg.dev_free(d)
    status = ctypes.c_uint32(GUARD32)
    c32, m32 = np.asarray(cids, dtype=np.uint32), np.asarray(mids, dtype=np.uint32)
    rc = bbg.lib.bbg_cells_verify(bbg.ctx, case.srs.handle, case.lines.handle, case.lg, case.lc, com.ctypes.data, com.shape[0], c32.ctypes.data, m32.ctypes.data,
                                  len(mids), values.ctypes.data, bad.ctypes.data, case.rho.ctypes.data, ctypes.byref(status))
    assert rc == -1 and status.value == 2 and b"not on the curve" in bbg.lib.bbg_last_error(), "the host form: BBG_E_INVALID with the status written"
    with pytest.raises(pkg.BbgError):
        case.one_call(changed(case.honest, proofs=bad))


# 2 ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(bbg, first):
    case = first
    com, cids, mids, values, proofs = case.honest
    K = len(mids)
    c32, m32 = np.asarray(cids, dtype=np.uint32), np.asarray(mids, dtype=np.uint32)
    q = g2_pair(bbg, case.l)
    one, three = bbg.g2_lines_prepare(q[:1]), bbg.g2_lines_prepare(np.stack([q[0], q[1], q[1]]))
    d_com, d_val, d_prf, d_st = bbg.dev_alloc(com.nbytes), bbg.dev_alloc(values.nbytes), bbg.dev_alloc(proofs.nbytes), bbg.dev_alloc(4)
    lib = bbg.lib
    try:
        for d, a in ((d_com, com), (d_val, values), (d_prf, proofs), (d_st, np.full(1, GUARD32, dtype=np.uint32))):
            bbg.dev_upload(d, a)
        bad_m = m32.copy()
        bad_m[0] = case.r

        def device(lines=case.lines.handle, srs=case.srs.handle, k=K, mi=m32, dv=d_val, ds=d_st, ncom=2, lg=case.lg):
            return lib.bbg_cells_verify_device(bbg.ctx, srs, lines, lg, case.lc, d_com, ncom, c32.ctypes.data, mi.ctypes.data, k, dv, d_prf, case.rho.ctypes.data, ds)

        def host(status, lines=case.lines.handle, k=K, mi=m32, vv=values.ctypes.data):
            return lib.bbg_cells_verify(bbg.ctx, case.srs.handle, lines, case.lg, case.lc, com.ctypes.data, 2, c32.ctypes.data, mi.ctypes.data, k, vv,
                                        proofs.ctypes.data, case.rho.ctypes.data, status)
        refused = {"a one-pair handle": dict(lines=one.handle), "a three-pair handle": dict(lines=three.handle), "a null handle": dict(lines=None),
                   "a null SRS": dict(srs=None), "K = 0": dict(k=0), "a cell id out of range": dict(mi=bad_m), "null values": dict(dv=None),
                   "a null status": dict(ds=None), "ncom = 0": dict(ncom=0), "log2n = 0": dict(lg=0), "the status on the values": dict(ds=d_val + 8)}
        for what, kw in refused.items():
            assert device(**kw) == -1 and lib.bbg_last_error(), what
        assert device(lines=three.handle) == -1 and b"exactly two points" in lib.bbg_last_error()
        status = ctypes.c_uint32(GUARD32)
        for what, kw in {"a one-pair handle": dict(lines=one.handle), "a three-pair handle": dict(lines=three.handle), "a null handle": dict(lines=None),
                         "K = 0": dict(k=0), "a cell id out of range": dict(mi=bad_m), "null values": dict(vv=None)}.items():
            assert host(ctypes.byref(status), **kw) == -1 and status.value == GUARD32, what
        assert host(None) == -1
        bbg.sync()
        assert int(bbg.dev_download(d_st, (1,), dtype=np.uint32)[0]) == GUARD32, "a refused call wrote the status word"
        assert np.array_equal(bbg.dev_download(d_val, values.shape), values), "a refused call wrote an input"
        assert device() == 0 and int(bbg.dev_download(d_st, (1,), dtype=np.uint32)[0]) == 1, "the legal call right after"
    finally:
        one.free()
        three.free()
        for d in (d_com, d_val, d_prf, d_st):
            bbg.dev_free(d)


# 3 ------------------------------------------------------------------------------------------------ stream order
def test_back_to_back_calls_keep_their_own_status(bbg, first):
    """Two calls with different batches and ONE synchronisation.  They share the context's 512 bytes of intermediates; what include/bbg.h
    documents is stream order over those plus a status destination per call, so each word must hold its own call's verdict."""
    case = first
    com, cids, mids, values, proofs = case.honest
    wrong = values.copy()
    wrong[0] = pm.fr_words([777])[0]
    d_com, d_prf, d_st = bbg.dev_alloc(com.nbytes), bbg.dev_alloc(proofs.nbytes), bbg.dev_alloc(16)
    d_good, d_wrong = bbg.dev_alloc(values.nbytes), bbg.dev_alloc(values.nbytes)
    try:
        for d, a in ((d_com, com), (d_prf, proofs), (d_good, values), (d_wrong, wrong), (d_st, np.full(4, GUARD32, dtype=np.uint32))):
            bbg.dev_upload(d, a)
        bbg.sync()
        for k, d_val in enumerate((d_good, d_wrong, d_good)):
            bbg.cells_verify_device(case.srs, case.lines, case.lg, case.lc, d_com, 2, cids, mids, d_val, d_prf, case.rho, d_st + 4 * k)
        bbg.sync()
        assert list(bbg.dev_download(d_st, (4,), dtype=np.uint32)) == [1, 0, 1, GUARD32]
    finally:
        for d in (d_com, d_prf, d_st, d_good, d_wrong):
            bbg.dev_free(d)


def test_device_form_is_ordered_on_the_callers_stream(pkg, first):
    """Under the discipline of tests/test_gpu_stream_order.py: a context of its own on a non-blocking stream, two passes, values and proofs
    zeroed on the stream right behind the call, the snapshot taken on the stream, one synchronisation of that stream."""
    import torch
    case = first
    env = Env()
    env.torch, env.ctx, env.s = torch, pkg.Bbg(0), torch.cuda.Stream()
    assert env.s.cuda_stream != 0
    env.ctx.set_stream(env.s.cuda_stream)
    com, cids, mids, values, proofs = case.honest
    srs = env.ctx.srs_synth_powers(pm.fr_words([X_INT])[0], case.n)
    lines = env.ctx.g2_lines_prepare(g2_pair(env.ctx, case.l))
    try:
        masters = [to_device(env, a) for a in (com, values, proofs)]
        env.ctx.sync()

        def body(inputs, outs):
            env.ctx.cells_verify_device(srs, lines, case.lg, case.lc, inputs[0].data_ptr(), 2, cids, mids, inputs[1].data_ptr(), inputs[2].data_ptr(), case.rho,
                                        outs[0].data_ptr())
            inputs[1].zero_()
            inputs[2].zero_()
            return [outs[0].clone(), inputs[1].clone(), inputs[2].clone()]
        status, zeroed_v, zeroed_p = unsynchronised(env, masters, [4], body)
        assert not zeroed_v.any() and not zeroed_p.any(), "the inputs were not overwritten"
        assert int(np.ascontiguousarray(status).view(np.uint32)[0]) == 1, "the verdict on the ORIGINAL inputs"
    finally:
        env.ctx.sync()
        lines.free()
        srs.free()
        env.ctx.close()
