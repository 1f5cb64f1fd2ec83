"""Stream ordering of bbg_open_points_device, bbg_kzg_verify_reduce_device and bbg_kzg_verify_device on a caller's own non-blocking stream,
under the discipline of tests/test_gpu_stream_order.py (helpers: tests/tools/stream_order.py): a context of its own on that stream, two
passes per section with the first one into scratch buffers, results poisoned on the stream, the call's device inputs zeroed on the stream
right behind it, snapshots taken on the stream, ONE synchronisation of that stream, and only the snapshots compared.  Expectations are the
integer model's (tests/tools/open_points_cases.py); no output of the library serves as one.

Back-to-back sections queue two calls at different sizes, so that they share the opening workspace and the MSM arena, or the packed arrays,
the working memory of bbg_g1_msm and the context's 512 bytes of verdict intermediates.  Between the two passes of a verifier section the same
batch runs under another challenge, so that an intermediate read too early is a wrong value and not a left-over right one."""
import numpy as np
import pytest

import open_points_cases as oc
import open_points_model as om
import pairing_model as pm
from stream_order import Env, to_device, unsynchronised, words

pytestmark = pytest.mark.gpu

LG = 6
N = 1 << LG
SEED = 0xBB254 + 0x57E0


@pytest.fixture(scope="module")
def env(pkg, oracle):
    import torch
    e = Env()
    e.torch, e.pkg, e.oracle = torch, pkg, oracle
    e.ctx = pkg.Bbg(0)
    e.s = torch.cuda.Stream()
    assert e.s.cuda_stream != 0, "torch.cuda.Stream() must be a stream of its own, not the null stream"
    e.ctx.set_stream(e.s.cuda_stream)
    e.srs = e.ctx.srs_synth_powers(oc.X_WORDS, N)
    e.lag = e.srs.lagrange(LG)
    e.lines = e.ctx.g2_lines_prepare(np.stack([e.ctx.g2_mul(pm.fr_words([oc.X_INT]))[0], pm.g2_words(pm.G2)]))
    e.big = oc.Batch(oracle, LG, 9, SEED, on_domain={4: 11})   # a second launch set of the MSM, one polynomial on the domain
    e.small = oc.Batch(oracle, LG, 3, SEED + 1)
    rng = np.random.default_rng(SEED + 2)
    e.rho_int, e.rho2_int = oc.rand_fr(rng), oc.rand_fr(rng)
    e.rho, e.rho2 = pm.fr_words([e.rho_int])[0], pm.fr_words([e.rho2_int])[0]
    e.ctx.sync()
    yield e
    e.ctx.sync()
    e.lines.free()
    e.lag.free()
    e.srs.free()
    e.ctx.close()


def up(env, a):
    return to_device(env, np.array(a, dtype=np.uint64))


def consumed(inputs):
    """Zeroes the inputs on the stream and returns their snapshots."""
    for t in inputs:
        t.zero_()
    return [t.clone() for t in inputs]


def expected_lr(b, rho_int, y=None):
    l, r = om.kzg_closed_form(b.c, b.z, b.y if y is None else y, b.w, rho_int)
    return np.stack([oc.g1(l), oc.g1(r)])


def test_open_points_is_ordered_on_the_callers_stream(env):
    b = env.big
    masters = [up(env, b.evals), up(env, b.z_words)]

    def body(inputs, outs):
        env.ctx.open_points_device(env.lag, LG, inputs[0].data_ptr(), inputs[1].data_ptr(), b.count, outs[0].data_ptr(), outs[1].data_ptr())
        zeroed = consumed(inputs)
        return [outs[0].clone(), outs[1].clone()] + zeroed
    y, proofs, z0, z1 = unsynchronised(env, masters, [b.count * 32, b.count * 64], body)
    assert not z0.any() and not z1.any(), "the inputs were not overwritten"
    assert np.array_equal(words(y, 4), b.y_words), "y of the ORIGINAL inputs"
    assert np.array_equal(words(proofs, 8), b.proofs), "the proofs of the ORIGINAL inputs"


def test_two_open_points_calls_share_the_workspace(env):
    """Nine polynomials, then three, then values only: one workspace, one MSM arena, three calls and one synchronisation."""
    a, b = env.big, env.small
    masters = [up(env, a.evals), up(env, a.z_words), up(env, b.evals), up(env, b.z_words)]

    def body(inputs, outs):
        env.ctx.open_points_device(env.lag, LG, inputs[0].data_ptr(), inputs[1].data_ptr(), a.count, outs[0].data_ptr(), outs[1].data_ptr())
        env.ctx.open_points_device(env.lag, LG, inputs[2].data_ptr(), inputs[3].data_ptr(), b.count, outs[2].data_ptr(), outs[3].data_ptr())
        env.ctx.open_points_device(None, LG, inputs[0].data_ptr(), inputs[1].data_ptr(), a.count, outs[4].data_ptr(), None)
        consumed(inputs)
        return [o.clone() for o in outs]
    ya, pa, yb, pb, ya2 = unsynchronised(env, masters, [a.count * 32, a.count * 64, b.count * 32, b.count * 64, a.count * 32], body)
    assert np.array_equal(words(ya, 4), a.y_words) and np.array_equal(words(pa, 8), a.proofs), "the first call"
    assert np.array_equal(words(yb, 4), b.y_words) and np.array_equal(words(pb, 8), b.proofs), "the second call"
    assert np.array_equal(words(ya2, 4), a.y_words), "the evaluation behind them"


def another_challenge(env, b):
    """Between the passes: the same batch under rho2, so that the packed scalars, L and R left behind differ from the checked call's."""
    def run():
        env.ctx.kzg_verify_reduce(b.commitments, b.z_words, b.y_words, b.proofs, env.rho2)
    return run


def test_kzg_verify_reduce_is_ordered_on_the_callers_stream(env):
    b = env.big
    masters = [up(env, a) for a in (b.commitments, b.z_words, b.y_words, b.proofs)]

    def body(inputs, outs):
        p = [t.data_ptr() for t in inputs]
        env.ctx.kzg_verify_reduce_device(p[0], p[1], p[2], p[3], b.count, env.rho, outs[0].data_ptr(), outs[1].data_ptr())
        zeroed = consumed(inputs)
        return [outs[0].clone(), outs[1].clone()] + zeroed
    got = unsynchronised(env, masters, [128, 4], body, between=another_challenge(env, b))
    assert all(not z.any() for z in got[2:]), "the inputs were not overwritten"
    assert np.array_equal(words(got[0], 8), expected_lr(b, env.rho_int)), "L and R of the ORIGINAL inputs"
    assert int(np.ascontiguousarray(got[1]).view(np.uint32)[0]) == 0, "no point off the curve"


def test_two_kzg_verify_calls_share_the_context(env):
    """A valid batch of nine, an invalid one of three, a reduction of the nine: each verdict in its own word, L and R of the third call."""
    a, b = env.big, env.small
    wrong_y = b.y_words.copy()
    wrong_y[1] = pm.fr_words([31337])[0]
    masters = [up(env, x) for x in (a.commitments, a.z_words, a.y_words, a.proofs, b.commitments, b.z_words, wrong_y, b.proofs)]

    def body(inputs, outs):
        p = [t.data_ptr() for t in inputs]
        env.ctx.kzg_verify_device(env.lines, p[0], p[1], p[2], p[3], a.count, env.rho, outs[0].data_ptr())
        env.ctx.kzg_verify_device(env.lines, p[4], p[5], p[6], p[7], b.count, env.rho, outs[1].data_ptr())
        env.ctx.kzg_verify_reduce_device(p[0], p[1], p[2], p[3], a.count, env.rho, outs[2].data_ptr(), None)
        consumed(inputs)
        return [o.clone() for o in outs]
    first, second, lr = unsynchronised(env, masters, [4, 4, 128], body, between=another_challenge(env, a))
    assert int(np.ascontiguousarray(first).view(np.uint32)[0]) == 1, "the valid batch"
    assert int(np.ascontiguousarray(second).view(np.uint32)[0]) == 0, "the invalid batch behind it"
    assert np.array_equal(words(lr, 8), expected_lr(a, env.rho_int)), "the reduction behind both"
