"""What tests/test_gpu_stream_order.py and tests/test_gpu_stream_order_device.py share: a context of its own on a caller's non-blocking
stream, and the one way an unsynchronised section is run (poison, queue, snapshot on the stream, synchronise the stream once, compare the
snapshot on the host).  The discipline itself is stated in the docstring of tests/test_gpu_stream_order.py."""
import contextlib

import numpy as np
import pytest

SRS_SEED = 0xBB254
N16 = 1 << 16
N_TINY = 4096  # the 8-bit-window path of csrc/msm_tiny.hip, which has its own copy of the slot and event code
POISON = 0x5A
SEED_K = 0x57A5
DEFAULTS = {"msm_async_reduce": 0, "msm_window": 0, "ecntt_mul": 1, "poly_limbs29": 1}


class Env:
    pass


@pytest.fixture(scope="module")
def env(pkg, oracle):
    """A context of its own on an ordinary non-blocking torch stream (the session-wide `bbg` fixture stays on torch's current stream), a
    hashed SRS of 2^16 points and its points for the oracle."""
    import torch
    e = Env()
    e.torch, e.pkg, e.oracle = torch, pkg, oracle
    e.ctx = pkg.Bbg(0)
    e.s = torch.cuda.Stream()
    assert e.s.cuda_stream != 0, "torch.cuda.Stream() must be a stream of its own, not the null stream"
    e.ctx.set_stream(e.s.cuda_stream)
    e.srs = e.ctx.srs_synth_hashed(SRS_SEED, N16)
    e.pts = e.srs.read()
    e.want = {}
    # The automatic width of a short MSM over a long SRS is the nearest width that already has window tables (msm_choose in csrc/msm.hip),
    # so the 8-bit tables are built once here: from then on 4096 and 1000 terms take msm_tiny.hip at the automatic width.
    e.ctx.set_option("msm_window", 8)
    try:
        e.ctx.msm(e.srs, pkg.synthetic_scalars(SEED_K, 64))
    finally:
        e.ctx.set_option("msm_window", 0)
    assert e.ctx.msm_plan(N_TINY, e.srs)[0] == 8 and e.ctx.msm_plan(1000, e.srs)[0] == 8
    assert e.ctx.msm_plan(N16, e.srs)[0] == 16
    yield e
    e.ctx.sync()
    e.srs.free()
    e.ctx.close()


@contextlib.contextmanager
def options(env, **kv):
    """Options are set before an unsynchronised section and restored after it ("msm_async_reduce" synchronises the device)."""
    for k, v in kv.items():
        env.ctx.set_option(k, v)
    try:
        yield
    finally:
        for k in kv:
            env.ctx.set_option(k, DEFAULTS[k])


def to_device(env, a):
    with env.torch.cuda.stream(env.s):
        return env.torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).cuda()


def poisoned(env, nbytes):
    return env.torch.full((nbytes,), POISON, dtype=env.torch.uint8, device="cuda")


def affine(env, snap):
    """Host bytes of k Jacobian results -> (k, 8) canonical affine points."""
    j = np.ascontiguousarray(snap).view(np.uint64).reshape(-1, 12)
    return np.stack([env.oracle.jac_to_affine(p) for p in j])


def words(snap, last):
    return np.ascontiguousarray(snap).view(np.uint64).reshape(-1, last)


def unsynchronised(env, masters, out_bytes, body, between=None, final_stream=None):
    """Runs body(inputs, outs) -> [snapshot tensors] on the context's stream: once into scratch buffers (first-use work, see the module
    docstring of tests/test_gpu_stream_order.py), then -- after a full synchronisation and the optional `between()` -- on poisoned result
    tensors; returns the snapshots as host arrays.  inputs: fresh device copies of `masters` per pass (a body may overwrite them); outs:
    one poisoned uint8 tensor per entry of out_bytes.  body must not synchronise the host; the only synchronisation after it is the
    stream's own."""
    torch = env.torch
    with torch.cuda.stream(env.s):
        body([m.clone() for m in masters], [poisoned(env, b) for b in out_bytes])
        env.ctx.sync()
        torch.cuda.synchronize()
        if between is not None:
            between()
        inputs = [m.clone() for m in masters]
        outs = [poisoned(env, b) for b in out_bytes]  # step 1
        snaps = body(inputs, outs)                    # steps 2 - 4
        (final_stream or env.s).synchronize()         # step 5
        return [t.cpu().numpy() for t in snaps]
