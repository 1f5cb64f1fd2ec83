#!/usr/bin/env python3
"""Timings of bbg_cells_verify_reduce_device (csrc/cells_verify.hip) -- the table in profiles/cells_verify.txt, which this
script writes (--out PATH for another place; the lines are printed as well).

Per case (log2n, log2cell, ncom, K) -- default (13, 6) with ncom = 1 / 8 / 64 and K = 128 / 1024 / 8192, then (20, 6, 8, 2^14); other cases
as arguments `LOG2N:LOG2CELL:NCOM:K` -- in ONE process:
  * the call: one warm-up, then REPS calls on device-resident inputs, each on a host clock up to a stream synchronisation;
  * its scopes from bbg_profile_get (HIP events on the stream) over REPS further calls;
  * the yardstick: two bbg_g1_batch_mul_device calls over K points and one bbg_ntt_device (inverse) at n, queued together and timed the same
    way, interleaved with the calls; and the ratio of the medians.
Cells are a seeded random choice of (commitment, cell) pairs, duplicates as they fall.  Proofs and commitments are points on the curve (a
hashed string: the reduction costs the same for valid and invalid proofs), values and rho spread over [0, 2r).  Medians and minima."""
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as ge  # noqa: E402
import coarse_inputs as ci  # noqa: E402

REPS = 9
SEED = 0xBB254 + 0x7E81F
SCOPES = ("cells_verify_powers", "cells_verify_fold", "ntt_pass", "msm_recode", "msm_accumulate", "msm_reduce", "cells_verify_mul", "cells_verify_segsum",
          "cells_verify_phi", "cells_verify_finish")
DEFAULT = [(13, 6, ncom, K) for ncom in (1, 8, 64) for K in (128, 1024, 8192)] + [(20, 6, 8, 1 << 14)]


def med_min(v):
    return f"{statistics.median(v):10.3f} {min(v):10.3f}"


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "cells_verify.txt")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    cases = [tuple(int(v) for v in a.split(":")) for a in args] or DEFAULT
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# one process; per case one warm-up and {REPS} timed runs, calls and yardstick interleaved; every pair of columns is median and minimum")
    emit("# in ms.  call / yardstick = the whole thing on a host clock, up to a synchronisation; the scopes are bbg_profile_get's (HIP events on")
    emit("# the stream) over further calls.  yardstick = bbg_g1_batch_mul_device x 2 over K points + bbg_ntt_device (inverse) at n.")
    emit("log2n log2cell  ncom      K  what                             ms(med min)")
    kmax, cmax, lmax = max(c[3] for c in cases), max(c[2] for c in cases), 1 << max(c[1] for c in cases)
    string = bbg.srs_synth_hashed(SEED, lmax)
    pool = bbg.srs_synth_hashed(SEED + 1, kmax + cmax)  # points on the curve: the proofs, then the commitments
    points = pool.read()
    pool.free()
    rho = ci.coarse_scalars(SEED + 2, 1, 0)[0]
    for lg, lc, ncom, K in cases:
        n, l, r = 1 << lg, 1 << lc, 1 << (lg - lc)
        rng = np.random.default_rng(SEED + lg + ncom + K)
        cids, mids = rng.integers(0, ncom, K).astype(np.uint32), rng.integers(0, r, K).astype(np.uint32)
        d_com, d_prf, d_val, d_out = bbg.dev_alloc(ncom * 64), bbg.dev_alloc(K * 64), bbg.dev_alloc(K * l * 32), bbg.dev_alloc(128)
        d_y, d_ys, d_yo = bbg.dev_alloc(n * 32), bbg.dev_alloc(K * 32), bbg.dev_alloc(K * 64)
        bbg.dev_upload(d_prf, points[:K])
        bbg.dev_upload(d_com, points[kmax:kmax + ncom])
        bbg.dev_upload(d_val, ci.coarse_scalars(SEED + 3, K * l, 0))
        bbg.dev_upload(d_y, ci.coarse_scalars(SEED + 4, n, 0))
        bbg.dev_upload(d_ys, ci.coarse_scalars(SEED + 5, K, 0))

        def call():
            bbg.cells_verify_reduce_device(string, lg, lc, d_com, ncom, cids, mids, d_val, d_prf, rho, d_out)

        def yardstick():
            bbg.g1_batch_mul_device(d_prf, d_ys, K, d_yo)
            bbg.g1_batch_mul_device(d_prf, d_ys, K, d_yo)
            bbg.ntt_device(d_y, lg, pkg.binding.IFFT)

        def timed(fn):
            bbg.sync()
            t0 = time.perf_counter()
            fn()
            bbg.sync()
            return 1e3 * (time.perf_counter() - t0)

        for fn in (call, yardstick):  # warm-up: the domain, the working memory, the string's table
            fn()
        bbg.sync()
        wall = {"call": [], "yardstick": []}
        for _ in range(REPS):
            wall["call"].append(timed(call))
            wall["yardstick"].append(timed(yardstick))
        scopes = {s: [] for s in SCOPES}
        for _ in range(REPS):
            bbg.profile_enable(True)
            call()
            bbg.sync()
            for s in SCOPES:
                scopes[s].append(bbg.profile_get(s)[0])
            bbg.profile_enable(False)
        tag = f"{lg:5d} {lc:8d} {ncom:5d} {K:6d}  "
        emit(f"{tag}{'bbg_cells_verify_reduce_device':32s} {med_min(wall['call'])}")
        for s in SCOPES:
            emit(f"{tag}{'  ' + s:32s} {med_min(scopes[s])}")
        emit(f"{tag}{'yardstick':32s} {med_min(wall['yardstick'])}")
        emit(f"{tag}{'call / yardstick':32s} {statistics.median(wall['call']) / statistics.median(wall['yardstick']):10.3f}")
        for d in (d_com, d_prf, d_val, d_out, d_y, d_ys, d_yo):
            bbg.dev_free(d)
    string.free()
    bbg.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
