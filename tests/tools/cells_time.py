#!/usr/bin/env python3
"""Timings of bbg_cells_recover_device (csrc/cells.hip) -- the table in profiles/cells_recover.txt, which this script writes
(--out PATH for another place; the lines are printed as well).

Per shape (log2n, log2cell) -- default (12, 6), the shape of the suite's time bound, (13, 6), the deployed 128-cell shape, then (16, 6) and
(20, 6); other shapes as arguments `LOG2N:LOG2CELL` -- with a seeded random half of the cells known (K = r / 2) and count = 1 and 8
polynomials, in ONE process:
  * the call: one warm-up, then REPS calls on device-resident values, each on a host clock up to a stream synchronisation;
  * its scopes from bbg_profile_get (HIP events on the stream) over REPS further calls;
  * the yardstick at the same n: bbg_ntt_device three times (inverse, coset, inverse coset) and bbg_fr_batch_invert_device of n values on
    one array, queued together and timed the same way, interleaved with the calls; and the ratio of the medians, call / (count x yardstick).
bbg_cells_values_device is timed beside them.  Medians and minima are printed."""
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
SEED = 0xBB254 + 0xCE115
COUNTS = (1, 8)
SCOPES = ("cells_z", "fr_batch_invert", "cells_scatter", "ntt_pass", "cells_divide", "cells_canon")


def med_min(v):
    return f"{statistics.median(v):10.3f} {min(v):10.3f}"


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "cells_recover.txt")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    shapes = [tuple(int(v) for v in a.split(":")) for a in args] or [(12, 6), (13, 6), (16, 6), (20, 6)]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# K = r / 2 cells known, a seeded random half.  one process; per row one warm-up and {REPS} timed runs, calls and yardstick interleaved;")
    emit("# every pair of columns is median and minimum in ms.  call / values / yardstick = the whole thing on a host clock, up to a")
    emit("# synchronisation; the scopes are bbg_profile_get's (HIP events on the stream) over further calls.  yardstick = bbg_ntt_device x 3")
    emit("# (inverse, coset, inverse coset) + bbg_fr_batch_invert_device of n values, one array.  values spread over [0, 2r)")
    emit("log2n log2cell count  what                             ms(med min)")
    for lg, lc in shapes:
        n, l, r = 1 << lg, 1 << lc, 1 << (lg - lc)
        K = r // 2
        ids = np.sort(np.random.default_rng(SEED + lg).permutation(r)[:K]).astype(np.uint32)
        cmax = max(COUNTS)
        d_v, d_o, d_y = bbg.dev_alloc(cmax * n * 32), bbg.dev_alloc(cmax * n * 32), bbg.dev_alloc(n * 32)
        known, full = ci.coarse_scalars(SEED + lg, K * l, 0), ci.coarse_scalars(SEED + lg + 1, n, 0)

        def fill(d, words):  # every polynomial of the call the same words
            for p in range(cmax):
                bbg.dev_upload(d + p * words.nbytes, words)

        fill(d_v, known)
        bbg.dev_upload(d_y, full)

        def yardstick():
            for op in (pkg.binding.IFFT, pkg.binding.COSET_FFT, pkg.binding.COSET_IFFT):
                bbg.ntt_device(d_y, lg, op)
            bbg.fr_batch_invert_device(d_y, d_y, n)

        def timed(fn):
            bbg.sync()
            t0 = time.perf_counter()
            fn()
            bbg.sync()
            return 1e3 * (time.perf_counter() - t0)

        for count in COUNTS:
            recover = lambda: bbg.cells_recover_device(ids, d_v, lg, lc, count, d_o)  # noqa: E731
            values = lambda: bbg.cells_values_device(d_o, lg, lc, count, d_v)  # noqa: E731  (the recovered coefficients back to values: d_v is rewritten)
            for fn in (recover, yardstick):  # warm-up: domains, working memory
                fn()
            bbg.sync()
            wall = {"call": [], "yardstick": []}
            for _ in range(REPS):
                wall["call"].append(timed(recover))
                wall["yardstick"].append(timed(yardstick))
            scopes = {s: [] for s in SCOPES}
            for _ in range(REPS):
                bbg.profile_enable(True)
                recover()
                bbg.sync()
                for s in SCOPES:
                    scopes[s].append(bbg.profile_get(s)[0])
                bbg.profile_enable(False)
            tag = f"{lg:5d} {lc:8d} {count:5d}  "
            emit(f"{tag}{'bbg_cells_recover_device':32s} {med_min(wall['call'])}")
            for s in SCOPES:
                emit(f"{tag}{'  ' + s:32s} {med_min(scopes[s])}")
            emit(f"{tag}{'yardstick (one polynomial)':32s} {med_min(wall['yardstick'])}")
            emit(f"{tag}{'call / (count x yardstick)':32s} {statistics.median(wall['call']) / (count * statistics.median(wall['yardstick'])):10.3f}")
            fill(d_o, full)
            values()
            emit(f"{tag}{'bbg_cells_values_device':32s} {med_min([timed(values) for _ in range(REPS)])}")
            fill(d_v, known)
        for d in (d_v, d_o, d_y):
            bbg.dev_free(d)
    bbg.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
