#!/usr/bin/env python3
"""Timings of the cell handle of bbg_open_all (bbg_open_all_prepare_cells, csrc/open_all.hip) -- the table in profiles/open_cells.txt, which
this script writes (--out PATH for another place; the lines are printed as well).

Per size (default 2^12, 2^16, 2^20) with cells of l = 64 points (--log2cell C for another), in ONE process and with both handles alive:
  * bbg_open_all_prepare_cells over a hashed string: the whole call on a host clock (it ends in a synchronisation), REPS times;
  * bbg_open_all_device through the cell handle on device-resident coefficients: one warm-up, then REPS calls, each the whole call up to
    a stream synchronisation on a host clock, with the profile scopes of that call from bbg_profile_get (HIP events on the stream);
  * beside it the same for the all-points handle of bbg_open_all_prepare at the same n, the calls of the two handles interleaved, and the
    ratio of the two medians.
Medians and minima are printed."""
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as ge  # noqa: E402
import coarse_inputs as ci  # noqa: E402

REPS = 5
SEED = 0xBB254
SCOPES = ("open_all_coeffs", "ntt_pass", "open_all_pointwise", "open_cells_sum", "ecntt_stages", "open_all_fold", "ecntt_normalize")


def med_min(v):
    return f"{statistics.median(v):10.3f} {min(v):10.3f}"


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "open_cells.txt")
    lc = 6
    for flag in ("--out", "--log2cell"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                out_path = args[i + 1]
            else:
                lc = int(args[i + 1])
            del args[i:i + 2]
    sizes = [int(a) for a in args] or [12, 16, 20]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# cells of 2^{lc} points.  one process, both handles alive; per size {REPS} prepares of each handle, one warm-up call and {REPS} timed calls of")
    emit("# each, interleaved; every pair of columns is median and minimum in ms.  prepare / call = the whole call on a host clock, up to a")
    emit("# synchronisation; the scopes are bbg_profile_get's (HIP events on the stream) for the same calls.  points: bbg_srs_synth_hashed;")
    emit("# coefficients spread over [0, 2r)")
    emit("log2n  what                               cells ms(med min)      all points ms(med min)")
    for lg in sizes:
        n = 1 << lg
        srs = bbg.srs_synth_hashed(SEED + lg, n)
        d_c, d_o = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64)
        bbg.dev_upload(d_c, ci.coarse_scalars(SEED + lg, n, 0))
        handles, prep = {}, {}
        for name, cell in (("cells", lc), ("all", 0)):
            ts, h = [], None
            for _ in range(REPS + 1):  # the first one builds the domains and grows the context's buffers: not counted
                if h is not None:
                    h.free()
                bbg.sync()
                t0 = time.perf_counter()
                h = bbg.open_all_prepare(srs, lg, cell)
                ts.append(1e3 * (time.perf_counter() - t0))
            handles[name], prep[name] = h, ts[1:]
        wall = {k: [] for k in handles}
        scopes = {k: {s: [] for s in SCOPES} for k in handles}
        for h in handles.values():  # warm-up
            h.open_device(d_c, d_o)
        bbg.sync()
        for _ in range(REPS):
            for name, h in handles.items():
                bbg.profile_enable(True)
                t0 = time.perf_counter()
                h.open_device(d_c, d_o)
                bbg.sync()
                wall[name].append(1e3 * (time.perf_counter() - t0))
                for s in SCOPES:
                    scopes[name][s].append(bbg.profile_get(s)[0])
                bbg.profile_enable(False)
        emit(f"{lg:5d}  {'prepare':32s} {med_min(prep['cells'])}   {med_min(prep['all'])}")
        emit(f"{lg:5d}  {'call':32s} {med_min(wall['cells'])}   {med_min(wall['all'])}")
        for s in SCOPES:
            emit(f"{lg:5d}  {'  ' + s:32s} {med_min(scopes['cells'][s])}   {med_min(scopes['all'][s])}")
        emit(f"{lg:5d}  {'proofs per call':32s} {handles['cells'].count:21d}   {handles['all'].count:21d}")
        emit(f"{lg:5d}  {'handle bytes':32s} {handles['cells'].device_bytes():21d}   {handles['all'].device_bytes():21d}")
        emit(f"{lg:5d}  {'call, cells / all points':32s} {statistics.median(wall['cells']) / statistics.median(wall['all']):21.3f}")
        for h in handles.values():
            h.free()
        for d in (d_c, d_o):
            bbg.dev_free(d)
        srs.free()
    bbg.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
