#!/usr/bin/env python3
"""The launch sequence of the Fr NTT's host dispatch, and the host cost of a launch-bound proof (profiles/ntt_dispatch.txt).

  ntt_dispatch_run.py trace      one transform of each op at 2^12, 2^17, 2^18, 2^21, 2^22 under defaults, then prover rounds 1 + 3 at 2^12
                                 gates: run it under `rocprofv3 --kernel-trace` (no counters) once per library and compare the sequences of
                                 (kernel, grid, workgroup, LDS) with `ntt_dispatch_run.py compare a_kernel_trace.csv b_kernel_trace.csv`
  ntt_dispatch_run.py time       rounds 1 + 3 at 2^12 gates, width 4: median of 20 after 3 warm-ups, host wall clock around a synchronise
  ntt_dispatch_run.py compare A B

BBG_LIB_PATH selects the library (another build of the same ABI)."""
import csv
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LG_PROVER, WIDTH = 12, 4


def prover_setup(pkg, bbg):
    from test_gpu_barycentric import make_prover
    n = 1 << LG_PROVER
    srs = bbg.srs_synth_hashed(5, n + 1)
    h = make_prover(pkg, bbg, srs, LG_PROVER, WIDTH)
    wires = [pkg.synthetic_scalars(600 + k, n) for k in range(4)]
    ch = pkg.synthetic_scalars(700, 8)
    com = np.zeros((WIDTH + 1, 12), dtype=np.uint64)

    def rounds_1_3():
        lib = bbg.lib
        wp = (ctypes.c_void_p * 4)(*[w.ctypes.data for w in wires])
        assert lib.bbg_prover_round1(h, wp, com.ctypes.data) == 0, lib.bbg_last_error()
        assert lib.bbg_prover_round3(h, ch[0].ctypes.data, ch[1].ctypes.data, ch[2:5].ctypes.data, com[WIDTH:].ctypes.data) == 0, lib.bbg_last_error()
        bbg.sync()

    def done():
        bbg.lib.bbg_prover_destroy(h)
        srs.free()
    return rounds_1_3, done


def trace(pkg, bbg):
    import torch
    for lg in (12, 17, 18, 21, 22):
        a = torch.from_numpy(pkg.synthetic_scalars(11, 1 << lg).view(np.int64).reshape(-1)).cuda()
        kc = pkg.synthetic_scalars(12, 1)[0]
        for op in range(8):
            bbg.ntt_device(a.data_ptr(), lg, op, 0, kc if op >= 4 else None)
        bbg.sync()
    rounds_1_3, done = prover_setup(pkg, bbg)
    rounds_1_3()
    done()


def timed(pkg, bbg):
    rounds_1_3, done = prover_setup(pkg, bbg)
    for _ in range(3):
        rounds_1_3()
    ms = []
    for _ in range(20):
        t0 = time.perf_counter()
        rounds_1_3()
        ms.append((time.perf_counter() - t0) * 1e3)
    done()
    print(f"rounds 1+3, 2^{LG_PROVER} gates, width {WIDTH}: median {statistics.median(ms):.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}  (20 after 3 warm-ups)")


def launches(path):
    with open(path, newline="") as f:
        seq = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))  # the order the host queued them in
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Workgroup_Size_X"], r["LDS_Block_Size"]) for r in seq]


def compare(a, b):
    la, lb = launches(a), launches(b)
    ntt = [sum(1 for r in l if "ntt_pass" in r[0]) for l in (la, lb)]
    print(f"{a}: {len(la)} launches ({ntt[0]} of pass kernels, {len(set(r[0] for r in la))} distinct kernels)")
    print(f"{b}: {len(lb)} launches ({ntt[1]} of pass kernels, {len(set(r[0] for r in lb))} distinct kernels)")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            print(f"first difference at launch {i}:\n  {x}\n  {y}")
            return 1
    if len(la) != len(lb):
        print("one sequence is a prefix of the other")
        return 1
    print("identical sequences of (kernel, grid x, grid y, workgroup, LDS bytes)")
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    import __graft_entry__ as ge
    import torch
    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    bbg.set_stream(torch.cuda.current_stream().cuda_stream)
    {"trace": trace, "time": timed}[mode](pkg, bbg)
    bbg.close()
