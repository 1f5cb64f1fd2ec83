#!/usr/bin/env python3
"""Timings of the batched pairing product check (bbg_pairing_product_device, csrc/pairing.hip) -- the table in profiles/pairing.txt.

    python tests/tools/pairing_time.py [OUT [RESOURCES]]      (OUT defaults to profiles/pairing.txt)

RESOURCES: a text file with what `make -C aztec-2.0_amd/csrc pairing.o EXTRA=-Rpass-analysis=kernel-resource-usage` printed; its lines for
the kernels of pairing.hip (name, VGPRs, scratch, occupancy) are copied into the table.

In ONE process on one MI355X, for pairs = 2 and 4 and count = 1, 64, 2^10, 2^14, 2^17: device-resident G1 points made by
bbg_g1_fixed_base_mul_device over scalars spread over [0, 2r), the G2 points [b_j] G2; one warm-up, then REPS = 9 calls, each sample the whole
call on a host clock ending in a stream synchronisation; then REPS calls with the timers on for the phases "pairing_miller" and
"pairing_final" (bbg_profile_get, HIP events on the stream).  bbg_g2_lines_prepare is timed the same way ("g2_lines" and the whole call).
There is no CPU build of the reference's pairing under oracle/_ref/, so no CPU comparison is quoted; the figure to set the rate against is
the multiplier ceiling: the measured peak of 33.8 T mads/s over about 160 mads per Fq product (136 in the Montgomery product itself) times
the Fq products of one check, counted below from the kernels' own operation counts."""
import hashlib
import importlib.util
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
import pairing_model as pm  # noqa: E402

REPS = 9
SEED = 0xBB254
COUNTS = (1, 64, 1 << 10, 1 << 14, 1 << 17)
PAIRS = (2, 4)
MADS_PER_SECOND = 33.8e12
MADS_PER_PRODUCT = 160
# Fq products per Fq12 operation (csrc/fq_tower.hip.h): product, squaring, sparse product with its two scalings, cyclotomic squaring,
# Frobenius map, inverse (two Fq6 squarings, one Fq6 inverse of 37, two Fq6 products; the Fq inversion itself is not a product)
F12_MUL, F12_SQR, F12_SPARSE, F12_CSQR, F12_FROB, F12_INV = 54, 36, 43, 18, 15, 97


def fq_products(pairs):
    spec = importlib.util.spec_from_file_location("gen_pairing_consts", os.path.join(ROOT, "scripts", "gen_pairing_consts.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cost = {"MUL": F12_MUL, "CSQR": F12_CSQR, "CONJ": 0, "FROB1": F12_FROB, "FROB2": F12_FROB, "FROB3": F12_FROB, "INV": F12_INV, "END": 0}
    names = {v: k for k, v in gen.OPS.items()}
    final = sum(cost[names[w & 255]] for w in gen.final_exponentiation_program())
    miller = len(pm.LOOP_BITS) * F12_SQR + pm.LINES * pairs * F12_SPARSE
    return miller, final


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pairing.txt")
    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # rewritten row by row: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# tests/tools/pairing_time.py: one process; per row one warm-up, then {REPS} calls, a sample the whole call on a host clock ending in a")
    emit("# stream synchronisation; ms, median (min .. max).  phases: bbg_profile_get medians over further calls (HIP events on the stream).")
    emit("# ceiling: 33.8 T mads/s over 160 mads per Fq product times the Fq products of one check (Miller loop + final exponentiation).")
    if len(sys.argv) > 2:
        emit("# -Rpass-analysis=kernel-resource-usage for csrc/pairing.hip:")
        keep = ("Function Name", "VGPRs:", "AGPRs", "ScratchSize", "Occupancy")
        for row in open(sys.argv[2]):
            if any(k in row for k in keep):
                emit("#   " + row.split("remark:")[-1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip())
    b = [int.from_bytes(hashlib.sha256(b"pairing_time %d" % j).digest(), "little") % pm.R for j in range(max(PAIRS))]
    q_words = bbg.g2_mul(pm.fr_words(b))
    for pairs in PAIRS:
        total, phase = [], []
        for rep in range(REPS + 1):
            bbg.profile_enable(True)
            t0 = time.perf_counter()
            h = bbg.g2_lines_prepare(q_words[:pairs])
            total.append(1e3 * (time.perf_counter() - t0))
            phase.append(bbg.profile_get("g2_lines")[0])
            bbg.profile_enable(False)
            h.free()
        emit(f"pairs {pairs}  bbg_g2_lines_prepare: {statistics.median(total[1:]):.3f} ({min(total[1:]):.3f} .. {max(total[1:]):.3f})   g2_lines {statistics.median(phase[1:]):.3f}")
    emit("pairs    count     call median       min       max    miller     final   checks/s   of ceiling")
    for pairs in PAIRS:
        miller_products, final_products = fq_products(pairs)
        ceiling = MADS_PER_SECOND / (MADS_PER_PRODUCT * (miller_products + final_products))
        emit(f"# pairs {pairs}: {miller_products} + {final_products} Fq products per check, ceiling {ceiling:.3e} checks/s")
        h = bbg.g2_lines_prepare(q_words[:pairs])
        for count in COUNTS:
            n = count * pairs
            d_s, d_p, d_o, d_st = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64), bbg.dev_alloc(count * 384), bbg.dev_alloc(count * 4)
            bbg.dev_upload(d_s, ci.coarse_scalars(SEED + count + pairs, n, 0))
            bbg.g1_fixed_base_mul_device(d_s, n, d_p)
            bbg.sync()
            samples = []
            for rep in range(REPS + 1):
                t0 = time.perf_counter()
                bbg.pairing_product_device(h, d_p, count, d_o, d_st)
                bbg.sync()
                samples.append(1e3 * (time.perf_counter() - t0))
            samples = samples[1:]
            ph = {"pairing_miller": [], "pairing_final": []}
            for rep in range(REPS):
                bbg.profile_enable(True)
                bbg.pairing_product_device(h, d_p, count, d_o, d_st)
                bbg.sync()
                for k in ph:
                    ph[k].append(bbg.profile_get(k)[0])
                bbg.profile_enable(False)
            status = bbg.dev_download(d_st, (count,), dtype=np.uint32)
            assert not status.any(), "a random product is not one and every point is on the curve"
            med = statistics.median(samples)
            rate = count / (med * 1e-3)
            emit(f"{pairs:5d} {count:8d}   {med:13.3f} {min(samples):9.3f} {max(samples):9.3f} {statistics.median(ph['pairing_miller']):9.3f} "
                 f"{statistics.median(ph['pairing_final']):9.3f} {rate:10.3e}   {100 * rate / ceiling:8.2f} %")
            for d in (d_s, d_p, d_o, d_st):
                bbg.dev_free(d)
        h.free()
    bbg.close()


if __name__ == "__main__":
    main()
