#!/usr/bin/env python3
"""us per group call with the caller's averages (rs_group_schedule_tti), with resident averages (rs_group_schedule_tti_at) and with
resident averages on the group's own run-time builds (rs_group_specialize_resident), and -- with the -DRS_STAMPS build -- the kernel's
load-phase cycles (profiles/group_resident_avg.md, profiles/group_resident_specialize.md).

    RS_DROPIN_TIMING=1 python tools/group_resident_latency.py [--variant plain|resident|resident-spec|both] [--calls 400]
    RS_HIP_LIB=radiosaber_amd/libradiosaber_hip_stamps.so python tools/group_resident_latency.py     # adds the stamped load phase

Workloads: 8 and 64 cells; 500 users x 25 RBGs and 100 users x 64 RBGs; scheduler 9; cqi_epoch on (new reports every 40 calls).
RS_TREE=<another checkout> measures that tree's package (the plain variant only, for a tree without resident averages).
resident-spec: specialize_resident() before the warm-up, whose first rounds are the builds' checked calls (80 rounds cover the 8); the
line ends with the kernel's name and the status of the builds.
RS_DROPIN_TIMING=1 makes the library print its own prepare / enqueue / wait / unpack split per group on stderr."""
import argparse
import ctypes as C
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, os.environ.get("RS_TREE", str(Path(__file__).resolve().parents[1])))
import radiosaber_amd as rs  # noqa: E402
from radiosaber_amd.api import lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="both", choices=("plain", "resident", "resident-spec", "both"))
ap.add_argument("--calls", type=int, default=400)
ap.add_argument("--warmup", type=int, default=80)
args = ap.parse_args()


def load_phase(g):
    """Stamp slot 9 of the launch (one of its workgroups; a resident kernel adds its update and gather to it), or None."""
    f = lib().rs_batch_debug_stamps
    f.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 20)()
    batch = C.cast(g._h, C.POINTER(C.c_void_p))[0]  # rs_group's first member is its batch
    return int(out[9]) if f(batch, 0, out) == 0 else None


for ues, R, G in ((25, 25, 4), (5, 64, 8)):
    for K in (8, 64):
        sc = rs.SliceConfig([ues] * 20, weight=[0.05] * 20)
        U = 20 * ues
        for variant in (("plain", "resident") if args.variant == "both" else (args.variant,)):
            g = rs.GroupScheduler(sc, R, G, K, sched=9)
            rng = np.random.default_rng(1)
            cqi = [rng.integers(1, 16, (U, R)).astype(np.uint8) for _ in range(K)]
            avg = [rng.uniform(1e4, 1e6, U) for _ in range(K)]
            if variant != "plain":
                for k in range(K):
                    g.set_avg(k, avg[k], 0.1)
            if variant == "resident-spec":
                g.specialize_resident()
            now, best = 0.1, []
            for rep in range(3):  # three repetitions: their spread is the yardstick for a difference between variants
                t0 = 0.0
                for i in range(args.warmup + args.calls):
                    if i == args.warmup:
                        t0 = time.perf_counter()
                    now += 0.001
                    calls = [dict(cqi=cqi[k], rand0=123 + i, rand1=456 + i, cqi_epoch=1 + i // 40) for k in range(K)]
                    if variant == "plain":
                        for k in range(K):
                            calls[k]["avg_rate"] = avg[k]
                        g.schedule_tti(calls)
                    else:
                        g.schedule_tti_at(calls, now)
                best.append((time.perf_counter() - t0) / args.calls * 1e6)
            lp = load_phase(g)
            print(f"{K:3d} cells x {U} UEs x {R} RBGs, {variant:13s}: " + " / ".join(f"{b:.1f}" for b in best) + " us per call (python)"
                  + (f", load phase {lp} cycles" if lp is not None else "")
                  + (f", {g.kernel_name}, {g.resident_jit_status()[1]}" if variant == "resident-spec" else ""), flush=True)
            g.close()
