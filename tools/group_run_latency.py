#!/usr/bin/env python3
"""us per cell-TTI of a backlogged K-cell host between two CQI reports: (a) 40 rs_group_schedule_tti_at calls against (b) one
rs_group_run_at of 40 (profiles/group_run.md).

    RS_DROPIN_TIMING=1 python tools/group_run_latency.py [--blocks 20] [--ttis 40]

Workloads: 8, 27 and 64 cells; 500 users x 25 RBGs and 100 users x 64 RBGs; scheduler 9; resident averages; cqi_epoch on, a new number
(the same reports) every block of 40 TTIs, so that the first TTI of a block stores the cells' images and the other 39 are image hits.
Both modes run in this process on the same library, on a group each, and alternate: a, b, a, b, a, b -- three repeats per mode; a gain
holds when (b)'s worst repeat lies below (a)'s best.  The arguments are marshalled once, outside the timed region: the time is that of
the library calls alone.  RS_DROPIN_TIMING=1 makes the library print its own prepare / enqueue / wait / unpack split per group on stderr
when the group is closed ((a) first, then (b); per CALL: a call of (b) is 40 TTIs)."""
import argparse
import ctypes as C
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, os.environ.get("RS_TREE", str(Path(__file__).resolve().parents[1])))
import radiosaber_amd as rs  # noqa: E402
from radiosaber_amd.api import _TtiIn, _TtiOut, _check, _marshal_tti, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=20, help="blocks of --ttis TTIs per repeat")
ap.add_argument("--warmup", type=int, default=3, help="blocks before the first timed one")
ap.add_argument("--ttis", type=int, default=40, help="TTIs between two report renewals (CQI_INTERVAL)")
ap.add_argument("--cells", type=int, nargs="*", default=[8, 27, 64])
args = ap.parse_args()
T = args.ttis


def marshal(sc, R, G, K, n_out, cqi):
    ins, outs, keep = (_TtiIn * K)(), (_TtiOut * (K * n_out))(), []
    for k in range(K):
        for j in range(n_out):
            tin, tout, res, arrays = _marshal_tti(sc.n_slices, R, G, 9, cqi[k], None, rand0=123, rand1=456)
            if j == 0:
                ins[k] = tin
            outs[k * n_out + j] = tout
            keep.append((res, arrays))
    return ins, outs, keep


for ues, R, G in ((25, 25, 4), (5, 64, 8)):
    for K in args.cells:
        sc = rs.SliceConfig([ues] * 20, weight=[0.05] * 20)
        U = 20 * ues
        rng = np.random.default_rng(1)
        cqi = [rng.integers(1, 16, (U, R)).astype(np.uint8) for _ in range(K)]
        avg = [rng.uniform(1e4, 1e6, U) for _ in range(K)]
        rands = np.ascontiguousarray(rng.integers(0, 2**31 - 1, (K, T, 2)).astype(np.int32))
        groups = {}
        for mode in "ab":
            g = rs.GroupScheduler(sc, R, G, K, sched=9)
            for k in range(K):
                g.set_avg(k, avg[k], 0.1)
            groups[mode] = [g, marshal(sc, R, G, K, 1 if mode == "a" else T, cqi), 0.1, 0]   # group, arguments, clock, blocks done
        L = lib()

        def block(mode):
            g, (ins, outs, _), now, done = groups[mode]
            for k in range(K):
                ins[k].cqi_epoch = 1 + done
            if mode == "a":
                t = np.zeros(K)
                for i in range(T):
                    now += 0.001
                    t[:] = now
                    for k in range(K):
                        ins[k].rand0, ins[k].rand1 = int(rands[k, i, 0]), int(rands[k, i, 1])
                    _check(L.rs_group_schedule_tti_at(g._h, K, None, ins, outs, t.ctypes.data_as(C.POINTER(C.c_double))))
            else:
                t = np.ascontiguousarray(np.broadcast_to(now + 0.001 * np.arange(1, T + 1), (K, T)))
                now = float(t[0, -1])
                _check(L.rs_group_run_at(g._h, K, None, ins, T, t.ctypes.data_as(C.POINTER(C.c_double)), rands.ctypes.data_as(C.POINTER(C.c_int32)), outs))
            groups[mode][2], groups[mode][3] = now, done + 1

        for mode in "ab":
            for _ in range(args.warmup):
                block(mode)
        us = {"a": [], "b": []}
        for rep in range(3):
            for mode in "ab":
                t0 = time.perf_counter()
                for _ in range(args.blocks):
                    block(mode)
                us[mode].append((time.perf_counter() - t0) / (args.blocks * T * K) * 1e6)
        verdict = "holds" if max(us["b"]) < min(us["a"]) else "does not hold"
        print(f"{K:3d} cells x {U} UEs x {R} RBGs: (a) {T} at-calls " + " / ".join(f"{x:.3f}" for x in us["a"]) + f"; (b) one run of {T} "
              + " / ".join(f"{x:.3f}" for x in us["b"]) + f" us per cell-TTI; the gain {verdict}; launches {groups['a'][0].launch_count} / "
              f"{groups['b'][0].launch_count}, {groups['b'][0].kernel_name}", flush=True)
        for mode in "ab":
            sys.stderr.write(f"-- {K} cells x {U} UEs x {R} RBGs, mode ({mode}):\n")
            sys.stderr.flush()
            groups[mode][0].close()
