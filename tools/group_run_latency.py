#!/usr/bin/env python3
"""us per cell-TTI of a backlogged K-cell host between two CQI reports: (a) 40 rs_group_schedule_tti_at calls against (b) one
rs_group_run_at of 40 (profiles/group_run.md); (b) against (j) the same run on the group's own run-time builds of the run kernel
(rs_group_specialize_run; profiles/group_run_specialize.md, where the mode was called c); (b) against (c) one rs_group_run_counted_at of
40 without outputs and (d) the same with outputs (profiles/group_run_counted.md); (d) against (r) one rs_group_run_records_at of 40
without outputs, grant records on (profiles/group_run_records.md).

    RS_DROPIN_TIMING=1 python tools/group_run_latency.py [--blocks 20] [--ttis 40] [--modes ab | bj | bcd | dr | ...] [--repeats 3]

Workloads: 8, 27 and 64 cells; 500 users x 25 RBGs and 100 users x 64 RBGs; scheduler 9; resident averages; cqi_epoch on, a new number
(the same reports) every block of 40 TTIs, so that the first TTI of a block stores the cells' images and the other 39 are image hits.
The modes run in this process on the same library, on a group each, and alternate: a, b, a, b, a, b -- three repeats per mode; a gain
holds when a later mode's worst repeat lies below the first mode's best.  (RS_TREE names another tree to import the package from: a
parent commit's library is measured by a process of its own, alternating with this one's -- --repeats 1 per process.)  Mode (j) warms up until the self-check of the build that
serves its runs has finished (RS_DROPIN_SELFCHECK_CALLS checked runs, default 8): no timed run is a checked one.  The arguments are marshalled once, outside the timed region: the time is that of
the library calls alone.  RS_DROPIN_TIMING=1 makes the library print its own prepare / enqueue / wait / unpack split per group on stderr
when the group is closed (in the order of --modes; per CALL: a call of (b), (c), (d), (j) or (r) is 40 TTIs)."""
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
ap.add_argument("--shapes", type=int, nargs="*", default=[0, 1], help="0: 500 users x 25 RBGs, 1: 100 users x 64 RBGs")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--modes", default="ab", help="letters of a: 40 at-calls, b: one run, j: the run on the group's own builds, c: one counted run without "
                "outputs, d: one counted run with outputs, r: one counted run without outputs, grant records on; the first is what the others are held against")
args = ap.parse_args()
assert args.modes and set(args.modes) <= set("abcdjr") and len(set(args.modes)) == len(args.modes)
T = args.ttis
M0 = args.modes[0]
NAMES = {"a": f"{T} at-calls", "b": f"one run of {T}", "j": f"one specialised run of {T}", "c": f"one counted run of {T} without outputs",
         "d": f"one counted run of {T}", "r": f"one counted run of {T} without outputs, with records"}
SHAPES = ((25, 25, 4), (5, 64, 8))


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


for ues, R, G in (SHAPES[i] for i in args.shapes):
    for K in args.cells:
        sc = rs.SliceConfig([ues] * 20, weight=[0.05] * 20)
        U = 20 * ues
        rng = np.random.default_rng(1)
        cqi = [rng.integers(1, 16, (U, R)).astype(np.uint8) for _ in range(K)]
        avg = [rng.uniform(1e4, 1e6, U) for _ in range(K)]
        rands = np.ascontiguousarray(rng.integers(0, 2**31 - 1, (K, T, 2)).astype(np.int32))
        groups = {}
        for mode in args.modes:
            g = rs.GroupScheduler(sc, R, G, K, sched=9, jit_run=mode == "j")
            for k in range(K):
                g.set_avg(k, avg[k], 0.1)
                if mode in "cdr":
                    g.set_avg_counters(k)
            groups[mode] = [g, marshal(sc, R, G, K, 1 if mode == "a" else T, cqi), 0.1, 0]   # group, arguments, clock, blocks done
        L = lib()
        if "r" in groups:   # (the caller's record lists, rs_group_grant_bound records per cell-TTI, allocated once like the other arguments)
            cap = groups["r"][0].grant_bound
            recs, n_recs = np.zeros((K, T, cap), rs.api.GRANT_RECORD), np.zeros((K, T), np.int32)

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
                run = L.rs_group_run_counted_at if mode in "cd" else L.rs_group_run_at
                if mode == "r":
                    _check(L.rs_group_run_records_at(g._h, K, None, ins, T, t.ctypes.data_as(C.POINTER(C.c_double)), rands.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     None, cap, recs.ctypes.data, n_recs.ctypes.data_as(C.POINTER(C.c_int32))))
                else:
                    _check(run(g._h, K, None, ins, T, t.ctypes.data_as(C.POINTER(C.c_double)), rands.ctypes.data_as(C.POINTER(C.c_int32)), None if mode == "c" else outs))
            groups[mode][2], groups[mode][3] = now, done + 1

        for mode in args.modes:
            for _ in range(args.warmup):
                block(mode)
        if "j" in groups:   # (the plain run is served by the lean build: its checked runs end here)
            for _ in range(64):
                if "to go" not in groups["j"][0].run_jit_status()[1].split("lean build:")[-1]:
                    break
                block("j")
            code, msg = groups["j"][0].run_jit_status()
            assert code == 1 and "to go" not in msg.split("lean build:")[-1] and groups["j"][0].kernel_name == "rs_group_run_kernel_jit", (code, msg)
        us = {mode: [] for mode in args.modes}
        for rep in range(args.repeats):
            for mode in args.modes:
                t0 = time.perf_counter()
                for _ in range(args.blocks):
                    block(mode)
                us[mode].append((time.perf_counter() - t0) / (args.blocks * T * K) * 1e6)
        line = f"{K:3d} cells x {U} UEs x {R} RBGs: ({M0}) {NAMES[M0]} " + " / ".join(f"{x:.3f}" for x in us[M0])
        for M1 in args.modes[1:]:
            verdict = "holds" if max(us[M1]) < min(us[M0]) else "does not hold"
            line += (f"; ({M1}) {NAMES[M1]} " + " / ".join(f"{x:.3f}" for x in us[M1]) + f" us per cell-TTI; the gain {verdict}; launches "
                     f"{groups[M0][0].launch_count} / {groups[M1][0].launch_count}, {groups[M1][0].kernel_name}")
        print(line + ("" if args.modes[1:] else " us per cell-TTI"), flush=True)
        for mode in args.modes:
            sys.stderr.write(f"-- {K} cells x {U} UEs x {R} RBGs, mode ({mode}):\n")
            sys.stderr.flush()
            groups[mode][0].close()
