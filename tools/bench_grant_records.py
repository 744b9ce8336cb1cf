#!/usr/bin/env python3
"""What the log of a backlogged batch costs: launches of --ttis TTIs of scheduler 9 at the headline shape (20 x 25 UEs x 25 RBGs) and
at the shipped 64-RBG shape (20 x 5 UEs x 64 RBGs), three ways, --repeats alternating repeats each:

  a  run                 the unlogged launch (the lean build)
  b  run_logged          with the rows a log needs copied back: rbg_to_user, tbs_bits, uinfo
  c  run_grant_records   one 32-byte record per grant (cap = ttis * grant_bound)

  python tools/bench_grant_records.py [--cells 64,512] [--ttis 2000] [--repeats 3] [--modes abc] [--shapes headline,r64]

Wall clock per call, copy back and host sort included: the rows or records on the host are what the calls are for; the host arrays
of (b) and (c) are allocated and touched once, outside the timed calls.  RS_RECORDS_TIMING=1 makes the library print (c)'s split
(launch and wait, copy back, host sort) per call on stderr.  One JSON line per
(shape, cells): ms per launch as mean (min - max) per mode, records per cell-TTI, bytes copied back per launch, the kernel's share of (a)
(HIP events), the device source hash.  RS_TREE=<checkout> imports the package from another tree -- the parent commit's, whose (b) is
the yardstick of profiles/batch_grant_records.md: in a process of its own, modes ab only."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(os.environ.get("RS_TREE") or Path(__file__).resolve().parents[1])
sys.path.insert(0, str(ROOT))
import radiosaber_amd as rs  # noqa: E402
from radiosaber_amd import api  # noqa: E402

SHAPES = {"headline": ([25] * 20, 25, 4), "r64": ([5] * 20, 64, 8)}


def logged_rows(b, n, rows):
    """run_logged with the three rows a log needs (the other two stay on the device), into arrays allocated and touched once, outside
    the timed calls: (b) is charged the launch and the copy back, not the host's page faults"""
    m, tb, ui = rows
    lg = api._BatchLog(api._p(m, C.c_int16), api._p(tb, C.c_int32), None, None, api._p(ui, C.c_int32), None)
    api._check(api.lib().rs_batch_run_logged_ex(b._h, n, C.byref(lg)))
    return m.nbytes + tb.nbytes + ui.nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="64,512")
    ap.add_argument("--ttis", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", default="abc")
    ap.add_argument("--shapes", default="headline,r64")
    ap.add_argument("--sched", type=int, default=9)
    a = ap.parse_args()
    if "c" in a.modes and not hasattr(rs.BatchScheduler, "run_grant_records"):
        raise SystemExit("this tree has no run_grant_records: --modes ab")
    for shape in a.shapes.split(","):
        ues, R, G = SHAPES[shape]
        for cells in (int(x) for x in a.cells.split(",")):
            b = rs.BatchScheduler(rs.SliceConfig(ues), R, G, cells, sched=a.sched, jit=True, cqi_epoch_wrap=True)
            b.seed(np.arange(cells, dtype=np.uint32) * 7919 + 805290992)
            b.synthesize_cqi(805290992, 8)
            copied = {"a": 0}
            rows = None
            if "b" in a.modes:
                rows = (np.ones((cells, a.ttis, R), np.int16), np.ones((cells, a.ttis, sum(ues)), np.int32), np.ones((cells, a.ttis, sum(ues)), np.int32))
            block = None   # (the caller's record block, allocated and touched once like (b)'s rows)
            if "c" in a.modes:
                block = np.ones((cells, a.ttis * b.grant_bound()), api.BATCH_GRANT_RECORD)
            n_rec = 0

            def call(mode):
                nonlocal n_rec
                t0 = time.perf_counter()
                if mode == "a":
                    b.run(a.ttis)
                elif mode == "b":
                    copied["b"] = logged_rows(b, a.ttis, rows)
                else:
                    recs = b.run_grant_records(a.ttis, out=block)
                    n_rec = sum(len(r) for r in recs)
                    copied["c"] = 32 * n_rec + 4 * cells
                return (time.perf_counter() - t0) * 1e3

            for mode in a.modes:      # warm-up: the builds of every mode are compiled and self-checked here
                call(mode)
            ms = {mode: [] for mode in a.modes}
            for _ in range(a.repeats):
                for mode in a.modes:
                    ms[mode].append(call(mode))
            kernel_a = float(np.min(b.run_timed(a.ttis, 2)))
            line = {"shape": shape, "sched": a.sched, "cells": cells, "ttis": a.ttis, "tree": str(ROOT), "source_hash": rs.device_source_hash(),
                    "kernel": b.kernel_name, "jit_status": b.jit_status()[0], "kernel_ms_a": round(kernel_a, 3)}
            for mode in a.modes:
                line[mode] = {"mean": round(float(np.mean(ms[mode])), 3), "min": round(min(ms[mode]), 3), "max": round(max(ms[mode]), 3),
                              "bytes_back": copied.get(mode, 0)}
            if "c" in a.modes:
                line["records_per_cell_tti"] = round(n_rec / (cells * a.ttis), 3)
            print(json.dumps(line), flush=True)
            b.close()


if __name__ == "__main__":
    main()
