#!/usr/bin/env python3
"""CQI epoch grids from device memory, measured (GPU box; profiles/cqi_device.md).

Three measurements, each at 512 cells x 500 UEs x 25 RBGs and at 512 cells x 100 UEs x 64 RBGs, the modes of each alternating within
one process; every figure is printed as median [min .. max] over the repeats, one JSON line per measurement:

  set     wall time of upload_cqi_epochs (validation and transposition on one host thread, hipFree / hipMalloc, the copy over PCIe)
          against set_cqi_epochs_device (rs_pack_cqi_kernel) for the same 8 epochs
  pack    the pack alone between two events on the batch's stream: (bytes read + bytes written) / time over back-to-back asynchronous
          writes of all 64 epochs, beside rs_hbm_copy_probe's figure from the same process
  ring    cqi_refresh = 1, cqi_epoch_wrap = 1, 64 epochs: every step writes 32 fresh epochs into the half that the next 32 TTIs read
          (write_cqi_epochs_device(..., sync=False), then run_async(32)) -- from a tensor made once (`ring_fixed`: the refill alone)
          and from torch.randint on torch's stream every step (`ring_randint`: a producer too) -- against the same batch cycling its
          64 grids without any refill (`cycle`, the mode of bench.py --cqi-refresh 1), in TTIs/s

    python tools/bench_cqi_device.py [--only set,pack,ring] [--repeats 5] [--steps 100] [--no-jit]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

CELLS = 512
SHAPES = {"500x25": (20, 25, 25, 4), "100x64": (20, 5, 64, 4)}   # slices, UEs per slice, RBGs, PRBs per RBG


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def stride_of(U, R):
    k = (U + 7) // 8
    return (8 * (k if k & 1 else k + 1) * R + 15) // 16 * 16


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", default="set,pack,ring")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100, help="ring: steps of 32 TTIs per timed repeat")
    ap.add_argument("--sched", type=int, default=9)
    ap.add_argument("--no-jit", action="store_true", help="ring: the kernels built into the library")
    args = ap.parse_args()
    from radiosaber_amd import toolchain
    toolchain.prefer_system_compiler()
    import torch
    import radiosaber_amd as rs
    from radiosaber_amd import sharding
    only = set(args.only.split(","))
    dev = torch.device("cuda", 0)
    probe = rs.hbm_copy_probe(0) if "pack" in only else None

    def batch(shape, refresh=40, wrap=False, jit=False):
        S, per, R, G = SHAPES[shape]
        b = rs.BatchScheduler(rs.SliceConfig([per] * S), R, G, CELLS, sched=args.sched, cqi_refresh=refresh, cqi_epoch_wrap=wrap, jit=jit)
        b.seed(sharding.seeds_for_cells(sharding.cell_ids_for_rank(0, 1, CELLS)))
        return b

    def grids(shape, n_epochs):
        S, per, R, _ = SHAPES[shape]
        return torch.randint(1, 16, (CELLS, n_epochs, S * per, R), dtype=torch.uint8, device=dev)

    for shape in args.shapes.split(","):
        S, per, R, _ = SHAPES[shape]
        U = S * per
        if "set" in only:
            t = grids(shape, 8)
            h = t.cpu().numpy()
            torch.cuda.synchronize()
            b = batch(shape)
            b.upload_cqi_epochs(h), b.set_cqi_epochs_device(t)   # warm-up of both
            host, device = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter(); b.upload_cqi_epochs(h); t1 = time.perf_counter(); b.set_cqi_epochs_device(t); t2 = time.perf_counter()
                host.append((t1 - t0) * 1e3), device.append((t2 - t1) * 1e3)
            b.close()
            print(json.dumps({"measurement": "set", "shape": shape, "cells": CELLS, "epochs": 8, "source_bytes": int(t.numel()),
                              "upload_cqi_epochs_ms": spread(host), "set_cqi_epochs_device_ms": spread(device),
                              "ratio_of_medians": spread(host)["median"] / spread(device)["median"]}), flush=True)
        if "pack" in only:
            n_epochs, launches = 64, 10
            t = grids(shape, n_epochs)
            b = batch(shape)
            b.set_cqi_epochs_device(t)
            stream = torch.cuda.ExternalStream(b.stream, device=dev)
            moved = CELLS * n_epochs * (U * R + stride_of(U, R))
            gbs = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(launches):
                    b.write_cqi_epochs_device(0, t, sync=False)
                e1.record(stream)
                e1.synchronize()
                gbs.append(launches * moved / (e0.elapsed_time(e1) * 1e-3) / 1e9)
            assert b.cqi_write_status() is None
            b.close()
            med = spread(gbs)["median"]
            # one grid per cell-TTI is what a batch at cqi_refresh = 1 consumes
            print(json.dumps({"measurement": "pack", "shape": shape, "cells": CELLS, "epochs": n_epochs, "bytes_per_launch": moved,
                              "launches_per_repeat": launches, "pack_gbs": spread(gbs), "copy_probe_gbs": probe,
                              "fraction_of_copy_probe": med / probe,
                              "grids_per_s": med * 1e9 / (U * R + stride_of(U, R))}), flush=True)
        if "ring" in only:
            n_epochs, half = 64, 32
            b = batch(shape, refresh=1, wrap=True, jit=not args.no_jit)
            b.set_cqi_epochs_device(grids(shape, n_epochs))
            b.prepare_launch(half)
            fixed = grids(shape, half)
            torch.cuda.synchronize()

            def run(mode):
                b.sync(), torch.cuda.synchronize()
                t0 = time.perf_counter()
                for step in range(args.steps):
                    if mode != "cycle":
                        t = fixed if mode == "ring_fixed" else torch.randint(1, 16, fixed.shape, dtype=torch.uint8, device=dev)
                        b.write_cqi_epochs_device((step % 2) * half, t, sync=False)
                    b.run_async(half)
                b.sync()
                return CELLS * half * args.steps / (time.perf_counter() - t0)

            modes = ("cycle", "ring_fixed", "ring_randint")
            for m in modes:
                run(m)   # warm-up
            rates = {m: [] for m in modes}
            for _ in range(args.repeats):
                for m in modes:
                    rates[m].append(run(m))
            assert b.cqi_write_status() is None
            line = {"measurement": "ring", "shape": shape, "cells": CELLS, "epochs": n_epochs, "ttis_per_step": half, "steps": args.steps,
                    "kernel": b.kernel_name, "jit": b.jit_status()[0]}
            for m in modes:
                line[m + "_ttis_per_s"] = spread(rates[m])
            for m in modes[1:]:
                line[m + "_over_cycle"] = spread(rates[m])["median"] / spread(rates["cycle"])["median"]
            b.close()
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
