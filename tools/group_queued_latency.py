#!/usr/bin/env python3
"""us per group call with resident bearers (rs_group_schedule_tti_queued) against what a finite-queue binding had before -- a resident
call followed by rs_group_set_pending per cell -- and, as the regression check, the plain and the resident call, which another
checkout can be measured on as well (profiles/group_queued.md).

    python tools/group_queued_latency.py [--variant plain|resident|resident+pending|queued|queued-spec|queued+host|counted|counted-spec|all|flows|flows-spec|plain-pf+host] [--calls 300]
    RS_TREE=<another checkout> python tools/group_queued_latency.py --variant plain     # that tree's package
    python tools/group_queued_latency.py --variant queued-spec --cells 27 --shapes 500x25x4 500x64x8 --sched 9 7

queued-spec: the queued call after rs_group_specialize_queued (profiles/group_queued_specialize.md); its warm-up holds the builds'
checked calls.  queued+host: the queued call followed by what a binding did on the CPU before rs_group_schedule_tti_counted --
DoStopSchedule's credit loop restated in numpy from user_tbs_bits and the data words, and the per-bearer byte and RB counters kept in
host arrays; counted: the counted call, which returns the bytes sent and keeps the counters on the device
(profiles/group_counted.md).  counted-spec / flows-spec: the counted call after rs_group_specialize_counted and the flows call after
rs_group_specialize_flows (profiles/group_counted_flows_specialize.md); their warm-up holds the builds' checked calls, as queued-spec's
does.  Workloads by default: 8 and 64 cells; 500 users x 25 RBGs and 100 users x 64 RBGs; scheduler 9; cqi_epoch on (new
reports every 40 calls).  --shapes takes users x RBGs x PRBs per RBG (20 equal slices).  Scheduler 7 names the users of one slice per
call, the slice rotating with the call, and gives no required_rbs.  Timed through the Python layer, marshalling included, like
tools/group_resident_latency.py: three repetitions per line, whose spread is the yardstick for a difference between lines; p50 / p99
are taken over the timed calls of all three.

flows / plain-pf+host (profiles/group_flows.md; not part of `all`): scheduler 1 whatever --sched says.  Every user has bearer 0 and
every fifth user bearer 1 as well, all with data, so a call holds 1.2 x users positions and the group is created with that many.
flows: rs_group_schedule_tti_flows, everything on the device.  plain-pf+host: what a scheduler-1 host did before -- per cell the
EWMA of every bearer in numpy, rs_group_schedule_tti with the flows' averages and the data_to_transmit gate, then
DL_PF_PacketScheduler::DoStopSchedule's credit (pending bytes, byte and RB counters per bearer) in numpy; it runs on an older checkout
too (RS_TREE)."""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, os.environ.get("RS_TREE", str(Path(__file__).resolve().parents[1])))
import radiosaber_amd as rs  # noqa: E402

VARIANTS = ("plain", "resident", "resident+pending", "queued", "queued-spec", "queued+host", "counted", "counted-spec")
FLOW_VARIANTS = ("flows", "flows-spec", "plain-pf+host")


def host_ewma(avg, pend, has, now, last):
    """UpdateAverageTransmissionRate of every existing bearer of one cell on the host, [U][2] arrays"""
    rate = (pend * np.int32(8)).astype(np.float64) / (now - last)
    a = ((1 - 0.02) * avg) + (0.02 * rate)
    avg[has] = np.where(a < 1, 1.0, a)[has]
    pend[has] = 0


def run_flows(variant, U, R, G, K, calls_n, warmup):
    """one line of the flows comparison"""
    uid = np.sort(np.concatenate([np.arange(U), np.arange(0, U, 5)])).astype(np.int32)
    fb = np.zeros(len(uid), np.uint8)
    fb[1:][uid[1:] == uid[:-1]] = 1
    F = len(uid)
    cap = -(-F // 20) * 20
    sc = rs.SliceConfig([cap // 20] * 20, weight=[0.05] * 20)
    g = rs.GroupScheduler(sc, R, G, K, sched=rs.RS_SCHED_PF)
    rng = np.random.default_rng(1)
    cqi = [rng.integers(1, 16, (U, R)).astype(np.uint8)[uid] for _ in range(K)]
    has = np.zeros((cap, 2), bool)
    has[uid, fb] = True
    avg = [np.where(has, rng.uniform(1e4, 1e6, (cap, 2)), 0.0) for _ in range(K)]
    data = np.where(fb == 0, 100000000, 300).astype(np.int32)
    pend = [np.zeros((cap, 2), np.int32) for _ in range(K)]
    host_bytes = [np.zeros((cap, 2), np.int64) for _ in range(K)]
    host_rbs = [np.zeros((cap, 2), np.int64) for _ in range(K)]
    if variant == "flows-spec":
        g.specialize_flows()
    if variant in ("flows", "flows-spec"):
        for k in range(K):
            g.set_flows(k, has, avg[k], 0.1)
    now, best, each = 0.1, [], []
    for rep in range(3):
        t0 = 0.0
        for i in range(warmup + calls_n):
            if i == warmup:
                t0 = time.perf_counter()
            last, now = now, now + 0.001
            calls = [dict(cqi=cqi[k], user_id=uid, data_to_transmit=data, cqi_epoch=1 + i // 40) for k in range(K)]
            t1 = time.perf_counter()
            if variant in ("flows", "flows-spec"):
                for k in range(K):
                    calls[k]["flow_bearer"] = fb
                g.schedule_tti_flows(calls, now)
            else:
                for k in range(K):
                    host_ewma(avg[k], pend[k], has, now, last)
                    calls[k]["avg_rate"] = avg[k][uid, fb]
                    del calls[k]["user_id"]  # (the plain call takes a user once: the host names its flows by position)
                res = g.schedule_tti(calls)
                for k in range(K):
                    sent = res[k].user_tbs_bits // 8
                    pend[k][uid, fb] += sent
                    host_bytes[k][uid, fb] += sent
                    host_rbs[k][uid, fb] += np.where(sent > 0, res[k].user_nprb, 0)
            if i >= warmup:
                each.append((time.perf_counter() - t1) * 1e6)
        best.append((time.perf_counter() - t0) / calls_n * 1e6)
    print(f"{K:3d} cells x {U} UEs ({F} flows) x {R} RBGs, {variant:16s}: " + " / ".join(f"{b:.1f}" for b in best) + f" us per call (python), p50 {np.percentile(each, 50):.1f} p99 {np.percentile(each, 99):.1f}, sched 1, {g.kernel_name}",
          flush=True)
    g.close()


def host_credit(res, data, ids, cum_bytes, cum_rbs):
    """DoStopSchedule's loop of one slot on the host, vectorised over the call positions: bearer 1 first, min(available, data) each,
    then m_cumulateBytes / m_cumulateRBs of the credited bearers"""
    available = res.user_tbs_bits // 8
    sent = np.zeros_like(data)
    sent[:, 1] = np.minimum(available, data[:, 1])
    sent[:, 0] = np.minimum(available - sent[:, 1], data[:, 0])
    rows = slice(None) if ids is None else ids
    cum_bytes[rows] += sent
    cum_rbs[rows] += np.where(sent > 0, res.user_nprb[:, None], 0)
    return sent
ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="all", choices=VARIANTS + ("all",) + FLOW_VARIANTS)
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--warmup", type=int, default=40)
ap.add_argument("--cells", type=int, nargs="+", default=[8, 64])
ap.add_argument("--shapes", nargs="+", default=["100x64x8", "500x25x4"], help="users x RBGs x PRBs per RBG")
ap.add_argument("--sched", type=int, nargs="+", default=[9])
args = ap.parse_args()

if args.variant in FLOW_VARIANTS:
    for shape in args.shapes:
        U, R, G = (int(v) for v in shape.split("x"))
        for K in args.cells:
            run_flows(args.variant, U, R, G, K, args.calls, args.warmup)
    sys.exit(0)

for sched, shape in ((s, x) for s in args.sched for x in args.shapes):
    U, R, G = (int(v) for v in shape.split("x"))
    ues = U // 20
    assert U == 20 * ues, "users: a multiple of 20 (20 equal slices)"
    for K in args.cells:
        sc = rs.SliceConfig([ues] * 20, weight=[0.05] * 20)
        for variant in (VARIANTS if args.variant == "all" else (args.variant,)):
            if variant == "queued-spec" and not hasattr(rs.GroupScheduler, "specialize_queued"):
                continue  # (RS_TREE names a checkout from before rs_group_specialize_queued)
            if variant == "counted" and not hasattr(rs.GroupScheduler, "schedule_tti_counted"):
                continue  # (... from before rs_group_schedule_tti_counted)
            if variant == "counted-spec" and not hasattr(rs.GroupScheduler, "specialize_counted"):
                continue  # (... from before rs_group_specialize_counted)
            g = rs.GroupScheduler(sc, R, G, K, sched=sched)
            if variant == "queued-spec":
                g.specialize_queued()
            if variant == "counted-spec":
                g.specialize_counted()
            rng = np.random.default_rng(1)
            cqi = [rng.integers(1, 16, (U, R)).astype(np.uint8) for _ in range(K)]
            avg = [rng.uniform(1e4, 1e6, U) for _ in range(K)]
            pending = np.full(U, 300, np.int32)
            data = np.tile(np.array([100000000, 300], np.int32), (U, 1))
            for k in range(K):
                if variant in ("resident", "resident+pending"):
                    g.set_avg(k, avg[k], 0.1)
                if variant in ("queued", "queued-spec", "queued+host", "counted", "counted-spec"):
                    g.set_bearers(k, np.ones((U, 2), bool), np.stack([avg[k], avg[k][::-1]], axis=1), 0.1)
                if variant in ("counted", "counted-spec"):
                    g.set_counters(k)
            host_bytes = [np.zeros((U, 2), np.int64) for _ in range(K)]
            host_rbs = [np.zeros((U, 2), np.int64) for _ in range(K)]
            now, best, each = 0.1, [], []
            for rep in range(3):
                t0 = 0.0
                for i in range(args.warmup + args.calls):
                    if i == args.warmup:
                        t0 = time.perf_counter()
                    now += 0.001
                    calls = [dict(cqi=cqi[k], rand0=123 + i, rand1=456 + i, cqi_epoch=1 + i // 40) for k in range(K)]
                    ids = None
                    if sched == 7:  # the served slice's users, a new slice (and a new image) every 40 calls
                        ids = np.arange(ues, dtype=np.int32) + ues * ((i // 40) % 20)
                        for k in range(K):
                            calls[k].update(cqi=cqi[k][ids], user_id=ids)
                    t1 = time.perf_counter()
                    if variant == "plain":
                        for k in range(K):
                            calls[k]["avg_rate"] = avg[k]
                        g.schedule_tti(calls)
                    elif variant in ("queued", "queued-spec", "queued+host", "counted", "counted-spec"):
                        for k in range(K):
                            calls[k]["data_to_transmit"] = data if ids is None else data[ids]
                        if variant in ("counted", "counted-spec"):
                            g.schedule_tti_counted(calls, now)
                        else:
                            res = g.schedule_tti_queued(calls, now)
                            if variant == "queued+host":
                                for k in range(K):
                                    host_credit(res[k], calls[k]["data_to_transmit"], ids, host_bytes[k], host_rbs[k])
                    else:
                        g.schedule_tti_at(calls, now)
                        if variant == "resident+pending":
                            for k in range(K):
                                g.set_pending(k, pending)
                    if i >= args.warmup:
                        each.append((time.perf_counter() - t1) * 1e6)
                best.append((time.perf_counter() - t0) / args.calls * 1e6)
            print(f"{K:3d} cells x {U} UEs x {R} RBGs, {variant:16s}: " + " / ".join(f"{b:.1f}" for b in best) + f" us per call (python), p50 {np.percentile(each, 50):.1f} p99 {np.percentile(each, 99):.1f}, sched {sched}, {g.kernel_name}",
                  flush=True)
            g.close()
