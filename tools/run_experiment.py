#!/usr/bin/env python3
"""What one line of the reference's experiment scripts does (NSDI23-radiosaber-experiments/*/run_*.sh):

    LTE-Sim SingleCellWithI 1 <sched> 1 30 <seed> <duration_s> <config.json>   2> <log>

on the GPU: one cell, the CQI traces and mapping file of the reference's cqi-traces-noise0 directory (or, without --traces,
synthetic grids drawn from the traces' CQI histogram), and the reference's stderr lines (what plot_*.py parse) written to --log.

    python tools/run_experiment.py --sched 9 --seed 0 --duration 12 --config <config.json> \\
        --traces <dir with ue*.log and mapping.config> --log maxcell_pf0.log

Every scheduler writes the per-bearer DoStopSchedule line "<ts> app: A cumu_bytes: B cumu_rbs: K hol_delay: H user: U slice: S"
(logfmt.BearerLogWriter).  Scheduler 1 too: DL_PF_PacketScheduler::DoStopSchedule prints that line, not the base class's
"<ts> flow: A cumu_bytes: B cumu_rbs: K hol_delay: H" line -- except that a backlogged configuration keeps, by default, the "flow:"
line earlier versions of this tool wrote for it (--sched1-line auto; `app` gives the reference's line there too).  A config with
internet_flow / video_app applications (exp-customization) runs on the queue model: InternetFlow bursts from
rs_internet_flow_arrivals at the config's rates, the video applications from the 1 280 kbit/s foreman trace
(tests/golden/video_foreman_1280k.json, --video-trace), and the log also carries the "ipflow start" / "ipflow end" lines of the
InternetFlow flows, with flow completion times from the batch's flow completion record.  --records takes the same lines from
unlogged launches: the device writes one 32-byte record per credited bearer instead of dense per-TTI rows, and the log is identical.
A backlogged configuration takes --records too: one 32-byte record per grant (run_grant_records), the same log.

Several runs in one launch: the reference's scripts start one process per (configuration file, seed) of a directory -- config-pf.json and
config-mt.json times nine seeds -- and a batch runs them as cells of one launch (per-cell configurations).  Name the
configuration files (--config a.json b.json: any numbers of slices and of users -- exp-fix20slices' 5, 10, 15 and 20 UEs per slice go
together, and so do exp-fixranues' 5, 10, 15 and 20 slices; the batch is created at the largest of each, the smaller cells' maps end
in absent users and their rows in absent slices), the seeds (--seeds 0,1,2)
and a --log template with {config} (the file's name without .json) and {seed}; --mapping takes the same two fields.  Every log is byte
for byte the log of the single run of its (configuration, seed).  Backlogged configurations only; scheduler 11 runs one cell per process.

    python tools/run_experiment.py --sched 9 --duration 12 --config config-pf.json config-mt.json --seeds 0,1,2,3,4,5,6,7,8 \\
        --records --log 'maxcell_{config}_{seed}.log'

The scheduler's arithmetic is bit-exact; the position of the libc rand() stream at the first scheduled TTI depends on
simulator set-up code outside this path (103 300 draws for the 100-UE configuration) and is taken
from --rand-skip, and the flow sizes come from our generator's own rand() stream per bearer (rs_internet_flow_arrivals), not
from the simulator's shared one: runs are statistically, not bitwise, those of the reference.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import radiosaber_amd as rs  # noqa: E402
from radiosaber_amd import logfmt  # noqa: E402

COMMON_SEEDS = (805290992, 749913912, 965326802, 697084729, 1518010490, 56234558, 1511265396, 1412837728, 947674421)

ap = argparse.ArgumentParser()
ap.add_argument("--sched", type=int, default=9, help="the reference's CLI scheduler number: 1, 7, 8, 9, 10, 11")
ap.add_argument("--seed", type=int, default=0, help="index into the reference's nine common seeds")
ap.add_argument("--duration", type=float, default=12.0, help="simulated seconds after the 0.1 s start-up")
ap.add_argument("--config", required=True, nargs="+", help="slice configuration JSON of the experiment directory; several files (any numbers "
                                                         "of slices and of users) run as cells of one batch")
ap.add_argument("--seeds", default=None, help="comma-separated indices into the nine common seeds: every configuration runs with each of "
                                              "them, all in one batch (instead of --seed)")
ap.add_argument("--traces", default=None, help="directory with ue<id>.log and the mapping file (default: synthetic CQI grids)")
ap.add_argument("--mapping", default="mapping.config", help="the mapping file's name in --traces; may carry {config} and {seed}")
ap.add_argument("--nb-rbs", type=int, default=512)
ap.add_argument("--rbg-size", type=int, default=8)
ap.add_argument("--rand-skip", type=int, default=0)
ap.add_argument("--video-trace", default=str(ROOT / "tests" / "golden" / "video_foreman_1280k.json"),
                help="frame sizes and times of the video applications (JSON: time_ms, bytes)")
ap.add_argument("--sched1-line", choices=("auto", "app", "flow"), default="auto",
                help="scheduler 1's counter line: app (DL_PF_PacketScheduler's own), flow (the base class's); auto = app with the queue "
                     "model, flow for backlogged configurations (this tool's earlier format)")
ap.add_argument("--log", default="-", help="where the stderr-format lines go ('-' = stdout); with several runs a template with {config} and/or {seed}")
ap.add_argument("--records", action="store_true",
                help="unlogged launches that return one record per credited bearer (queue-model configurations: run_records) or per grant "
                     "(backlogged configurations: run_grant_records) instead of logged launches with dense rows; the log is the same")
a = ap.parse_args()

# the runs: every configuration with every seed, in this order the cells of one batch
seed_ids = [int(x) for x in a.seeds.split(",")] if a.seeds is not None else [a.seed]
runs = [(Path(path).name[:-5] if path.endswith(".json") else Path(path).name, rs.SliceConfig.from_json(path), k) for path in a.config for k in seed_ids]
n_cells = len(runs)
# the batch is created at the largest slice count and the largest user count: a configuration that has both, else an even split
S_max, U_max = max(cfg.n_slices for _, cfg, _ in runs), max(cfg.n_users for _, cfg, _ in runs)
sc = next((cfg for _, cfg, _ in runs if cfg.n_slices == S_max and cfg.n_users == U_max), None)
if sc is None:
    if U_max < S_max:
        raise SystemExit(f"several runs in one batch: {S_max} slices need at least as many users (the largest configuration has {U_max})")
    sc = rs.SliceConfig([U_max // S_max + (1 if s < U_max % S_max else 0) for s in range(S_max)])
R = a.nb_rbs // a.rbg_size
n_ttis = int(round(a.duration * 1000))
U = sc.n_users
seeds = [COMMON_SEEDS[k] if 0 <= k < 9 else COMMON_SEEDS[0] for _, _, k in runs]
seed = seeds[0]
queues = any(int(t.get("internet_flow", 0)) or int(t.get("video_app", 0)) for _, cfg, _ in runs for t in cfg.traffic)
if a.records and not queues and a.sched == 11:
    raise SystemExit("--records: scheduler 11 writes no grant records (its kernel is another one)")
logs = [a.log.format(config=name, seed=k) for name, _, k in runs]
if n_cells > 1:
    if queues:
        raise SystemExit("several runs in one batch: backlogged configurations only (the queue model keeps one configuration per batch)")
    if a.sched == 11:
        raise SystemExit("several runs in one batch: scheduler 11 reads one configuration (its kernel is another one)")
    if len(set(logs)) != n_cells:
        raise SystemExit("several runs in one batch: --log needs {config} and / or {seed} so that every run has a log of its own")
# (the queue model's batches run without the PHY error model's draws: its parity with the oracle is pinned that way)
b = rs.BatchScheduler(sc, R, a.rbg_size, n_cells, sched=a.sched, phy_error_draws=not queues, jit=True)
if n_cells > 1:
    b.set_cell_configs([cfg for _, cfg, _ in runs])
b.seed(np.array(seeds, np.uint32), np.full(n_cells, a.rand_skip, np.int64))
if a.traces:
    maps = []
    for name, cfg, k in runs:
        mapping = rs.read_trace_mapping(Path(a.traces) / a.mapping.format(config=name, seed=k))
        row = np.zeros(U, np.int32)  # (the entries of a smaller cell's absent users are stored and ignored)
        row[:cfg.n_users] = mapping[np.arange(cfg.n_users) % len(mapping)]
        maps.append(row)
    trace, mixed = rs.load_trace_dir(a.traces, n_traces=int(max(m.max() for m in maps)) + 1, nb_rbs=a.nb_rbs, rbg_size=a.rbg_size)
    if mixed:
        raise SystemExit(f"{mixed} RBGs carry different CQI on their PRBs: the batched replay needs uniform RBGs")
    b.set_trace(trace, np.stack(maps))
elif n_cells == 1:
    b.synthesize_cqi(seed, (n_ttis + 39) // 40)
else:
    # a single run draws its grids under (its seed, cell 0) at its own user count: each distinct (seed, user count)'s grids are drawn
    # that way once, on the device, and uploaded as the epoch grids of the cells that run with them (an absent user's rows: any valid
    # CQI, stored and ignored)
    drawn = {}
    for sd, (_, cfg, _) in zip(seeds, runs):
        if (sd, cfg.n_users) in drawn:
            continue
        one = rs.BatchScheduler(cfg, R, a.rbg_size, 1, sched=a.sched)
        one.synthesize_cqi(sd, (n_ttis + 39) // 40)
        grid = one.download_cqi_epochs(0)
        one.close()
        drawn[(sd, cfg.n_users)] = np.concatenate([grid, np.ones((grid.shape[0], U - cfg.n_users, R), grid.dtype)], axis=1)
    b.upload_cqi_epochs(np.stack([drawn[(sd, cfg.n_users)] for sd, (_, cfg, _) in zip(seeds, runs)]))

flows = {}
if queues:
    # the applications of single-cell-with-interference.h:308-440, started at 0.1 s and stopped at the end of the run
    stop = 0.1 + n_ttis / 1000.0
    u2s = sc.user_to_slice
    bursts = {}
    video = None
    for u in range(U):
        tr = sc.traffic[u2s[u]]
        for j in range(int(tr.get("internet_flow", 0))):
            rate = tr["if_bitrate"][j] / sc.ues_per_slice[u2s[u]]  # single-cell-with-interference.h:415-416
            bursts[(0, u, j)] = rs.internet_flow_arrivals(rate, 0.1, stop, 1000 * seed_ids[0] + 2 * u + j)
            flows[(u, j)] = bursts[(0, u, j)]
        if int(tr.get("video_app", 0)) and not int(tr.get("internet_flow", 0)):
            if video is None:
                video = json.loads(Path(a.video_trace).read_text())
            t, ts = 0.1, []
            for k in range(len(video["bytes"])):  # TraceBased::Send: the next frame TimeToSend * 0.001 after this one
                if k:
                    t = (video["time_ms"][k] - video["time_ms"][k - 1]) * 0.001 + t
                if t >= stop:
                    break
                ts.append(t)
            bursts[(0, u, 0)] = rs.frames_to_bursts(ts, video["bytes"][:len(ts)])
    b.set_bearers(sc.bearer_kinds())
    b.set_arrivals(bursts)

flow_line = a.sched == 1 and (a.sched1_line == "flow" or (a.sched1_line == "auto" and not queues))
writers = [logfmt.BearerLogWriter(logfmt.app_ids(cfg), cfg.user_to_slice, pf_flows=queues and a.sched == 1, flows=flows, flow_format=flow_line)
           for _, cfg, _ in runs]
outs = [sys.stdout if path == "-" else open(path, "w") for path in logs]
done = 0
while done < n_ttis:  # logged launches of at most 2 000 TTIs keep the host log small
    n = min(2000, n_ttis - done)
    t_first = b.clock()[0]
    if a.records and not queues:
        # a backlogged batch: one record per grant; the rows the writer reads are rebuilt from them (the map is not among them)
        for c, recs in enumerate(b.run_grant_records(n)):
            rows = logfmt.rows_from_grant_records(recs, n, runs[c][1].n_users, R, done, with_map=False)
            by, hol = logfmt.bearer_rows_from_users(rows["tbs_bits"])
            rbs = logfmt.bearer_prbs(np.zeros((n, R), np.int16), rows["uinfo"] & 0xFFFF, a.rbg_size)
            lines = writers[c].lines(by, hol, rbs, float(t_first[c]), None)
            outs[c].write("\n".join(lines) + ("\n" if lines else ""))
        done += n
        continue
    if a.records:
        records = b.run_records(n)[0]
        rec = {(u, k): v for (c, u, k), v in b.flow_record().items() if (u, k) in flows}
        lines = writers[0].record_lines(records, float(t_first[0]), n, rec)
        outs[0].write("\n".join(lines) + ("\n" if lines else ""))
        done += n
        continue
    got = b.run_logged(n, bearers=queues)
    for c in range(n_cells):
        nu = runs[c][1].n_users  # (a cell of fewer users than the batch's: its rows are the first nu)
        if queues:
            by, hol = got["bearer_bytes"][c], got["bearer_hol"][c]
            rec = {(u, k): v for (cc, u, k), v in b.flow_record().items() if (u, k) in flows}
        else:
            by, hol = logfmt.bearer_rows_from_users(got["tbs_bits"][c][:, :nu])
            rec = None
        rbs = logfmt.bearer_prbs(got["rbg_to_user"][c], got["nprb"][c][:, :nu], a.rbg_size, pf_flows=queues and a.sched == 1)
        lines = writers[c].lines(by, hol, rbs, float(t_first[c]), rec)
        outs[c].write("\n".join(lines) + ("\n" if lines else ""))
    done += n
for out in outs:
    if out is not sys.stdout:
        out.close()
if n_cells == 1:
    print(f"{n_ttis} TTIs, {U} UEs, sched {a.sched}: per-slice Mbps " +
          " ".join(f"{x:.2f}" for x in (np.asarray(b.slice_bytes(), np.float64) * 8 / 1e6 / a.duration)), file=sys.stderr)
else:
    totals = b.slice_totals()["cum_bytes"]
    for c, (name, cfg, k) in enumerate(runs):
        print(f"{name} seed {k}: {n_ttis} TTIs, {cfg.n_users} UEs, sched {a.sched}: per-slice Mbps " +
              " ".join(f"{x:.2f}" for x in (totals[c][:cfg.n_slices].astype(np.float64) * 8 / 1e6 / a.duration)), file=sys.stderr)
b.close()
