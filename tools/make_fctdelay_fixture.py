#!/usr/bin/env python3
"""Write tests/golden/fctdelay_reducers.json: two small logs in the reference's stderr format, written by radiosaber_amd.logfmt's
BearerLogWriter from synthetic per-bearer rows (no GPU), and what the reference's own reducers of the customised-slice experiment
(get_fct, get_hol and get_throughput of NSDI23-radiosaber-experiments/exp-customization/plot_fctdelay.py) return on them.

    python tools/make_fctdelay_fixture.py --plot-script <path to plot_fctdelay.py>

Only those three function definitions are taken from the script (through ast; its module level draws plots), and they are run
here, in the build container: the fixture holds log text and numbers, no line of the script.  tests/test_flow_logfmt.py checks
logfmt's reducers against it.
"""
import argparse
import ast
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from radiosaber_amd import logfmt  # noqa: E402
from radiosaber_amd.api import SliceConfig  # noqa: E402

OUT = ROOT / "tests" / "golden" / "fctdelay_reducers.json"


def synthetic_log(seed: int, first_ts: int, n_ttis: int):
    """A customised-slice style cell (backlogged, one-flow, two-flow and video slices) with random rows and a consistent record."""
    rng = np.random.default_rng(seed)
    traffic = [{"backlog_flow": 1}, {"internet_flow": 1, "if_bitrate": [12]}, {"internet_flow": 2, "if_bitrate": [9, 3]},
               {"video_app": 1, "video_bitrate": [1280]}]
    sc = SliceConfig([2, 3, 2, 2], traffic=traffic)
    kinds = sc.bearer_kinds()
    U = sc.n_users
    ifb = logfmt.internet_flow_bearers(sc)
    t0 = 0.1 + (first_ts - 100) * 0.001
    ticks = [t0]
    for _ in range(n_ttis - 1):
        ticks.append(ticks[-1] + 0.001)
    by = np.zeros((n_ttis, U, 2), np.int64)
    hol = np.zeros((n_ttis, U, 2), np.float64)
    live = kinds > 0
    by[(rng.random((n_ttis, U, 2)) < 0.5) & live[None]] = 1
    by *= rng.integers(40, 5000, by.shape)
    for u in range(U):
        for k in range(2):
            if kinds[u, k] == 2:
                pick = np.flatnonzero(by[:, u, k])
                hol[pick, u, k] = np.maximum(rng.choice([0.003, 0.00001, 0.0125, 0.1], len(pick)), 0.00001)
    flows, done = {}, {}
    for (u, k) in zip(*np.nonzero(ifb)):
        u, k = int(u), int(k)
        n = int(rng.integers(3, 9))
        t = np.sort(rng.integers(-5, n_ttis, n)) * 0.001 + t0
        sizes = rng.choice([1460, 2920, 4380, 7300, 1490, 58400], n)
        flows[(u, k)] = (t, (sizes // 1490).astype(np.int32), (sizes % 1490).astype(np.int32))
        tti = np.full(n, -1, np.int32)
        tm = np.full(n, -1.0)
        sent = np.flatnonzero(by[:, u, k])
        for i in range(n):
            later = sent[np.asarray(ticks)[sent] >= t[i]]
            if len(later) and rng.random() < 0.8:
                tti[i] = later[min(int(rng.integers(0, 3)), len(later) - 1)]
                tm[i] = ticks[tti[i]]
        done[(u, k)] = (tti, tm)
    rbs = np.repeat(rng.integers(8, 64, (n_ttis, U))[:, :, None], 2, axis=2)
    w = logfmt.BearerLogWriter(logfmt.app_ids(sc), sc.user_to_slice, flows=flows, first_ts=first_ts)
    return w.lines(by, hol, rbs, ticks[0], done)


def load_reducers(script: Path):
    tree = ast.parse(script.read_text())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("get_fct", "get_hol", "get_throughput")]
    assert len(keep) == 3, [n.name for n in keep]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), str(script), "exec"), ns)
    return ns["get_fct"], ns["get_hol"], ns["get_throughput"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plot-script", required=True, type=Path, help="the reference's exp-customization/plot_fctdelay.py")
    a = ap.parse_args()
    get_fct, get_hol, get_throughput = load_reducers(a.plot_script)
    logs = {"fct_hol": synthetic_log(1, 9960, 80), "throughput": synthetic_log(2, 21960, 80)}
    cases = []
    with tempfile.TemporaryDirectory() as d:
        for name, lines in logs.items():
            path = Path(d) / f"{name}.log"
            path.write_text("\n".join(lines) + "\n")
            if name == "fct_hol":
                for lo, hi, prio in ((1, 2, False), (2, 2, True), (0, 3, False), (1, 1, True)):
                    cases.append({"log": name, "fn": "fct", "args": [lo, hi, prio], "out": get_fct(str(path), lo, hi, prio)})
                for lo, hi in ((1, 3), (0, 0), (3, 3)):
                    cases.append({"log": name, "fn": "hol", "args": [lo, hi], "out": get_hol(str(path), lo, hi)})
            else:
                for lo, hi in ((0, 4), (1, 3), (2, 2)):
                    cases.append({"log": name, "fn": "throughput", "args": [lo, hi], "out": get_throughput(str(path), lo, hi)})
    OUT.write_text(json.dumps({"logs": logs, "cases": cases}, indent=1) + "\n")
    print(f"{OUT}: {sum(len(v) for v in logs.values())} log lines, {len(cases)} cases")


if __name__ == "__main__":
    main()
