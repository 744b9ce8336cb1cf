"""GPU: the queue model's flow completion record (rs_batch_flow_record) and per-bearer DoStopSchedule rows
(rs_batch_run_logged_bearers) against the CPU oracle, stepped one TTI at a time.

PARITY UNPINNED like the queue model itself (tests/PINS.md): what the oracle's packet-level queues (rso_cell_step_queues) imply --
a burst completes in the first TTI after whose DoStopSchedule the dequeued packets (arrived up to t_k minus queued) cover it; a
bearer's head-of-line delay is t_k minus the time stamp of its head burst before that TTI's dequeue, at least 1e-5."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, synth_cqi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HIST = (152600, 56656, 270880, 2088792, 3509504, 1595568, 4145392, 5295816, 1903424,
        6890232, 4770864, 2842552, 3579624, 96000, 1227696)


def _customize_case(rs, n_cells, n_ttis):
    cfg = json.loads((GOLDEN / "experiment_configs.json").read_text())["exp-customization/exp-customize-20slices/config.json"]
    sc = rs.SliceConfig(cfg["ues_per_slice"], cfg["weight"], cfg["algo_alpha"], cfg["algo_beta"], cfg["algo_epsilon"],
                        cfg["algo_psi"], cfg["traffic"])
    video = json.loads((GOLDEN / "video_foreman_1280k.json").read_text())
    stop = 0.1 + n_ttis / 1000.0 + 0.01
    bursts = {}
    for c in range(n_cells):
        for u in range(sc.n_users):
            tr = cfg["traffic"][sc.user_to_slice[u]]
            for j in range(int(tr["internet_flow"])):
                rate = tr["if_bitrate"][j] / cfg["ues_per_slice"][sc.user_to_slice[u]]
                bursts[(c, u, j)] = rs.internet_flow_arrivals(rate, 0.1, stop, 1000 * c + 2 * u + j)
            if int(tr["video_app"]):
                t, ts = 0.1, []
                for k in range(len(video["bytes"])):
                    if k:
                        t = (video["time_ms"][k] - video["time_ms"][k - 1]) * 0.001 + t
                    if t >= stop:
                        break
                    ts.append(t)
                bursts[(c, u, 0)] = rs.frames_to_bursts(ts, video["bytes"][:len(ts)])
    return sc, sc.bearer_kinds(), bursts, 64, 8


def _short_gap_bursts(rng, n_ttis, mean_gap_ms, mean_bytes):
    """Bursts on the applications' millisecond grid with short gaps; every fourth one a whole number of full packets (last = 0)."""
    t, ts, sizes, k = 0.1, [], [], 0
    while True:
        gap = int(rng.geometric(1.0 / mean_gap_ms)) if ts else 0
        k += gap
        if k >= n_ttis + 5:
            break
        t = t + gap / 1000.0 if gap else t
        ts.append(t)
        n = int(max(40, rng.exponential(mean_bytes)))
        sizes.append(max(1, n // 1490) * 1490 if len(ts) % 4 == 0 else n)
    b = np.array(sizes, np.int64)
    return np.array(ts), (b // 1490).astype(np.int32), (b % 1490).astype(np.int32)


def _random_case(rs, n_cells, n_ttis, seed):
    ues = [6, 5, 7, 4]
    sc = rs.SliceConfig(ues, algo_alpha=[1, 1, 1, 0], algo_beta=[1, 0, 0, 0])
    code = {"B": rs.BEARER_BACKLOG, "Q": rs.BEARER_QUEUE, "-": rs.BEARER_NONE}
    kinds = np.array([[code[x] for x in ("QQ", "Q-", "BQ", "Q-")[s]] for s in sc.user_to_slice], np.uint8)
    rng = np.random.default_rng(seed)
    bursts = {(c, u, k): _short_gap_bursts(rng, n_ttis, 2, 3000)
              for c in range(n_cells) for u in range(sc.n_users) for k in range(2) if kinds[u, k] == rs.BEARER_QUEUE}
    return sc, kinds, bursts, 25, 4


def _oracle_expect(rs, oracle, sc, kinds, bursts, R, G, sched, grids, seeds, n_ttis):
    """Step the oracle TTI by TTI: per-bearer bytes and HoL rows, and the completion TTI / clock of every burst."""
    ticks = oracle.clock_ticks(100, n_ttis)
    n_cells = grids.shape[0]
    U = sc.n_users
    exp_bytes = np.zeros((n_cells, n_ttis, U, 2), np.int64)
    exp_hol = np.zeros((n_cells, n_ttis, U, 2), np.float64)
    done = {}
    for c in range(n_cells):
        cell = oracle.Cell(sc.ues_per_slice, R, G, sched, weights=sc.weight, alpha=sc.algo_alpha, beta=sc.algo_beta,
                           epsilon=sc.algo_epsilon, psi=sc.algo_psi)
        cell.enable_queues(kinds)
        for (cc, u, k), (t, nf, la) in bursts.items():
            if cc == c:
                cell.set_arrivals(u, k, t, nf, la)
        rng = oracle.Rng(int(seeds[c]))
        out = cell.new_out()
        cum = np.zeros((n_ttis + 1, U, 2), np.int64)
        qpk = np.zeros((n_ttis, U, 2), np.int64)
        for n in range(n_ttis):
            if n % 40 == 0:
                cell.set_cqi(grids[c, n // 40])
            assert cell.step_queues(float(ticks[n]), rng, out) == 0
            st = cell.bearer_state()
            cum[n + 1], qpk[n] = st["cum_bytes"], st["queue_packets"]
        exp_bytes[c] = np.diff(cum, axis=0)
        for (cc, u, k), (t, nf, la) in bursts.items():
            if cc != c:
                continue
            pk = np.cumsum(np.asarray(nf, np.int64) + (np.asarray(la) > 0))
            n_arr = np.searchsorted(t, ticks, side="right")
            arrived = np.where(n_arr > 0, pk[np.maximum(n_arr - 1, 0)], 0)
            dequeued = arrived - qpk[:, u, k]
            before = np.concatenate([[0], dequeued[:-1]])  # dequeued before this TTI's DoStopSchedule
            tti = np.searchsorted(dequeued, pk, side="left")  # first TTI whose dequeued count covers the burst
            tti = np.where(tti < n_ttis, tti, -1).astype(np.int32)
            done[(c, u, k)] = (tti, np.where(tti >= 0, ticks[np.maximum(tti, 0)], -1.0))
            for n in np.flatnonzero(exp_bytes[c, :, u, k] > 0):
                if arrived[n] - before[n] > 0:
                    h = int(np.searchsorted(pk, before[n], side="right"))
                    hol = ticks[n] - t[h]
                    exp_hol[c, n, u, k] = hol if hol >= 0.00001 else 0.00001
    return exp_bytes, exp_hol, done


def _batch(rs, sc, kinds, bursts, R, G, sched, grids, seeds, **kw):
    b = rs.BatchScheduler(sc, R, G, grids.shape[0], sched=sched, **kw)
    b.set_bearers(kinds)
    b.set_arrivals(bursts)
    b.seed(seeds)
    b.upload_cqi_epochs(grids)
    return b


def _check_record(got, want, what):
    assert got.keys() == want.keys()
    for key in want:
        np.testing.assert_array_equal(got[key][0], want[key][0], err_msg=f"{what}: done_tti of {key}")
        assert got[key][1].tobytes() == want[key][1].tobytes(), f"{what}: done_time of {key}"


def _run_variants(rs, oracle, case, sched, n_ttis, launches, every_kind=True):
    sc, kinds, bursts, R, G = case
    n_cells = 2
    grids = synth_cqi(11 + sched, (n_cells, (n_ttis + 39) // 40, sc.n_users, R), HIST)
    seeds = np.array([21, 22], np.uint32)
    exp_bytes, exp_hol, done = _oracle_expect(rs, oracle, sc, kinds, bursts, R, G, sched, grids, seeds, n_ttis)
    # what the record must show: flows split over several TTIs, several completions in one TTI, bursts with last_bytes = 0
    split = multi = whole = 0
    for (c, u, k), (tti, _) in done.items():
        t, nf, la = bursts[(c, u, k)]
        ok = tti >= 0
        size = nf.astype(np.int64) * 1490 + la
        split += int((size[ok] > exp_bytes[c, tti[ok], u, k]).sum())
        multi += int((np.bincount(tti[ok]) >= 2).sum()) if ok.any() else 0
        whole += int((la[ok] == 0).sum())
    assert split > 0 and (not every_kind or (multi > 0 and whole > 0)), (split, multi, whole)
    variants = [("built-in", dict(jit=False)),
                ("run-time, LDS words, self-check on", dict(jit=True, queue_state_lds=1, selfcheck=1)),
                ("run-time, HBM words, self-check off", dict(jit=True, queue_state_lds=-1, selfcheck=-1))]
    for name, kw in variants:
        b = _batch(rs, sc, kinds, bursts, R, G, sched, grids, seeds, **kw)
        if kw["jit"]:
            assert b.jit_status()[0] == 1, b.jit_status()
        got = [b.run_logged(n, bearers=True) for n in launches]
        rec = b.flow_record()
        if kw.get("selfcheck") == 1:
            assert b.jit_status()[0] == 1 and "agree" in b.jit_status()[1], b.jit_status()
        b.close()
        by = np.concatenate([g["bearer_bytes"] for g in got], axis=1)
        ho = np.concatenate([g["bearer_hol"] for g in got], axis=1)
        np.testing.assert_array_equal(by, exp_bytes, err_msg=f"{name}: bearer bytes")
        assert ho.tobytes() == exp_hol.tobytes(), f"{name}: bearer HoL delays ({np.argwhere(ho != exp_hol)[:5].tolist()})"
        _check_record(rec, done, name)
    # one long unlogged launch (the lean build when it qualifies): the same record
    b = _batch(rs, sc, kinds, bursts, R, G, sched, grids, seeds, jit=True)
    b.run(n_ttis)
    _check_record(b.flow_record(), done, "unlogged launch")
    b.close()
    return sum(int((tti >= 0).sum()) for tti, _ in done.values())


@pytest.mark.parametrize("sched", [1, 7, 9])
def test_flow_record_and_bearer_rows_of_the_customize_experiment(rs, oracle, sched):
    n_ttis = 420
    # (InternetFlow's sizes are never whole packets, and its flows start at least a millisecond apart: the short-gap case below has those)
    n_done = _run_variants(rs, oracle, _customize_case(rs, 2, n_ttis), sched, n_ttis, [1, 159, 260], every_kind=False)
    assert n_done > 100


@pytest.mark.parametrize("sched", [1, 7, 9])
def test_flow_record_with_short_gaps(rs, oracle, sched):
    n_ttis = 400
    n_done = _run_variants(rs, oracle, _random_case(rs, 2, n_ttis, 40 + sched), sched, n_ttis, [137, 263])
    assert n_done > 300


def test_flow_record_is_not_in_the_checkpoint(rs, oracle):
    """A resumed batch records the flows that complete after the resume, exactly as the uninterrupted batch did."""
    sc, kinds, bursts, R, G = _random_case(rs, 2, 400, 5)
    grids = synth_cqi(3, (2, 10, sc.n_users, R), HIST)
    seeds = np.array([7, 8], np.uint32)
    n1, n2 = 170, 230
    for jit in (False, True):
        a = _batch(rs, sc, kinds, bursts, R, G, 9, grids, seeds, jit=jit)
        a.run(n1)
        blob = a.checkpoint()
        a.run(n2)
        full = a.flow_record()
        a.close()
        b = _batch(rs, sc, kinds, bursts, R, G, 9, grids, seeds, jit=jit)
        assert all((tti == -1).all() for tti, _ in b.flow_record().values())
        b.restore(blob)
        b.run(n2)
        res = b.flow_record()
        b.close()
        late = 0
        for key, (tti, tm) in full.items():
            after = tti >= n1
            late += int(after.sum())
            np.testing.assert_array_equal(res[key][0], np.where(after, tti, -1), err_msg=f"{key} jit={jit}")
            assert res[key][1].tobytes() == np.where(after, tm, -1.0).tobytes(), f"{key} jit={jit}"
        assert late > 100


def test_run_experiment_writes_the_customize_outputs(rs, tmp_path):
    """tools/run_experiment.py on the customised-slice configuration with the three schedulers of its run script: the reducers find
    completed flows in slices 5-9 and 10-14 and HoL samples in 15-19; scheduler 1's counter lines carry the 13 fields of the
    app: .. user: .. slice: line."""
    from radiosaber_amd import logfmt
    cfg = json.loads((GOLDEN / "experiment_configs.json").read_text())["exp-customization/exp-customize-20slices/config.json"]
    ref_cfg = {"ues_per_slice": cfg["ues_per_slice"], "slices": [
        dict(n_slices=1, weight=cfg["weight"][s], algo_alpha=cfg["algo_alpha"][s], algo_beta=cfg["algo_beta"][s],
             algo_epsilon=cfg["algo_epsilon"][s], algo_psi=cfg["algo_psi"][s], **cfg["traffic"][s]) for s in range(20)]}
    path = tmp_path / "config.json"
    path.write_text(json.dumps(ref_cfg))
    for sched, name in ((1, "single"), (7, "nvs"), (9, "maxcell")):
        log = tmp_path / f"{name}_0.log"
        r = subprocess.run([sys.executable, str(ROOT / "tools" / "run_experiment.py"), "--config", str(path), "--sched", str(sched),
                            "--duration", "2", "--log", str(log)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = log.read_text().splitlines()
        counters = [ln for ln in lines if ln.split()[0].isdigit()]
        assert counters and all(len(ln.split()) == 13 for ln in counters), name
        assert len(logfmt.fct_from_log(lines, 5, 9)) > 50, name
        assert len(logfmt.fct_from_log(lines, 10, 14, priority_only=True)) > 10, name
        assert len(logfmt.hol_from_log(lines, 15, 19)) > 100, name
