"""GPU: the batch queue model on the directed edge populations of tests/queue_edges.py -- device == oracle == plain per-packet model.

Every population (exact fits, runs of full packets, many head advances in one grant, arrival instants, the split over two bearers, the
two gates of schedulers 1 and 7: tests/test_queue_edge_inputs.py proves on the CPU that each edge occurs and that the oracle agrees
with the plain model) runs through the built-in kernel, the run-time build with the bearers' words in LDS and the one with them in HBM,
logged, once as a single launch and once as launches of one TTI each (every fragment chain and every pending DoStopSchedule then
crosses a launch boundary, the head burst's cached shape is reloaded from HBM); and through one unlogged launch of the lean build.
Everything is compared exactly, floating-point values bitwise.  PARITY UNPINNED like the queue model itself (tests/PINS.md)."""
import numpy as np
import pytest

import queue_edges as qe

pytestmark = pytest.mark.gpu

LOGGED = [("built-in", dict(jit=False)), ("lds", dict(jit=True, queue_state_lds=1)), ("hbm", dict(jit=True, queue_state_lds=-1))]
_CACHE = {}


def _expected(oracle, name):
    """(population, stepped oracle, plain model's [cells][T][U][2] credited bytes and HoL, its completion TTIs): computed once per family"""
    if name not in _CACHE:
        pops = _CACHE.setdefault("populations", {p.name: p for p in qe.all_populations(oracle)})
        p = pops[name]
        run = qe.oracle_run(oracle, p)
        credited = np.zeros((p.n_cells, p.n_ttis, p.n_users, 2), np.int64)
        hol = np.zeros((p.n_cells, p.n_ttis, p.n_users, 2), np.float64)
        done = {}
        for c in range(p.n_cells):
            for u, m in enumerate(qe.plain_cell(oracle, p, run, c)):
                credited[c, :, u], hol[c, :, u] = m["credited"], m["hol"]
                for k, tti in m["done"].items():
                    done[(c, u, k)] = tti
        _CACHE[name] = (p, run, credited, hol, done)
    return _CACHE[name]


def _batch(rs, p, **kw):
    sc = rs.SliceConfig(p.ues, algo_alpha=p.alpha or [], algo_beta=p.beta or [])
    b = rs.BatchScheduler(sc, p.R, p.G, p.n_cells, sched=p.sched, **kw)
    b.set_bearers(p.kind_codes())
    b.set_arrivals(p.bursts)
    if kw.get("jit"):
        assert b.jit_status()[0] == 1, b.jit_status()
    b.seed(p.seeds())
    b.upload_cqi_epochs(p.grids())
    return b


def _check_final(rs, p, run, done, b, what):
    rec, bst, st = b.flow_record(), b.bearer_state(), b.state()
    assert rec.keys() == run["done"].keys() == done.keys()
    for key, (tti, tm) in run["done"].items():
        np.testing.assert_array_equal(rec[key][0], tti, err_msg=f"{what}: done_tti of {key}")
        np.testing.assert_array_equal(rec[key][0], done[key], err_msg=f"{what}: done_tti of {key} against the plain model")
        assert rec[key][1].tobytes() == tm.tobytes(), f"{what}: done_time of {key}"
    for key in ("cum_bytes", "cum_rbs", "queue_bytes", "queue_packets"):
        np.testing.assert_array_equal(bst[key], run[key][:, -1], err_msg=f"{what}: {key}")
    live = np.broadcast_to(p.kind_codes() != rs.BEARER_NONE, bst["avg_rate"].shape)
    assert bst["avg_rate"][live].tobytes() == run["avg_rate"][live].tobytes(), f"{what}: bearer PF averages"
    assert st["slice_state"].tobytes() == run["slice_state"].tobytes(), f"{what}: slice state"
    np.testing.assert_array_equal(st["cum_bytes"], run["cum_bytes"][:, -1].sum(-1), err_msg=f"{what}: per-user bytes")


def test_the_bearer_codes_are_the_populations(rs):
    assert (rs.BEARER_NONE, rs.BEARER_BACKLOG, rs.BEARER_QUEUE) == (qe.KIND["-"], qe.KIND["B"], qe.KIND["Q"]) and rs.FULL_PACKET == qe.FULL


@pytest.mark.parametrize("split", ["one-launch", "one-tti-launches"])
@pytest.mark.parametrize("variant", [v[0] for v in LOGGED])
@pytest.mark.parametrize("family", list(qe.FAMILY_CELLS))
def test_logged_launches_on_the_edge_populations(rs, oracle, family, variant, split):
    p, run, credited, hol, done = _expected(oracle, family)
    what = f"{family}, {variant}, {split}"
    b = _batch(rs, p, **dict(LOGGED)[variant])
    got = [b.run_logged(n, bearers=True) for n in ([p.n_ttis] if split == "one-launch" else [1] * p.n_ttis)]
    if variant != "built-in":
        assert b.jit_status()[0] == 1, b.jit_status()
    cat = {k: np.concatenate([g[k] for g in got], axis=1) for k in ("rbg_to_user", "tbs_bits", "bearer_bytes", "bearer_hol")}
    np.testing.assert_array_equal(cat["rbg_to_user"], run["maps"], err_msg=f"{what}: RBG map")
    np.testing.assert_array_equal(cat["tbs_bits"], run["tbs"], err_msg=f"{what}: TBS")
    np.testing.assert_array_equal(cat["bearer_bytes"], run["bearer_bytes"], err_msg=f"{what}: bearer bytes")
    np.testing.assert_array_equal(cat["bearer_bytes"], credited, err_msg=f"{what}: bearer bytes against the plain model")
    bad = np.argwhere(cat["bearer_hol"] != run["bearer_hol"])[:5].tolist()
    assert cat["bearer_hol"].tobytes() == run["bearer_hol"].tobytes() == hol.tobytes(), f"{what}: HoL delays at {bad}"
    _check_final(rs, p, run, done, b, what)
    b.close()


@pytest.mark.parametrize("family", list(qe.FAMILY_CELLS))
def test_one_unlogged_launch_of_the_lean_build(rs, oracle, family, monkeypatch):
    monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    p, run, _, _, done = _expected(oracle, family)
    b = _batch(rs, p, jit=True)
    b.run(p.n_ttis)
    assert b.jit_status()[0] == 1 and "unavailable" not in b.jit_status()[1], b.jit_status()
    _check_final(rs, p, run, done, b, f"{family}, lean build")
    b.close()
