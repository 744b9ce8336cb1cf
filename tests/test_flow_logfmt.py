"""The customised-slice experiment's log lines and reducers (no GPU): application ids, the per-bearer counter line of every scheduler,
the ipflow lines and their place around a TTI, and the reducers against what the reference's own get_fct / get_hol /
get_throughput return on the same logs (tests/golden/fctdelay_reducers.json, tools/make_fctdelay_fixture.py)."""
import json

import numpy as np
import pytest

from conftest import GOLDEN
from radiosaber_amd import logfmt
from radiosaber_amd.api import SliceConfig


def _customize():
    cfg = json.loads((GOLDEN / "experiment_configs.json").read_text())["exp-customization/exp-customize-20slices/config.json"]
    return SliceConfig(cfg["ues_per_slice"], cfg["weight"], cfg["algo_alpha"], cfg["algo_beta"], cfg["algo_epsilon"],
                       cfg["algo_psi"], cfg["traffic"])


def test_app_ids_of_the_customize_config():
    sc = _customize()
    ids = logfmt.app_ids(sc)
    first = np.searchsorted(sc.user_to_slice, np.arange(20))
    # slices 0-4: one backlogged flow per UE (54 UEs), ids 0..53 at priority 0
    assert ids[0].tolist() == [0, -1] and ids[first[5] - 1].tolist() == [53, -1]
    # slices 5-9: one InternetFlow per UE; the first UE of slice 5 is user 54
    assert first[5] == 54 and ids[54].tolist() == [54, -1]
    # slices 10-14: two InternetFlows per UE (priorities 0 and 1), after the 47 UEs of slices 5-9
    assert first[10] == 101 and ids[101].tolist() == [101, 102]
    # slices 15-19: one video application per UE, after the 55 two-flow UEs
    assert first[15] == 156 and ids[156].tolist() == [211, -1]
    assert sc.n_users == 194 and ids[193].tolist() == [248, -1]
    live = ids >= 0
    assert (live == (sc.bearer_kinds() > 0)).all()
    assert sorted(ids[live].tolist()) == list(range(249))
    ifb = logfmt.internet_flow_bearers(sc)
    assert ifb[54].tolist() == [True, False] and ifb[101].tolist() == [True, True] and not ifb[156].any() and not ifb[0].any()


def test_app_ids_without_traffic_are_user_ids():
    sc = SliceConfig([3, 2])
    assert logfmt.app_ids(sc)[:, 0].tolist() == [0, 1, 2, 3, 4]
    assert (logfmt.app_ids(sc)[:, 1] == -1).all()


@pytest.mark.parametrize("x,s", [(0.0, "0"), (0.003, "0.003"), (0.00001, "1e-05"), (0.0125, "0.0125"), (0.1234567, "0.123457"),
                                 (1.0, "1"), (0.0030000000000001137, "0.003"), (123456.0, "123456"), (1234567.0, "1.23457e+06"),
                                 (0.000123, "0.000123")])
def test_doubles_print_like_an_ostream(x, s):
    assert logfmt.fmt_double(x) == s


def _two_user_writer(pf_flows=False):
    sc = SliceConfig([1, 1], traffic=[{"internet_flow": 2, "if_bitrate": [9, 3]}, {"backlog_flow": 1}])
    flows = {(0, 0): (np.array([0.1, 0.1, 0.1025]), np.array([1, 0, 2], np.int32), np.array([10, 700, 0], np.int32)),
             (0, 1): (np.array([0.101]), np.array([0], np.int32), np.array([300], np.int32))}
    return logfmt.BearerLogWriter(logfmt.app_ids(sc), sc.user_to_slice, pf_flows=pf_flows, flows=flows), sc


def test_counter_and_ipflow_lines_around_a_tti():
    w, sc = _two_user_writer()
    n, U = 4, 2
    by = np.zeros((n, U, 2), np.int64)
    hol = np.zeros((n, U, 2))
    by[0, 0, 0], hol[0, 0, 0] = 1000, 0.00001
    by[1, 0, 0], hol[1, 0, 0] = 1200, 0.001
    by[1, 0, 1], hol[1, 0, 1] = 310, 0.00001
    by[1, 1, 0] = 5000
    by[3, 0, 0], hol[3, 0, 0] = 3000, 0.0005
    rbs = np.full((n, U, 2), 8)
    t = [0.1]
    for _ in range(n - 1):
        t.append(t[-1] + 0.001)
    done = {(0, 0): (np.array([1, 1, 3], np.int32), np.array([t[1], t[1], t[3]])), (0, 1): (np.array([1], np.int32), np.array([t[1]]))}
    lines = w.lines(by, hol, rbs, t[0], done)
    assert lines == [
        "ipflow start app: 0 flow: 0 flowsize: 1500",
        "ipflow start app: 0 flow: 1 flowsize: 700",
        "100 app: 0 cumu_bytes: 1000 cumu_rbs: 8 hol_delay: 1e-05 user: 0 slice: 0",
        "ipflow start app: 1 flow: 0 flowsize: 300",
        "101 app: 1 cumu_bytes: 310 cumu_rbs: 8 hol_delay: 1e-05 user: 0 slice: 0",   # priority 1 before 0 (transport, NVS)
        f"ipflow end app: 1 flow: 0 fct: {t[1] - 0.101:g} flowsize: 300 priority: 1",
        "101 app: 0 cumu_bytes: 2200 cumu_rbs: 16 hol_delay: 0.001 user: 0 slice: 0",
        f"ipflow end app: 0 flow: 0 fct: {t[1] - 0.1:g} flowsize: 1500 priority: 0",
        f"ipflow end app: 0 flow: 1 fct: {t[1] - 0.1:g} flowsize: 700 priority: 0",
        "101 app: 2 cumu_bytes: 5000 cumu_rbs: 8 hol_delay: 0 user: 1 slice: 1",
        "ipflow start app: 0 flow: 2 flowsize: 2980",   # time 0.1025: the first TTI whose clock is >= it is TTI 3
        "103 app: 0 cumu_bytes: 5200 cumu_rbs: 24 hol_delay: 0.0005 user: 0 slice: 0",
        f"ipflow end app: 0 flow: 2 fct: {t[3] - 0.1025:g} flowsize: 2980 priority: 0",
    ]
    assert all(len(x.split()) == 13 for x in lines if x[0].isdigit())
    # the next launch continues the stamps and the counters
    more = w.lines(by[:1], hol[:1], rbs[:1], t[3] + 0.001, None)
    assert more == ["104 app: 0 cumu_bytes: 6200 cumu_rbs: 32 hol_delay: 1e-05 user: 0 slice: 0"]


def test_dl_pf_bearer_order_and_flow_prbs():
    w, sc = _two_user_writer(pf_flows=True)
    by = np.zeros((1, 2, 2), np.int64)
    by[0, 0] = [100, 200]
    rbg_to_user = np.array([[0, 1, 1, -1, 2]])  # flow ids 2 * user + priority
    rbs = logfmt.bearer_prbs(rbg_to_user, np.zeros((1, 2), np.int32), 4, pf_flows=True)
    assert rbs[0].tolist() == [[4, 8], [4, 0]]
    lines = w.lines(by, np.zeros((1, 2, 2)), rbs, 0.1, None)
    assert [x for x in lines if x[0].isdigit()] == ["100 app: 0 cumu_bytes: 100 cumu_rbs: 4 hol_delay: 0 user: 0 slice: 0",
                                                   "100 app: 1 cumu_bytes: 200 cumu_rbs: 8 hol_delay: 0 user: 0 slice: 0"]
    # transport / NVS schedulers: the user's PRBs go to every bearer that transmitted
    assert logfmt.bearer_prbs(np.array([[0, 1]]), np.array([[8, 4]]), 4)[0].tolist() == [[8, 8], [4, 4]]


def test_rows_of_a_batch_without_queues_give_the_old_counter_lines():
    """One backlogged bearer per UE: the same lines as stderr_lines."""
    rng = np.random.default_rng(3)
    tbs = rng.integers(0, 4, (6, 5)) * rng.integers(100, 3000, (6, 5))
    rbg = rng.integers(-1, 5, (6, 7))
    nprb = rng.integers(0, 30, (6, 5))
    u2s = [0, 0, 1, 1, 1]
    old = logfmt.stderr_lines(tbs, rbg, u2s, 4, nprb=nprb)
    sc = SliceConfig([2, 3])
    by, hol = logfmt.bearer_rows_from_users(tbs)
    w = logfmt.BearerLogWriter(logfmt.app_ids(sc), sc.user_to_slice, pf_flows=False)
    assert w.lines(by, hol, logfmt.bearer_prbs(rbg, nprb, 4), 0.1) == old
    # ... and the base class's "flow:" line when asked for it
    old_pf = logfmt.stderr_lines(tbs, rbg, u2s, 4, nprb=nprb, pf_format=True)
    w = logfmt.BearerLogWriter(logfmt.app_ids(sc), sc.user_to_slice, flow_format=True)
    assert w.lines(by, hol, logfmt.bearer_prbs(rbg, nprb, 4), 0.1) == old_pf


def test_reducers_equal_the_reference_reducers_on_the_fixture_logs():
    fx = json.loads((GOLDEN / "fctdelay_reducers.json").read_text())
    fns = {"fct": logfmt.fct_from_log, "hol": logfmt.hol_from_log, "throughput": logfmt.slice_throughput_window}
    seen = set()
    for case in fx["cases"]:
        got = fns[case["fn"]](fx["logs"][case["log"]], *case["args"])
        assert got == case["out"], case
        seen.add(case["fn"])
        if case["out"]:
            seen.add(case["fn"] + "+")
    assert seen == {"fct", "hol", "throughput", "fct+", "hol+", "throughput+"}


def test_fct_reducer_rules():
    lines = ["ipflow start app: 7 flow: 0 flowsize: 100",            # app 7 never scheduled: kept whatever the slice
             "ipflow start app: 1 flow: 0 flowsize: 100",
             "ipflow start app: 2 flow: 0 flowsize: 100",
             "100 app: 1 cumu_bytes: 5 cumu_rbs: 8 hol_delay: 0.002 user: 1 slice: 3",
             "100 app: 2 cumu_bytes: 5 cumu_rbs: 8 hol_delay: 0 user: 2 slice: 9",
             "ipflow end app: 1 flow: 0 fct: 0.004 flowsize: 100 priority: 1",
             "ipflow end app: 2 flow: 0 fct: 0.5 flowsize: 100 priority: 0",
             "10001 app: 1 cumu_bytes: 9 cumu_rbs: 16 hol_delay: 0.1 user: 1 slice: 3",
             "ipflow start app: 1 flow: 1 flowsize: 100",            # after ts_shoot: not counted
             "ipflow end app: 1 flow: 1 fct: 0.2 flowsize: 100 priority: 1",
             "ipflow end app: 7 flow: 0 fct: 0.3 flowsize: 100 priority: 0"]
    assert logfmt.fct_from_log(lines, 3, 5) == [0.3, 0.004]
    assert logfmt.fct_from_log(lines, 3, 5, priority_only=True) == [0.004]
    assert logfmt.fct_from_log(lines, 9, 9) == [0.3, 0.5]
    assert logfmt.hol_from_log(lines, 3, 3) == [0.002, 0.1]
