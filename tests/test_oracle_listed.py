"""rso_cell_allocate_listed (one RBsAllocation() for a listed set of users, the per-user gate an input) tied to the oracle paths
that existed before it: wherever a call of it describes what rso_cell_step / rso_cell_step_queues / rso_cell_allocate already
compute, all seven output fields must be identical.  UNPINNED like those paths (tests/PINS.md): this file shows that the new entry
point is not a free-standing restatement, not that it equals the reference."""
import numpy as np

from conftest import synth_cqi

HIST = (152600, 56656, 270880, 2088792, 3509504, 1595568, 4145392, 5295816, 1903424,
        6890232, 4770864, 2842552, 3579624, 96000, 1227696)
FIELDS = ("target_rbs", "quota_rbgs", "rbg_to_user", "user_nprb", "user_final_cqi", "user_mcs", "user_tbs_bits")


def _same(a, b, msg):
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f"{msg}: {f}")


def _bursts(rng, n_ttis, mean_gap_ms, mean_bytes):
    t, k, out_t, out_b = 0.1, 0, [], []
    while k < n_ttis:
        out_t.append(t)
        out_b.append(int(max(40, rng.exponential(mean_bytes))))
        gap = int(rng.geometric(1.0 / mean_gap_ms))
        k += gap
        t = t + gap / 1000.0
    b = np.array(out_b, np.int64)
    return np.array(out_t), (b // 1490).astype(np.int32), (b % 1490).astype(np.int32)


def _queue_cell(oracle, sched, ues, kinds_of, R, G, seed, n_ttis, mean_bytes, **kw):
    cell = oracle.Cell(ues, R, G, sched, **kw)
    code = {"B": 1, "Q": 2, "-": 0}
    kinds = np.array([[code[kinds_of[s][0]], code[kinds_of[s][1]]] for s in cell.u2s], np.uint8)
    cell.enable_queues(kinds)
    rng = np.random.default_rng(seed)
    for u in range(cell.U):
        for k in range(2):
            if kinds[u, k] == 2:
                cell.set_arrivals(u, k, *_bursts(rng, n_ttis, 5, mean_bytes))
    return cell, kinds


def test_sched7_without_gate_equals_every_tti_of_a_step_run(oracle):
    ues, R, G, n_ttis = [7, 3, 11], 25, 4, 60
    w = [0.5, 0.2, 0.3]
    run = oracle.Cell(ues, R, G, oracle.SCHED_NVS, weights=w)
    one = oracle.Cell(ues, R, G, oracle.SCHED_NVS, weights=w)
    run.set_last_update(0.1)
    first = np.concatenate([[0], np.cumsum(ues)])
    served = set()
    for k, now in enumerate(oracle.clock_ticks(100, n_ttis)):
        if k % 10 == 0:
            cqi = synth_cqi(300 + k, (run.U, R), HIST)
            run.set_cqi(cqi)
            one.set_cqi(cqi)
        a, b = run.new_out(), one.new_out()
        assert run.step(float(now), 0, 0, a) == 0
        s = a.served_slice
        served.add(s)
        ids = np.arange(first[s], first[s + 1], dtype=np.int32)
        avg = run.state()["avg_rate"]  # the averages the allocation of this TTI read (the update precedes it)
        assert one.allocate_listed(avg, b, ids, slice_id=s) == 0
        _same(a, b, f"tti {k} slice {s}")
        assert b.served_slice == s
        assert one.allocate_listed(avg, b, None, slice_id=s) == 0  # NULL list: every user of the slice
        _same(a, b, f"tti {k} slice {s} (no list)")
    assert served == {0, 1, 2}


def test_sched7_gate_reproduces_a_queue_run_where_it_binds(oracle):
    ues, R, G, n_ttis = [6, 9, 4], 25, 4, 120
    cell, _ = _queue_cell(oracle, oracle.SCHED_NVS, ues, ["Q-", "QQ", "Q-"], R, G, 5, n_ttis, 120, alpha=[0, 1, 0], psi=[1, 1, 0])
    rng = oracle.Rng(9)
    calls = bound = diverted = 0
    for k, now in enumerate(oracle.clock_ticks(100, n_ttis)):
        if k % 10 == 0:
            cell.set_cqi(synth_cqi(500 + k, (cell.U, R), HIST))
        a, b, free = cell.new_out(), cell.new_out(), cell.new_out()
        assert cell.step_queues(float(now), rng, a) == 0
        act, _, req = cell.gates()
        ids = np.flatnonzero(act).astype(np.int32)
        if len(ids) == 0:
            assert (a.rbg_to_user < 0).all()
            continue
        avg = cell.state()["avg_rate"]
        assert cell.allocate_listed(avg, b, ids, slice_id=a.served_slice, gate=req[ids]) == 0
        _same(a, b, f"tti {k}")
        assert cell.allocate_listed(avg, free, ids, slice_id=a.served_slice) == 0  # the same call, m_requiredRBs formed inside
        _same(a, free, f"tti {k} (own m_requiredRBs)")
        calls += 1
        bound += int((a.rbg_to_user < 0).sum())
        assert cell.allocate_listed(avg, free, ids, slice_id=a.served_slice, gate=np.full(len(ids), 2**31 - 1)) == 0
        diverted += int(((a.rbg_to_user != free.rbg_to_user) & (a.rbg_to_user >= 0)).sum())
    assert calls > 60 and bound > 0 and diverted > 0, (calls, bound, diverted)


def test_sched1_backlogged_gate_equals_allocate(oracle):
    ues, R, G = [5, 8], 25, 4
    a_cell = oracle.Cell(ues, R, G, oracle.SCHED_PF)
    b_cell = oracle.Cell(ues, R, G, oracle.SCHED_PF)
    rng = np.random.default_rng(3)
    for it in range(6):
        cqi = synth_cqi(40 + it, (a_cell.U, R), HIST)
        a_cell.set_cqi(cqi)
        b_cell.set_cqi(cqi)
        avg = rng.uniform(1e3, 5e6, a_cell.U)
        a, b = a_cell.new_out(), b_cell.new_out()
        assert a_cell.allocate(avg, 0, 0, a) == 0
        assert b_cell.allocate_listed(avg, b, gate=np.full(a_cell.U, 100000000)) == 0
        _same(a, b, f"it {it}")
        assert b_cell.allocate_listed(avg, b, np.arange(a_cell.U)) == 0
        _same(a, b, f"it {it} (listed, no gate)")


def test_sched1_gate_reproduces_a_queue_run(oracle):
    """step_pf_flows races FLOWS (2 * user + bearer); a listed call on a cell whose "users" are those flows, with the run's
    m_dataToTransmit as the gate, gives the same map; the transport blocks add up per user."""
    ues, R, G, n_ttis = [4, 5], 25, 4, 100
    cell, _ = _queue_cell(oracle, oracle.SCHED_PF, ues, ["Q-", "QQ"], R, G, 11, n_ttis, 200)
    U = cell.U
    flows = oracle.Cell([2 * U], R, G, oracle.SCHED_PF)
    rng = oracle.Rng(2)
    calls = left = 0
    for k, now in enumerate(oracle.clock_ticks(100, n_ttis)):
        if k % 10 == 0:
            cqi = synth_cqi(700 + k, (U, R), HIST)
            cell.set_cqi(cqi)
            flows.set_cqi(np.repeat(cqi, 2, axis=0))
        a, b = cell.new_out(), flows.new_out()
        assert cell.step_queues(float(now), rng, a) == 0
        _, data, _ = cell.gates()
        ids = np.flatnonzero(data.reshape(-1) > 0).astype(np.int32)
        if len(ids) == 0:
            assert (a.rbg_to_user < 0).all()
            continue
        avg = cell.bearer_state()["avg_rate"].reshape(-1)
        assert flows.allocate_listed(avg, b, ids, gate=data.reshape(-1)[ids]) == 0
        np.testing.assert_array_equal(a.rbg_to_user, b.rbg_to_user, err_msg=f"tti {k}")
        np.testing.assert_array_equal(a.user_nprb, b.user_nprb.reshape(U, 2).sum(1), err_msg=f"tti {k}")
        np.testing.assert_array_equal(a.user_tbs_bits, b.user_tbs_bits.reshape(U, 2).sum(1), err_msg=f"tti {k}")
        calls += 1
        left += int((a.rbg_to_user < 0).sum())
    assert calls > 50 and left > 0, (calls, left)


def test_transport_schedulers_listing_every_user_equals_allocate(oracle):
    ues, R, G = [6, 5, 0, 7], 25, 4
    w = [0.4, 0.3, 0.1, 0.2]
    for sched in (oracle.SCHED_SEQUENTIAL, oracle.SCHED_MAXCELL):
        a_cell = oracle.Cell(ues, R, G, sched, weights=w)
        b_cell = oracle.Cell(ues, R, G, sched, weights=w)
        rng = np.random.default_rng(sched)
        for it in range(10):
            cqi = synth_cqi(90 + it, (a_cell.U, R), HIST)
            a_cell.set_cqi(cqi)
            b_cell.set_cqi(cqi)
            avg = rng.uniform(1e3, 5e6, a_cell.U)
            r0, r1 = int(rng.integers(0, 2**31 - 1)), int(rng.integers(0, 2**31 - 1))
            a, b = a_cell.new_out(), b_cell.new_out()
            assert a_cell.allocate(avg, r0, r1, a) == 0
            ids = np.arange(a_cell.U) if it % 2 else None
            assert b_cell.allocate_listed(avg, b, ids, rand0=r0, rand1=r1) == 0
            _same(a, b, f"sched {sched} it {it}")
            assert a_cell.state()["slice_state"].tobytes() == b_cell.state()["slice_state"].tobytes()
        assert a_cell.state()["slice_state"].any(), "no slice offset was ever carried"
        out = b_cell.new_out()
        assert b_cell.allocate_listed(avg, out, gate=np.ones(b_cell.U)) == -9  # these schedulers have no per-user gate


def test_listed_call_leaves_a_queue_cell_undisturbed(oracle):
    """`active` is set from the list for the call and restored after it."""
    cell, _ = _queue_cell(oracle, oracle.SCHED_MAXCELL, [3, 4], ["Q-", "Q-"], 12, 2, 4, 20, 400)
    cell.set_cqi(synth_cqi(1, (cell.U, 12), HIST))
    rng, out = oracle.Rng(1), cell.new_out()
    assert cell.step_queues(0.1, rng, out) == 0
    before = [x.copy() for x in cell.gates()]
    assert cell.allocate_listed(np.full(cell.U, 1e5), out, [1, 5]) == 0
    assert set(out.rbg_to_user) <= {1, 5}
    for x, y in zip(before, cell.gates()):
        np.testing.assert_array_equal(x, y)


def test_a_negative_metric_wins_what_the_gate_closes_to_the_others(oracle):
    """Worked by hand.  One slice, 3 users x 2 RBGs of 2 PRBs, every CQI 9, sched 7, metric = kbps(9) / ((1 + avg) / 1000):
    avg = (-3, 1000, 5000) gives (negative, largest, smaller).  required = (5, 2, 0):
    RBG 0: user 2 never competes (0 < 0 is false); user 1's metric is the largest: user 1, who then holds 2 PRBs.
    RBG 1: user 1 is closed (2 < 2 is false), user 2 is closed; user 0's negative metric is above lowest(): user 0.
    Without the gate user 1 takes both."""
    cell = oracle.Cell([3], 2, 2, oracle.SCHED_NVS)
    cell.set_cqi(np.full((3, 2), 9, np.uint8))
    avg = np.array([-3.0, 1000.0, 5000.0])
    out = cell.new_out()
    assert cell.allocate_listed(avg, out, [0, 1, 2], slice_id=0, gate=[5, 2, 0]) == 0
    assert out.rbg_to_user.tolist() == [1, 0]
    assert out.user_nprb.tolist() == [2, 2, 0]
    assert cell.allocate_listed(avg, out, [0, 1, 2], slice_id=0) == 0
    assert out.rbg_to_user.tolist() == [1, 1]
    # among negative metrics the one closer to zero wins, and -0.0 (1 + avg = -inf) beats both
    assert cell.allocate_listed(np.array([-3.0, -5.0, -2.0]), out, slice_id=0) == 0
    assert out.rbg_to_user.tolist() == [1, 1]
    assert cell.allocate_listed(np.array([-3.0, -5.0, -np.inf]), out, slice_id=0) == 0
    assert out.rbg_to_user.tolist() == [2, 2]


def test_a_nan_metric_is_never_picked(oracle):
    """alpha = 1: metric = HoL * pow(se, 1) / pow((1 + avg) / 1000, 1); avg = -1 and HoL = 0 give 0 * inf = NaN, and `NaN > target`
    is false whatever the target (downlink-nvs-scheduler.cpp:298): alone, the user gets nothing; beside a negative metric it loses."""
    cell = oracle.Cell([2], 2, 2, oracle.SCHED_NVS, alpha=[1])
    cell.set_cqi(np.full((2, 2), 9, np.uint8))
    cell.set_queue_state([0.0, 0.5], [1, 1])
    out = cell.new_out()
    assert cell.allocate_listed(np.array([-1.0, -3.0]), out, [0], slice_id=0) == 0
    assert out.rbg_to_user.tolist() == [-1, -1]
    assert cell.allocate_listed(np.array([-1.0, -3.0]), out, [0, 1], slice_id=0) == 0
    assert out.rbg_to_user.tolist() == [1, 1]


def test_the_gpu_cases_meet_their_input_conditions(oracle):
    """The case builders of tests/test_gpu_dropin_oracle.py assert, from the oracle's outputs alone, that a gate left RBGs unallocated
    and diverted RBGs, that a negative metric won and a NaN occurred, and that a flow met the scheduler-1 break with equality.  Run
    them here, where no device is needed, on the smallest grid of each (the device tests run them again on every grid)."""
    import test_gpu_dropin_oracle as T
    for variant, gated in T.VARIANTS7:
        if gated or variant == "anydouble":
            T.cases7(oracle, variant, gated, *T.GRIDS7[2])
    for per_prb in (False, True):
        T.cases1(oracle, 65, *T.GRIDS1[0], per_prb)
    T.group_cases7(oracle, 3, 25, 4)
