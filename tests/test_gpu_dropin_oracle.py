"""Drop-in calls of scheduler 7, of the two per-user gates (rs_tti_in.required_rbs, sched 7; rs_tti_in.data_to_transmit, sched 1) and
of calls that name a subset of the cell's users, against the oracle's per-call entry point rso_cell_allocate_listed: every call, all
seven rs_tti_out fields (and the slice offsets where the scheduler carries them).

UNPINNED (tests/PINS.md): the oracle restates downlink-nvs-scheduler.cpp:275-312 / :360-390, downlink-packet-scheduler.cpp:179-331
and downlink-transport-scheduler.cpp:453-675 from the cited lines; these tests prove device == oracle, not device == reference.

Shapes: the gate race scans users 64 lanes at a time, so the served slice (sched 7) / the flows (sched 1) come in sizes 1, 5 or 12,
63, 64, 65 and 130 -- one chunk, the chunk boundary on both sides and three chunks -- on grids of 25, 64 and 6 RBGs.  The expected
outputs of a case are computed once, on the CPU, before the device is asked; the conditions that keep a case from passing vacuously
(the gate bound and diverted, a negative metric won, a NaN occurred, a flow met `tbs >= data * 8` with equality) are asserted there,
from the inputs and the oracle's outputs alone."""
import numpy as np
import pytest

from conftest import synth_cqi

HIST = (152600, 56656, 270880, 2088792, 3509504, 1595568, 4145392, 5295816, 1903424,
        6890232, 4770864, 2842552, 3579624, 96000, 1227696)
FIELDS = ("target_rbs", "quota_rbgs", "rbg_to_user", "user_nprb", "user_final_cqi", "user_mcs", "user_tbs_bits")
PER_USER = ("user_nprb", "user_final_cqi", "user_mcs", "user_tbs_bits")


# ---------------------------------------------------------------------------------------------------------------------------
# the two sides of one call
# ---------------------------------------------------------------------------------------------------------------------------

def oracle_call(cell, ids, cqi=None, avg_rate=None, slice_id=-1, gate=None, hol_delay=None, prio_has_data=None, cqi_prb=None,
                rand0=0, rand1=0):
    """The oracle's answer to one drop-in call: the call's rows (position i = user ids[i]) scattered into the cell's arrays, then
    rso_cell_allocate_listed.  Users outside the call get CQI 1 and average 1: they are not listed, nothing reads them."""
    ids = np.arange(cell.U) if ids is None else np.asarray(ids)
    if cqi_prb is not None:
        full = np.ones((cell.U, cell.R * cell.rbg_size), np.uint8)
        full[ids] = cqi_prb
        cell.set_cqi_prb(full)
    else:
        full = np.ones((cell.U, cell.R), np.uint8)
        full[ids] = cqi
        cell.set_cqi(full)
    avg = np.ones(cell.U)
    avg[ids] = avg_rate
    if hol_delay is not None:
        hol, prio = np.zeros(cell.U), np.ones(cell.U, np.uint8)
        hol[ids] = hol_delay
        if prio_has_data is not None:
            prio[ids] = prio_has_data
        cell.set_queue_state(hol, prio)
    out = cell.new_out()
    rc = cell.allocate_listed(avg, out, ids.astype(np.int32), slice_id=slice_id, gate=gate, rand0=rand0, rand1=rand1)
    assert rc == 0, f"rso_cell_allocate_listed rc = {rc}"
    rest = np.ones(cell.U, bool)
    rest[ids] = False
    for f in PER_USER:
        assert not getattr(out, f)[rest].any(), f"oracle: {f} of a user outside the call"
    return out


def same_call(res, out, ids, what, upper=False):
    """rs_tti_out (per-user arrays by call position) against the oracle's outputs (by user id): all seven fields."""
    ids = np.arange(len(out.user_nprb)) if ids is None else np.asarray(ids)
    for f in FIELDS:
        want = getattr(out, f)
        np.testing.assert_array_equal(getattr(res, f), want[ids] if f in PER_USER else want, err_msg=f"{what}: {f}")
    if upper:
        np.testing.assert_array_equal(res.upper_rbg, out.upper_rbg, err_msg=f"{what}: upper_rbg")
        np.testing.assert_array_equal(res.upper_user, out.upper_user, err_msg=f"{what}: upper_user")


# ---------------------------------------------------------------------------------------------------------------------------
# scheduler 7
# ---------------------------------------------------------------------------------------------------------------------------

SIZES7 = [1, 5, 63, 64, 65, 130]            # one ragged config: the listed ids of a slice do not start at 0
FIRST7 = np.concatenate([[0], np.cumsum(SIZES7)])
GRIDS7 = [(25, 4), (64, 8), (6, 1)]
CALLS_PER_SIZE = 8
# (variant, with the m_requiredRBs gate)
VARIANTS7 = [("plain", False), ("ties", False), ("latemax", False), ("gate", True), ("custom", False), ("custom", True),
             ("genexp", False), ("genexp", True), ("anydouble", False), ("anydouble", True)]
# the pools of test_drop_in_accepts_any_double (tests/test_gpu_round3.py)
AVG_POOLS = [np.array([1.0, 1e12, 1e300]), np.array([1.0, 3.4e41, 1e38, 1e300]), np.array([1e300]), np.array([np.inf, 1e5]),
             np.array([0.25, 1.0, 1e-300]), np.array([-0.5, -1.0, -3.0, 2.0]), np.array([1.0, 98000.0, 1e12])]
HOL_POOLS = [np.array([1e-5, 0.0, 1e6]), np.array([1e-300, 1e300, 1.0]), np.array([0.0])]


def config7(variant):
    S = len(SIZES7)
    kw = dict(weight=[1.0 / S] * S)
    if variant == "custom":
        kw.update(algo_alpha=[1] * S)
    if variant == "genexp":
        kw.update(algo_epsilon=[3, -1, 2, 3, -1, 2], algo_psi=[2, 2, -1, 2, 2, -1])
    if variant == "anydouble":
        kw.update(algo_alpha=[1, 0, 1, 1, 0, 1])  # HoL 0 x an infinite 1 / (1 + avg) is how a NaN metric arises
    return kw


def _gate_draw(rng, n, G, j):
    """required_rbs of call j of a slice: 0 for everybody once, the edge values {0, 1, G-1, G, G+1, 3G, 1e6, 2^31-1}, uniform 0..40"""
    if j == 0:
        return np.zeros(n, np.int32)
    if j % 2:
        return rng.choice(np.array([0, 1, G - 1, G, G + 1, 3 * G, 10**6, 2**31 - 1], np.int64), n).astype(np.int32)
    return rng.integers(0, 41, n).astype(np.int32)


def cases7(oracle, variant, gated, R, G):
    """[(call kwargs, ids, oracle out)] of one (variant, gate, grid): CALLS_PER_SIZE calls per slice size, sizes interleaved."""
    cfg = config7(variant)
    cell = oracle.Cell(SIZES7, R, G, oracle.SCHED_NVS, weights=cfg["weight"], alpha=cfg.get("algo_alpha"),
                       epsilon=cfg.get("algo_epsilon"), psi=cfg.get("algo_psi"))
    alpha = cfg.get("algo_alpha", [0] * len(SIZES7))
    rng = np.random.default_rng(7000 + 100 * R + 10 * len(variant) + int(gated))
    cases = []
    unallocated = diverted = negative_wins = nans = 0
    for it in range(CALLS_PER_SIZE * len(SIZES7)):
        sl, j = it % len(SIZES7), it // len(SIZES7)
        n = SIZES7[sl]
        ids = np.arange(FIRST7[sl], FIRST7[sl + 1], dtype=np.int32)
        cqi = synth_cqi(7000 + 97 * R + it, (n, R), HIST)
        avg = rng.uniform(1e3, 5e6, n)
        kw = {}
        # identical rows, identical averages: lanes of every chunk hold the same metric, the first user wins -- in the gate variant
        # (one call per size) the first user still below its m_requiredRBs, which a later chunk must not take over with an equal metric
        if variant == "ties" or (variant == "gate" and j == 2):
            cqi = np.repeat(cqi[:1], n, axis=0)
            avg = np.full(n, 98000.0)
        if variant == "latemax":  # the strict maximum sits with the slice's last user (user 129 of the three-chunk slice)
            cqi[-1] = 15
            cqi[:-1] = np.minimum(cqi[:-1], 14)
            avg[-1] = 1.0
        if variant == "genexp":
            avg = np.exp(rng.uniform(np.log(1.0), np.log(5e7), n))
        if variant == "custom":
            kw["hol_delay"] = rng.uniform(1e-5, 0.4, n)
            kw["prio_has_data"] = (rng.random(n) < 0.8).astype(np.uint8)
            if j == 1:  # nobody has prioritized data: every metric is 0, the first eligible user takes the RBG
                kw["prio_has_data"][:] = 0
        if variant == "anydouble":
            avg = rng.choice(AVG_POOLS[it % len(AVG_POOLS)], n)
            if it % len(AVG_POOLS) == 5 and it % len(HOL_POOLS) != 2:
                # averages below -1 alone (the pool's -3 and two more): every metric is negative, and they order among themselves
                avg = rng.choice(np.array([-3.0, -7.0, -1e6]), n)
            kw["hol_delay"] = rng.choice(HOL_POOLS[it % len(HOL_POOLS)], n)
            kw["prio_has_data"] = (rng.random(n) < 0.8).astype(np.uint8)
        need = _gate_draw(rng, n, G, j) if gated else None
        out = oracle_call(cell, ids, cqi, avg, slice_id=sl, gate=need, **kw)
        cases.append((dict(cqi=cqi, avg_rate=avg, user_id=ids, **({"required_rbs": need} if gated else {}), **kw), ids, out))
        # ---- what the case must have exercised, from the inputs and the oracle's outputs
        win = out.rbg_to_user
        if variant == "ties":
            assert (win == ids[0]).all()
        if variant == "latemax":
            assert (win == ids[-1]).all()
        if variant == "custom" and j == 1 and not gated:
            assert (win == ids[0]).all()
        if gated:
            free = oracle_call(cell, ids, cqi, avg, slice_id=sl, **kw)
            unallocated += int((win < 0).sum())
            diverted += int(((win >= 0) & (win != free.rbg_to_user)).sum())
            if j == 0:
                assert (win < 0).all() and not out.user_nprb.any()
            assert (out.user_nprb[ids] < need.astype(np.int64) + G).all()  # at most one RBG beyond m_requiredRBs - 1
        if variant == "anydouble":
            # eps = psi = 1: metric = [HoL *] kbps / ((1 + avg) / 1000): its sign is that of 1 + avg (HoL >= 0), and it is a NaN
            # exactly when HoL = 0 meets 1 + avg = 0 (0 * kbps / 0)
            k = 1.0 + avg
            counts = np.ones(n, bool) if not alpha[sl] else (kw["prio_has_data"] != 0) & (kw["hol_delay"] > 0)
            neg = (k < 0) & counts
            negative_wins += int(neg[win[win >= 0] - ids[0]].sum())
            if alpha[sl]:
                nans += int(((kw["prio_has_data"] != 0) & (kw["hol_delay"] == 0) & (k == 0)).sum())
    if gated:
        assert unallocated > 0, "the m_requiredRBs gate never left an RBG unallocated"
        assert diverted > 0, "the m_requiredRBs gate never took an RBG from the ungated winner"
    if variant == "anydouble":
        assert negative_wins > 0, "no user with a negative metric won an RBG"
        assert nans > 0, "no NaN metric occurred"
    return cfg, cases


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS7, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("variant,gated", VARIANTS7, ids=[v + ("+gate" if g and v != "gate" else "") for v, g in VARIANTS7])
def test_sched7_calls_against_the_oracle(rs, oracle, variant, gated, grid):
    R, G = grid
    cfg, cases = cases7(oracle, variant, gated, R, G)
    ts = rs.TtiScheduler(rs.SliceConfig(SIZES7, **cfg), R, G, sched=7)
    for it, (kw, ids, out) in enumerate(cases):
        same_call(ts.schedule_tti(**kw), out, ids, f"sched 7 {variant} gate {gated} {R}x{G} call {it} (slice of {len(ids)})")
    ts.close()


# ---------------------------------------------------------------------------------------------------------------------------
# scheduler 1: the passed "users" are flows
# ---------------------------------------------------------------------------------------------------------------------------

FLOWS1 = [1, 12, 64, 65, 130]
GRIDS1 = [(25, 4), (64, 8)]


def cases1(oracle, n, R, G, per_prb):
    """8 calls of n flows with data_to_transmit: 0; uniform 20..150 (twice); 100000000 for half the flows; and four calls whose
    flows report one CQI over the whole band and carry exactly tbs // 8 or tbs // 8 + 1 bytes of a one-RBG or a two-RBG block at that
    CQI -- the two sides of `tbs >= data * 8` (downlink-packet-scheduler.cpp:260)."""
    cell = oracle.Cell([n], R, G, oracle.SCHED_PF)
    tabs = oracle.tables()
    rng = np.random.default_rng(1000 + 10 * n + R + int(per_prb))
    cases = []
    left = equal_side = 0
    for it in range(8):
        cqi = synth_cqi(1100 + 31 * n + it, (n, R), HIST)
        avg = rng.uniform(1e3, 5e6, n)
        data = rng.integers(20, 151, n).astype(np.int32)
        edge = it >= 4
        if it == 0:
            data[:] = 0
        if it == 3:
            data[: (n + 1) // 2] = 100000000  # backlogged flows beside the finite ones: they take what the others leave
        if edge:
            cqi = np.repeat(cqi[:, :1], R, axis=1)
            for i in range(n):
                blocks = 1 + (i + it) % 2
                fc = oracle.final_cqi(np.full(blocks * G, cqi[i, 0], np.uint8))
                tbs = oracle.lib().rso_tbs_bits(int(tabs["cqi_to_mcs"][fc - 1]), blocks * G)
                data[i] = tbs // 8 + ((i + it) // 2) % 2
        kw = dict(cqi=cqi, avg_rate=avg, data_to_transmit=data)
        if per_prb:
            prb = np.repeat(cqi, G, axis=1)
            if not edge:  # reports that differ inside an RBG; the metric reads the first PRB of each RBG
                noise = rng.integers(0, 3, prb.shape).astype(np.int64) - 1
                noise[:, ::G] = 0
                prb = np.clip(prb.astype(np.int64) + noise, 1, 15).astype(np.uint8)
            kw = dict(cqi=None, cqi_prb=prb, avg_rate=avg, data_to_transmit=data)
        out = oracle_call(cell, None, cqi, avg, gate=data, cqi_prb=kw.get("cqi_prb"))
        cases.append((kw, None, out))
        left += int((out.rbg_to_user < 0).sum())
        # a flow stops taking RBGs the moment its block carries its data: a final block of exactly data * 8 bits met the '>=' as '=='
        equal_side += int(((out.user_nprb > 0) & (out.user_tbs_bits == data.astype(np.int64) * 8)).sum())
    assert equal_side > 0, "no flow was satisfied on the == side of the break"
    if n * 2 <= R:
        assert left > 0, "every RBG was taken: the satisfied-flow break never emptied the race"
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("per_prb", [False, True], ids=["rbg", "prb"])
@pytest.mark.parametrize("grid", GRIDS1, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("n", FLOWS1)
def test_sched1_gate_against_the_oracle(rs, oracle, n, grid, per_prb):
    R, G = grid
    cases = cases1(oracle, n, R, G, per_prb)
    ts = rs.TtiScheduler(rs.SliceConfig([n]), R, G, sched=1)
    for it, (kw, ids, out) in enumerate(cases):
        same_call(ts.schedule_tti(**kw), out, ids, f"sched 1 n {n} {R}x{G} per_prb {per_prb} call {it}")
    ts.close()


# ---------------------------------------------------------------------------------------------------------------------------
# calls that name a subset of the users: the transport schedulers
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sched", [8, 9, 10, 101, 103])
def test_subset_calls_against_the_oracle(rs, oracle, sched):
    """10 calls, each naming a random ascending subset of 1..U users; call 3 names no user of slice 1 (a slice without a listed user
    has no target and no quota, downlink-transport-scheduler.cpp:463-477); slice_rbs_offset_ is carried across the calls on both
    sides and compared after every one."""
    ues, R, G = [6, 5, 0, 7], 25, 4
    w = [0.4, 0.3, 0.1, 0.2]
    U = sum(ues)
    ts = rs.TtiScheduler(rs.SliceConfig(ues, weight=w), R, G, sched=sched)
    cell = oracle.Cell(ues, R, G, sched, weights=w)
    rng = np.random.default_rng(800 + sched)
    sizes = set()
    for it in range(10):
        ids = np.sort(rng.choice(U, int(rng.integers(1, U + 1)), replace=False)).astype(np.int32)
        if it == 3:
            ids = ids[(ids < 6) | (ids >= 11)]
            ids = ids if len(ids) else np.array([0], np.int32)
        if it == 7:
            ids = np.arange(U, dtype=np.int32)
        sizes.add(len(ids))
        n = len(ids)
        cqi = synth_cqi(8000 + 10 * sched + it, (n, R), HIST)
        avg = rng.uniform(1e3, 5e6, n)
        r0, r1 = int(rng.integers(0, 2**31 - 1)), int(rng.integers(0, 2**31 - 1))
        out = oracle_call(cell, ids, cqi, avg, rand0=r0, rand1=r1)
        if it == 3:
            assert out.quota_rbgs[1] == 0 and out.target_rbs[1] == 0
        res = ts.schedule_tti(cqi, avg, r0, r1, user_id=ids)
        same_call(res, out, ids, f"sched {sched} call {it} ({n} of {U} users)", upper=sched == 10)
        assert ts.slice_offset.tobytes() == cell.state()["slice_state"].tobytes(), f"sched {sched} call {it}: slice offsets"
    assert len(sizes) > 3
    ts.close()


# ---------------------------------------------------------------------------------------------------------------------------
# run-time builds, checked against the built-in kernel on every call (RS_JIT_SELFCHECK=2) and against the oracle here
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_runtime_builds_of_the_gated_calls(rs, oracle, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    R, G = 25, 4
    cfg, cases = cases7(oracle, "gate", True, R, G)
    ts = rs.TtiScheduler(rs.SliceConfig(SIZES7, **cfg), R, G, sched=7, jit=True)
    mine = [c for c in cases if len(c[1]) == 65]
    assert len(mine) == CALLS_PER_SIZE
    for it, (kw, ids, out) in enumerate(mine):
        same_call(ts.schedule_tti(**kw), out, ids, f"sched 7 gate, run-time build, call {it}")
    assert ts.jit_status()[0] == 1, ts.jit_status()
    ts.close()
    ts = rs.TtiScheduler(rs.SliceConfig([65]), R, G, sched=1, jit=True)
    for it, (kw, ids, out) in enumerate(cases1(oracle, 65, R, G, False)):
        same_call(ts.schedule_tti(**kw), out, ids, f"sched 1 gate, run-time build, call {it}")
    assert ts.jit_status()[0] == 1, ts.jit_status()
    ts.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the group surface: every cell against an oracle cell of its own
# ---------------------------------------------------------------------------------------------------------------------------

def _group_calls7(rng, K, R, G, it, ids):
    """One launch's calls.  Cell (it % K) has a sparse gate: three users below 2G PRBs, everybody else at 0, so that most of the
    band stays unallocated; the other cells draw like the single-cell gate variant, where 65 users' needs exceed the band."""
    calls = []
    for k in range(K):
        n = len(ids)
        need = _gate_draw(rng, n, G, 1 + (it + k) % 2)
        if k == it % K:
            few = rng.choice(n, 3, replace=False)
            sparse = np.zeros(n, np.int32)
            sparse[few] = rng.integers(1, 2 * G + 1, 3)
            need = sparse
        calls.append(dict(cqi=synth_cqi(9100 + 17 * it + k, (n, R), HIST), avg_rate=rng.uniform(1e3, 5e6, n), user_id=ids,
                          hol_delay=rng.uniform(1e-5, 0.4, n), prio_has_data=(rng.random(n) < 0.8).astype(np.uint8),
                          required_rbs=need))
    return calls


GROUP7_UES, GROUP7_ALPHA = [5, 65], [1, 1]
GROUP7_IDS = np.arange(5, 70, dtype=np.int32)


def group_cases7(oracle, K, R, G, n_tti=6):
    """(launches, resident): per launch (calls, [oracle out per cell]); the resident launch also carries the averages to set.  The
    gate must have left RBGs unallocated and diverted RBGs from the ungated winner: asserted here, from the oracle's outputs alone."""
    ids = GROUP7_IDS
    cells = [oracle.Cell(GROUP7_UES, R, G, oracle.SCHED_NVS, alpha=GROUP7_ALPHA) for _ in range(K)]
    rng = np.random.default_rng(31)
    launches = []
    unallocated = diverted = 0
    for it in range(n_tti):
        calls = _group_calls7(rng, K, R, G, it, ids)
        outs = []
        for k in range(K):
            kw = {x: calls[k][x] for x in ("cqi", "avg_rate", "hol_delay", "prio_has_data")}
            out = oracle_call(cells[k], ids, slice_id=1, gate=calls[k]["required_rbs"], **kw)
            free = oracle_call(cells[k], ids, slice_id=1, **kw)
            unallocated += int((out.rbg_to_user < 0).sum())
            diverted += int(((out.rbg_to_user >= 0) & (out.rbg_to_user != free.rbg_to_user)).sum())
            outs.append(out)
        launches.append((calls, outs))
    assert unallocated > 0, "the m_requiredRBs gate never left an RBG unallocated"
    assert diverted > 0, "the m_requiredRBs gate never took an RBG from the ungated winner"
    a0 = [rng.uniform(1e3, 5e6, sum(GROUP7_UES)) for _ in range(K)]
    calls = _group_calls7(rng, K, R, G, 99, ids)
    outs = []
    for k in range(K):
        kw = {x: calls[k][x] for x in ("cqi", "hol_delay", "prio_has_data")}
        outs.append(oracle_call(cells[k], ids, avg_rate=a0[k][ids], slice_id=1, gate=calls[k]["required_rbs"], **kw))
        del calls[k]["avg_rate"]
    return launches, (calls, outs, a0)


@pytest.mark.gpu
def test_group_gated_calls_against_the_oracle(rs, oracle):
    """K = 3 cells in one launch: scheduler 7 with the gate on a customised slice of 65 users, scheduler 1 with the gate on 65
    flows; then one resident call of scheduler 7 (rs_group_schedule_tti_at accepts required_rbs: pack_tti is shared), at
    now == last_update so that the resident averages are the ones set."""
    K, R, G = 3, 25, 4
    ids = GROUP7_IDS
    launches, (calls, outs, a0) = group_cases7(oracle, K, R, G)
    g = rs.GroupScheduler(rs.SliceConfig(GROUP7_UES, algo_alpha=GROUP7_ALPHA), R, G, K, sched=7)
    for it, (tti_calls, tti_outs) in enumerate(launches):
        res = g.schedule_tti(tti_calls)
        for k in range(K):
            same_call(res[k], tti_outs[k], ids, f"group sched 7 TTI {it} cell {k}")
    # resident averages
    for k in range(K):
        g.set_avg(k, a0[k], 0.25)
    res = g.schedule_tti_at(calls, 0.25)
    for k in range(K):
        same_call(res[k], outs[k], ids, f"group sched 7 resident call, cell {k}")
    g.close()
    # ---- scheduler 1
    n = 65
    g = rs.GroupScheduler(rs.SliceConfig([n]), R, G, K, sched=1)
    per_cell = [cases1(oracle, n, R, G, False) for _ in range(K)]
    for it in range(8):
        order = [(it + k) % 8 for k in range(K)]  # the cells of one launch run different calls of the series
        res = g.schedule_tti([per_cell[k][order[k]][0] for k in range(K)])
        for k in range(K):
            same_call(res[k], per_cell[k][order[k]][2], None, f"group sched 1 TTI {it} cell {k}")
    g.close()
