"""The inter-slice policies (rs_interslice.h) and the UpperBound path on the directed inputs of tests/interslice_edges.py:
GreedyByRow pairs in which a slice closes on the even RBG and still holds the odd RBG's maximum, SubOpt's equal losses behind zero
to three rehashes of the `slice_fewer` hashtable, Vogel differences of exactly 2.0 against a running maximum of 2, the records
at which MaximizeCell's scan closes a slice or makes its last grant around positions 63, 64 and 128, UpperBound's ties at the
cut key, quotas that are negative, zero or above R, and S and R of 32, 33 and 64.  tests/test_interslice_edge_inputs.py proves on
the CPU that the cases bind (every mutant model differs on at least three of them) and that the oracle equals the plain models on
them; here the kernels meet them on every surface that runs the step: drop-in calls (built-in and run-time builds, subset calls),
group calls (plain and resident) and batches (built-in and run-time builds, one unlogged lean launch for scheduler 9).  Every
comparison is bitwise: device == oracle on every output field, and the RBG-to-slice map, read through user_to_slice, == the plain
model (scheduler 10: upper_rbg / upper_user against the model where it is whole, its order-free facts above 16 RBGs, and
device == oracle alone for the one case whose quota exceeds R, where the reference reads past its vector).

Found by these tests: no difference between the kernels, the oracle and the plain models.  Writing them showed two inputs of
VogelApproximate that no TTI can produce -- the 1.0 of a lone empty slice and all slices closed before the RBGs run out: the
quota step gives a slice without a listed user the quota 0 and makes the quotas sum to R -- so those stay CPU cases of the bare
policy function; and that SubOpt without its clamp of negative quotas computes the same map as with it (interslice_edges'
docstring), so no case can tell the two apart."""
import numpy as np
import pytest

import interslice_edges as ie
from test_gpu_dropin_oracle import same_call
from test_gpu_quota_edges import call_kw, config_of
from test_interslice_edge_inputs import check_upper, eff_and_quota, oracle_answer, plain_map, slice_map
from test_quota_edge_inputs import arrays, case_ids, oracle_cell

pytestmark = pytest.mark.gpu

FAMILY_OF = {sched: f for f, sched in ie.SCHED_OF.items()}
SCHEDS = (8, 9, 10, 101, 103)


def report(what, family, cs):
    """every case of the family ran on this surface"""
    print(f"inter-slice edge cases run, {what}: {family} {len(cs)}")
    assert len(cs) == len(ie.cases(family)) and {c.name for c in cs} == {c.name for c in ie.cases(family)}, what


def check_policy(oracle, c, sched, rbg_to_user, eff, quota, what, upper=None):
    """the device's map (scheduler 10: its lists) against the plain model of the scheduler's policy on (eff, quota)"""
    if sched == 10:
        if upper is not None:
            checked = check_upper(c, eff, quota, upper[0], upper[1], what)
            assert checked != bool(c.plants.get("oracle_only")), what
        elif c.R <= 16 and max(quota) <= c.R:
            # a batch logs no lists: the map reports, per RBG, the user of the lowest slice that took it
            lists = ie.plain_upper_bound(eff, quota)
            want = [min([s for s, rbgs in lists.items() if r in rbgs], default=-1) for r in range(c.R)]
            assert slice_map(c, rbg_to_user) == want, f"{what}: RBG-to-slice map against the plain model"
        return
    assert slice_map(c, rbg_to_user) == plain_map(oracle, FAMILY_OF[sched], eff, quota), f"{what}: RBG-to-slice map against the plain model"


def check_call(oracle, res, c, sched, what):
    out, after = oracle_answer(oracle, c, sched)
    same_call(res, out, case_ids(c), what, upper=sched == 10)
    assert res.quota_rbgs.tolist() == c.plants["quota"], f"{what}: the planted quotas"
    eff, quota = eff_and_quota(c, out)
    check_policy(oracle, c, sched, res.rbg_to_user, eff, quota, what, upper=(res.upper_rbg, res.upper_user) if sched == 10 else None)
    return after


# ---------------------------------------------------------------------------------------------------------------------------
# drop-in calls
# ---------------------------------------------------------------------------------------------------------------------------

def _dropin(rs, oracle, sched, cs, jit):
    builds = 0
    for group in ie.by_config(cs):
        ts = rs.TtiScheduler(config_of(rs, group[0]), group[0].R, group[0].G, sched=sched, jit=jit)
        for rnd in range(2 if jit else 1):    # (a run-time build's first calls run beside the built-in kernel)
            for c in group:
                what = f"sched {sched} {'run-time build' if jit else 'built-in'} {c.name}"
                ts.slice_offset = c.state
                res = ts.schedule_tti(**call_kw(c))
                after = check_call(oracle, res, c, sched, what)
                assert ts.slice_offset.tobytes() == after.tobytes(), f"{what}: slice offsets afterwards"
        if jit:
            assert ts.jit_status()[0] == 1, ts.jit_status()
            builds += 1
        ts.close()
    return builds


@pytest.mark.parametrize("sched", SCHEDS)
def test_dropin_calls(rs, oracle, sched):
    """Every case of the scheduler's family through the built-in kernel: slice_offset set, one call (a subset call where the case
    lists its users), every output field, the map against the plain model, slice_offset afterwards.  Scheduler 9's built-in kernel
    takes the fixed-point vector scan up to 32 RBGs -- with 32-bit RBG and slice sets where S <= 32 too (4 x 4, 25 x 20, 32 x 32,
    8 x 6, the tiny shapes), 64-bit sets otherwise -- and the record-at-a-time scan above (33 x 33, 64 x 64)."""
    family = FAMILY_OF[sched]
    cs = ie.cases(family)
    _dropin(rs, oracle, sched, cs, False)
    report(f"drop-in sched {sched}", family, cs)


@pytest.mark.parametrize("sched", SCHEDS)
def test_dropin_runtime_builds(rs, oracle, sched):
    """The context's own build on 20 users x 25 RBGs, 32 x 32 and 33 x 33, every case of those shapes twice over.  S = 20 and 32:
    SubOpt ranks the slices in registers (kRegs), Vogel's masks are 32-bit; S = R = 33: the walk over the hash order and 64-bit
    masks in a build with constant shape.  MaximizeCell's scan (the dispatch in rs_phase_p4_serial.inc): 20 x 25 and 32 x 32 take
    the scan over the sort loop's unsorted segments, with 32-bit sets (K32), where the build's sort runs in registers (the host
    picks EPT > 0), and the vector form with 32-bit sets otherwise; 33 x 33 is above RS_VEC_MAX_R and takes the record-at-a-time
    scan."""
    family = FAMILY_OF[sched]
    cs = [c for c in ie.cases(family) if c.plants["shape"] in ie.JIT_SHAPES]
    shapes = {c.plants["shape"] for c in cs}
    assert shapes == ({"A20"} if sched == 10 else set(ie.JIT_SHAPES)), shapes
    builds = _dropin(rs, oracle, sched, cs, True)
    assert builds == len(shapes) <= 3
    print(f"inter-slice edge cases run, drop-in run-time builds sched {sched}: {family} {len(cs)} on {builds} adopted builds")


# ---------------------------------------------------------------------------------------------------------------------------
# group calls
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [9, 101, 103])
def test_group_calls_plain_and_resident(rs, oracle, sched):
    """One group per configuration, one case per cell: set_slice_offset, one plain launch; the offsets again, set_avg, one resident
    launch at now == last_update (the averages are used as given).  The group kernels are built-in ones: scheduler 9 scans as in
    test_dropin_calls (the vector form up to 32 RBGs, record at a time above)."""
    family = FAMILY_OF[sched]
    cs = ie.cases(family)
    for group in ie.by_config(cs):
        g = rs.GroupScheduler(config_of(rs, group[0]), group[0].R, group[0].G, len(group), sched=sched)
        for form in ("plain", "resident"):
            calls = [call_kw(c) for c in group]
            for k, c in enumerate(group):
                g.set_slice_offset(k, c.state)
            if form == "plain":
                res = g.schedule_tti(calls)
            else:
                for k, c in enumerate(group):
                    g.set_avg(k, arrays(c)[1], 0.1)
                    del calls[k]["avg_rate"]
                res = g.schedule_tti_at(calls, 0.1)
            for k, c in enumerate(group):
                what = f"group sched {sched} {form} {c.name}"
                after = check_call(oracle, res[k], c, sched, what)
                assert g.slice_offset(k).tobytes() == after.tobytes(), f"{what}: slice offsets afterwards"
        g.close()
    report(f"group sched {sched}", family, cs)


# ---------------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------------

BATCH_TTIS = (1, 3)
SEED0 = 5200


def _oracle_cell_for_batch(oracle, c, sched):
    cqi, avg = arrays(c)
    cell = oracle_cell(oracle, c, sched)
    cell.set_cqi(cqi)
    cell.set_avg_rate(avg)
    cell.set_last_update(0.1)
    return cell


def _new_batch(rs, group, sched, jit):
    c0 = group[0]
    b = rs.BatchScheduler(config_of(rs, c0), c0.R, c0.G, len(group), sched=sched, jit=jit, cqi_epoch_wrap=True)
    b.seed(np.arange(len(group), dtype=np.uint32) + SEED0)
    b.upload_cqi_epochs(np.stack([np.stack([arrays(c)[0]] * 2) for c in group]))
    b.write_state(avg_rate=np.stack([arrays(c)[1] for c in group]), slice_state=np.array([c.state for c in group]))
    return b


def _batch(rs, oracle, sched, group, jit):
    """One batch, cell k started from case k (a batch schedules every user: the cases' subset lists do not apply): offsets and
    averages through write_state, constant reports, 1 + 3 logged TTIs on the batch's own rand() streams"""
    n = sum(BATCH_TTIS)
    b = _new_batch(rs, group, sched, jit)
    logs = [b.run_logged(t) for t in BATCH_TTIS]
    st = b.state()
    status = b.jit_status()
    b.close()
    assert status[0] == (1 if jit else 0), status
    quota = np.concatenate([x["quota"] for x in logs], axis=1)
    maps = np.concatenate([x["rbg_to_user"] for x in logs], axis=1)
    tbs = np.concatenate([x["tbs_bits"] for x in logs], axis=1)
    ticks = oracle.clock_ticks(100, n)
    for k, c in enumerate(group):
        cell = _oracle_cell_for_batch(oracle, c, sched)
        rng = oracle.Rng(SEED0 + k)
        for t in range(n):
            what = f"batch sched {sched} {'run-time build' if jit else 'built-in'} {c.name} TTI {t}"
            r0, r1 = rng.rand(), rng.rand()
            out = cell.new_out()
            assert cell.step(float(ticks[t]), r0, r1, out) == 0
            assert quota[k, t].tolist() == out.quota_rbgs.tolist(), f"{what}: quotas"
            if t == 0 and c.listed is None:
                assert quota[k, t].tolist() == c.plants["quota"], f"{what}: the planted quotas"
            np.testing.assert_array_equal(maps[k, t], out.rbg_to_user, err_msg=f"{what}: RBG map")
            np.testing.assert_array_equal(tbs[k, t], out.user_tbs_bits, err_msg=f"{what}: transport blocks")
            check_policy(oracle, c, sched, maps[k, t], out.slice_eff.tolist(), quota[k, t].tolist(), what)
        assert st["slice_state"][k].tobytes() == cell.state()["slice_state"].tobytes(), f"batch sched {sched} {c.name}: final slice state"
        assert st["avg_rate"][k].tobytes() == cell.state()["avg_rate"].tobytes(), f"batch sched {sched} {c.name}: final averages"


def _lean_launch(rs, oracle, group):
    """scheduler 9's lean build: one unlogged TTI from the cases' offsets, compared on the state it leaves (the offsets hold the
    RBGs every slice got, the averages the block every user got)"""
    b = _new_batch(rs, group, 9, True)
    b.prepare_launch(1)
    b.run(1)
    st = b.state()
    status = b.jit_status()
    b.close()
    assert status[0] == 1, status
    tick = float(oracle.clock_ticks(100, 1)[0])
    for k, c in enumerate(group):
        cell = _oracle_cell_for_batch(oracle, c, 9)
        rng = oracle.Rng(SEED0 + k)
        out = cell.new_out()
        assert cell.step(tick, rng.rand(), rng.rand(), out) == 0
        if c.listed is None:
            assert out.quota_rbgs.tolist() == c.plants["quota"], c.name
        assert st["slice_state"][k].tobytes() == cell.state()["slice_state"].tobytes(), f"lean launch {c.name}: slice state"
        assert st["avg_rate"][k].tobytes() == cell.state()["avg_rate"].tobytes(), f"lean launch {c.name}: averages"


BATCHES = [(s, False) for s in SCHEDS] + [(s, True) for s in (9, 8, 101, 103)]


@pytest.mark.parametrize("sched,jit", BATCHES, ids=[f"{s}-{'jit' if j else 'builtin'}" for s, j in BATCHES])
def test_batches(rs, oracle, monkeypatch, sched, jit):
    """Every case of the scheduler's family as the start of one cell: the map of EVERY TTI equals the plain policy applied to that
    TTI's logged quotas and the oracle's slice_eff, and the oracle's map, transport blocks and final state; TTI 0 carries the
    planted quotas.  The run-time builds take the cases of the three shapes 20 x 25, 32 x 32 and 33 x 33 (MaximizeCell's scan
    there: as in test_dropin_runtime_builds); scheduler 9's also run one unlogged TTI on the lean build."""
    family = FAMILY_OF[sched]
    cs = ie.cases(family)
    if jit:
        monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
        cs = [c for c in cs if c.plants["shape"] in ie.JIT_SHAPES]
        assert {c.plants["shape"] for c in cs} == set(ie.JIT_SHAPES)
    for group in ie.by_config(cs):
        _batch(rs, oracle, sched, group, jit)
        if jit and sched == 9:
            _lean_launch(rs, oracle, group)
    if not jit:
        report(f"batches sched {sched}", family, cs)
    else:
        print(f"inter-slice edge cases run, batch run-time builds sched {sched}: {family} {len(cs)}")
