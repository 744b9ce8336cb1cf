"""rs_tti_in.cqi_epoch in a group call: every cell of a group keeps its own device-resident CQI image (and per-PRB copy), decided per
cell and per call.  Against the CPU oracle, against twin contexts that are handed the true reports, with poisoned blocks wherever the
image must serve; the image follows the cell through cell_ids, rejected calls move nothing, RS_GROUP_IMAGE=0 switches it all off."""
import numpy as np
import pytest

from conftest import synth_cqi
from test_gpu_group import FIELDS, HIST, _ewma, _same, _twin_calls

pytestmark = pytest.mark.gpu

SMALL = ([3, 4, 0, 2, 5], 12, 2)
SMALL_W = [0.3, 0.2, 0.1, 0.15, 0.25]


def _differs(a, b):
    return any(not np.array_equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def _rand2(rng):
    return int(rng.integers(0, 2**31 - 1)), int(rng.integers(0, 2**31 - 1))


def _poison(kw):
    """The same call with every report of the caller's block replaced by CQI 15."""
    kw = dict(kw)
    if kw.get("cqi_prb") is not None:
        kw["cqi_prb"] = np.full_like(kw["cqi_prb"], 15)
    else:
        kw["cqi"] = np.full_like(kw["cqi"], 15)
    return kw


# ---------------------------------------------------------------------------------------------------------------------------
# 1. against the CPU oracle, reports renewed every 40 calls
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [([5] * 20, 64, 8), ([25] * 20, 25, 4)], ids=["20x5x64", "20x25x25"])
@pytest.mark.parametrize("sched", [8, 9, 10, 101, 103, 1])
def test_group_with_epochs_against_the_oracle(rs, oracle, sched, shape):
    """K = 7 cells, 95 TTIs, new reports (and a new number) at TTI 0, 40 and 80 -- CQI_INTERVAL: every field of every cell and the final
    slice offsets equal the oracle's, and the counters say 3 K stores, 92 K reuses."""
    ues, R, G = shape
    K, n_ttis, S, U = 7, 95, len(ues), sum(ues)
    sc = rs.SliceConfig(ues, weight=[1.0 / S] * S)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    cells = [oracle.Cell(ues, R, G, sched, weights=[1.0 / S] * S) for _ in range(K)]
    rng = np.random.default_rng(300 + sched)
    avg = [rng.uniform(1e3, 5e6, U) for _ in range(K)]
    cqi = [None] * K
    for it in range(n_ttis):
        calls, outs = [], []
        for k in range(K):
            if it % 40 == 0:
                cqi[k] = synth_cqi(19000 + 1000 * sched + 100 * k + it, (U, R), HIST)
            r0, r1 = _rand2(rng)
            cells[k].set_cqi(cqi[k])
            out = cells[k].new_out()
            assert cells[k].allocate(avg[k], r0, r1, out) == 0
            outs.append(out)
            calls.append(dict(cqi=cqi[k], avg_rate=avg[k].copy(), rand0=r0, rand1=r1, cqi_epoch=1 + it // 40))
        res = g.schedule_tti(calls)
        for k in range(K):
            _same(res[k], outs[k], f"sched {sched} TTI {it} cell {k}", upper=sched == 10)
            avg[k] = _ewma(avg[k], res[k].user_tbs_bits)
    assert g.launch_count == n_ttis
    assert g.image_stats == (92 * K, 3 * K, 0)
    for k in range(K):
        assert g.slice_offset(k).tobytes() == cells[k].state()["slice_state"].tobytes(), f"cell {k}: slice offsets"
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the caller's block is not read on a reuse (fails on a group that ignores cqi_epoch)
# ---------------------------------------------------------------------------------------------------------------------------

def test_group_cqi_epoch_never_trusts_more_than_it_can_check(rs):
    """test_cqi_epoch_never_trusts_more_than_it_can_check for a group: the same list of (users, given block, true reports, number), but
    cell k starts it k calls late (subset calls through cell_ids), so that one launch serves cells from their images, stores images and
    reads blocks without a promise side by side.  Every cell against a twin context that is handed the TRUE reports with cqi_epoch = 0;
    wherever the given block is not the truth the test first shows that reading it would have changed the answer."""
    ues, R, G, K = [5] * 20, 64, 8, 5
    U = sum(ues)
    sc = rs.SliceConfig(ues)
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    twins = [rs.TtiScheduler(sc, R, G, sched=9) for _ in range(K)]
    probe = rs.TtiScheduler(sc, R, G, sched=9)
    rng = np.random.default_rng(3)
    all_ids = np.arange(U)
    some = all_ids[::2].copy()
    fewer = all_ids[:60].copy()
    MODE = dict(read_store=1, image=2, plain=0)
    plans = []
    for k in range(K):
        cqi = synth_cqi(1 + k, (U, R), HIST)
        poisoned = np.full_like(cqi, 15)
        plans.append([(all_ids, cqi, cqi, 5, "read_store", "new number: read"),
                      (all_ids, poisoned, cqi, 5, "image", "same number: the image serves the call, the caller's block is not read"),
                      (some, cqi[some], cqi[some], 5, "read_store", "same number, other users: read again"),
                      (some, poisoned[some], cqi[some], 5, "image", "... and then served from the image"),
                      (fewer, cqi[fewer], cqi[fewer], 5, "read_store", "same number, other user count: read again"),
                      (all_ids, poisoned, poisoned, 6, "read_store", "new number: the new block is read"),
                      (all_ids, cqi, poisoned, 6, "image", "... and kept"),
                      (all_ids, cqi, cqi, 0, "plain", "no promise: read"),
                      (all_ids, poisoned, poisoned, 0, "plain", "no promise: read again")])
    avg = [rng.uniform(1e3, 5e6, U) for _ in range(K)]
    n_steps = len(plans[0])
    want_stats = [0, 0, 0]
    mixed_launches = 0
    for it in range(n_steps + K - 1):
        named = [k for k in range(K) if 0 <= it - k < n_steps]
        calls, refs, whats, modes = [], [], [], set()
        for k in named:
            ids, given, truth, epoch, mode, what = plans[k][it - k]
            r0, r1 = _rand2(rng)
            before = twins[k].slice_offset
            ref = twins[k].schedule_tti(truth, avg[k][ids], r0, r1, user_id=ids)
            if not np.array_equal(given, truth):  # no vacuous pass: a context that reads the given block answers differently
                probe.slice_offset = before
                assert _differs(probe.schedule_tti(given, avg[k][ids], r0, r1, user_id=ids), ref), f"cell {k} step {it - k}: the poison is harmless"
            calls.append(dict(cqi=given, avg_rate=avg[k][ids], rand0=r0, rand1=r1, user_id=ids, cqi_epoch=epoch))
            refs.append(ref)
            whats.append(f"call {it} cell {k} step {it - k}: {what}")
            modes.add(MODE[mode])
            want_stats[{2: 0, 1: 1, 0: 2}[MODE[mode]]] += 1
        mixed_launches += modes == {0, 1, 2}
        res = g.schedule_tti(calls, cell_ids=named)
        for j, k in enumerate(named):
            _same(res[j], refs[j], whats[j])
            assert g.slice_offset(k).tobytes() == twins[k].slice_offset.tobytes(), whats[j]
    assert mixed_launches >= 1, "no launch mixed the three modes"
    assert g.image_stats == tuple(want_stats) == (3 * K, 4 * K, 2 * K)
    g.close()
    for t in twins + [probe]:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the image follows the cell, not the slot
# ---------------------------------------------------------------------------------------------------------------------------

def test_the_image_follows_the_cell_not_the_slot(rs):
    ues, R, G, K = [5] * 20, 64, 8, 4
    U = sum(ues)
    sc = rs.SliceConfig(ues)
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    twins = [rs.TtiScheduler(sc, R, G, sched=9) for _ in range(K)]
    probe = rs.TtiScheduler(sc, R, G, sched=9)
    rng = np.random.default_rng(33)
    truth = [synth_cqi(70 + k, (U, R), HIST) for k in range(K)]
    number = [3] * K
    avg = [rng.uniform(1e3, 5e6, U) for _ in range(K)]
    poisoned = np.full((U, R), 15, np.uint8)

    def call(cells, fresh=()):
        """One group call naming `cells` in this order; the cells in `fresh` send their (new) true reports, the others a poisoned block."""
        calls, refs = [], []
        for k in cells:
            r0, r1 = _rand2(rng)
            before = twins[k].slice_offset
            ref = twins[k].schedule_tti(truth[k], avg[k], r0, r1)
            given = truth[k] if k in fresh else poisoned
            if k not in fresh:
                probe.slice_offset = before
                assert _differs(probe.schedule_tti(poisoned, avg[k], r0, r1), ref), f"cell {k}: the poison is harmless"
            calls.append(dict(cqi=given, avg_rate=avg[k], rand0=r0, rand1=r1, cqi_epoch=number[k]))
            refs.append(ref)
        res = g.schedule_tti(calls, cell_ids=cells)
        for j, k in enumerate(cells):
            _same(res[j], refs[j], f"cells {cells} fresh {fresh}: cell {k} in slot {j}")
            avg[k] = _ewma(avg[k], res[j].user_tbs_bits)

    call([0, 1, 2, 3], fresh=(0, 1, 2, 3))
    call([2, 0, 3, 1])            # every cell in another slot
    call([3, 1])                  # a subset ...
    call([0, 2])                  # ... and the rest: cells 0 and 2 kept their images while they were not named
    for k in (1, 2):              # new reports for two cells, sent from slots that held other cells' grids before
        truth[k] = synth_cqi(170 + k, (U, R), HIST)
        number[k] = 4
    call([2, 1], fresh=(1, 2))
    call([1, 3, 0, 2])            # cells 1, 2 under number 4, cells 0, 3 still under number 3: all from their images
    assert g.image_stats == (4 + 2 + 2 + 4, 4 + 2, 0)
    g.close()
    for t in twins + [probe]:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. a rejected call moves nothing
# ---------------------------------------------------------------------------------------------------------------------------

def test_a_rejected_call_moves_no_image(rs):
    ues, R, G, K = [5] * 20, 64, 8, 4
    U = sum(ues)
    sc = rs.SliceConfig(ues)
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    twins = [rs.TtiScheduler(sc, R, G, sched=9) for _ in range(K)]
    rng = np.random.default_rng(44)
    truth = [synth_cqi(90 + k, (U, R), HIST) for k in range(K)]
    avg = [rng.uniform(1e3, 5e6, U) for _ in range(K)]
    poisoned = np.full((U, R), 15, np.uint8)

    def kws(blocks, numbers):
        out = []
        for k in range(K):
            r0, r1 = _rand2(rng)
            out.append(dict(cqi=blocks[k], avg_rate=avg[k], rand0=r0, rand1=r1, cqi_epoch=numbers[k]))
        return out

    first = kws(truth, [7] * K)
    res = g.schedule_tti(first)
    for k in range(K):
        _same(res[k], twins[k].schedule_tti(**dict(first[k], cqi_epoch=0)), f"first call, cell {k}")
    launches, stats = g.launch_count, g.image_stats
    assert stats == (0, K, 0)
    offsets = [g.slice_offset(k).tobytes() for k in range(K)]

    def rejected(calls, frag):
        with pytest.raises(rs.RadioSaberError) as e:
            g.schedule_tti(calls)
        assert e.value.code == -1 and frag in str(e.value), str(e.value)  # RS_ERR_INVALID
        assert g.launch_count == launches and g.image_stats == stats
        assert [g.slice_offset(k).tobytes() for k in range(K)] == offsets

    # cell 2 announces new reports (a slot that would store an image) and they are out of range; the slots before it were packed
    bad = kws([poisoned, poisoned, np.zeros((U, R), np.uint8), poisoned], [7, 7, 8, 7])
    rejected(bad, "CQI 0")
    # one cell gives per-PRB reports, the others per-RBG ones
    mixed = kws([poisoned] * K, [7] * K)
    mixed[1]["cqi"], mixed[1]["cqi_prb"] = None, np.full((U, R * G), 15, np.uint8)
    rejected(mixed, "cqi_prb")
    # every cell is still served from the image of the first call -- cell 2 under number 7 too
    again = kws([poisoned] * K, [7] * K)
    res = g.schedule_tti(again)
    for k in range(K):
        ref = twins[k].schedule_tti(**dict(again[k], cqi=truth[k], cqi_epoch=0))
        _same(res[k], ref, f"after the rejections, cell {k}")
    assert g.launch_count == launches + 1 and g.image_stats == (K, K, 0)
    g.close()
    for t in twins:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. / 7. held reports against independent contexts: per-PRB reports, the staged-copy path, customised slices
# ---------------------------------------------------------------------------------------------------------------------------

def _drive_held_reports(rs, sc, sched, R, G, K, n_ttis, variant, renew, seed):
    """Cell k holds its users and reports for `renew` TTIs (its renewals `k` TTIs out of step with cell 0's, so that a launch mixes
    stores and reuses) while averages, rand() pairs, HoL delays and priority flags change on every call.  The group is given the
    numbers and -- on every call that its images must serve -- a poisoned block; the twin contexts get the same numbers and the true
    reports.  Outputs, slice state and the counters."""
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    twins = [rs.TtiScheduler(sc, R, G, sched=sched) for _ in range(K)]
    rng = np.random.default_rng(seed)
    base, number = [None] * K, [0] * K
    n_store = n_reuse = 0
    for it in range(n_ttis):
        fresh = _twin_calls(rng, sc, sched, R, G, K, it, variant, seed=seed + 13 * it)
        true_calls, given = [], []
        for k in range(K):
            renewed = it == 0 or (it + k) % renew == 0
            if renewed:
                base[k] = fresh[k]
                number[k] += 1
            n = len(base[k]["user_id"])
            kw = dict(base[k], avg_rate=rng.uniform(1.0, 1e6, n), cqi_epoch=number[k])
            kw["rand0"], kw["rand1"] = _rand2(rng)
            if variant == "custom":
                kw["hol_delay"] = rng.uniform(1e-5, 0.3, n)
                kw["prio_has_data"] = (rng.random(n) < 0.8).astype(np.uint8)
            true_calls.append(kw)
            given.append(kw if renewed else _poison(kw))
            n_store += renewed
            n_reuse += not renewed
        res = g.schedule_tti(given)
        for k in range(K):
            one = twins[k].schedule_tti(**true_calls[k])
            _same(res[k], one, f"sched {sched} {variant} TTI {it} cell {k}", upper=sched == 10)
            assert g.slice_offset(k).tobytes() == twins[k].slice_offset.tobytes(), f"sched {sched} {variant} TTI {it} cell {k}: slice state"
    assert n_reuse > n_store > K
    assert g.image_stats == (n_reuse, n_store, 0)
    assert g.launch_count == n_ttis
    g.close()
    for t in twins:
        t.close()


@pytest.mark.parametrize("sched", [9, 8])
def test_group_epochs_with_per_prb_reports_and_the_copy_path(rs, sched, monkeypatch):
    """Per-PRB reports: a reuse sends neither the grid nor the per-PRB block (both poisoned here) -- link adaptation reads the cell's
    device copy.  Then the plain call on the staged-copy path, where whole slots travel, stale grid areas included."""
    ues, R, G = SMALL
    sc = rs.SliceConfig(ues, weight=SMALL_W)
    _drive_held_reports(rs, sc, sched, R, G, 5, 14, "prb", renew=4, seed=71000 + sched)
    monkeypatch.setenv("RS_DROPIN_COPY", "1")
    _drive_held_reports(rs, sc, sched, R, G, 5, 14, "plain", renew=4, seed=72000 + sched)


@pytest.mark.parametrize("sched", [9, 8, 10, 1])
def test_group_epochs_with_customised_slices(rs, sched):
    """alpha = 1 slices (hol_delay / prio_has_data change on every call, the reports are held): the slots are device copies."""
    ues, R, G = SMALL
    sc = rs.SliceConfig(ues, weight=SMALL_W, algo_alpha=[1, 1, 0, 1, 0], algo_beta=[0, 1, 0, 1, 0])
    _drive_held_reports(rs, sc, sched, R, G, 5, 14, "custom", renew=4, seed=73000 + sched)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. scheduler 7: the served slice changes, a reuse needs the same slice twice running
# ---------------------------------------------------------------------------------------------------------------------------

def test_group_epochs_scheduler_7(rs):
    """Every cell serves a slice for two calls running (the cells one call out of step), then the next slice; the caller's number
    changes every 6 calls only.  Under one number the library itself must notice the other user list (read and store), and the second
    call of a slice is served from the image (poisoned block).  Against independent contexts given the same numbers and the truth."""
    ues, R, G, K, n_ttis = [6, 7, 0, 5, 8], 12, 2, 5, 24
    sc = rs.SliceConfig(ues, weight=SMALL_W)
    U = sc.n_users
    u2s = np.asarray(sc.user_to_slice)
    live = [s for s in range(len(ues)) if ues[s]]
    g = rs.GroupScheduler(sc, R, G, K, sched=7)
    twins = [rs.TtiScheduler(sc, R, G, sched=7) for _ in range(K)]
    rng = np.random.default_rng(7)
    grids = {}
    last = [None] * K   # (number, slice) of the cell's last call
    want = [0, 0, 0]
    for it in range(n_ttis):
        number = 1 + it // 6
        true_calls, given = [], []
        for k in range(K):
            sl = live[((it + k) // 2) % len(live)]
            ids = np.flatnonzero(u2s == sl).astype(np.int32)
            if (k, number) not in grids:
                grids[(k, number)] = synth_cqi(7000 + 50 * k + number, (U, R), HIST)
            r0, r1 = _rand2(rng)
            kw = dict(cqi=grids[(k, number)][ids], avg_rate=rng.uniform(1.0, 1e6, len(ids)), user_id=ids, rand0=r0, rand1=r1,
                      required_rbs=rng.integers(0, 3 * G, len(ids)).astype(np.int32), cqi_epoch=number)
            reuse = last[k] == (number, sl)
            last[k] = (number, sl)
            want[0 if reuse else 1] += 1
            true_calls.append(kw)
            given.append(_poison(kw) if reuse else kw)
        res = g.schedule_tti(given)
        for k in range(K):
            _same(res[k], twins[k].schedule_tti(**true_calls[k]), f"TTI {it} cell {k}")
            assert g.slice_offset(k).tobytes() == twins[k].slice_offset.tobytes(), f"TTI {it} cell {k}: slice state"
    assert want[0] > K and want[1] > want[0]
    assert g.image_stats == tuple(want)
    g.close()
    for t in twins:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. RS_GROUP_IMAGE=0
# ---------------------------------------------------------------------------------------------------------------------------

def test_rs_group_image_0_reads_every_block(rs, monkeypatch):
    """The control: with RS_GROUP_IMAGE=0 in the environment of the group's creation every cqi_epoch counts as 0 -- the poisoned block
    IS read (results equal a twin that is fed the poisoned block) and no cell-TTI is served from an image."""
    ues, R, G, K = [5] * 20, 64, 8, 3
    U = sum(ues)
    sc = rs.SliceConfig(ues)
    monkeypatch.setenv("RS_GROUP_IMAGE", "0")
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    monkeypatch.delenv("RS_GROUP_IMAGE")
    twins = [rs.TtiScheduler(sc, R, G, sched=9) for _ in range(K)]
    truth_twins = [rs.TtiScheduler(sc, R, G, sched=9) for _ in range(K)]
    rng = np.random.default_rng(8)
    truth = [synth_cqi(800 + k, (U, R), HIST) for k in range(K)]
    avg = [rng.uniform(1e3, 5e6, U) for _ in range(K)]
    poisoned = np.full((U, R), 15, np.uint8)
    for step, blocks in enumerate((truth, [poisoned] * K)):
        calls = []
        for k in range(K):
            r0, r1 = _rand2(rng)
            calls.append(dict(cqi=blocks[k], avg_rate=avg[k], rand0=r0, rand1=r1))
        res = g.schedule_tti([dict(c, cqi_epoch=5) for c in calls])
        for k in range(K):
            _same(res[k], twins[k].schedule_tti(**calls[k]), f"step {step} cell {k}: a twin fed the given block")
            if step == 1:
                assert _differs(res[k], truth_twins[k].schedule_tti(**dict(calls[k], cqi=truth[k]))), f"cell {k}: the poison is harmless"
            else:
                truth_twins[k].schedule_tti(**calls[k])
    assert g.image_stats == (0, 0, 2 * K)
    g.close()
    for t in twins + truth_twins:
        t.close()
