"""CPU proof that the near-tie populations of tests/near_ties.py bind (no GPU needed): every gap band and every placement occurs, measured
from the plain numpy scan rather than from the generator's plan; the set holds items a kernel that trusted stage 1 alone, or filtered
at 1 - 2^-22 instead of 1 - 2^-19, would get wrong; and the oracle's scans (`unpinned` in tests/PINS.md) agree with the plain scan on
every population -- device == oracle (tests/test_gpu_near_ties.py) == plain numpy (here).

Scheduler 7's runs: the library has no call that reports the run length.  Drop-in and group contexts carve their LDS with the gate
scratch (rs_carve's `queue` branch, rs_device.h): they scan the served slice UNSPLIT, whatever its size, and the populations of
nvs_set / group_set(7) claim no run boundary.  Batches split a slice whose 8-aligned window is longer than RS_NVS_WHOLE_SLICE into
8-aligned runs of 8, 16 or 32 users counted from the slice's aligned start; batch_set(7) places pairs at users 7|8, 16|15 and 31|32 of
such a slice, boundaries of runs of 8, of 8 and 16, and of every run length."""
import collections
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import near_ties as nt

_P3 = (Path(__file__).resolve().parents[1] / "radiosaber_amd" / "csrc" / "rs_phase_p3.inc").read_text()
KTOL = float.fromhex(re.search(r"const float kTol = (0x[0-9a-fp.\-]+)f;", _P3).group(1))   # 1 - 2^-19
TOL = Fraction(5, 4) * Fraction(1, 2**18)   # the widest near band's upper edge


@pytest.fixture(scope="module")
def eff(oracle):
    return np.array([0.0] + [oracle.lib().rso_efficiency_from_cqi(c) for c in range(1, 16)])


def all_sets(eff):
    """{scheduler: populations}: what tests/test_gpu_near_ties.py runs (schedulers 8, 10, 101, 103 share scheduler 9's)."""
    sets = {9: nt.transport_set(eff), 1: nt.pf_set(eff), 7: nt.nvs_set(eff)}
    for sched in sets:
        sets[sched] = sets[sched] + nt.group_set(eff, sched) + nt.batch_set(eff, sched)
    return sets


def test_structural_constants_are_the_sources(eff):
    assert KTOL == 1 - 2.0**-19 and nt.PF_SEG == 32 and nt.P3_BLOCK == 32 and nt.HOLD_MAX_AGE == 40
    # scheduler 7's batches: slice 1's window is longer than the threshold of either kind of build, so it is scanned in runs, and
    # the directed pairs straddle multiples of 8 counted from the slice's aligned start (user 0)
    assert nt.batch_window(nt.BATCH_UES) > nt.NVS_WHOLE_SLICE
    for p in nt.batch_set(eff, 7):
        assert p.base[1] == 0
        pairs = [sorted(pl.users[:2]) for pl in p.planted if "run-boundary" in pl.tags]
        assert [7, 8] in pairs and [15, 16] in pairs and [31, 32] in pairs
    # the drop-in and group populations of scheduler 7 claim none: those contexts scan the served slice unsplit
    assert not any("run-boundary" in pl.tags for p in nt.nvs_set(eff) + nt.group_set(eff, 7) for pl in p.planted)


def test_every_band_and_placement_occurs(eff):
    bands, tags = collections.Counter(), collections.Counter()
    avgs = set()
    for sched, pops in all_sets(eff).items():
        for p in pops:
            its = {(i["slice"], i["rbg"]): i for i in nt.items(p, eff)}
            num, den = nt.num_of(eff, sched), nt.den_of(p.avg, sched)
            control = p.name.endswith("control")
            for i in its.values():
                if i["runner"] is not None and not control:
                    assert 0 <= i["gap"] <= TOL, (p.name, i)   # by construction: every item of a single-call population is a near-tie
            for pl in p.planted:
                it = its[(0 if sched == 1 else pl.slice, pl.rbg)]
                a = pl.users[0]
                assert it["winner"] in pl.users and it["runner"] in pl.users, (p.name, pl)
                # the anchor holds the largest exact metric (or shares it): the scan's winner is the first user at that metric
                gaps = [nt.exact_gap(num, den, p.cqi[a, pl.rbg], a, p.cqi[b, pl.rbg], b) for b in pl.users[1:]]
                assert gaps == pl.gaps
                for b, g, band in zip(pl.users[1:], gaps, pl.bands):
                    lo, hi = nt.BANDS[band]
                    assert lo <= g <= hi
                    bands[band] += 1
                    if band == "zero" and p.cqi[a, pl.rbg] != p.cqi[b, pl.rbg]:
                        bands["zero, two classes"] += 1
                tied = [u for u, g in zip(pl.users[1:], gaps) if num[p.cqi[u, pl.rbg]] / den[u] >= num[p.cqi[a, pl.rbg]] / den[a]]
                assert it["winner"] == min([a] + tied)
                if it["winner"] != a:
                    tags["a rounded tie goes to an earlier challenger"] += 1
                for t in pl.tags:
                    tags[t] += 1
                kind, side = nt.classify(a, pl.users[1], p.base[pl.slice])
                tags[f"{kind}/{side}"] += 1
                avgs.add(round(float(np.log2(p.avg[a]))))
                # the field: every other user of the slice loses by 2^-10 ... 2^-6 (a tuple of another RBG: a CQI class, 7 % or more)
                lo_u, hi_u = (0, len(p.avg)) if sched == 1 else (int(p.first[pl.slice]), int(p.first[pl.slice + 1]))
                for u in range(lo_u, hi_u):
                    if u not in pl.users and p.avg[u] < 1e200:
                        g = nt.exact_gap(num, den, p.cqi[a, pl.rbg], a, p.cqi[u, pl.rbg], u)
                        assert Fraction(1, 2**10) < g < Fraction(1, 2), (p.name, pl, u)
                        tags["field user within 2^-6"] += int(g <= Fraction(1, 2**6) * Fraction(1025, 1024))
    print("\nper band:", dict(bands))
    print("per placement:", dict(tags))
    for b in list(nt.BANDS) + ["zero, two classes"]:
        assert bands[b] > 0, b
    for kind in nt.PLACEMENTS:
        for side in ("before", "after"):
            assert tags[f"{kind}/{side}"] > 0, (kind, side)
    for t in ("first", "last", "unaligned", "ragged", "several", "classes", "seg31|32", "seg63|64", "run-boundary", "first-slot",
              "last-slot", "field user within 2^-6", "a rounded tie goes to an earlier challenger"):
        assert tags[t] > 0, t
    # averages from 1 to close to 2^51: log2 of the anchors' averages
    assert {0, 6, 10, 17, 22, 50} <= avgs | {a + 1 for a in avgs} | {a - 1 for a in avgs}, sorted(avgs)


def test_stage_one_alone_would_fail(eff):
    """The set holds items on which (a) the stage-1 order of winner and runner-up is the reverse of the exact order under at least one
    rounding of the two reciprocals, (b) a filter at 1 - 2^-22 (and the mutant value 1 - 2^-23) would drop a true winner that leads
    by a positive exact gap, (c) three or more users survive the real
    filter and the winner is neither the first survivor nor the user with the largest stage-1 value under any of the three roundings."""
    reversed_, dropped22, dropped23, dropped19, several = 0, 0, 0, 0, 0
    for sched, pops in all_sets(eff).items():
        for p in pops:
            num, den = nt.num_of(eff, sched), nt.den_of(p.avg, sched)
            first = p.first
            for i in nt.items(p, eff):
                if i["runner"] is None:
                    continue
                lo, hi = (0, len(p.avg)) if sched == 1 else (int(first[i["slice"]]), int(first[i["slice"] + 1]))
                row = p.cqi[lo:hi, i["rbg"]]
                s1 = {k: nt.stage1(num[row], np.minimum(den[lo:hi], 1e30), k) for k in (-1, 0, 1)}
                w, r = i["winner"] - lo, i["runner"] - lo
                if i["gap"] > 0 and any(s1[kr][r] > s1[kw][w] for kw in s1 for kr in s1):
                    reversed_ += 1
                # (b): only items whose winner leads by a positive gap -- on exact ties one FP32 ulp either way proves nothing
                if i["gap"] > 0:
                    worst = float(s1[1].max())
                    dropped22 += int(float(s1[-1][w]) < np.float32(worst) * np.float32(1 - 2.0**-22))
                    dropped23 += int(float(s1[-1][w]) < np.float32(worst) * np.float32(1 - 2.0**-23))
                    dropped19 += int(float(s1[-1][w]) < np.float32(worst) * np.float32(KTOL))
                surv = np.flatnonzero(s1[0] >= s1[0].max() * np.float32(KTOL))
                if len(surv) >= 3 and w != surv[0] and all(w != int(np.argmax(s1[k])) for k in s1):
                    several += 1
    print(f"\nstage-1 order reversed: {reversed_}; true winner (positive gap) below (1 - 2^-22) of the largest stage-1 value: {dropped22}, "
          f"below (1 - 2^-23): {dropped23}; "
          f"three or more survivors, winner neither first nor stage-1 largest: {several}")
    assert reversed_ > 0 and dropped22 > 0 and dropped23 >= dropped22 and several > 0
    assert dropped19 == 0   # the real tolerance keeps every true winner, whatever the reciprocals' last bit does


def _oracle_winners(oracle, p, ids=None):
    """[S][R] per-slice winners the oracle's call scanned (scheduler 1: [1][R], scheduler 7: the served slice 1's row alone)."""
    cell = oracle.Cell(p.ues, p.R, 4, p.sched)
    cell.set_cqi(p.cqi)
    out = cell.new_out()
    if p.sched == 1:
        assert cell.allocate(p.avg, 0, 0, out) == 0
        return out.rbg_to_user[None, :].astype(np.int64)
    if p.sched == 7:
        assert cell.allocate_listed(p.avg, out, slice_id=1) == 0
        return out.rbg_to_user[None, :].astype(np.int64)
    lst = None if ids is None else np.asarray(ids, np.int32)
    assert cell.allocate_listed(p.avg, out, lst, rand0=5, rand1=9) == 0
    return out.slice_user.T.astype(np.int64)


def test_the_oracle_agrees_with_the_plain_scan(oracle, eff):
    """Second opinion on the oracle's `unpinned` scans: scheduler 1's whole map, scheduler 7's served slice, and for schedulers 8, 9, 10
    the per-slice winners RBsAllocation hands to the inter-slice step (rso_tti_out.slice_user), full calls and subset calls."""
    n = 0
    for sched, pops in all_sets(eff).items():
        for p in pops:
            want = nt.winners(p, eff)
            if sched == 7:
                want = want[1:2]
            np.testing.assert_array_equal(_oracle_winners(oracle, p), want, err_msg=p.name)
            n += want.size
            if sched == 9:
                for other in (8, 10):
                    q = nt.Population(p.name, other, p.ues, p.R, p.cqi, p.avg, p.planted, p.base)
                    np.testing.assert_array_equal(_oracle_winners(oracle, q), want, err_msg=f"{p.name} sched {other}")
                ids = subset_ids(p)
                np.testing.assert_array_equal(_oracle_winners(oracle, p, ids), nt.winners(p, eff, ids), err_msg=f"{p.name} subset")
    print(f"\noracle == plain numpy scan on {n} items")


def subset_ids(p):
    """A call that leaves out three field users in front of slice 1's anchors: the same pairs, other block positions."""
    used = {u for pl in p.planted for u in pl.users}
    drop = [u for u in range(int(p.first[1]), int(p.first[2])) if u not in used][:3]
    return np.array([u for u in range(len(p.avg)) if u not in drop], np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# the hold margin: the populations of nt.margin_population put the held-winner rule at risk
# ---------------------------------------------------------------------------------------------------------------------------

def held_at_scan(p, eff, pl):
    """the device's held test (scan_item) on a planted item at the full scan, in float32 as in tests/test_hold_margin.py"""
    from test_hold_margin import held
    num, den = nt.num_of(eff, p.sched), nt.den_of(p.avg, p.sched)
    lo, hi = int(p.first[pl.slice]), int(p.first[pl.slice + 1])
    s1 = nt.stage1(num[p.cqi[lo:hi, pl.rbg]], den[lo:hi])
    order = np.sort(s1)
    w = pl.users[0] - lo
    return bool(s1[w] == order[-1] and held(s1[w], order[-2], np.array(p.avg[pl.users[0]])))


def margin_winners(oracle, p, n_ttis, seed=31):
    """[n_ttis][S][R] per-item winners of the plain scan over the averages the oracle's run holds in each TTI (the oracle stepped as
    rso_run_synth steps it: clock from tick 100, rand0 / rand1 from the glibc restatement), and the oracle's RBG maps."""
    cell = oracle.Cell(p.ues, p.R, 4, p.sched, weights=nt.MARGIN_WEIGHTS)
    cell.set_cqi(p.cqi)
    cell.set_avg_rate(p.avg)
    cell.set_last_update(0.1)
    ticks, rng = oracle.clock_ticks(100, n_ttis), oracle.Rng(seed)
    wins, maps = [], []
    for t in range(n_ttis):
        out = cell.new_out()
        assert cell.step(float(ticks[t]), rng.rand(), rng.rand(), out) == 0
        q = nt.Population(p.name, p.sched, p.ues, p.R, p.cqi, cell.state()["avg_rate"], p.planted, p.base)   # the averages TTI t scanned
        want = nt.winners(q, EFF[0])
        np.testing.assert_array_equal(out.slice_user.T, want, err_msg=f"margin TTI {t}: oracle against the plain scan")
        wins.append(want)
        maps.append(out.rbg_to_user.copy())
    return np.stack(wins), np.stack(maps)


EFF = [None]


@pytest.mark.parametrize("sched", [9, 8])
def test_the_margin_populations_put_held_winners_at_risk(oracle, eff, sched):
    """Every (avg_w, k) of the issue occurs; at the full scan of TTI 0 the items with k >= 1.1 pass the device's held test and those
    with k <= 0.9 do not; and within RS_HOLD_MAX_AGE TTIs of that scan the per-item winner (plain scan over the oracle's averages,
    which the oracle's own per-slice winners equal in every TTI) changes in at least one item -- in scheduler 8's run among them an
    item whose winner and runner-up both went unserved until then: the decay case."""
    EFF[0] = eff
    p = nt.margin_population(eff, sched)
    combos = {(pl.tags - {t for t in pl.tags if t.startswith("k=")}).pop() + " " + [t for t in pl.tags if t.startswith("k=")][0] for pl in p.planted}
    assert len(combos) == len(nt.MARGIN_AVGS) * len(nt.MARGIN_K)
    held = {(pl.slice, pl.rbg): held_at_scan(p, eff, pl) for pl in p.planted}
    for pl in p.planted:
        if pl.gaps[0] >= 1.1:
            assert held[(pl.slice, pl.rbg)], pl
        if pl.gaps[0] <= 0.9:
            assert not held[(pl.slice, pl.rbg)], pl
    wins, maps = margin_winners(oracle, p, nt.HOLD_MAX_AGE)
    assert (wins[0, :4] == np.array([[pl.users[0] for pl in p.planted if pl.slice == s] for s in range(4)])).all()
    changed = decay = 0
    for pl in p.planted:
        w = wins[:, pl.slice, pl.rbg]
        moved = np.flatnonzero(w != w[0])
        if len(moved):
            changed += 1
            t = int(moved[0])
            decay += int(not np.isin(maps[:t], pl.users[:2]).any() and w[t] == pl.users[1])
    print(f"\nsched {sched}: held at the full scan {sum(held.values())} of {len(held)} items; winner changed within {nt.HOLD_MAX_AGE} TTIs in "
          f"{changed} items, {decay} of them by decay alone (neither user served)")
    assert changed > 0
    if sched == 8:   # (MaximizeCell happens to serve those items first; GreedyByRow's run holds the pure decay case)
        assert decay > 0


def test_the_flows_populations_bind(oracle, eff):
    """Scheduler 1's flows form: the plain scan over the 2U flow positions has every RBG's runner-up within 2^-18, pairs at positions
    31|32 and 63|64, and users whose two bearers are a near-tie apart with bearer 0 ahead and with bearer 1 ahead; the oracle's
    queue path (rso_cell_step_queues, InfiniteBuffer bearers started from these averages) hands the first TTI's RBGs to the plain
    scan's winners."""
    for k, a in enumerate(nt.GROUP_AVGS):
        cqi, avg2, fl = nt.flows_population(eff, a, 300 + k)
        its = nt.items(fl, eff)
        assert all(0 <= i["gap"] <= TOL for i in its)
        pairs = [sorted((i["winner"], i["runner"])) for i in its]
        assert [31, 32] in pairs and [63, 64] in pairs
        den = avg2
        near = np.abs(den[:, 1] / den[:, 0] - 1) < 2.0**-18
        assert (near & (den[:, 0] <= den[:, 1])).any() and (near & (den[:, 0] > den[:, 1])).any()
        cell = oracle.Cell([nt.FLOW_USERS], fl.R, 4, 1)
        cell.enable_queues(np.ones((nt.FLOW_USERS, 2), np.uint8))
        cell.set_bearer_avg(avg2)
        cell.set_cqi(cqi)
        out = cell.new_out()
        assert cell.step_queues(float(oracle.clock_ticks(100, 1)[0]), oracle.Rng(1), out) == 0
        # the first TTI's EWMA multiplies every average by the same factor before the race; the gate is wide open (InfiniteBuffer)
        scaled = nt.Population(fl.name, 1, fl.ues, fl.R, fl.cqi, cell.bearer_state()["avg_rate"].reshape(-1), fl.planted, fl.base)
        np.testing.assert_array_equal(out.rbg_to_user, nt.winners(scaled, eff)[0])
