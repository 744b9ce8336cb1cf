"""One TTI of a group of drop-in cells in a single kernel launch (rs_group_schedule_tti, GroupScheduler): against the CPU oracle,
against K independent contexts (the single call is the yardstick where the oracle has no per-call entry point), subset calls,
rejections, one launch per call, and the completion counter under 2 000 back-to-back calls."""
import numpy as np
import pytest

from conftest import synth_cqi

pytestmark = pytest.mark.gpu

HIST = (152600, 56656, 270880, 2088792, 3509504, 1595568, 4145392, 5295816, 1903424,
        6890232, 4770864, 2842552, 3579624, 96000, 1227696)
FIELDS = ("rbg_to_user", "target_rbs", "quota_rbgs", "user_nprb", "user_final_cqi", "user_mcs", "user_tbs_bits")
SCHEDS = (1, 7, 8, 9, 10, 101, 103)  # every scheduler rs_create accepts except 11


def _same(a, b, what, upper=False):
    fields = FIELDS + (("upper_rbg", "upper_user") if upper else ())
    if all(np.array_equal(getattr(a, f), getattr(b, f)) for f in fields):
        return
    for f in fields:  # the first difference is the message
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f"{what}: {f}")


def _ewma(avg, tbs_bits):
    """RadioBearer::UpdateAverageTransmissionRate over one TTI (ref: src/flows/radio-bearer.cpp:139-164)."""
    rate = (tbs_bits // 8 * 8) / 0.001
    return np.maximum(1.0, (1 - 0.02) * avg + 0.02 * rate)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [([5] * 20, 64, 8), ([25] * 20, 25, 4)], ids=["20x5x64", "20x25x25"])
@pytest.mark.parametrize("sched", [8, 9, 10, 101, 103, 1])
def test_group_against_the_oracle(rs, oracle, sched, shape):
    """K = 7 cells, 60 TTIs, every cell with its own CQI grids, averages (fed back through the reference's EWMA) and rand() pair:
    every output field of every cell equals rso_cell_allocate on a per-cell oracle object, and so do the slice offsets at the end."""
    ues, R, G = shape
    K, n_ttis, S, U = 7, 60, len(ues), sum(ues)
    sc = rs.SliceConfig(ues, weight=[1.0 / S] * S)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    assert g.kernel_name.startswith("rs_group_kernel<%d," % sched)
    cells = [oracle.Cell(ues, R, G, sched, weights=[1.0 / S] * S) for _ in range(K)]
    rng = np.random.default_rng(100 + sched)
    avg = [rng.uniform(1e3, 5e6, U) for _ in range(K)]
    cqi = [None] * K
    for it in range(n_ttis):
        calls, outs = [], []
        for k in range(K):
            if it % 20 == 0:
                cqi[k] = synth_cqi(9000 + 1000 * sched + 100 * k + it, (U, R), HIST)
            r0, r1 = int(rng.integers(0, 2**31 - 1)), int(rng.integers(0, 2**31 - 1))
            cells[k].set_cqi(cqi[k])
            out = cells[k].new_out()
            assert cells[k].allocate(avg[k], r0, r1, out) == 0
            outs.append(out)
            calls.append(dict(cqi=cqi[k], avg_rate=avg[k].copy(), rand0=r0, rand1=r1))
        res = g.schedule_tti(calls)
        for k in range(K):
            _same(res[k], outs[k], f"sched {sched} TTI {it} cell {k}", upper=sched == 10)
            avg[k] = _ewma(avg[k], res[k].user_tbs_bits)
    assert g.launch_count == n_ttis
    for k in range(K):
        assert g.slice_offset(k).tobytes() == cells[k].state()["slice_state"].tobytes(), f"cell {k}: slice offsets"
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (b) against K independent contexts
# ---------------------------------------------------------------------------------------------------------------------------

def _twin_calls(rng, sc, sched, R, G, K, it, variant, seed):
    """One TTI's keyword dictionaries for K cells: per-cell user subsets (ascending ids, another n per cell and TTI; scheduler 7:
    the users of one slice, another slice per cell), per-cell grids, averages and rand() pairs, and the variant's optional inputs."""
    S, U = sc.n_slices, sc.n_users
    u2s = np.asarray(sc.user_to_slice)
    live = [s for s in range(S) if (u2s == s).any()]
    calls = []
    for k in range(K):
        if sched == 7:
            ids = np.flatnonzero(u2s == live[(k + it) % len(live)])
        else:
            ids = np.sort(rng.choice(U, int(rng.integers(1, U + 1)), replace=False))
        n = len(ids)
        cqi = synth_cqi(seed + 977 * it + 31 * k, (n, R), HIST)
        avg = rng.choice([1.0, 98000.0, 5e5], n) if it == 3 else rng.uniform(1.0, 1e6, n)  # exact ties too
        kw = dict(cqi=cqi, avg_rate=avg, user_id=ids.astype(np.int32), rand0=int(rng.integers(0, 2**31 - 1)), rand1=int(rng.integers(0, 2**31 - 1)))
        if variant == "prb":
            prb = np.repeat(cqi, G, axis=1)
            prb[:, 1::G] = np.maximum(1, prb[:, 1::G] - 1)
            kw["cqi"], kw["cqi_prb"] = None, prb
        if variant == "custom":
            kw["hol_delay"] = rng.uniform(1e-5, 0.3, n)
            kw["prio_has_data"] = (rng.random(n) < 0.8).astype(np.uint8)
        if variant == "gates" and sched == 7:
            kw["required_rbs"] = rng.integers(0, 3 * G, n).astype(np.int32)
        if variant == "gates" and sched == 1:
            kw["data_to_transmit"] = rng.integers(0, 4000, n).astype(np.int32)
        if variant == "range" and k == 1:
            # ONE cell's averages leave the FP32 filter's safe range (huge, tiny, negative): that call runs the exact FP64 scan for
            # every cell, and the in-range cells must still equal their single-context twins, which ran the filtered scan
            kw["avg_rate"] = avg * rng.choice([1e-30, 1.0, 1e40, -1.0], n)
        calls.append(kw)
    return calls


# (schedulers 1 and 7 alone have a gate)
TWIN_CASES = [(s, v) for s in SCHEDS for v in ("plain", "prb", "custom", "gates", "genexp", "range") if v != "gates" or s in (1, 7)]


@pytest.mark.parametrize("sched,variant", TWIN_CASES)
def test_group_equals_independent_contexts(rs, sched, variant):
    """The group's outputs and slice state equal those of K TtiScheduler objects fed the same inputs, bit for bit."""
    ues, R, G, K, n_ttis = [3, 4, 0, 2, 5], 12, 2, 5, 10
    S = len(ues)
    kw = {}
    if variant == "custom":  # alpha = 1 with beta 0 and 1, and a plain slice beside them
        kw = dict(algo_alpha=[1, 1, 0, 1, 0], algo_beta=[0, 1, 0, 1, 0])
    if variant == "genexp":
        kw = dict(algo_epsilon=[2, 1, 1, 0, 3], algo_psi=[1, 2, 1, 3, 0])
    sc = rs.SliceConfig(ues, weight=[0.3, 0.2, 0.1, 0.15, 0.25], **kw)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    twins = [rs.TtiScheduler(sc, R, G, sched=sched) for _ in range(K)]
    rng = np.random.default_rng(500 + 7 * sched + len(variant))
    for it in range(n_ttis):
        calls = _twin_calls(rng, sc, sched, R, G, K, it, variant, seed=40000 + sched)
        res = g.schedule_tti(calls)
        for k in range(K):
            one = twins[k].schedule_tti(**calls[k])
            _same(res[k], one, f"sched {sched} {variant} TTI {it} cell {k}", upper=sched == 10)
            assert g.slice_offset(k).tobytes() == twins[k].slice_offset.tobytes(), f"sched {sched} {variant} TTI {it} cell {k}: slice state"
    assert g.launch_count == n_ttis
    g.close()
    for t in twins:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (c) subset calls
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [9, 8, 7])
def test_subset_calls_leave_the_other_cells_alone(rs, sched):
    """cell_ids alternates between the even cells and all cells: an untouched cell's slice state does not move, and the final state
    equals the twins that skipped the same TTIs."""
    ues, R, G, K = [3, 4, 0, 2, 5], 12, 2, 6
    sc = rs.SliceConfig(ues, weight=[0.3, 0.2, 0.1, 0.15, 0.25])
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    twins = [rs.TtiScheduler(sc, R, G, sched=sched) for _ in range(K)]
    rng = np.random.default_rng(77 + sched)
    for it in range(12):
        cells = list(range(0, K, 2)) if it % 2 == 0 else list(range(K))
        if it == 5:
            cells = cells[::-1]  # any order
        before = [g.slice_offset(k).tobytes() for k in range(K)]
        calls = _twin_calls(rng, sc, sched, R, G, len(cells), it, "plain", seed=60000 + sched)
        res = g.schedule_tti(calls, cell_ids=cells)
        for j, k in enumerate(cells):
            _same(res[j], twins[k].schedule_tti(**calls[j]), f"sched {sched} TTI {it} cell {k}")
        for k in range(K):
            if k not in cells:
                assert g.slice_offset(k).tobytes() == before[k], f"TTI {it}: cell {k} was not named, its slice state moved"
            assert g.slice_offset(k).tobytes() == twins[k].slice_offset.tobytes(), f"TTI {it} cell {k}"
    g.close()
    for t in twins:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (d) rejections
# ---------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_launch_nothing_and_move_no_state(rs):
    ues, R, G, K = [3, 4, 0, 2, 5], 12, 2, 4
    sc = rs.SliceConfig(ues, weight=[0.3, 0.2, 0.1, 0.15, 0.25])
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    rng = np.random.default_rng(5)
    good = _twin_calls(rng, sc, 9, R, G, K, 0, "plain", seed=1)
    g.schedule_tti(good)
    g.set_slice_offset(2, np.arange(5, dtype=np.float64) - 2.0)
    assert g.slice_offset(2).tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0]
    launches = g.launch_count
    state = [g.slice_offset(k).tobytes() for k in range(K)]

    def rejected(calls, cell_ids=None, frag=""):
        with pytest.raises(rs.RadioSaberError) as e:
            g.schedule_tti(calls, cell_ids=cell_ids)
        assert e.value.code == -1 and frag in str(e.value), str(e.value)  # RS_ERR_INVALID
        assert g.launch_count == launches
        assert [g.slice_offset(k).tobytes() for k in range(K)] == state

    mixed = [dict(c) for c in good]
    prb = np.repeat(mixed[2]["cqi"], G, axis=1)
    mixed[2]["cqi"], mixed[2]["cqi_prb"] = None, prb
    rejected(mixed, frag="cqi_prb")
    rejected(good, cell_ids=[0, 1, 1, 3], frag="twice")
    rejected(good, cell_ids=[0, 1, 2, K], frag="outside")
    rejected(good, cell_ids=[0, -1, 2, 3], frag="outside")
    empty = [dict(c) for c in good]
    empty[3].update(cqi=np.zeros((0, R), np.uint8), avg_rate=np.zeros(0), user_id=np.zeros(0, np.int32))
    rejected(empty, frag="n_users 0")
    bad_cqi = [dict(c) for c in good]
    bad_cqi[K - 1]["cqi"] = np.zeros_like(good[K - 1]["cqi"])  # the LAST cell is wrong: the cells before it were packed, not launched
    rejected(bad_cqi, frag="CQI 0")
    rejected(good + good[:1], frag="outside 1..4")  # more calls than cells
    with pytest.raises(rs.RadioSaberError) as e:
        rs.GroupScheduler(sc, R, G, K, sched=rs.RS_SCHED_NVS_NONGREEDY)
    assert "RS_SCHED_NVS_NONGREEDY" in str(e.value)
    # and the group still works
    g.schedule_tti(good)
    assert g.launch_count == launches + 1
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (e) one launch per call, (f) completion
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 7, 300])
def test_one_launch_per_call(rs, K):
    """rs_group_launch_count grows by exactly 1 per successful call -- also with more cells than the device has compute units, where
    the workgroups cannot all be resident at once; every cell's answer is that of a single context fed the same inputs."""
    ues, R, G = [3, 4, 0, 2, 5], 12, 2
    sc = rs.SliceConfig(ues, weight=[0.3, 0.2, 0.1, 0.15, 0.25])
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    twin = rs.TtiScheduler(sc, R, G, sched=9)
    rng = np.random.default_rng(K)
    for it in range(4):
        calls = _twin_calls(rng, sc, 9, R, G, K, it, "plain", seed=3000)
        offsets = [g.slice_offset(k) for k in range(K)]
        res = g.schedule_tti(calls)
        assert g.launch_count == it + 1
        for k in range(K):  # one twin context stands in for all K: it is given cell k's slice state first
            twin.slice_offset = offsets[k]
            _same(res[k], twin.schedule_tti(**calls[k]), f"K {K} TTI {it} cell {k}")
            assert g.slice_offset(k).tobytes() == twin.slice_offset.tobytes()
    g.close()
    twin.close()


def test_two_thousand_back_to_back_calls_complete_with_every_output_in_place(rs):
    """The completion counter: 2 000 back-to-back calls at K = 32 on the smallest shape, every output of every call compared with
    twin contexts.  The twins' answers are computed first (they do not depend on the group), so that the group's calls follow each
    other with nothing but the comparison in between -- a missing fence would show as a stale output here."""
    ues, R, G, K, n_calls = [2, 2], 6, 2, 32, 2000
    sc = rs.SliceConfig(ues)
    rng = np.random.default_rng(2000)
    U = sc.n_users
    grids = [synth_cqi(50 + i, (U, R), HIST) for i in range(16)]
    twins = [rs.TtiScheduler(sc, R, G, sched=9) for _ in range(K)]
    plan, want = [], []
    for it in range(n_calls):
        calls = [dict(cqi=grids[int(rng.integers(0, 16))], avg_rate=rng.uniform(1.0, 1e6, U), rand0=int(rng.integers(0, 2**31 - 1)),
                      rand1=int(rng.integers(0, 2**31 - 1))) for _ in range(K)]
        plan.append(calls)
        want.append([twins[k].schedule_tti(**calls[k]) for k in range(K)])
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    for it in range(n_calls):
        res = g.schedule_tti(plan[it])
        for k in range(K):
            _same(res[k], want[it][k], f"call {it} cell {k}")
    assert g.launch_count == n_calls
    for k in range(K):
        assert g.slice_offset(k).tobytes() == twins[k].slice_offset.tobytes()
    g.close()
    for t in twins:
        t.close()
