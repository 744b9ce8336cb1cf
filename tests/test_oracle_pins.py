"""Pins of the CPU oracle (not gpu): every golden vector / known-answer value the reference offers
for this path, plus the reference pieces that compile from their own sources (oracle/_ref).

  * AMC tables         vs the reference's copy inside unittest/test_effective_sinr.cpp (oracle/_ref)
                       and vs the numbers in AMCModule.cpp (tests/golden/amcmodule_tbs_table.json)
  * EESM               vs src/utility/eesm-effective-sinr.h compiled in place (oracle/_ref)
  * MaximizeCell/Vogel vs unittest/test_tp_algos.cpp compiled in place (oracle/_ref)
  * unit programs      their printed outputs
  * rand()             vs this image's libc
  * whole sched-9 loop vs SURVEY.md Appendix A (values printed by the unmodified reference)
"""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

KA = json.loads((GOLDEN / "appendix_a.json").read_text())


def _ref(oracle, name):
    L = oracle.ref_lib(name)
    if L is None:
        pytest.skip(f"oracle/_ref/{name} not built (reference tree absent)")
    return L


def test_tables_match_golden_fixture(oracle):
    g = np.load(GOLDEN / "amc_tables.npz")
    t = oracle.tables()
    for k in ("tbs", "mcs_to_itbs", "cqi_to_mcs", "sinr_for_cqi"):
        assert (t[k] == g[k]).all(), k


def test_tables_match_reference_unittest_copy(oracle):
    L = _ref(oracle, "libref_unittest_eesm.so")
    for fn, rt in (("ref_ut_tbs_table", C.c_int), ("ref_ut_mcs_to_itbs", C.c_int), ("ref_ut_cqi_to_mcs", C.c_int),
                   ("ref_ut_sinr_for_cqi", C.c_double)):
        getattr(L, fn).restype = C.POINTER(rt)
    t = oracle.tables()
    assert (np.ctypeslib.as_array(L.ref_ut_tbs_table(), (110, 27)) == t["tbs"]).all()
    assert (np.ctypeslib.as_array(L.ref_ut_mcs_to_itbs(), (29,)) == t["mcs_to_itbs"]).all()
    assert (np.ctypeslib.as_array(L.ref_ut_cqi_to_mcs(), (15,)) == t["cqi_to_mcs"]).all()
    assert (np.ctypeslib.as_array(L.ref_ut_sinr_for_cqi(), (15,)) == t["sinr_for_cqi"]).all()
    # its GetTBSizeFromMCS(mcs, nbRBs) for nbRBs <= 110
    for mcs in range(29):
        for n in (1, 8, 16, 55, 110):
            assert L.ref_ut_tbs(mcs, n) == oracle.lib().rso_tbs_bits(mcs, n)


def test_tables_match_amcmodule_text(oracle):
    # the numeric initialiser of AMCModule.cpp's TransportBlockSizeTable in text order, comments stripped (a data fixture taken
    # apart from amc_tables.npz)
    g = json.loads((GOLDEN / "amcmodule_tbs_table.json").read_text())
    assert g["shape"] == [110, 27] and len(g["values"]) == 110 * 27
    nums = np.array(g["values"]).reshape(110, 27)
    assert (nums == oracle.tables()["tbs"]).all()


def test_efficiency_and_kbps_known_answers(oracle):
    for c in range(1, 16):
        e = oracle.lib().rso_efficiency_from_cqi(c)
        assert e == KA["eff_of_cqi"][c - 1]
        assert e * 180000 / 1000 == KA["kbps_of_cqi"][c - 1]


def test_eesm_matches_reference_header(oracle):
    L = _ref(oracle, "libref_eesm.so")
    L.ref_eesm_effective_sinr.restype = C.c_double
    L.ref_eesm_effective_sinr.argtypes = [C.POINTER(C.c_double), C.c_int]
    rng = np.random.default_rng(0)
    sinr = oracle.tables()["sinr_for_cqi"]
    for _ in range(3000):
        n = int(rng.integers(1, 513))
        v = np.ascontiguousarray(sinr[rng.integers(0, 15, n)] if rng.random() < 0.7 else rng.uniform(-10, 40, n))
        a = oracle.eesm(v)
        b = L.ref_eesm_effective_sinr(v.ctypes.data_as(C.POINTER(C.c_double)), n)
        assert a == b or (np.isinf(a) and np.isinf(b)), (n, a, b)
    for n in (1, 10, 11, 26, 27, 63, 64, 110, 111, 512, 513):
        assert L.ref_get_rbg_size(n) == oracle.lib().rso_rbg_size(n)


def test_eesm_unit_program_known_answer(oracle):
    v = np.array([20.0] * 7 + [8.0])
    eff = oracle.eesm(v)
    assert f"{eff:.6g}" == "9.23711"
    cqi = oracle.lib().rso_cqi_from_sinr(eff)
    assert cqi - 1 == 6
    assert oracle.lib().rso_tbs_bits(int(oracle.tables()["cqi_to_mcs"][cqi - 1]), 8) == 1608


def test_reference_unit_programs_print_the_recorded_outputs(oracle):
    exe1, exe2 = oracle.REF_DIR / "test_effective_sinr", oracle.REF_DIR / "test_tp_algos"
    if not exe1.exists() or not exe2.exists():
        pytest.skip("oracle/_ref unit programs not built")
    o1 = subprocess.run([str(exe1)], capture_output=True, text=True).stdout.split("\n")
    assert o1[:2] == KA["unittest_outputs"]["test_effective_sinr"]
    o2 = subprocess.run([str(exe2)], capture_output=True, text=True).stdout
    assert o2.rstrip("\n") == KA["unittest_outputs"]["test_tp_algos"]


def test_uniform_cqi_round_trip(oracle):
    for c, exp in KA["uniform_cqi_roundtrip"].items():
        got = [oracle.final_cqi(np.full(n, int(c), np.uint8)) for n in KA["uniform_cqi_roundtrip_n"]]
        assert got == exp, (c, got, exp)


def test_tbs_out_of_bounds_rule(oracle):
    # 120 PRBs at final CQI 15 (mcs 28, itbs 26): 5*T[23][26] + T[-1][26] = 5*17568 + 0
    assert oracle.lib().rso_tbs_bits(28, 120) == KA["tbs_120prb_cqi15_bits"]
    t = oracle.tables()
    for mcs in (0, 9, 17, 28):
        itbs = t["mcs_to_itbs"][mcs]
        for n in (111, 113, 115, 120, 256, 512):
            tail = (t["mcs_to_itbs"][5 + itbs] if itbs <= 23 else 0) if n % 5 == 0 else t["tbs"][n % 5 - 1][itbs]
            assert oracle.lib().rso_tbs_bits(mcs, n) == 5 * t["tbs"][n // 5 - 1][itbs] + tail


def test_rand_matches_libc(oracle):
    libc = C.CDLL("libc.so.6")
    for seed in (805290992, 749913912, 1, 0, 12345, 2**31 - 1):
        libc.srand(seed)
        g = oracle.Rng(seed)
        assert [libc.rand() for _ in range(2000)] == [g.rand() for _ in range(2000)]
    # Appendix A lists the first three values of srand(805290992) (as printf evaluated them)
    g = oracle.Rng(805290992)
    assert sorted(g.rand() for _ in range(3)) == sorted(KA["rand_first3_as_listed"])
    g = oracle.Rng(805290992)
    for _ in range(KA["config"]["rand_skip"]):
        g.rand()
    assert [g.rand(), g.rand()] == KA["sched_draws"][0]


def test_maximize_cell_matches_reference_unit_code(oracle):
    L = _ref(oracle, "libref_tp_algos.so")
    args = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.ref_maximize_cell_int.argtypes = args
    eff = np.array([0.0] + KA["eff_of_cqi"])
    rng = np.random.default_rng(11)
    for trial in range(400):
        R, S = [(25, 20), (64, 20), (12, 3), (16, 7), (64, 64), (5, 3)][trial % 6]
        levels = int(rng.integers(2, 17))
        grid = np.ascontiguousarray(rng.integers(0, levels, (R, S)), np.int32)
        quota = np.zeros(S, np.int32)
        for _ in range(R):
            quota[rng.integers(0, S)] += 1
        if trial % 9 == 0:  # negative quotas occur in the reference
            quota[0] -= 3
            quota[S - 1] += 3
        out = np.empty(R, np.int32)
        L.ref_maximize_cell_int(grid.ctypes.data_as(C.POINTER(C.c_int)), quota.ctypes.data_as(C.POINTER(C.c_int)),
                                R, S, out.ctypes.data_as(C.POINTER(C.c_int)))
        got = oracle.interslice("maximize_cell", eff[grid], quota)
        assert (got == out).all(), trial


def test_vogel_matches_reference_unit_code(oracle):
    L = _ref(oracle, "libref_tp_algos.so")
    L.ref_vogel_int.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
    # the unit program's own case
    grid = np.array([[8, 10, 9], [2, 10, 7], [2, 10, 2], [2, 10, 2], [2, 10, 2]], np.int32)
    quota = np.array([1, 3, 1], np.int32)
    got = oracle.interslice("vogel", grid.astype(np.float64), quota)
    assert got.tolist() == [2, 0, 1, 1, 1]
    rng = np.random.default_rng(2)
    for trial in range(200):
        R, S = int(rng.integers(2, 20)), int(rng.integers(2, 8))
        grid = np.ascontiguousarray(rng.integers(1, 16, (R, S)), np.int32)
        quota = np.zeros(S, np.int32)
        for _ in range(R):
            quota[rng.integers(0, S)] += 1
        out = np.empty(R, np.int32)
        L.ref_vogel_int(grid.ctypes.data_as(C.POINTER(C.c_int)), quota.ctypes.data_as(C.POINTER(C.c_int)), R, S,
                        out.ctypes.data_as(C.POINTER(C.c_int)))
        got = oracle.interslice("vogel", grid.astype(np.float64), quota)
        assert (got == out).all(), trial


def test_subopt_properties(oracle):
    """SubOpt (ref: downlink-transport-scheduler.cpp:274-349) has no reference output to pin against (no CLI number, not in
    the unit program): parity unpinned.  Checked here: quotas are met exactly when they sum to R; on grids without equal
    losses (continuous values, where the hashtable order cannot matter) it equals a plain Python restatement; and every
    move goes from an over-quota to an under-quota slice."""
    rng = np.random.default_rng(8)
    eff = np.array([0.0] + KA["eff_of_cqi"])
    for trial in range(150):
        R, S = int(rng.integers(2, 40)), int(rng.integers(1, 30))
        ties = trial % 2 == 0
        grid = eff[rng.integers(0, 16, (R, S))] if ties else rng.uniform(0.0, 5.0, (R, S))
        quota = np.zeros(S, np.int32)
        for _ in range(R):
            quota[rng.integers(0, S)] += 1
        if trial % 7 == 0 and S > 1:  # negative quotas count as 0
            quota[0] = -2
        out = oracle.interslice("subopt", grid, quota)
        q = np.maximum(quota, 0)
        got = np.bincount(out, minlength=S)
        if q.sum() == R:
            assert (got == q).all(), trial
        first = grid.argmax(1)
        moved = out != first
        have = np.bincount(first, minlength=S)
        assert (have[first[moved]] > q[first[moved]]).all() and (have[out[moved]] < q[out[moved]]).all()
        if not ties:
            own = first.copy()
            cnt = have.copy()
            more = {j: cnt[j] - q[j] for j in range(S) if cnt[j] > q[j]}
            fewer = {j: q[j] - cnt[j] for j in range(S) if cnt[j] < q[j]}
            while more and fewer:
                loss, i, j = min((grid[i, own[i]] - grid[i, j], i, j) for i in range(R) if own[i] in more for j in fewer)
                f = own[i]
                own[i] = j
                cnt[f] -= 1
                cnt[j] += 1
                more[f] -= 1
                fewer[j] -= 1
                if more[f] <= 0 or cnt[f] <= 0:
                    del more[f]
                if fewer[j] <= 0:
                    del fewer[j]
            assert (own == out).all(), trial


def test_greedy_by_row_properties(oracle):
    rng = np.random.default_rng(4)
    eff = np.array([0.0] + KA["eff_of_cqi"])
    for _ in range(100):
        R, S = 25, 20
        grid = eff[rng.integers(0, 16, (R, S))]
        quota = np.zeros(S, np.int32)
        for _ in range(R):
            quota[rng.integers(0, S)] += 1
        out = oracle.interslice("greedy_by_row", grid, quota)
        assert (np.bincount(out, minlength=S) == quota).all()
        left = quota.copy()
        for r in range(R):
            ok = left > 0
            best = np.flatnonzero(ok & (grid[r] == grid[r][ok].max()))[0]
            assert out[r] == best
            left[best] -= 1


def test_clock_and_first_ewma(oracle):
    t = 0.0
    for _ in range(100):
        t += 0.001
    assert t == KA["t_100"] and (t + 0.001) - t == KA["dt_101"]
    c = oracle.Cell([1], 12, 2, oracle.SCHED_MAXCELL)
    c.set_cqi(np.full((1, 12), 10, np.uint8))
    out = c.new_out()
    assert c.step(t, 0, 0, out) == 0
    # the averages are updated BEFORE the allocation: 0.98*100000 + 0.02*0
    c2 = oracle.Cell([1], 12, 2, oracle.SCHED_MAXCELL)
    c2.set_cqi(np.full((1, 12), 10, np.uint8))
    logs = c2.run_synth(np.full((1, 1, 12), 10, np.uint8), 1, 1)
    assert c2.state()["avg_rate"][0] == KA["first_avg"]
    assert (logs["rbg_to_user"] == 0).all()


def _ref_clock(oracle, n):
    L = _ref(oracle, "libref_clock.so")
    L.ref_clock_run.argtypes = [C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    out = np.zeros(n)
    app_now, app_before = C.c_double(), C.c_int()
    assert L.ref_clock_run(n, 0.1, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(app_now), C.byref(app_before)) == n
    return out, app_now.value, app_before.value


def test_clock_matches_reference_event_core(oracle):
    """The oracle's t_k against the reference's own Simulator/Calendar compiled in place (oracle/_ref/libref_clock.so):
    subframes scheduled at Now() + 0.001 (simulator.cc:117-126), the application start event at exactly 0.1 s, which the
    calendar runs after subframe 99 and before subframe 100 (t_100 = 0.10000000000000007 > 0.1)."""
    ref, app_now, app_before = _ref_clock(oracle, 700)
    assert (oracle.clock_ticks(0, 700) == ref).all()
    assert (oracle.clock_ticks(100, 300) == ref[100:400]).all()
    assert app_now == 0.1 and app_before == 100 and ref[99] < 0.1 < ref[100]
    assert ref[100] == KA["t_100"] and ref[101] - ref[100] == KA["dt_101"]
    # the first EWMA interval of a bearer created at 0.1 s
    assert ref[100] - app_now == float.fromhex("0x1.4p-54")


def test_clock_matches_committed_reference_fixture(oracle):
    """Same pin from the recorded outputs of libref_clock.so (tests/golden/ref_clock.json, tools/make_clock_fixture.py):
    holds where oracle/_ref is absent."""
    fx = json.loads((GOLDEN / "ref_clock.json").read_text())
    ref = np.array([float.fromhex(x) for x in fx["subframe_start"]])
    assert (oracle.clock_ticks(0, len(ref)) == ref).all()
    assert float.fromhex(fx["app_start_now"]) == 0.1 and fx["subframes_before_app_start"] == 100
    if oracle.ref_lib("libref_clock.so") is not None:
        live, _, _ = _ref_clock(oracle, len(ref))
        assert (live == ref).all(), "fixture is stale: rerun tools/make_clock_fixture.py"


def test_prb_grid_matches_reference(oracle, rs):
    """100 MHz -> 512 PRBs -> RBG size 8 -> 64 RBGs (bandwidth-manager.cpp:38,98-102; eesm-effective-sinr.h:82-103): the
    product's rs_dl_prbs_for_bandwidth / rs_get_rbg_size against the reference's BandwidthManager compiled in place and its
    recorded outputs."""
    fx = json.loads((GOLDEN / "ref_clock.json").read_text())["dl_prbs"]
    for bw, n in fx.items():
        assert rs.dl_prbs_for_bandwidth(float(bw)) == n
    assert rs.dl_prbs_for_bandwidth(100) == 512 and rs.get_rbg_size(512) == 8
    L = oracle.ref_lib("libref_bw.so")
    if L is not None:
        L.ref_dl_subchannels.argtypes = [C.c_double]
        for bw in (1.4, 3, 5, 10, 15, 20, 100, 7, 0, 99.9):
            assert rs.dl_prbs_for_bandwidth(bw) == L.ref_dl_subchannels(bw)
    E = oracle.ref_lib("libref_eesm.so")
    for n in range(1, 513):
        assert rs.get_rbg_size(n) == oracle.lib().rso_rbg_size(n)
        if E is not None:
            assert rs.get_rbg_size(n) == E.ref_get_rbg_size(n)
    with pytest.raises(rs.RadioSaberError):
        rs.get_rbg_size(513)


def cqi_keys_of_eff(eff):
    """flow_spectraleff (0 or one of the 15 CQI efficiencies, strictly increasing in the CQI) -> integer CQI keys."""
    table = np.array([0.0] + KA["eff_of_cqi"])
    keys = np.searchsorted(table, eff)
    assert (table[keys] == eff).all()
    return np.ascontiguousarray(keys, np.int32)


def ref_maximize_cell(L, keys, quota):
    R, S = keys.shape
    out = np.empty(R, np.int32)
    q = np.ascontiguousarray(quota, np.int32)
    L.ref_maximize_cell_int.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.ref_maximize_cell_int(keys.ctypes.data_as(C.POINTER(C.c_int)), q.ctypes.data_as(C.POINTER(C.c_int)), R, S,
                            out.ctypes.data_as(C.POINTER(C.c_int)))
    return out


def test_maximize_cell_on_real_tti_inputs_matches_reference_unit_code(oracle):
    """The reference's own MaximizeCell (unittest/test_tp_algos.cpp compiled in place) fed with the (flow_spectraleff, quota)
    of real TTIs -- PF state evolving over 120 TTIs, three CQI epochs, 25 and 64 RBGs -- must give the RBG -> slice map the
    oracle's TTI loop applied."""
    L = _ref(oracle, "libref_tp_algos.so")
    import radiosaber_amd as rsm
    for ues, R, G, w in (([5] * 20, 25, 4, None), ([25] * 20, 25, 4, None), ([5] * 20, 64, 8, None),
                         ([10] * 5, 25, 4, [0.62, 0.3, 0.05, 0.02, 0.01])):
        cell = oracle.Cell(ues, R, G, oracle.SCHED_MAXCELL, weights=w)
        U = cell.U
        from conftest import synth_cqi
        grids = synth_cqi(3, (3, U, R), rsm.TRACE_CQI_HISTOGRAM)
        g = oracle.Rng(12345)
        ticks = oracle.clock_ticks(100, 120)
        cell.set_last_update(0.1)
        out = cell.new_out()
        for n in range(120):
            if n % 40 == 0:
                cell.set_cqi(grids[n // 40])
            assert cell.step(float(ticks[n]), g.rand(), g.rand(), out) == 0
            keys = cqi_keys_of_eff(out.slice_eff)
            want = ref_maximize_cell(L, keys, out.quota_rbgs)
            u2s = cell.u2s
            got = np.where(out.rbg_to_user >= 0, u2s[np.maximum(out.rbg_to_user, 0)], -1)
            assert (got == want).all(), (ues, R, n)
            # and the user the apply step picked is the slice's best user on that RBG
            for r in range(R):
                if want[r] >= 0:
                    assert out.rbg_to_user[r] == out.slice_user[r, want[r]]


def test_run_synth_many_equals_single_runs(oracle):
    import radiosaber_amd as rsm
    from conftest import synth_cqi
    tmpl = oracle.Cell([5] * 20, 25, 4, oracle.SCHED_MAXCELL)
    grids = synth_cqi(9, (2, tmpl.U, 25), rsm.TRACE_CQI_HISTOGRAM)
    seeds = np.arange(6, dtype=np.uint32) + 77
    total, used = oracle.run_synth_many(tmpl, 6, grids, seeds, 80, threads=3)
    assert used == 3
    want = 0
    for s in seeds:
        c = oracle.Cell([5] * 20, 25, 4, oracle.SCHED_MAXCELL)
        c.run_synth(grids, int(s), 80, log=False)
        want += int(c.state()["cum_bytes"].sum())
    assert total == want
    # ... and the per-cell form bench.py's parity_sample uses: every cell on its OWN grids, every cell's final state returned
    own = synth_cqi(10, (6, 2, tmpl.U, 25), rsm.TRACE_CQI_HISTOGRAM)
    st = oracle.run_synth_cells(tmpl, own, seeds, 80, threads=3)
    assert st["threads"] == 3
    for i, s in enumerate(seeds):
        c = oracle.Cell([5] * 20, 25, 4, oracle.SCHED_MAXCELL)
        c.run_synth(own[i], int(s), 80, log=False)
        ref = c.state()
        assert (st["cum_bytes"][i] == ref["cum_bytes"]).all() and (st["cum_rbs"][i] == ref["cum_rbs"]).all()
        assert st["avg_rate"][i].tobytes() == ref["avg_rate"].tobytes() and st["slice_state"][i].tobytes() == ref["slice_state"].tobytes()


PIN_KINDS = ("_ref", "appendix-a", "libc", "structural", "unpinned")


def test_pin_ledger_covers_every_oracle_entry_point():
    """tests/PINS.md must name every function oracle/rs_oracle.h declares, with a known pin kind."""
    root = GOLDEN.parents[1]
    header = (root / "oracle" / "rs_oracle.h").read_text()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(rso_[a-z_0-9]+)\s*\(", header))
    assert len(declared) > 30
    rows = [ln for ln in (root / "tests" / "PINS.md").read_text().splitlines() if ln.startswith("| `rso_")]
    named = set()
    for ln in rows:
        cols = [c.strip() for c in ln.strip("|").split("|")]
        assert len(cols) == 4, ln
        named.update(re.findall(r"`(rso_[a-z_0-9]+)", cols[0]))
        kinds = re.findall(r"`([a-z_\-]+)`", cols[2])
        assert kinds and all(k in PIN_KINDS for k in kinds), f"unknown pin kind in: {ln}"
    assert declared - named == set(), f"oracle entry points without a ledger row: {sorted(declared - named)}"
    assert named - declared == set(), f"ledger rows for functions that no longer exist: {sorted(named - declared)}"


def test_appendix_a_trace_replay(oracle, traces):
    """The reference's own run: first scheduled TTI and the counters after 200 TTIs."""
    cfg = KA["config"]
    assert traces["mapping"][0][:3].tolist() == KA["user_trace_first3"]
    c = oracle.Cell(cfg["ues_per_slice"], cfg["n_rbgs"], cfg["rbg_size"], cfg["sched"], weights=[cfg["weight"]] * 20)
    logs = c.run_trace(traces["cqi"], traces["mapping"][0], cfg["seed"], cfg["rand_skip"], 200)
    first = KA["first_tti"]
    for s, (t, q) in first["quota"].items():
        assert (logs["target"][0][int(s)], logs["quota"][0][int(s)]) == (t, q)
    m = logs["rbg_to_user"][0]
    for u, info in first["users"].items():
        u = int(u)
        rb = np.flatnonzero(m == u)
        tr = traces["mapping"][0][u]
        assert [[int(r), int(traces["cqi"][tr, 2, r])] for r in rb] == info["rbgs"]
        assert logs["final_cqi"][0][u] == info["final_cqi"]
    assert (logs["tbs_bits"][0] > 0).sum() == first["n_users_served"]
    for u, (cb, cr) in first["cumu"].items():
        assert logs["tbs_bits"][0][int(u)] // 8 == cb and (m == int(u)).sum() * 8 == cr
    st = c.state()
    for u, (cb, cr) in KA["after_200_ttis"]["cumu"].items():
        assert (st["cum_bytes"][int(u)], st["cum_rbs"][int(u)]) == (cb, cr)


def test_trace_fixture_histogram_matches_survey(traces):
    import radiosaber_amd as rs
    assert traces["hist"][1:].tolist() == list(rs.TRACE_CQI_HISTOGRAM)
    assert traces["cqi"].shape == (158, 40, 64) and traces["cqi"].min() >= 1 and traces["cqi"].max() <= 15
