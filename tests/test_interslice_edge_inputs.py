"""The directed inputs of tests/interslice_edges.py on the CPU: the hashtable model equals std::unordered_map (every prefix of
ascending keys up to 64, the fewer-sets of every committed case with the erasures the case performs); every family has its minimum
number of cases and every case carries what it plants (keys, quotas, the structural positions of the scan cases, the events of
the Vogel cases); every mutant model differs from the plain one on at least three cases of its family; and the oracle -- whose
SubOpt, GreedyByRow and UpperBound rows are `unpinned` in tests/PINS.md -- equals the plain models on every case, through
rso_cell_allocate_listed and through the bare policy functions."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import interslice_edges as ie
from test_quota_edge_inputs import oracle_case_call, oracle_cell

ROOT = Path(__file__).resolve().parents[1]
POLICY = {"gbr": "greedy_by_row", "subopt": "subopt", "vogel": "vogel", "scan": "maximize_cell"}


# ---------------------------------------------------------------------------------------------------------------------------
# what a case is, from the oracle's call
# ---------------------------------------------------------------------------------------------------------------------------

_calls = {}


def oracle_answer(oracle, c, sched=None):
    """(out, slice state afterwards) of the case's one call, computed once per (case, scheduler) and never changed"""
    sched = ie.SCHED_OF[c.family] if sched is None else sched
    if (c.name, sched) not in _calls:
        cell = oracle_cell(oracle, c, sched)
        out = oracle_case_call(oracle, cell, c)
        _calls[(c.name, sched)] = (out, cell.state()["slice_state"].copy())
    return _calls[(c.name, sched)]


def slice_map(c, rbg_to_user):
    """rbg_to_user read through user_to_slice"""
    u2s = c.u2s
    return [u2s[u] if u >= 0 else -1 for u in np.asarray(rbg_to_user).tolist()]


_order = {}


def order_of(oracle, eff):
    """the record order of MaximizeCell: the plain stable sort up to 16 records, std::sort's own result above (rso_maximize_cell_order)"""
    if len(eff) * len(eff[0]) <= 16:
        return ie.stable_order(eff)
    key = np.array(eff).tobytes()
    if key not in _order:
        _order[key] = oracle.maximize_cell_order(np.array(eff)).tolist()
    return _order[key]


_plain = {}


def plain_map(oracle, family, eff, quota):
    """the plain model's RBG-to-slice map of a transport policy (cached by input)"""
    key = (family, np.array(eff).tobytes(), tuple(quota))
    if key not in _plain:
        if family == "gbr":
            got = ie.plain_greedy_by_row(eff, quota)
        elif family == "subopt":
            got = ie.plain_subopt(eff, quota)
        elif family == "vogel":
            got = ie.plain_vogel(eff, quota)[0]
        else:
            got = ie.plain_maximize_cell(order_of(oracle, eff), quota)
        _plain[key] = got
    return _plain[key]


def check_upper(c, eff, quota, upper_rbg, upper_user, what):
    """scheduler 10's lists against the model: whole up to 16 RBGs, the order-free facts above"""
    if any(q > c.R for q in quota):
        return False                          # the reference reads past its vector: device == oracle only
    upper_rbg, upper_user = np.asarray(upper_rbg), np.asarray(upper_user)
    u2s = c.u2s
    for s in range(c.S):
        n = max(quota[s], 0)
        got = upper_rbg[s, :n].tolist()
        assert (upper_rbg[s, n:] == -1).all() and (upper_user[s, n:] == -1).all() and -1 not in got, f"{what}: slice {s} holds {n} RBGs"
        assert all(u2s[u] == s for u in upper_user[s, :n]), f"{what}: slice {s}'s users"
    if c.R <= 16:
        want = ie.plain_upper_bound(eff, quota)
        for s in range(c.S):
            assert upper_rbg[s, :max(quota[s], 0)].tolist() == want.get(s, []), f"{what}: slice {s} against the plain model"
    else:
        for s, (taken, surely) in ie.upper_bound_facts(eff, quota).items():
            got = upper_rbg[s, :quota[s]].tolist()
            assert len(set(got)) == len(got) and surely <= set(got), f"{what}: slice {s}: RBGs above the cut"
            assert [eff[i][s] for i in got] == taken, f"{what}: slice {s}: the taken keys, in descending order"
    return True


def eff_and_quota(c, out):
    return out.slice_eff.tolist(), out.quota_rbgs.tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# the hashtable model
# ---------------------------------------------------------------------------------------------------------------------------

def test_hashtable_model_equals_the_real_container(oracle, tmp_path):
    exe = tmp_path / "umap_order_dump"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(ROOT / "tests" / "csrc" / "umap_order_dump.cpp")], check=True)
    experiments = []
    for n in range(1, 65):
        experiments.append((list(range(n)), []))
        experiments.append((list(range(64 - n, 64)), []))
        experiments.append(([k for k in range(64) if (k * 7 + n) % 5 < 3][:n], []))
    n_prefix = len(experiments)
    for c in ie.cases("subopt"):
        tr = {}
        ie.plain_subopt(*_inputs(oracle, c), trace=tr)
        if tr["inserted"]:
            experiments.append((tr["inserted"], tr["erased"]))
    text = "".join(" ".join(map(str, ins)) + " ; " + " ".join(map(str, era)) + "\n" for ins, era in experiments)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120, check=True).stdout
    blocks = [[list(map(int, line[1:].split())) for line in b.split("\n") if line] for b in out.split(".\n")[:-1]]
    assert len(blocks) == len(experiments)
    rehashed, erasures, sizes = set(), 0, set()
    for (ins, era), got in zip(experiments, blocks):
        m = ie.UMap()
        for k in ins:
            m.insert(k)
        want = [list(m.order)]
        for k in era:
            m.erase(k)
            want.append(list(m.order))
        assert got == want, (ins, era)
        rehashed.add(m.rehashes - 1)
        erasures += len(era)
        sizes.add(len(ins))
    assert rehashed >= {0, 1, 2, 3} and erasures > 100 and set(range(1, 65)) <= sizes and len(experiments) > n_prefix + 20


def test_rehash_thresholds():
    assert [ie.umap_rehashes(n) for n in (13, 14, 29, 30, 59, 60, 64)] == [0, 1, 1, 2, 2, 3, 3]
    assert ie.umap_order([1, 2, 3]) == [3, 2, 1] and ie.umap_order([2, 5, 15]) == [5, 15, 2]
    assert ie.integral_differences() == [(11, 1), (14, 8)] and ie.EFF[11] - ie.EFF[1] == 2.0 == ie.EFF[14] - ie.EFF[8]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases bind
# ---------------------------------------------------------------------------------------------------------------------------

def test_family_counts_and_planted_keys_and_quotas(oracle):
    total = 0
    for f in ie.FAMILIES:
        n = len(ie.cases(f))
        print(f"inter-slice edge cases, {f}: {n}")
        assert n >= ie.MIN_CASES[f], f
        total += n
    assert total <= ie.MAX_CASES
    assert {c.plants["shape"] for c in ie.all_cases()} == set(ie.SHAPES)
    for c in ie.all_cases():
        out, _ = oracle_answer(oracle, c)
        assert out.quota_rbgs.tolist() == c.plants["quota"], c.name
        assert out.target_rbs.tolist() == [q * c.G for q in c.plants["quota"]], c.name
        if c.plants["keys"] is not None:
            assert out.slice_eff.tobytes() == np.array(ie.eff_of(c.plants["keys"])).tobytes(), f"{c.name}: the keys arrive as planted"
        else:
            assert max(c.ues) > 1 and {ie.key_of(e) for e in out.slice_eff.ravel().tolist()} <= set(range(1, 16)), c.name


def _inputs(oracle, c):
    if c.plants["keys"] is not None:
        return ie.eff_of(c.plants["keys"]), c.plants["quota"]
    return oracle_answer(oracle, c)[0].slice_eff.tolist(), c.plants["quota"]


def _separated(oracle, family, mutant, plain):
    names = []
    for c in ie.cases(family):
        eff, quota = _inputs(oracle, c)
        if mutant(eff, quota) != plain(eff, quota):
            names.append(c.name)
    return names


def _report(mutant, names):
    print(f"mutant {mutant}: differs on {len(names)} cases")
    assert len(names) >= 3, (mutant, names)


def test_gbr_cases_bind(oracle):
    _report("gbr last maximum", _separated(oracle, "gbr", ie.gbr_last_maximum, ie.plain_greedy_by_row))
    _report("gbr stale pair", _separated(oracle, "gbr", ie.gbr_stale_pair, ie.plain_greedy_by_row))
    seen, pairs = set(), 0
    for c in ie.cases("gbr"):
        eff, quota = _inputs(oracle, c)
        m = ie.plain_greedy_by_row(eff, quota)
        assert -1 not in m, c.name
        for r, s in c.plants.get("pairs", []):
            # the slice takes the even RBG with its last unit and still holds the odd RBG's maximum
            assert r % 2 == 0 and m[r] == s and quota[s] == m[:r + 1].count(s) and m[r + 1] != s, c.name
            assert max(range(c.S), key=lambda k: (eff[r + 1][k], -k)) == s, c.name
            pairs += 1
            seen |= {"lane 63"} if s == 63 else set()
        if len(c.plants.get("pairs", [])) >= 2:
            seen.add("consecutive pairs")
        seen |= {"odd R"} if c.R % 2 and c.R > 1 else set()
        seen |= {"R 1"} if c.R == 1 else set()
        seen |= {"S 64"} if c.S == 64 else set()
        if min(quota) < 0 and 0 in quota and max(quota) > c.R:
            seen.add("negative, zero, above R")
        if all(len(set(row)) == 1 for row in eff) and set(quota) == {1}:
            seen.add("identical rows, quota 1")
        if c.listed is not None:
            seen.add("subset")
    assert pairs >= 20
    assert seen == {"lane 63", "consecutive pairs", "odd R", "R 1", "S 64", "negative, zero, above R", "identical rows, quota 1", "subset"}, seen


def test_subopt_cases_bind(oracle):
    _report("subopt ascending ties", _separated(oracle, "subopt", ie.subopt_ascending, ie.plain_subopt))
    _report("subopt descending ties", _separated(oracle, "subopt", ie.subopt_descending, ie.plain_subopt))
    assert _separated(oracle, "subopt", ie.subopt_unclamped, ie.plain_subopt) == []      # no mutant (interslice_edges' docstring)
    seen, rehashes = set(), set()
    for c in ie.cases("subopt"):
        eff, quota = _inputs(oracle, c)
        tr = {}
        ie.plain_subopt(eff, quota, trace=tr)
        order = ie.umap_order(tr["inserted"])
        if order != sorted(order) and order != sorted(order, reverse=True):
            rehashes.add(ie.umap_rehashes(len(order)))
        if "fewer" in c.plants:
            assert tr["inserted"] == c.plants["fewer"], c.name
        seen |= {"chain longer than S"} if tr["moves"] > c.S else set()
        seen |= {"negative quotas"} if min(quota) < 0 else set()
        seen |= {"empty slice 0"} if c.ues[0] == 0 else set()
        seen |= {"subset"} if c.listed is not None and not all(c.has) else set()
        seen |= {f"S {c.S}"} if c.S in (32, 33, 64) else set()
        if any(at < tr["moves"] for at in tr["erased_at"]):
            seen.add("erased in mid-run")
    assert rehashes >= {0, 1, 2, 3}, rehashes       # hash orders neither ascending nor descending behind 0, 1, 2 and 3 rehashes
    assert seen == {"chain longer than S", "negative quotas", "empty slice 0", "subset", "S 32", "S 33", "S 64", "erased in mid-run"}, seen


def test_vogel_cases_bind(oracle):
    plain = lambda eff, quota: ie.plain_vogel(eff, quota)[0]
    for name, kw in ie.VOGEL_MUTANTS.items():
        _report(f"vogel {name}", _separated(oracle, "vogel", lambda eff, quota: ie.plain_vogel(eff, quota, **kw)[0], plain))
    count = {t: 0 for t in ie.VOGEL_TAGS}
    sizes = set()
    for c in ie.cases("vogel"):
        eff, quota = _inputs(oracle, c)
        tr = []
        m, stopped = ie.plain_vogel(eff, quota, trace=tr)
        assert not stopped and -1 not in m, c.name
        tags = ie.vogel_tags(tr)
        assert set(c.plants.get("tags", [])) <= tags, (c.name, tags)
        assert "1.0 of a lone empty slice" not in tags, c.name      # (no TTI reaches it: bare_cases)
        for t in tags:
            count[t] += 1
        sizes |= {c.S, c.R}
    print("vogel cases per event: " + ", ".join(f"{t} {n}" for t, n in count.items()))
    assert min(count.values()) >= 3, count
    assert {32, 33, 64} <= sizes


def test_scan_cases_bind(oracle):
    stable = lambda eff, quota: ie.plain_maximize_cell(ie.stable_order(eff), quota)
    plain = lambda eff, quota: ie.plain_maximize_cell(order_of(oracle, eff), quota)
    _report("scan stable order above 16 records", _separated(oracle, "scan", stable, plain))
    seen = set()
    for c in ie.cases("scan"):
        eff, quota = _inputs(oracle, c)
        order = order_of(oracle, eff)
        flat = [eff[x // c.S][x % c.S] for x in order]
        assert sorted(order) == list(range(c.R * c.S)) and flat == sorted(flat, reverse=True), c.name
        pos = {}
        ie.plain_maximize_cell(order, quota, positions=pos)
        p = c.plants
        if "close" in p:
            s, at = p["close"]
            assert pos["closes"][s] == at and c.R <= 32, c.name
            seen.add(f"closes at {at}")
        if "last_grant_below" in p:
            assert len(pos["grants"]) == c.R and pos["grants"][-1] < p["last_grant_below"] and c.R <= 32, c.name
            seen.add("R-th grant in the first vector")
        if "last_grant_above" in p:
            assert len(pos["grants"]) == c.R and pos["grants"][-1] > p["last_grant_above"] and c.R <= 32, c.name
            seen.add("R-th grant beyond 128")
        if p.get("live_after_first_vector"):
            assert pos["live_after_first_vector"] >= p["live_after_first_vector"] and c.R <= 32, c.name
            seen.add("more than 64 live")
        if min(quota) < 0 and 0 in quota and max(quota) > c.R:
            seen.add("negative, zero, above R")
        seen |= {f"R {c.R}"} if c.R in (32, 33, 64) else set()
        seen |= {f"S {c.S}"} if c.S in (32, 33, 64) else set()
        if c.R * c.S <= 16:
            seen.add(f"{c.R} x {c.S}")
            assert order == oracle.maximize_cell_order(np.array(eff)).tolist(), f"{c.name}: std::sort is stable up to 16 records"
    assert seen == {"closes at 63", "closes at 64", "R-th grant in the first vector", "R-th grant beyond 128", "more than 64 live",
                    "negative, zero, above R", "R 32", "R 33", "R 64", "S 32", "S 33", "S 64", "4 x 4", "8 x 2", "2 x 8", "16 x 1", "1 x 16"}, seen


def test_upper_cases_bind(oracle):
    seen = set()
    for c in ie.cases("upper"):
        eff, quota = _inputs(oracle, c)
        if c.plants.get("oracle_only"):
            assert max(quota) > c.R, c.name
            seen.add("above R")
            continue
        assert max(quota) <= c.R, c.name
        ties = False
        for s, (taken, surely) in ie.upper_bound_facts(eff, quota).items():
            col = [eff[i][s] for i in range(c.R)]
            ties = ties or col.count(taken[-1]) > taken.count(taken[-1])      # the cut key goes on behind the cut
        if ties:
            seen.add("ties at the cut" + (", whole model" if c.R <= 16 else ", 25 RBGs"))
        assert ties or not c.plants.get("cut_ties"), c.name
        seen |= {"quota 0"} if any(q == 0 and c.has[s] for s, q in enumerate(quota)) else set()
        seen |= {"negative"} if min(quota) < 0 else set()
        seen |= {"exactly R"} if max(quota) == c.R else set()
        seen |= {"R 25"} if c.R == 25 else set()
        seen |= {"whole"} if c.R <= 16 else set()
    assert seen == {"above R", "ties at the cut, whole model", "ties at the cut, 25 RBGs", "quota 0", "negative", "exactly R", "R 25", "whole"}, seen


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle against the plain models
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ie.FAMILIES)
def test_oracle_equals_the_plain_models(oracle, family):
    """Every case through rso_cell_allocate_listed with the family's scheduler (8, 101, 103, 9 in full; 10 as far as the model is
    whole), and the four bare policy functions on every case's keys and quotas, whatever its family."""
    n = 0
    for c in ie.cases(family):
        out, _ = oracle_answer(oracle, c)
        eff, quota = eff_and_quota(c, out)
        if family == "upper":
            checked = check_upper(c, eff, quota, out.upper_rbg, out.upper_user, c.name)
            assert checked != bool(c.plants.get("oracle_only")), c.name
        else:
            assert slice_map(c, out.rbg_to_user) == plain_map(oracle, family, eff, quota), f"{c.name}: RBG-to-slice map"
            for s in range(c.S):
                assert all(out.slice_user[r][s] >= 0 for r in range(c.R) if plain_map(oracle, family, eff, quota)[r] == s), c.name
        for fam, fn in POLICY.items():
            if fam == "vogel" and c.S * c.R > 1100 and family != "vogel":
                continue          # (the plain Vogel on 64 x 64 takes a second per case: its own family's cases are enough there)
            assert oracle.interslice(fn, np.array(eff), quota).tolist() == plain_map(oracle, fam, eff, quota), f"{c.name}: bare {fn}"
        n += 1
    assert n == len(ie.cases(family))


def test_oracle_equals_the_plain_model_on_inputs_no_tti_reaches(oracle):
    stops = lone = 0
    for name, policy, keys, quota in ie.bare_cases():
        eff = ie.eff_of(keys)
        tr = []
        m, stopped = ie.plain_vogel(eff, quota, trace=tr)
        assert oracle.interslice(policy, np.array(eff), quota).tolist() == m, name
        stops += int(stopped)
        assert stopped == (-1 in m), name
        if "1.0 of a lone empty slice" in ie.vogel_tags(tr):
            lone += 1
    assert stops >= 2 and lone >= 2


def test_subopt_on_random_grids_with_ties(oracle):
    """test_oracle_pins.py::test_subopt_properties compares with a Python loop on grids without equal losses; here 150 grids drawn
    from three or four key values, so that equal losses are the rule, against plain_subopt and its model of the hashtable order."""
    rng = np.random.default_rng(101)
    tied = differ = 0
    for it in range(150):
        R, S = int(rng.integers(2, 41)), int(rng.integers(2, 41))
        palette = rng.choice(np.arange(1, 16), size=int(rng.integers(2, 5)), replace=False)
        keys = rng.choice(palette, size=(R, S)).tolist()
        quota = np.bincount(rng.integers(0, S, R), minlength=S).tolist()
        if it % 3 == 0:
            a, b = int(rng.integers(0, S)), int(rng.integers(0, S))
            if a != b:
                d = quota[a] + int(rng.integers(1, 4))
                quota[a] -= d
                quota[b] += d
        eff = ie.eff_of(keys)
        want = ie.plain_subopt(eff, quota)
        assert oracle.interslice("subopt", np.array(eff), quota).tolist() == want, (it, R, S)
        tied += int(ie.subopt_ascending(eff, quota) != want or ie.subopt_descending(eff, quota) != want)
        differ += int(ie.subopt_ascending(eff, quota) != want and ie.subopt_descending(eff, quota) != want)
    print(f"random grids with ties: {tied} of 150 depend on the hashtable order, {differ} differ from both sorted orders")
    assert tied >= 50 and differ >= 10
