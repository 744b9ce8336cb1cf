"""The directed inputs of tests/quota_edges.py on the CPU: every case plants what its tag claims (from the plain model's intermediates
and from struct.pack bit patterns), every family has its minimum number of cases, and the oracle -- whose rows for this path are
`unpinned` in tests/PINS.md and which spells the same C expressions as the kernel -- equals the plain model on every case:
rso_cell_allocate_listed's targets, quotas and slice state for schedulers 8, 9, 10, 101 and 103, scheduler 8's RBG-to-slice map on the
oracle's own slice keys, scheduler 7's served slice and EWMAs over 5 steps of Cell.step.

Last, a float32 numpy model of the kernels' idiv_small and the bound up to which it equals C division (IDIV_EXACT_BELOW)."""
from fractions import Fraction

import numpy as np
import pytest

import quota_edges as qe
from test_gpu_dropin_oracle import oracle_call

# idiv_small(a, b), 1 <= b <= 64, equals C's a / b for every |a| below this; it first fails at a = +-(2^25 + 2), b = 1, where the
# conversion of a to float32 is off by two.  Found by test_idiv_small_first_failure's search and once by an exhaustive scan of
# |a| <= 2^28 for every b.
IDIV_EXACT_BELOW = 2**25 + 2


def arrays(c):
    return np.array(c.cqi, np.uint8), np.array(c.avg, np.float64)


def case_ids(c):
    return None if c.listed is None else np.array(c.listed, np.int32)


def oracle_cell(oracle, c, sched):
    cell = oracle.Cell(c.ues, c.R, c.G, sched, weights=c.w)
    cell.set_slice_offset(c.state)
    return cell


def oracle_case_call(oracle, cell, c, r0=None, r1=None):
    cqi, avg = arrays(c)
    ids = case_ids(c)
    rows = slice(None) if ids is None else ids
    return oracle_call(cell, ids, cqi[rows], avg[rows], rand0=c.r0 if r0 is None else r0, rand1=c.r1 if r1 is None else r1)


def granted_of(c, sched, out):
    """RBGs per slice as :595 / :606 count them"""
    if sched == 10:
        return [int((out.upper_rbg[s] >= 0).sum()) for s in range(c.S)]
    u2s = np.array(c.u2s)
    m = out.rbg_to_user
    return [int((u2s[m[m >= 0]] == s).sum()) for s in range(c.S)]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases bind
# ---------------------------------------------------------------------------------------------------------------------------

def test_family_counts():
    for f in qe.FAMILIES:
        n = len(qe.cases(f))
        print(f"quota edge cases, {f}: {n}")
        assert n >= qe.MIN_CASES[f], f
    for c in qe.all_cases():
        if c.family != "nvs":
            t = c.steps()["target"]
            assert max(abs(x) for x in t) < 2**15, c.name     # batch logs are int16


def test_trunc_cases_bind():
    seen = set()
    for c in qe.cases("trunc"):
        st, p = c.steps(), c.plants
        if "sums" in p:
            for s in range(c.S):
                x = c.nb * c.w[s] + c.state[s]
                assert x == p["sums"][s] and int(x) == p["raw"][s] == st["raw"][s], c.name
                seen.add("negative fraction" if -1 < x < 0 else "negative" if x < 0 else "integer" if x == int(x) else "fraction")
                if x != int(x) and c.state[s] != int(c.state[s]) and c.state[s] * 2 != int(c.state[s] * 2):
                    seen.add("fractional offset")
        else:
            assert st["target"] == p["target"] and st["quota0"] == p["quota0"] and st["extra_rbs"] == 0, c.name
            for t, q in zip(st["target"], st["quota0"]):
                if t < 0:
                    assert q == -((-t) // c.G) and q != t // c.G or t % c.G == 0, c.name   # toward zero, not the floor
                    seen.add(f"target {t}" if -t <= c.G + 1 else "target below")
    assert {"negative fraction", "negative", "integer", "fraction", "fractional offset"} <= seen
    assert {"target -1", "target -3", "target -4", "target -5"} <= seen     # -1, -G + 1, -G, -G - 1 at G = 4


def test_product_cases_bind():
    grids = {}
    heads = 0
    for c in qe.cases("product"):
        p = c.plants
        for sl, ref, fus in [(p["slice"], p["reference"], p["fused"])] + ([p["also"]] if "also" in p else []):
            assert qe.reference_target(c.nb, c.w[sl], c.state[sl]) == ref != fus == qe.fused_target(c.nb, c.w[sl], c.state[sl]), c.name
            # the product is inexact and the exact sum lies on the other side of an integer
            exact = Fraction(c.nb) * Fraction(c.w[sl]) + Fraction(c.state[sl])
            assert Fraction(c.nb * c.w[sl]) != Fraction(c.nb) * Fraction(c.w[sl]) and int(exact) == fus, c.name
        a, b = c.steps(), c.steps(target_of=qe.fused_target)
        assert (a["target"], a["quota"]) != (b["target"], b["quota"]), c.name
        assert a["first0"] == p["head"], c.name
        heads += int(p["head"] == p["slice"] and a["rem"] != 0)
        grids[(c.R, c.G)] = grids.get((c.R, c.G), 0) + 1
    assert set(grids) == set(qe.PRODUCT_GRIDS) and min(grids.values()) >= 2
    assert heads >= 2, "no binding slice that also receives the remainder"
    c = qe.cases("product")[0]
    assert (c.nb, c.w[0], c.state[0]) == (100, 0.05, -6.0)
    # grids of 8, 32 or 512 PRBs cannot hold such a case: nb * w is exact there
    assert all(qe.no_product_triples_on(nb) for nb in (8, 32, 512))


def test_negdiv_cases_bind():
    seen_rbs, seen_rbgs, negative_rem_heads = set(), set(), 0
    for c in qe.cases("negdiv"):
        st, p = c.steps(), c.plants
        n = p["n"]
        assert st["n"] == n and st["extra_rbs"] == p["extra_rbs"], c.name
        e = st["extra_rbs"]
        assert st["share"] * n + st["rem"] == e and abs(st["rem"]) < n and (st["rem"] == 0 or (st["rem"] < 0) == (e < 0)), c.name
        if e < 0 and e % n:
            assert st["share"] != e // n, c.name     # where the floor would differ
        if "rem" in p:
            assert st["rem"] == p["rem"] and st["first0"] == p["first0"], c.name
            seen_rbs.add((n, e))
            negative_rem_heads += int(st["rem"] < 0)
        if "extra_rbgs" in p:
            assert st["extra_rbgs"] == p["extra_rbgs"] and st["rem_g"] == p["rem_g"] and st["first1"] == p["first1"], c.name
            assert st["share_g"] == 0, c.name
            seen_rbgs.add((n, st["extra_rbgs"]))
            negative_rem_heads += int(st["rem_g"] < 0)
    for n in (1, 2, 3, 4):
        for e in (-1, -(n - 1), -n, -(n + 1), 1, n - 1, n, n + 1):
            assert e == 0 or (n, e) in seen_rbs, (n, e)
        assert any(k == n and e < -200 for k, e in seen_rbs) and any(k == n and e > 200 for k, e in seen_rbs)
    assert {(4, -2), (4, -1), (4, 1), (4, 3), (3, -1), (3, 2), (2, 1)} <= seen_rbgs
    assert negative_rem_heads >= 8


def test_rotate_cases_bind():
    seen, sizes, differ, big = set(), set(), 0, 0
    for c in qe.cases("rotate"):
        st, p, S = c.steps(), c.plants, c.S
        assert st["first0"] == p["first0"] and st["first1"] == p["first1"], c.name
        assert 0 <= c.r0 <= qe.RAND_MAX - S and 0 <= c.r1 <= qe.RAND_MAX - S, c.name
        big += int(c.r0 > 2**30) + int(c.r1 > 2**30)
        sizes.add(S)
        if S > 1:
            assert st["rem"] != 0 and st["rem_g"] != 0, c.name      # else the head of the rotation would not show
            for r, f in ((c.r0, st["first0"]), (c.r1, st["first1"])):
                seen.add((S, {0: "0", 1: "1", S - 1: "S-1"}.get(r % S, "other")))
                start = r % S
                if not c.ues[start]:
                    seen.add("starts on an empty slice")
                elif not c.has[start]:
                    seen.add("starts on a slice with no listed user")
                if f < start:
                    seen.add("wraps")
            differ += int(st["first0"] != st["first1"])
    assert sizes == {1, 3, 5, 64}
    assert {(S, k) for S in (3, 5) for k in ("0", "1", "S-1")} <= seen and (64, "S-1") in seen
    assert {"starts on an empty slice", "starts on a slice with no listed user", "wraps"} <= seen
    assert differ >= 4 and big >= 6


def test_policy_cases_bind():
    seen = set()
    for c in qe.cases("policy"):
        q = c.steps()["quota"]
        assert q == c.plants["quota"] and sum(q) == c.R, c.name
        seen |= {"negative"} if min(q) < 0 else set()
        seen |= {"zero"} if 0 in q else set()
        seen |= {"above R"} if max(q) > c.R else set()
        seen |= {"all R"} if sorted(q) == [0] * (c.S - 1) + [c.R] else set()
        assert any(len({c.cqi[u][r] for u in range(c.U)}) == 1 for r in range(c.R)), c.name   # equal keys across slices
    assert seen == {"negative", "zero", "above R", "all R"}


def test_nvs_cases_bind():
    seen = set()
    for c in qe.cases("nvs"):
        p, has = c.plants, c.has
        pick, after = qe.plain_nvs_pick(c.w, c.state, has)
        assert pick == p["pick"], c.name
        score = [qe.bits(c.w[s] / c.state[s]) if c.state[s] != 0 else None for s in range(c.S)]
        word = lambda s: (score[s][0] << 32) | score[s][1]
        if "equal" in p:
            assert len({score[s] for s in p["equal"]}) == 1 and pick == p["equal"][-1], c.name
            assert all(word(s) <= word(pick) for s in range(c.S) if has[s]), c.name
            seen.add(f"equal {len(p['equal'])}")
        if "ulp" in p:
            a, b = p["ulp"]
            assert word(a) == word(b) + 1 and pick == a, c.name
            seen.add("ulp " + ("first" if a < b else "last"))
        if "straddle" in p:
            a, b = p["straddle"]
            assert score[a][0] == score[b][0] and score[a][1] >= 0x80000000 > score[b][1] and pick == a, c.name
            assert score[a][1] - score[b][1] < 64, c.name    # (either side of the sign bit of the low word, a few ulps apart)
            seen.add("straddle " + ("first" if a < b else "last"))
        if "hilo" in p:
            a, b = p["hilo"]
            assert score[a][0] > score[b][0] and score[a][1] < score[b][1] and pick == a, c.name
            seen.add("hilo")
        if "infinite" in p:
            assert c.state[p["infinite"]] == 5e-324 and score[p["infinite"]] == (0x7FF00000, 0), c.name
            assert 0x7FE00000 <= score[p["finite"]][0] < 0x7FF00000, c.name
            seen.add("infinite")
        if "ignored" in p:
            s = p["ignored"]
            assert not has[s] and (c.state[s] == 0 or all(word(s) >= word(k) for k in range(c.S) if has[k])), c.name
            seen.add("ignored zero" if c.state[s] == 0 else "ignored best")
        if "fused" in p:
            e = p["fused"]
            assert c.state[pick] == e and after[pick] == (1 - qe.BETA) * e + qe.BETA * 1 != qe.fused_ewma(e), c.name
            seen.add("fused")
        if sum(has) == 1 and not has[0]:
            seen.add("alone, not slice 0")
        if c.S == 64:
            seen.add("S 64")
        if sum(1 for s in range(c.S) if has[s] and c.state[s] == 0) >= 2:
            seen.add("two zeros")
        if any(has[s] and c.state[s] == 0 and any(has[k] and c.state[k] != 0 for k in range(s)) for s in range(c.S)):
            seen.add("zero after a score")
    assert {"equal 2", "equal 3", "ulp first", "ulp last", "straddle first", "straddle last", "hilo", "infinite", "ignored zero",
            "ignored best", "fused", "alone, not slice 0", "S 64", "two zeros", "zero after a score"} <= seen, seen


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle against the plain model
# ---------------------------------------------------------------------------------------------------------------------------

ONE_CALL = ("trunc", "product", "negdiv", "rotate", "policy")


@pytest.mark.parametrize("sched", qe.TRANSPORT)
def test_oracle_quotas_equal_the_plain_model(oracle, sched):
    n = 0
    for f in ONE_CALL:
        for c in qe.cases(f):
            cell = oracle_cell(oracle, c, sched)
            out = oracle_case_call(oracle, cell, c)
            target, quota = qe.plain_quotas(c.nb, c.G, c.w, c.state, c.has, c.r0, c.r1)
            assert out.target_rbs.tolist() == target, f"sched {sched} {c.name}: targets"
            assert out.quota_rbgs.tolist() == quota, f"sched {sched} {c.name}: quotas"
            want = qe.plain_offsets_after(target, granted_of(c, sched, out), c.G)
            assert cell.state()["slice_state"].tolist() == want, f"sched {sched} {c.name}: offsets afterwards"
            n += 1
    assert n == sum(len(qe.cases(f)) for f in ONE_CALL)


def test_oracle_greedy_by_row_equals_the_plain_model(oracle):
    ties = 0
    for f in ONE_CALL:
        for c in qe.cases(f):
            cell = oracle_cell(oracle, c, 8)
            out = oracle_case_call(oracle, cell, c)
            keys = out.slice_eff.tolist()
            want = qe.plain_greedy_by_row(keys, out.quota_rbgs.tolist())
            u2s = np.array(c.u2s)
            got = [int(u2s[u]) if u >= 0 else -1 for u in out.rbg_to_user]
            assert got == want, f"{c.name}: RBG-to-slice map"
            if f == "policy":
                has = c.has
                ties += sum(1 for row in keys if len({row[s] for s in range(c.S) if has[s]}) < sum(has))
    assert ties > 0, "no equal keys across slices in the policy cases"


@pytest.mark.parametrize("sched", qe.TRANSPORT)
def test_oracle_chains_equal_the_plain_model(oracle, sched):
    for c in qe.cases("chain"):
        cell = oracle_cell(oracle, c, sched)
        before = list(c.state)
        flips = 0
        for t in range(qe.CHAIN_TTIS):
            r0, r1 = c.rands[t]
            out = oracle_case_call(oracle, cell, c, r0, r1)
            target, quota = qe.plain_quotas(c.nb, c.G, c.w, before, c.has, r0, r1)
            assert (out.target_rbs.tolist(), out.quota_rbgs.tolist()) == (target, quota), f"sched {sched} {c.name} TTI {t}"
            after = cell.state()["slice_state"].tolist()
            assert after == qe.plain_offsets_after(target, granted_of(c, sched, out), c.G), f"sched {sched} {c.name} TTI {t}: offsets"
            flips += sum(1 for a, b in zip(before, after) if a * b < 0)
            before = after
        assert flips > 0, f"sched {sched} {c.name}: no offset changed sign"


def test_oracle_slice_pick_equals_the_plain_model(oracle):
    for c in qe.cases("nvs"):
        cell = oracle.Cell(c.ues, c.R, c.G, oracle.SCHED_NVS, weights=c.w)
        cell.set_slice_offset(c.state)
        cell.set_cqi(np.array(c.cqi, np.uint8))
        ewma = list(c.state)
        for t, now in enumerate(oracle.clock_ticks(100, 5)):
            out = cell.new_out()
            assert cell.step(float(now), 0, 0, out) == 0
            pick, ewma = qe.plain_nvs_pick(c.w, ewma, c.has)
            assert out.served_slice == pick, f"{c.name} step {t}: served slice"
            got = cell.state()["slice_state"]
            assert got.tobytes() == np.array(ewma, np.float64).tobytes(), f"{c.name} step {t}: EWMAs"
            if t == 0:
                assert pick == c.plants["pick"]


# ---------------------------------------------------------------------------------------------------------------------------
# idiv_small
# ---------------------------------------------------------------------------------------------------------------------------

def idiv_small_model(a, b):
    """Restates radiosaber_amd/csrc/rs_wave.h:92-101 (idiv_small) on numpy arrays: one correctly rounded float32 division of the
    converted operands, truncation, and the +-1 fix-up from the remainder, with its separate branches for negative numerators."""
    a = np.asarray(a, np.int64)
    q = (a.astype(np.float32) / np.float32(b)).astype(np.int64)
    r = a - q * b
    pos = a >= 0
    q = np.where(pos & (r < 0), q - 1, np.where(pos & (r >= b), q + 1, q))
    q = np.where(~pos & (r > 0), q + 1, np.where(~pos & (r <= -b), q - 1, q))
    return q


def c_division(a, b):
    a = np.asarray(a, np.int64)
    return np.sign(a) * (np.abs(a) // b)


def test_idiv_small_is_c_division_where_the_quota_step_uses_it():
    a = np.arange(-2**17, 2**17 + 1, dtype=np.int64)
    for b in range(1, 65):
        np.testing.assert_array_equal(idiv_small_model(a, b), c_division(a, b), err_msg=f"b = {b}")


def _first_failure(b, lo, hi, chunk=1 << 22):
    for start in range(lo, hi + 1, chunk):
        a = np.arange(start, min(start + chunk, hi + 1), dtype=np.int64)
        bad = (idiv_small_model(a, b) != c_division(a, b)) | (idiv_small_model(-a, b) != c_division(-a, b))
        if bad.any():
            return int(a[np.argmax(bad)])
    return None


def test_idiv_small_first_failure():
    """The smallest |a| at which idiv_small(a, b) != a / b for some 1 <= b <= 64: IDIV_EXACT_BELOW = 2^25 + 2 (b = 1), found by
    scanning b = 1 upwards from 2^24.  Below 2^24 every divisor is exact by argument: the conversion is exact and the rounded quotient
    is within one of the true one, which is what the fix-up repairs (the test above covers |a| <= 2^17 exhaustively).  For b >= 2 the
    argument reaches the bound: up to 2^25 + 2 the conversion is off by at most 2, i.e. by at most 1 in the quotient together with
    the quotient's own rounding (it is below 2^24).  Those divisors are scanned over the last 2^16 numerators below the bound, where
    the errors are largest (an exhaustive scan of every b over |a| <= 2^28 was run once: the next divisor to fail is 3, at
    50331662)."""
    assert _first_failure(1, 2**24, IDIV_EXACT_BELOW + 2**16) == IDIV_EXACT_BELOW
    for b in range(2, 65):
        assert _first_failure(b, IDIV_EXACT_BELOW - 2**16, IDIV_EXACT_BELOW) is None, b
    assert _first_failure(3, 50331662 - 1000, 50331662 + 1000) == 50331662
    # the header states the same figure where it gives the setters' domain
    from pathlib import Path
    header = (Path(__file__).resolve().parents[1] / "include" / "radiosaber_hip.h").read_text()
    assert "2^25 + 2 (33554432 + 2" in header
