"""CPU proof that the edge populations of tests/queue_edges.py bind (no GPU needed), and the oracle's second opinion for the queue
model: every event class of the RLC dequeue and every planted case of the two gates occurs, measured from the plain model's event log
and from the oracle's RBG maps rather than from the builder's plan; the oracle's per-packet std::deque (`rso_cell_step_queues`,
`unpinned` in tests/PINS.md) agrees with the plain Python model on every population, TTI by TTI; and two deliberately wrong variants
of the model (a fragment at an exact fit; no 8-byte rule) are caught -- device == oracle (tests/test_gpu_queue_edges.py) == plain
model (here)."""
import collections

import numpy as np
import pytest

import queue_edges as qe


@pytest.fixture(scope="module")
def pops(oracle):
    return qe.all_populations(oracle)


@pytest.fixture(scope="module")
def runs(oracle, pops):
    return {p.name: qe.oracle_run(oracle, p) for p in pops}


@pytest.fixture(scope="module")
def link(oracle):
    return oracle.lib().rso_tbs_bits, oracle.tables()["cqi_to_mcs"]


def test_the_grants_are_what_the_populations_are_built_on(oracle, pops):
    """bits per TTI of a lone backlogged user by uniform CQI (the round trip through EESM gives a final CQI of c or c - 1)"""
    bits = [int(oracle.lib().rso_tbs_bits(int(oracle.tables()["cqi_to_mcs"][qe.backlogged_grant(oracle, 9, [1], 6, 2, [c])[1][0] - 1]), 12))
            for c in range(1, 16)]
    assert bits == [328, 520, 840, 840, 1672, 1864, 2408, 3112, 3112, 3880, 4776, 5544, 6456, 7224, 8760]
    assert [int(qe.backlogged_grant(oracle, 9, [1], 6, 2, [c])[0][0]) for c in (1, 9, 15)] == [41, 389, 1095]
    assert int(qe.backlogged_grant(oracle, 9, [1], 25, 4, [15])[0][0]) == 9422
    # deterministic builders, every cell present, at most 48 TTIs and 128 cells per batch
    assert {p.name: p.n_cells for p in pops} == qe.FAMILY_CELLS
    again = qe.all_populations(oracle)
    for p, q in zip(pops, again):
        assert p.n_ttis <= 48 and p.n_cells <= 128 and len(p.plan) == p.n_cells
        assert p.cqi.tobytes() == q.cqi.tobytes() and p.bursts.keys() == q.bursts.keys()
        assert all(a.tobytes() == b.tobytes() for k in p.bursts for a, b in zip(p.bursts[k], q.bursts[k]))


def test_a_lone_packet_of_b_minus_8_bytes_fits_and_one_byte_more_does_not(oracle):
    ticks = oracle.clock_ticks(100, 3)
    for size, want in ((381, [389, 0, 0]), (382, [389, 9, 0])):
        m = qe.plain_user("Q-", {0: ([ticks[0]], [0], [size])}, ticks, [(389, 12)] * 3)
        assert m["credited"][:, 0].tolist() == want and m["queue_packets"][-1, 0] == 0


def test_the_oracle_agrees_with_the_plain_model_and_every_event_class_occurs(oracle, pops, runs):
    events, per_family = collections.Counter(), {}
    for p in pops:
        bad, ev = qe.disagreements(oracle, p, runs[p.name])
        assert not bad, (p.name, bad[:10], [p.plan[c] for c, _, _ in bad[:3]])
        events += ev
        per_family[p.name] = ev
    print("\ncells and TTIs per family:", {p.name: (p.n_cells, p.n_ttis) for p in pops})
    print("event counts:", {k: events[k] for k in qe.CLASSES})
    print("further events:", {k: v for k, v in sorted(events.items()) if k not in qe.CLASSES and not k.startswith("fragment-leaves-")},
          "; fragments that leave 10 bytes or more:", sum(v for k, v in events.items() if k.startswith("fragment-leaves-") and int(k[16:]) > 9))
    missing = [k for k in qe.CLASSES if events[k] == 0]
    assert not missing, missing
    # where the issue places them
    fit = per_family["fit"]
    assert fit["whole-exact"] >= 3 and all(fit[f"whole-with-room-{r}"] >= 3 for r in range(1, 9))
    assert all(fit[f"fragment-leaves-{r}"] >= 3 for r in range(1, 10)) and fit["fragment-continues"] >= 40
    rn = per_family["runs"]
    assert rn["run-capped-by-grant"] > 0 and rn["run-capped-by-burst"] > 0 and rn["run-ends-at-burst-end"] > 0 and rn["queue-emptied"] > 0
    assert rn["whole-exact"] >= 2      # a grant that ends exactly on the burst's boundary
    mh = per_family["many-heads"]
    assert max(int(k[6:]) for k in mh if k.startswith("heads-")) >= 10 and mh["whole-with-room-8"] >= 2 and mh["fragment-of-1-byte"] >= 2
    assert fit["fragment-of-1-byte"] >= 3    # d = -9: room of 9 after the first packet
    ins = per_family["instants"]
    for k in ("arrival-on-tick", "arrival-ulp-late", "arrival-ulp-early", "arrival-into-empty", "arrival-into-nonempty", "arrival-right-after-emptied"):
        assert ins[k] > 0, k
    for kinds in ("QQ", "BQ"):
        assert all(per_family[f"split-{kinds}"][f"second-bearer-offered-{r}"] >= 1 for r in range(10)), kinds
    assert per_family["split-QQ"]["nothing-sent"] >= 8    # offers of 1 .. 8 bytes: credited, nothing dequeued
    assert per_family["split-QB"]["second-bearer-offered-0"] >= 11


def test_an_ulp_late_burst_waits_a_tti_and_the_silent_stretch_occurs(oracle, pops, runs):
    p = next(p for p in pops if p.name == "instants")
    run = runs[p.name]
    ticks = oracle.clock_ticks(100, p.n_ttis)
    # cell 0, user 0: the burst one ulp after tick 2 is queued in TTI 3, the one an ulp before tick 5 in TTI 5
    qp = run["queue_packets"][0, :, 0, 0]
    by = run["bearer_bytes"][0, :, 0, 0]
    assert by[2] == 0 and by[3] > 0 and by[5] > 0 and qp[2] == 0
    # cell 3: nobody has data in TTIs 3 .. 11: nothing is allocated (and the oracle draws no rand() there), then both users return --
    # user 0 with a burst stamped on the tick (the 1e-5 floor), user 1 with one queued a TTI before (an ulp after tick 11)
    idle = (run["maps"][3] < 0).all(1)
    assert idle[3:12].all() and not idle[12] and not idle[0]
    assert run["bearer_hol"][3, 12, 0, 0] == 0.00001 and run["bearer_hol"][3, 12, 1, 0] == ticks[12] - p.bursts[(3, 1, 0)][0][1]


def test_every_gate_case_occurs_and_the_gate_functions_match_the_oracles_maps(oracle, pops, runs, link):
    tbs_bits, cqi_to_mcs = link
    seen7, seen1 = collections.Counter(), collections.Counter()
    for p in pops:
        if not p.name.startswith("gate"):
            continue
        run = runs[p.name]
        for c in range(p.n_cells):
            row = run["maps"][c, 0]
            if p.sched == 7:
                pl = p.plan[c]
                took = int((row == 0).sum())
                assert (row[:took] == 0).all() and (row[took:] == 1).all(), (p.name, c, row)   # a prefix: the RBG after which user 0 left
                assert pl["first"] * 8 == (p.G * pl["k"] + pl["dm"]) * tbs_bits(int(cqi_to_mcs[pl["wide"] - 1]), 1) + pl["e"]
                need = qe.required_prbs(pl["first"], oracle.final_cqi([int(p.cqi[c, 0])] * (p.R * p.G)), tbs_bits, cqi_to_mcs)
                assert need == p.G * pl["k"] + pl["dm"] - (pl["e"] < 0)
                assert took == qe.rbgs_until_left(pl["first"], 7, p.R, p.G, pl["wide"], tbs_bits, cqi_to_mcs) == -(-need // p.G), (p.name, pl, took)
                seen7[(p.G, pl["k"], pl["dm"], pl["e"], took)] += 1
                seen7[("need mod G", p.G, need % p.G)] += 1
            else:
                fc = int(run["final_cqi"][c, 0, 0])
                assert fc == p.plan[c]["final_cqi"]
                pos = 0
                for b, fl in enumerate(p.plan[c]["flows"]):
                    took = int((row == b).sum())
                    assert (row[pos:pos + took] == b).all(), (p.name, c, row)
                    assert took == qe.rbgs_until_left(fl["data"], 1, p.R, p.G, fc, tbs_bits, cqi_to_mcs) == fl["k"] + (fl["d"] > 0), (fl, took)
                    assert qe.block_carries(took, p.G, fc, fl["data"], tbs_bits, cqi_to_mcs)
                    assert took == 1 or not qe.block_carries(took - 1, p.G, fc, fl["data"], tbs_bits, cqi_to_mcs)
                    # the whole block is credited, with no min against the data
                    assert run["bearer_bytes"][c, 0, 0, b] == tbs_bits(int(cqi_to_mcs[fc - 1]), took * p.G) // 8
                    seen1[(b, fl["k"], fl["d"], took)] += 1
                    pos += took
                assert (row[pos:] == 2).all()
    print("\nscheduler 7 (G, k, dm, e, RBGs taken):", sorted((k, v) for k, v in seen7.items() if k[0] != "need mod G"))
    print("scheduler 1 (bearer, k, d, RBGs taken):", sorted(seen1.items()))
    for G in (2, 4):
        assert all(sum(v for key, v in seen7.items() if key[:4] == (G, k, dm, e)) == 1 for k in (1, 2, 3) for dm in (-1, 0, 1) for e in (-8, 0, 8))
        assert {key[2] for key in seen7 if key[:2] == ("need mod G", G)} >= {0, 1, G - 1}
        assert {key[4] for key in seen7 if key[0] == G} >= {1, 2, 3, 4}
    for b in (0, 1):
        assert all(seen1[(b, k, d, k + (d > 0))] == 1 for k in (1, 2, 3) for d in (-1, 0, 1))


@pytest.mark.parametrize("variant, family", [("frag_ge", "fit"), ("ignore_min_room", "fit"), ("frag_ge", "runs"), ("ignore_min_room", "split-QQ")])
def test_a_wrong_model_is_caught(oracle, pops, runs, variant, family):
    """'>=' for '>' at the fragment test turns every exact fit into a fragment that leaves 0 bytes behind; without the rule that room of
    at most 8 sends nothing, room of 1 .. 7 'sends' a fragment of negative size.  The populations hold both."""
    p = next(p for p in pops if p.name == family)
    bad, _ = qe.disagreements(oracle, p, runs[p.name], **{variant: True})
    assert bad, f"the {family} population does not tell the model with {variant} from the right one"
    cells = {c for c, _, _ in bad}
    if family == "fit":
        want = {0} if variant == "frag_ge" else set(range(-7, 0))
        assert {p.plan[c]["d"] for c in cells} >= want, sorted(p.plan[c]["d"] for c in cells)
