"""MaximizeCell's greedy scan over the array std::__introsort_loop leaves (rs_interslice.h: interslice_maximize_cell_segments), as
a plain model on the CPU: the grants equal the serial greedy's over std::sort's output.

What the device does: the loop (rs_sort_device.h, tagged form) leaves sub-ranges of at most 16 records, ordered against each other
and unordered inside, each record carrying its sub-range's first position (a heap-sorted range: every position its own).  Wave 0
takes the positions below the last sub-range start at or before 64 and decides them in final order without moving them
(wave_stable_before_desc: per lane the lanes whose record comes before its own); what is still live of the rest is filtered in
array order and goes, cut where the carried start changes, through the same step.  The serial loop comes from the product's own pieces (tests/csrc/sort_segments_dump.cpp over rs_sort_emul.h), which also
checks the loop against std::sort itself."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = Path(__file__).resolve().parents[1]

SHAPES = {17: (17, 1), 40: (8, 5), 48: (16, 3), 64: (16, 4), 65: (13, 5), 80: (16, 5), 500: (25, 20), 1024: (32, 32), 1280: (64, 20)}


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    exe = tmp_path_factory.mktemp("seg") / "sort_segments_dump"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(ROOT / "tests" / "csrc" / "sort_segments_dump.cpp")], check=True)

    def run(arrays):
        """[(ids in the loop's order, sub-range start of every position)] for a list of key arrays"""
        text = "".join(f"{len(k)} " + " ".join(str(int(x)) for x in k) + "\n" for k in arrays)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = []
        for k, line in zip(arrays, r.stdout.strip().split("\n")):
            w = np.array(line.split(), np.int64)
            assert len(w) == 2 * len(k)
            out.append((w[:len(k)], w[len(k):]))
        return out
    return run


# ---- the serial greedy of the reference (downlink-transport-scheduler.cpp:362-369) over records (key, rbg, slice) ----

def greedy_serial(records, R, quota):
    """records in scan order; returns the slice of every RBG (-1: none)"""
    owner = np.full(R, -1, np.int64)
    left = np.array(quota, np.int64).copy()
    for (_, r, s) in records:
        if owner[r] < 0 and left[s] > 0:
            owner[r] = s
            left[s] -= 1
    return owner


# ---- the device's steps ----

def wave_stable_rank_desc(keys, valid):
    """the rank a stable sort by descending key gives every valid lane, as (records with a larger key) + (equal keys in lower
    lanes), from the four bit planes of the keys as lane masks: what the popcount of wave_stable_before_desc must equal"""
    n = len(keys)
    assert n <= 64
    plane = [sum(1 << i for i in range(n) if (keys[i] >> b) & 1) for b in range(4)]
    vm = sum(1 << i for i in range(n) if valid[i])
    full = (1 << 64) - 1

    def same_as(k):  # valid lanes that hold key k
        d = 0
        for b in range(4):
            d |= plane[b] ^ (full if (k >> b) & 1 else 0)
        return vm & ~d & full
    cnt = [bin(same_as(q)).count("1") for q in range(16)]
    inc = np.cumsum(cnt)  # the row scan: records of a key up to q
    ranks = []
    for i in range(n):
        above = int(inc[15] - inc[keys[i] & 15])
        rank_eq = bin(same_as(keys[i]) & ((1 << i) - 1)).count("1")
        ranks.append(above + rank_eq)
    return ranks


def wave_stable_before_desc(keys, valid):
    """rs_interslice.h: per lane the mask of the valid lanes a stable sort by descending key puts before it -- compared from the
    top bit plane down, no record moves"""
    n = len(keys)
    full = (1 << 64) - 1
    plane = [sum(1 << i for i in range(n) if (keys[i] >> b) & 1) for b in range(4)]
    vm = sum(1 << i for i in range(n) if valid[i])
    out = []
    for i in range(n):
        gt, eq = 0, full
        for b in (3, 2, 1, 0):
            mine = full if (keys[i] >> b) & 1 else 0
            gt |= eq & plane[b] & ~mine & full
            eq &= ~(plane[b] ^ mine) & full
        out.append((gt | (eq & ((1 << i) - 1))) & vm)
    return out


def wave_sort_records_desc(vec):
    """the records of one vector in the order the device's decision step meets them"""
    keys = [k for (k, _, _) in vec]
    before = wave_stable_before_desc(keys, [True] * len(vec))
    ranks = [bin(b).count("1") for b in before]
    assert ranks == wave_stable_rank_desc(keys, [True] * len(vec)) and sorted(ranks) == list(range(len(vec)))
    out = [None] * len(vec)
    for rec, rk in zip(vec, ranks):
        out[rk] = rec
    return out


def greedy_segments(arr, seg, R, quota, stats=None):
    """arr: records in the loop's order, seg: their sub-range starts.  Mirrors interslice_maximize_cell_segments."""
    owner = np.full(R, -1, np.int64)
    left = np.array(quota, np.int64).copy()
    src = [(rec, int(f)) for rec, f in zip(arr, seg)]
    n_taken, pos, n_vec, first = 0, 0, 0, True
    while n_taken < R and pos < len(src):
        rest = len(src) - pos
        if rest <= 64:
            ln = rest
        elif src[pos + 64][1] != src[pos + 63][1]:
            ln = 64
        else:
            ln = next(j for j in range(64) if src[pos + j][1] == src[pos + 63][1])
        assert 0 < ln <= 64 and (rest <= 64 or ln > 48)
        vec = wave_sort_records_desc([rec for rec, _ in src[pos:pos + ln]])
        for (_, r, s) in vec:  # (the fixed-point iteration of rs_scan_decide_records is this scan on one vector)
            if owner[r] < 0 and left[s] > 0:
                owner[r] = s
                left[s] -= 1
                n_taken += 1
        n_vec += 1
        pos += ln
        if n_taken < R and len(src) - pos > 64:
            src = [(rec, f) for rec, f in src[pos:] if owner[rec[1]] < 0 and left[rec[2]] > 0]
            pos = 0
            if stats is not None and first:
                stats["live_after_first"] = len(src)
        first = False
    if stats is not None:
        stats["vectors"] = n_vec
    return owner


def quotas_for(rng, R, S, tries):
    """quota vectors: the quota step's usual spread, and skewed ones -- one or two slices hold nearly all of it, the others 0, 1 or
    negative -- which keep many records live behind the first vector"""
    for t in range(tries):
        if t % 3 == 0:
            yield rng.multinomial(R, np.ones(S) / S).astype(np.int64)
        else:
            q = rng.integers(-2, 2, S).astype(np.int64)
            heavy = rng.choice(S, size=min(S, 1 + t % 2), replace=False)
            q[heavy] = R
            yield q


def check_array(keys, ids, seg, rng, tries):
    N = len(keys)
    R, S = SHAPES[N]
    arr = [(int(keys[i]), int(i) // S, int(i) % S) for i in ids]  # array index rbg * S + slice
    final = sorted(arr, key=lambda rec: -rec[0])  # the final insertion sort: stable by descending key
    # the sub-ranges are ordered against each other and at most 16 long unless heap-sorted
    starts = sorted(set(int(f) for f in seg))
    max_from = np.maximum.accumulate(np.array([k for (k, _, _) in arr] + [0])[::-1])[::-1]
    for a, b in zip(starts, starts[1:] + [N]):
        assert b - a <= 16 and all(int(f) == a for f in seg[a:b])
        assert min(k for (k, _, _) in arr[a:b]) >= max_from[b]
    deep = 0
    for quota in quotas_for(rng, R, S, tries):
        stats = {}
        want = greedy_serial(final, R, quota)
        got = greedy_segments(arr, seg, R, quota, stats)
        assert (got == want).all(), (N, quota.tolist())
        deep += stats.get("live_after_first", 0) > 64
    return deep


def test_sort_killer_arrays(loop):
    d = np.load(GOLDEN / "sort_killers.npz")
    meta = json.loads(bytes(d["meta"]).decode())
    names = [k for k in meta if len(d[k]) in SHAPES]
    assert {"n500_wg", "n500_wave", "n1280_wg"} <= set(names)
    rng = np.random.default_rng(11)
    res = loop([d[k] for k in names])
    long_runs = 0
    for name, (ids, seg) in zip(names, res):
        # a heap-sorted range: a run of positions that are their own sub-range
        own = seg == np.arange(len(seg))
        run = best = 0
        for o in own:
            run = run + 1 if o else 0
            best = max(best, run)
        assert best > 16, name
        long_runs += best > 64
        check_array(d[name], ids, seg, rng, 40)
    assert long_runs > 0  # heap-sorted runs longer than a vector


def test_random_arrays_and_quotas_that_keep_more_than_a_vector_live(loop):
    rng = np.random.default_rng(5)
    arrays = []
    for N in (17, 64, 65, 80, 500, 1024):
        for classes in (1, 2, 16):
            for rep in range(3):
                arrays.append(rng.integers(16 - classes, 16, N) if rep else rng.integers(0, classes, N))
    res = loop(arrays)
    deep = {}
    for keys, (ids, seg) in zip(arrays, res):
        deep[len(keys)] = deep.get(len(keys), 0) + check_array(keys, ids, seg, rng, 60)
    # inputs that leave more than 64 live records behind the first vector exist in the set (several vectors, cuts inside the survivors)
    assert deep[500] > 0 and deep[1024] > 0, deep


def test_wave_rank_is_the_stable_sort():
    rng = np.random.default_rng(2)
    for _ in range(200):
        n = int(rng.integers(1, 65))
        keys = rng.integers(0, int(rng.integers(1, 17)), n).tolist()
        valid = (rng.random(n) < 0.8).tolist()
        ranks = wave_stable_rank_desc(keys, valid)
        before = wave_stable_before_desc(keys, valid)
        order = sorted([i for i in range(n) if valid[i]], key=lambda i: -keys[i])
        assert [ranks[i] for i in order] == list(range(len(order)))
        for pos, i in enumerate(order):  # the lanes before lane i are exactly the ones the stable sort puts before it
            assert before[i] == sum(1 << j for j in order[:pos])
