"""Near-tie populations for the two-stage arg-max and a plain numpy FP64 reference of the metric scan.

Nothing here imports the kernels or the oracle: the callers pass the 16 spectral efficiencies (index = CQI, 0 unused), everything else
is IEEE double arithmetic and fractions.Fraction.

The scan (`plain_argmax`): metric = num[cqi[u]] / den[u], one rounded double division; users ascending; strict '>' from the scheduler's
start value (-1 transport schedulers, 0 scheduler 1, lowest() scheduler 7).  Denominators (`den_of`): (1 + avg) / 1000.0 for schedulers
7, 8, 9, 10 (and 101, 103), avg itself for scheduler 1.  Numerators (`num_of`): eff * 180000 / 1000 and eff * 180000.

A population plants, per (slice, RBG) item, a tuple of users -- an anchor, who holds the item's largest exact metric, and one or more
challengers whose exact metrics lie a prescribed relative gap g = 1 - metric_challenger / metric_anchor below it (`solve`: the
challenger's denominator from the rational equation, rounded, then stepped ulp by ulp until the exact rational gap of the doubles lands
in the band).  The tuple's users report their own CQI class on that RBG only; on the other RBGs they report one class less (7 % or more
below) and another tuple meets.  The remaining users of the slice are the field: 2^-9 ... 2^-6 below the anchors on every RBG."""
import math
import re
from dataclasses import dataclass, field
from fractions import Fraction
from pathlib import Path

import numpy as np

# the structural constants come from the sources (read as text: nothing is imported from the kernels)
_CSRC = Path(__file__).resolve().parents[1] / "radiosaber_amd" / "csrc"
_KERNELS, _DEVICE_H = (_CSRC / "rs_kernels.hip").read_text(), (_CSRC / "rs_device.h").read_text()
P3_BLOCK = int(re.search(r"#define RS_P3_BLOCK (\d+)", _KERNELS).group(1))          # users per stage-1 block: 32
HOLD_MAX_AGE = int(re.search(r"#define RS_HOLD_MAX_AGE (\d+)", _KERNELS).group(1))  # 40
PF_SEG = int(re.search(r"#define RS_PF_SEG (\d+)", _DEVICE_H).group(1))             # 32
NVS_WHOLE_SLICE = int(re.search(r"#define RS_NVS_WHOLE_SLICE (\d+)", _DEVICE_H).group(1))  # 64
LOAD = 8   # users per stage-1 step (one 8-byte CQI load): blocks, windows and runs are aligned to it

START = {1: 0.0, 7: -np.finfo(np.float64).max}   # every other scheduler: -1.0
TRANSPORT = (7, 8, 9, 10, 101, 103)

# gap bands: name -> (lo, hi), g = 1 - metric_challenger / metric_anchor as an exact rational
BANDS = {"zero": (Fraction(0), Fraction(0)), "ulp": (Fraction(1, 2**54), Fraction(1, 2**51))}
for _b in (45, 35, 28, 24, 22, 21, 20, 19, 18, 12):
    BANDS[f"2^-{_b}"] = (Fraction(3, 4) * Fraction(1, 2**_b), Fraction(5, 4) * Fraction(1, 2**_b))
NEAR = [b for b in BANDS if b != "2^-12"]      # everything but the control
PLACEMENTS = ("same8", "same32", "next", "two")
BASE_AVGS = (1.0, 64.0, 1e3, 98000.0, 5e6, 2.0**50)  # (the last one's larger classes and field reach up to 2^51)


def start_of(sched):
    return START.get(sched, -1.0)


def num_of(eff, sched):
    """[16] numerators by CQI as the reference forms them (index 0: 0)."""
    e = np.asarray(eff, np.float64)
    return e * 180000. if sched == 1 else e * 180000 / 1000


def den_of(avg, sched):
    a = np.asarray(avg, np.float64)
    return a.copy() if sched == 1 else (1 + a) / 1000.0


def plain_argmax(num, den, cqi_row, lo, hi, start):
    """(winner or -1, its metric) of users lo..hi-1: the reference's loop, nothing else."""
    best, bu = start, -1
    for u in range(lo, hi):
        metric = num[cqi_row[u]] / den[u]
        if metric > best:
            best, bu = metric, u
    return bu, best


def exact_gap(num, den, ca, ua, cb, ub):
    """1 - metric_b / metric_a of the doubles, as a Fraction"""
    return 1 - (Fraction(float(num[cb])) / Fraction(float(den[ub]))) / (Fraction(float(num[ca])) / Fraction(float(den[ua])))


def stage1(num, den, ulp=0):
    """The kernels' stage-1 value fl32(num) * rcp32(fl32(den)) with the reciprocal `ulp` FP32 ulps off the rounded one (v_rcp_f32 is a
    1-ulp instruction) -- the emulation of tests/test_round4_models.py without its position bits."""
    r = (np.float32(1.0) / np.asarray(den).astype(np.float32)).astype(np.float32)
    if ulp:
        r = np.nextafter(r, np.float32(np.inf) if ulp > 0 else np.float32(-np.inf))
    return (np.asarray(num).astype(np.float32) * r).astype(np.float32)


def _step(x, k):
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


def solve(sched, num, avg_a, ca, cb, band, reach=400):
    """avg_b such that a user of CQI class cb with that average is `band` below a user of class ca with average avg_a.
    Returns (avg_b, achieved gap as a Fraction) or None when no double within `reach` ulps of the rounded solution lands in the band."""
    lo, hi = BANDS[band]
    t = (lo + hi) / 2
    den_a = Fraction(float(den_of(avg_a, sched)))
    want = den_a * Fraction(float(num[cb])) / Fraction(float(num[ca])) / (1 - t)
    a0 = float(want if sched == 1 else want * 1000 - 1)
    for i in range(2 * reach + 1):
        k = (i + 1) // 2 * (1 if i % 2 else -1)
        a = _step(a0, k)
        d = float(den_of(a, sched))
        g = 1 - (Fraction(float(num[cb])) / Fraction(d)) / (Fraction(float(num[ca])) / den_a)
        if lo <= g <= hi:
            return a, g
    return None


def classify(a, b, base):
    """Where user b sits relative to user a in blocks of RS_P3_BLOCK (32) users that start at `base` (the slice's 8-aligned start):
    one of PLACEMENTS (or 'far') and 'before' / 'after'.  The names count in the widest block: the speculating schedulers (8, 9,
    101, 103) rank 16 users per block, for them a 'same32' pair 16 or more apart already sits in neighbouring blocks."""
    ba, bb = (a - base) // P3_BLOCK, (b - base) // P3_BLOCK
    if ba == bb:
        kind = "same8" if (a - base) // LOAD == (b - base) // LOAD else "same32"
    else:
        kind = {1: "next", 2: "two"}.get(abs(ba - bb), "far")
    return kind, "before" if b < a else "after"


@dataclass
class Planted:
    slice: int
    rbg: int
    users: list          # anchor first
    classes: list
    bands: list          # per challenger
    gaps: list           # achieved, Fractions
    tags: set = field(default_factory=set)


@dataclass
class Population:
    name: str
    sched: int
    ues: list
    R: int
    cqi: np.ndarray      # [U][R]
    avg: np.ndarray      # [U]
    planted: list
    base: list           # per slice: the index the scan's blocks start from

    @property
    def first(self):
        return np.concatenate([[0], np.cumsum(self.ues)])


def build(name, sched, eff, ues, R, base_avg, seed, classes=(7, 8, 9, 10), forced=(), zero_pair=(4, 7), huge_user=False,
          positions_from_slice=False, control=False):
    """One population.  forced: [(slice, anchor, challenger, tag)] user pairs for the first RBGs of that slice.  positions_from_slice:
    blocks count from the slice's first user (scheduler 7's calls pass the served slice alone).  huge_user: the last field user of
    the largest slice gets avg = 1e300 (the call switches itself to the exact scan of every user).  control: every first challenger
    2^-12 below its anchor, far outside the filter's tolerance; every other population keeps to the bands of NEAR.  zero_pair: two
    CQI classes whose numerators' ratio is a power of two, for exact ties across classes (the anchor of such a tuple sits at half
    the base average; a base of 1.0 keeps to one class, so that no average falls below 1)."""
    if base_avg < 2.0:
        zero_pair = (classes[0], classes[0])
    rng = np.random.default_rng(seed)
    num = num_of(eff, sched)
    first = np.concatenate([[0], np.cumsum(ues)]).astype(int)
    U = int(first[-1])
    cqi = np.zeros((U, R), np.uint8)
    avg = np.zeros(U)
    c0 = classes[0]
    level = Fraction(float(num[c0])) / Fraction(float(den_of(base_avg, sched)))   # the anchors' metric, about

    def avg_at(c, below):  # an average that puts a class-c user `below` (relative) under the level; no band to hit
        den = Fraction(float(num[c])) / (level * (1 - Fraction(below)))
        return float(den if sched == 1 else den * 1000 - 1)

    planted, bases = [], []
    band_names = ["2^-12"] if control else NEAR
    for s, n in enumerate(ues):
        s0 = int(first[s])
        base = s0 if positions_from_slice else s0 & ~(LOAD - 1)
        bases.append(base)
        if n == 0:
            continue
        free = list(range(s0, s0 + n))
        tuples = []
        n_tuples = min(R, max(1, n // 3)) if n >= 2 else 0
        mine = [f for f in forced if f[0] == s]
        for t in range(n_tuples):
            tags = set()
            pair = None
            if t < len(mine):
                _, a, b, tag = mine[t]
                if a in free and b in free and a != b:
                    pair = (a, b)
                    tags.add(tag)
            if pair is None:
                # the rotation: placement kind and side by tuple number and seed; leader at the slice's first / last user twice
                want_kind = PLACEMENTS[(t + seed) % 4]
                want_side = ("before", "after")[((t + seed) // 4 + t) % 2]
                anchors = list(free)
                rng.shuffle(anchors)
                if t == len(mine) and s0 in free:
                    anchors = [s0] + anchors
                if t == len(mine) + 1 and s0 + n - 1 in free:
                    anchors = [s0 + n - 1] + anchors
                for relax in (0, 1, 2):
                    for a in anchors:
                        cands = [b for b in free if b != a and (relax == 2 or classify(a, b, base)[0] == want_kind)
                                 and (relax >= 1 or classify(a, b, base)[1] == want_side)]
                        if cands:
                            pair = (a, int(rng.choice(cands)))
                            break
                    if pair:
                        break
            a, b = pair
            free.remove(a)
            free.remove(b)
            users = [a, b]
            if t % 4 == 2 and len(free) >= 4:   # several challengers: two more, anywhere in the slice
                extra = [int(x) for x in rng.choice(free, 2, replace=False)]
                for x in extra:
                    free.remove(x)
                users += extra
                tags.add("several")
            tuples.append((users, tags))
        # averages and classes of the tuples
        for t, (users, tags) in enumerate(tuples):
            a = users[0]
            ca = classes[(t + s) % len(classes)]
            band0 = band_names[(t * 5 + s * 3 + seed) % len(band_names)]
            cls, bands, gaps = [ca], [], []
            if band0 == "zero" and t % 2 == 1:
                ca = zero_pair[0]
                cls = [ca]
            avg[a] = avg_at(ca, 0)
            for j, b in enumerate(users[1:]):
                if j == 0:
                    band = band0
                else:   # the further challengers: within FP32's resolution of the anchor, all different
                    band = ("2^-24", "2^-28", "2^-22", "2^-35")[(t + j) % 4]
                cb = ca if (t + j) % 2 == 0 else classes[(classes.index(ca) + 1 + j) % len(classes)] if ca in classes else ca
                if band == "zero" and t % 2 == 1:
                    cb = zero_pair[1]
                got = solve(sched, num, avg[a], ca, cb, band)
                if got is None and cb != ca:      # this pair of classes cannot reach the band: the same class can
                    cb = ca
                    got = solve(sched, num, avg[a], ca, cb, band)
                assert got is not None, (name, band, ca, cb, avg[a])
                avg[b], g = got
                cls.append(cb)
                bands.append(band)
                gaps.append(g)
                kind, side = classify(a, b, base)
                if j == 0:
                    tags |= {kind, side}
            if a == s0:
                tags.add("first")
            if a == s0 + n - 1:
                tags.add("last")
            if a % 8:
                tags.add("unaligned")
            if s0 % 8:
                tags.add("ragged")
            if len(set(cls)) > 1:
                tags.add("classes")
            for u, c in zip(users, cls):
                cqi[u, :] = c - 1          # one class less wherever another tuple meets
            for r in range(R):
                if r % len(tuples) == t:
                    for u, c in zip(users, cls):
                        cqi[u, r] = c
                    planted.append(Planted(s, r, list(users), cls, bands, gaps, set(tags)))
        # the field
        for i, u in enumerate(free):
            c = classes[int(rng.integers(0, len(classes)))]
            cqi[u, :] = c
            avg[u] = avg_at(c, 2.0 ** -rng.uniform(6, 9))
        if huge_user and n == max(ues) and free:
            avg[free[-1]] = 1e300
    planted.sort(key=lambda p: (p.slice, p.rbg))
    return Population(name, sched, list(ues), R, cqi, avg, planted, bases)


def items(pop, eff):
    """Every (slice, RBG) item of a population from the plain scan: dict(slice, rbg, winner, runner, gap) with gap the exact rational
    1 - metric_runner / metric_winner (runner: the best of the others, by exact rational metric; None in a slice of one user).
    Scheduler 1's item is the whole RBG: its scan knows no slices."""
    num, den = num_of(eff, pop.sched), den_of(pop.avg, pop.sched)
    first = pop.first
    spans = [(0, 0, int(first[-1]))] if pop.sched == 1 else [(s, int(first[s]), int(first[s + 1])) for s in range(len(pop.ues))]
    out = []
    for s, lo, hi in spans:
        if hi == lo:
            continue
        for r in range(pop.R):
            w, _ = plain_argmax(num, den, pop.cqi[:, r], lo, hi, start_of(pop.sched))
            exact = {u: Fraction(float(num[pop.cqi[u, r]])) / Fraction(float(den[u])) for u in range(lo, hi)}
            others = [u for u in range(lo, hi) if u != w]
            runner = max(others, key=lambda u: (exact[u], -u)) if others else None
            gap = None if runner is None else 1 - exact[runner] / exact[w]
            out.append(dict(slice=s, rbg=r, winner=w, runner=runner, gap=gap))
    return out


def winners(pop, eff, ids=None):
    """[S][R] (scheduler 1: [1][R]) plain-scan winners of a call that lists the users `ids` (None: all); -1 without a listed user."""
    num, den = num_of(eff, pop.sched), den_of(pop.avg, pop.sched)
    first = pop.first
    listed = np.ones(int(first[-1]), bool) if ids is None else np.isin(np.arange(int(first[-1])), ids)
    spans = [(0, int(first[-1]))] if pop.sched == 1 else [(int(first[s]), int(first[s + 1])) for s in range(len(pop.ues))]
    out = np.full((len(spans), pop.R), -1, np.int64)
    for s, (lo, hi) in enumerate(spans):
        for r in range(pop.R):
            best, bu = start_of(pop.sched), -1
            for u in range(lo, hi):
                if listed[u]:
                    metric = num[pop.cqi[u, r]] / den[u]
                    if metric > best:
                        best, bu = metric, u
            out[s, r] = bu
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the set the tests share
# ---------------------------------------------------------------------------------------------------------------------------

RAGGED = [3, 70, 0, 9, 14]      # slices start at users 0, 3, 73, 73, 82: unaligned
NVS_SPLIT = [6, 90]             # more than 32 users per slice on average: the built-in kernels scan the served slice in runs
R_OF = (8, 4, 25)


def transport_set(eff, sched=9):
    """One population per base average on the ragged slices (R cycles through 8, 4, 25) and the exact-scan case."""
    pops = []
    for i, a in enumerate(BASE_AVGS):
        forced = [(1, 3, 4, "first-slot"), (1, 72, 5, "last-slot")] if i % 2 else []
        pops.append(build(f"t{sched}-avg{a:g}", sched, eff, RAGGED, R_OF[i % 3], a, 40 + i, forced=forced))
    pops.append(build(f"t{sched}-exact-scan", sched, eff, RAGGED, 8, 98000.0, 50, huge_user=True))
    pops.append(build(f"t{sched}-control", sched, eff, RAGGED, 8, 98000.0, 51, control=True))
    return pops


def pf_set(eff):
    """Scheduler 1: 96 flows in one scan; pairs either side of the RS_PF_SEG boundaries at users 31/32 and 63/64, both orders."""
    pops = []
    for i, a in enumerate(BASE_AVGS):
        b1, b2 = PF_SEG, 2 * PF_SEG
        forced = [(0, b1 - 1, b1, "seg31|32"), (0, b2, b2 - 1, "seg63|64")] if i % 2 == 0 else [(0, b1, b1 - 1, "seg31|32"), (0, b2 - 1, b2, "seg63|64")]
        pops.append(build(f"pf-avg{a:g}", 1, eff, [96 - 7 * (i % 3)], R_OF[i % 3], a, 60 + i, forced=forced))
    pops.append(build("pf-exact-scan", 1, eff, [96], 8, 98000.0, 70, huge_user=True, forced=[(0, PF_SEG - 1, PF_SEG, "seg31|32")]))
    pops.append(build("pf-control", 1, eff, [96], 8, 98000.0, 71, control=True))
    return pops


def nvs_set(eff):
    """Scheduler 7, the served slice alone (positions count from its first user): slice 1 of NVS_SPLIT and slice 1 of RAGGED.  Drop-in
    and group contexts carve their LDS with the gate scratch (rs_carve's queue != 0 branch): the served slice is scanned UNSPLIT
    there whatever its size, so these populations hold no run boundary -- batches do (batch_set)."""
    pops = []
    for i, a in enumerate(BASE_AVGS):
        pops.append(build(f"nvs-avg{a:g}", 7, eff, NVS_SPLIT, R_OF[i % 3], a, 80 + i, positions_from_slice=True))
    pops.append(build("nvs-ragged", 7, eff, RAGGED, 8, 98000.0, 90, positions_from_slice=True))
    pops.append(build("nvs-exact-scan", 7, eff, NVS_SPLIT, 8, 1e3, 91, huge_user=True, positions_from_slice=True))
    pops.append(build("nvs-control", 7, eff, NVS_SPLIT, 8, 1e3, 92, control=True, positions_from_slice=True))
    return pops


GROUP_AVGS = (64.0, 98000.0, 5e6)
BATCH_UES = [3, 70, 9, 14]


def group_set(eff, sched):
    """Three populations of one shape (R = 8), one per cell of a group call: schedulers 9 (RAGGED), 1 (96 flows), 7 (NVS_SPLIT).
    Every average is at least 1 (what rs_group_set_avg accepts)."""
    ues = {1: [96], 7: NVS_SPLIT}.get(sched, RAGGED)
    forced = {1: [(0, PF_SEG - 1, PF_SEG, "seg31|32"), (0, 2 * PF_SEG, 2 * PF_SEG - 1, "seg63|64")]}.get(sched, [])
    pops = [build(f"group{sched}-avg{a:g}", sched, eff, ues, 8, a, 100 + 10 * sched + k, forced=forced, positions_from_slice=sched == 7,
                  zero_pair=(7, 7)) for k, a in enumerate(GROUP_AVGS)]
    assert all(p.avg.min() >= 1 for p in pops)
    return pops


def batch_window(ues):
    """the longest 8-aligned slice window of a batch (what rs_carve's NVS rule is keyed on for batches)"""
    first = np.concatenate([[0], np.cumsum(ues)]).astype(int)
    return max(((int(first[s + 1]) + LOAD - 1) & ~(LOAD - 1)) - (int(first[s]) & ~(LOAD - 1)) for s in range(len(ues)) if ues[s])


def batch_set(eff, sched):
    """Two populations (cells) for a batch: R = 8, no empty slice; scheduler 1: 96 flows.  Scheduler 7: slice 1's window of 80 users
    is longer than RS_NVS_WHOLE_SLICE, so built-in and run-time builds scan it in 8-aligned runs of 8, 16 or 32 users counted from
    the slice's aligned start (user 0 here): pairs sit either side of users 7|8 (runs of 8), 16|15 (8, 16) and 31|32 (any run)."""
    ues = [96] if sched == 1 else BATCH_UES
    forced = [(1, 7, 8, "run-boundary"), (1, 16, 15, "run-boundary"), (1, 31, 32, "run-boundary")] if sched == 7 else []
    return [build(f"batch{sched}-avg{a:g}", sched, eff, ues, 8, a, 200 + 10 * sched + k, forced=forced, zero_pair=(7, 7))
            for k, a in enumerate((1e3, 98000.0))]


# ---------------------------------------------------------------------------------------------------------------------------
# around the hold margin mu = 2^-18 + 2 / (1 + avg_w)
# ---------------------------------------------------------------------------------------------------------------------------

MARGIN_AVGS = (64.0, 65.0, 1e3, 1e5)
MARGIN_K = (0.5, 0.9, 1.0, 1.1, 2.0)
MARGIN_UES = [12, 12, 12, 12, 4]
MARGIN_WEIGHTS = [0.01, 0.01, 0.01, 0.01, 0.96]   # slices 0..3 receive an RBG every dozen TTIs: their winners starve, and decay


def mu_of(avg_w):
    return 2.0**-18 + 2.0 / (1.0 + avg_w)


def margin_population(eff, sched=9, R=8):
    """One cell.  Slice s < 4: winners with average MARGIN_AVGS[s] (CQI class 2), per RBG r a runner-up of class 15 whose exact
    metric is the winner's / (1 + k mu(avg_w)), k = MARGIN_K[r % 5] (the stage-1 gap is that within 2^-21); winner before the
    runner-up on even pairs, after it on odd ones.  On the other RBGs a pair reports one class less (15 % or more below); two
    field users per slice sit 10 % below.  The runner-up's larger average decays like the winner's while neither is served, and
    the '+1' of (1 + avg) / 1000 takes up to about mu from the winner's lead over RS_HOLD_MAX_AGE TTIs: the case mu is sized for.
    Slice 4 (4 users, weight 0.96) takes nearly every RBG.  planted[i].gaps holds k."""
    num = num_of(eff, sched)
    first = np.concatenate([[0], np.cumsum(MARGIN_UES)]).astype(int)
    U = int(first[-1])
    cqi = np.zeros((U, R), np.uint8)
    avg = np.zeros(U)
    planted = []
    cw, cv = 2, 15   # the widest ratio of numerators: the runner-up's average is 22 times the winner's, the decay costs the winner most
    for s, aw in enumerate(MARGIN_AVGS):
        s0 = int(first[s])
        den_w = Fraction(float(den_of(aw, sched)))
        for j, k in enumerate(MARGIN_K):
            w, v = (s0 + j, s0 + 5 + j) if j % 2 == 0 else (s0 + 5 + j, s0 + j)
            den_v = den_w * Fraction(float(num[cv])) / Fraction(float(num[cw])) * (1 + Fraction(k) * Fraction(mu_of(aw)))
            avg[w], avg[v] = aw, float(den_v * 1000 - 1)
            cqi[w, :], cqi[v, :] = cw - 1, cv - 1
            for r in range(R):
                if r % len(MARGIN_K) == j:
                    cqi[w, r], cqi[v, r] = cw, cv
                    planted.append(Planted(s, r, [w, v], [cw, cv], ["margin"], [k], {f"avg_w={aw:g}", f"k={k:g}"}))
        for u in (s0 + 10, s0 + 11):
            cqi[u, :] = cw
            avg[u] = (1 + aw) * 1.1 - 1
    s0 = int(first[4])
    cqi[s0:, :] = 8
    avg[s0:] = [9000.0, 11000.0, 13000.0, 15000.0]
    planted.sort(key=lambda p: (p.slice, p.rbg))
    return Population(f"margin{sched}", sched, list(MARGIN_UES), R, cqi, avg, planted, [int(f) & ~(LOAD - 1) for f in first[:-1]])


# ---------------------------------------------------------------------------------------------------------------------------
# scheduler 1's flows: a call position is one bearer of one user, position = 2 * user + bearer
# ---------------------------------------------------------------------------------------------------------------------------

FLOW_USERS = 40


def flows_population(eff, base_avg, seed):
    """(cqi [U][R], avg [U][2], population over the 2U flow positions).  A near-tie population of scheduler 1 over U users gives
    each user's CQI row and the average of ONE of its bearers; the other bearer sits 3 % below (a field flow) except where the
    user anchors a tuple: there the second bearer is a same-class challenger of its own, 2^-24 ... ulp below -- bearer 0 the
    anchor for even users, bearer 1 for odd ones (both orders).  Users PF_SEG / 2 - 1 and PF_SEG / 2 (and PF_SEG - 1, PF_SEG)
    are a forced pair whose flows sit at positions 31 | 32 (63 | 64): either side of the segment boundary."""
    h = PF_SEG // 2
    forced = [(0, h - 1, h, "seg31|32"), (0, 2 * h, 2 * h - 1, "seg63|64")]
    p = build(f"flows-avg{base_avg:g}", 1, eff, [FLOW_USERS], 8, base_avg, seed, forced=forced, zero_pair=(7, 7))
    num = num_of(eff, 1)
    U = FLOW_USERS
    avg2 = np.zeros((U, 2))
    own = np.zeros(U, int)   # the bearer that carries the population's average
    own[[h - 1, 2 * h - 1]] = 1   # positions 31 and 63; their partners (users h, 2h) keep bearer 0: positions 32 and 64
    anchors = {pl.users[0]: pl for pl in p.planted}
    bands = ("2^-24", "ulp", "zero", "2^-35", "2^-20")
    for u in range(U):
        if u in anchors and u not in (h - 1, h, 2 * h - 1, 2 * h):
            own[u] = u % 2
            c = anchors[u].classes[0]
            mate, _ = solve(1, num, p.avg[u], c, c, bands[u % len(bands)])
        else:
            mate = p.avg[u] * 1.03
        avg2[u, own[u]], avg2[u, 1 - own[u]] = p.avg[u], mate
    flows = Population(p.name, 1, [2 * U], p.R, np.repeat(p.cqi, 2, axis=0), avg2.reshape(-1), p.planted, [0])
    return p.cqi, avg2, flows
