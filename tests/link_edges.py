"""Directed edge inputs for the step after the allocation -- the EESM sum over a user's PRBs, the final CQI, the MCS and the transport
block -- and a plain exact model of it.

Nothing here imports the kernels or the oracle; the tables are arguments (`Tables`): E from rs.link_tables(pinned=...) of the surface
under test, everything else from oracle.tables().  tests/test_abi.py::test_link_tables_of_the_gpu_box_match_reference_known_answers
requires the libm of the box to be the pinned glibc 2.35 one, so math.log / math.log10 below are the reference's log / log10; the
model relies on that.  It uses Python floats (IEEE doubles, one rounding per operation), no numpy reductions:

  * plain_final_cqi (downlink-transport-scheduler.cpp:638-650, eesm-effective-sinr.h:33-46, AMCModule.cpp:253-261): ONE addition per
    PRB in PRB order, one division by the PRB count; a mean of exactly 0 gives 15 (log(0) = -inf, log10 of +inf passes every table
    entry); else -log, 10 * log10 and the count of table SINRs at or below the result ('<=').  This is the reference's expression in
    dB, deliberately not the kernels' comparison of the mean with 13 precomputed thresholds.
  * plain_tbs_bits (AMCModule.cpp:306-317): T[n - 1][itbs] up to 110 PRBs, beyond 5 * T[n / 5 - 1][itbs] + T[n % 5 - 1][itbs], where
    the row T[-1] of the as-shipped -O0 build is McsToItbs[5 + itbs] up to iTBS 23 and 0 above.
  * plain_flows (downlink-packet-scheduler.cpp:179-331): scheduler 1's loop over the RBGs with the break `tbs >= data * 8` after
    every RBG a flow takes.

What the families aim at.  A two-CQI search (c < d <= 11, up to 24 RBGs of each, G in {1, 4, 8}, ascending against descending,
31 680 users per G) found no user whose final CQI depends on the ORDER of its RBGs.  What is observable is the NUMBER and SEQUENCE
of the additions and the division, and it shows at users who hold several RBGs of one CQI: sum / n then lies within an ulp or two
of E[c], and E[c] within an ulp of the threshold between c and c - 1.  `alternatives` restates four evaluations a kernel could be
tempted by (n * E / n, E alone, per-RBG partial sums, pairwise); tests/test_link_edge_inputs.py counts the uniform users on which
each gives another final CQI.

Shapes (R x G), the smallest at which each code path of the kernels exists: A 25 x 4 (the headline grid; 32-bit lane masks in
run-time builds), B 64 x 8 (512 PRBs: 64-bit masks, lanes >= 32, blocks beyond 110 PRBs, k * G meets every n of the recorded round
trip), C 32 x 3 (the largest R on 32-bit masks, an odd G), D 33 x 2 (the first R beyond them).

How a call steers who holds what.
  * `map` calls (schedulers 1 and 7, one slice): every user reports the wanted CQI on the RBGs it is to hold and CQI 1 elsewhere, all
    averages equal, so the owner's metric is the strict maximum on its RBGs.  A user who is to hold an RBG of CQI 1 gets an average
    1.5 times smaller (eff(2) = 2 eff(1)): it wins its own RBGs and nobody else's; a call has at most one such user.  An idle user
    (CQI 1 everywhere, an average a thousand times larger) pads every call of a shape to one user count; a filler takes what no case
    wants.
  * `flows` calls (scheduler 1): rows uniform over the band, averages 64 times apart so that the flows take the band one after the
    other, each until `tbs >= data * 8`.
  * `gate` calls (scheduler 7): the same with required_rbs instead of data: every user takes exactly its k RBGs.
  * `slices` calls (schedulers 8, 9, 10, 101, 103): one user per slice with a uniform row, equal weights and slice offsets chosen so
    that the quotas are the wanted RBG counts (quota_edges.plain_quotas confirms it); whichever RBGs the inter-slice step hands a
    slice, its user holds k RBGs of CQI c.
  * `wide_population` (scheduler 7, queue model): rows of one CQI whose wideband CQI over all R * G PRBs is another, and first-bearer
    data for which m_requiredRBs then allows another number of RBGs.

Found by these tests: no difference between the kernels, the oracle, this model and the recorded values."""
import math
from dataclasses import dataclass

import quota_edges as qe

SHAPES = {"A": (25, 4), "B": (64, 8), "C": (32, 3), "D": (33, 2)}
FAMILIES = ("uniform", "zero", "mixed", "prb", "tbs", "flow_break", "shrinking_block", "slices")
BACKLOG = 100000000
MIN_NORMAL = 2.2250738585072014e-308
BASE_AVG = 98000.0
TRANSPORT = qe.TRANSPORT
TRANSPORT_K = {"A": (1, 2, 3, 4, 5, 8, 9, 25), "B": (1, 2, 3, 4, 5, 8, 9, 16, 32, 33, 64), "C": (1, 2, 3, 4, 5, 8, 9, 32),
               "D": (1, 2, 3, 4, 5, 8, 9, 33)}


# ---------------------------------------------------------------------------------------------------------------------------
# the plain model
# ---------------------------------------------------------------------------------------------------------------------------

@dataclass
class Tables:
    E: list              # [16] exp(-10^(sinr/10)) by CQI (index 0 unused)
    sinr: list           # [15] table SINR of CQI i + 1
    eff: list            # [16] spectral efficiency by CQI
    tbs: list            # [110][27]
    mcs_to_itbs: list    # [29]
    cqi_to_mcs: list     # [15]


def make_tables(link, otab):
    """link: rs.link_tables(pinned=...); otab: oracle.tables()"""
    return Tables([float(x) for x in link["eesm_e"]], [float(x) for x in otab["sinr_for_cqi"]], [float(x) for x in link["eff"]],
                  [[int(x) for x in row] for row in otab["tbs"]], [int(x) for x in otab["mcs_to_itbs"]], [int(x) for x in otab["cqi_to_mcs"]])


def cqi_from_mean(sinr, x):
    if x == 0:
        return 15
    db = 10 * math.log10(-math.log(x))
    cqi = 1
    while cqi <= 14 and sinr[cqi] <= db:
        cqi += 1
    return cqi


def plain_mean(E, cqi_per_prb):
    s = 0.0
    for c in cqi_per_prb:
        s = s + E[c]
    return s / len(cqi_per_prb)


def plain_final_cqi(E, sinr, cqi_per_prb):
    return cqi_from_mean(sinr, plain_mean(E, cqi_per_prb))


def plain_tbs_bits(t, fcqi, nprb):
    itbs = t.mcs_to_itbs[t.cqi_to_mcs[fcqi - 1]]
    if nprb <= 110:
        return t.tbs[nprb - 1][itbs]
    sub, rest = nprb // 5, nprb % 5
    tail = t.tbs[rest - 1][itbs] if rest else (t.mcs_to_itbs[5 + itbs] if itbs <= 23 else 0)
    return 5 * t.tbs[sub - 1][itbs] + tail


def plain_prbs(G, rbgs, row, per_prb=False):
    """the CQIs of a user's PRBs in PRB order: row is its [R] per-RBG or [R * G] per-PRB report"""
    out = []
    for r in sorted(rbgs):
        out += list(row[r * G:(r + 1) * G]) if per_prb else [row[r]] * G
    return [int(c) for c in out]


def plain_block(t, G, rbgs, row, per_prb=False):
    """(nprb, final CQI, MCS, TBS bits) of a user holding `rbgs`; all 0 for a user holding none"""
    prbs = plain_prbs(G, rbgs, row, per_prb)
    if not prbs:
        return (0, 0, 0, 0)
    fc = plain_final_cqi(t.E, t.sinr, prbs)
    return (len(prbs), fc, t.cqi_to_mcs[fc - 1], plain_tbs_bits(t, fc, len(prbs)))


def holdings(n, rbg_to_user, upper_rbg=None):
    """the RBGs of every call position, ascending, from a map of call positions -- or, for the upper-bound scheduler (several slices
    may take one RBG: the map cannot say it), from its per-slice lists, one user per slice"""
    if upper_rbg is not None:
        return [sorted(int(r) for r in row if r >= 0) for row in upper_rbg]
    held = [[] for _ in range(n)]
    for r, u in enumerate(rbg_to_user):
        if u >= 0:
            held[u].append(r)
    return held


def plain_blocks(t, G, held, rows, per_prb=False):
    """[n][4] for every row (call position) from the RBG lists of `holdings`"""
    return [list(plain_block(t, G, held[u], rows[u], per_prb)) for u in range(len(rows))]


_blocks = {}


def uniform_tbs(t, G, c, k):
    key = (t.E[1], t.E[14], G, c, k)
    if key not in _blocks:
        fc = plain_final_cqi(t.E, t.sinr, [c] * (k * G))
        _blocks[key] = plain_tbs_bits(t, fc, k * G)
    return _blocks[key]


def plain_flows(t, R, G, cqi, avg, data):
    """Scheduler 1 with the data gate: the RBG map (flow indices, -1 = nobody)"""
    n = len(cqi)
    done, held, out = [False] * n, [[] for _ in range(n)], []
    for r in range(R):
        best, pick = 0.0, -1
        for i in range(n):
            metric = (t.eff[cqi[i][r]] * 180000.) / avg[i]
            if metric > best and not done[i]:
                best, pick = metric, i
        out.append(pick)
        if pick < 0:
            continue
        held[pick].append(r)
        if plain_block(t, G, held[pick], cqi[pick])[3] >= data[pick] * 8:
            done[pick] = True
    return out


def alternatives(t, G, c, k):
    """the final CQI of k RBGs of CQI c under four other evaluations of the mean: {name: final CQI}"""
    n, e = k * G, t.E[c]
    per = 0.0
    for _ in range(G):
        per = per + e
    by_rbg = 0.0
    for _ in range(k):
        by_rbg = by_rbg + per
    level = [e] * n
    while len(level) > 1:
        level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    means = {"n*E/n": (n * e) / n, "E alone": e, "per-RBG partial sums": by_rbg / n, "pairwise": level[0] / n}
    return {name: cqi_from_mean(t.sinr, x) for name, x in means.items()}


def unreachable(t, R, G):
    """the (c, k) no data gate stops at: a block no larger than an earlier one of the same flow"""
    out = set()
    for c in range(1, 16):
        top = -1
        for k in range(1, R + 1):
            b = uniform_tbs(t, G, c, k)
            if b <= top:
                out.add((c, k))
            top = max(top, b)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------------------------------------------------------

@dataclass
class User:
    family: str
    held: dict                 # RBG -> CQI: what the user is to hold (map calls)
    c: int = 0                 # uniform / flows / slices: the one CQI
    k: int = 0                 # ... and the RBG count wanted
    tag: str = ""
    data: int = BACKLOG        # flows: data_to_transmit
    side: str = ""             # flow_break: "stops" / "goes on"
    takes: int = 0             # flows: the RBGs the flow takes with the band to itself


@dataclass
class Call:
    shape: str
    kind: str                  # map / flows / gate / slices
    users: list
    cqi: list = None           # [n][R]
    avg: list = None           # [n]
    data: list = None          # flows: data_to_transmit [n]; gate: required_rbs [n]
    cqi_prb: list = None       # [n][R * G] (per-PRB variants of a map or flows call)
    w: list = None             # slices
    offset: list = None        # slices
    name: str = ""

    @property
    def R(self):
        return SHAPES[self.shape][0]

    @property
    def G(self):
        return SHAPES[self.shape][1]

    @property
    def n(self):
        return len(self.users)

    @property
    def per_prb(self):
        return self.cqi_prb is not None

    def rows(self):
        return self.cqi_prb if self.per_prb else self.cqi


MAP_USERS = 8     # every map call and every flows call has this many users (idle ones pad it): one context serves a shape


def _map_call(shape, users, name):
    R, G = SHAPES[shape]
    users = list(users)
    owner = {}
    for u in users:
        for r in u.held:
            assert 0 <= r < R and r not in owner, f"{name}: RBG {r} wanted twice"
            owner[r] = u
    rest = [r for r in range(R) if r not in owner]
    if rest:
        users.append(User("filler", {r: 7 for r in rest}, tag="filler"))
    assert len(users) <= MAP_USERS, f"{name}: {len(users)} users"
    while len(users) < MAP_USERS:
        users.append(User("idle", {}, tag="idle"))
    low = [u for u in users if 1 in u.held.values()]
    assert len(low) <= 1, f"{name}: two users are to hold an RBG of CQI 1"
    cqi = [[u.held.get(r, 1) for r in range(R)] for u in users]
    avg = [BASE_AVG * 1000 if u.family == "idle" else (BASE_AVG / 1.5 if u in low else BASE_AVG) for u in users]
    return Call(shape, "map", users, cqi, avg, name=name)


def _positions(R, layout):
    """the order in which a call's users take the RBGs: 0 blocks from RBG 0 up, 1 a stride through the band (nobody's RBGs are
    contiguous; on 64 and 33 RBGs every larger user has lanes on both sides of 31/32), 2 blocks from the top down"""
    if layout == 0:
        return list(range(R))
    if layout == 2:
        return list(range(R - 1, -1, -1))
    s = next(s for s in (3, 5, 7) if math.gcd(s, R) == 1)
    return [(p * s) % R for p in range(R)]


def partitions(R):
    """RBG counts that sum to R, every k in 1 .. R among them; the first puts a user of 1 RBG beside users of 2, 3, 4, 5 and 9"""
    first = [1, 2, 3, 4, 5, 9]
    left = R - sum(first)
    out = [first + ([left] if left else [])]
    seen = set(out[0])
    for k in range(1, R + 1):
        if k in seen:
            continue
        out.append([k, R - k] if k < R else [k])
        seen |= set(out[-1])
    assert seen >= set(range(1, R + 1))
    return out


def uniform_calls(shape):
    R, G = SHAPES[shape]
    out = []
    for pi, part in enumerate(partitions(R)):
        for t in range(15):
            layout = (pi + t) % 3
            pos = _positions(R, layout)
            users, at = [], 0
            for j, k in enumerate(part):
                c = 1 + (t + 2 * j) % 15
                users.append(User("uniform", {r: c for r in pos[at:at + k]}, c=c, k=k, tag=f"layout {layout}"))
                at += k
            out.append(_map_call(shape, users, f"uniform {shape} {part} rotation {t} layout {layout}"))
    return out


def zero_calls(shape):
    R, G = SHAPES[shape]
    out = []

    def user(cqis, tag):
        return User("zero", dict(cqis), tag=tag)

    # CQI 15 alone: the mean is exactly 0
    for layout in (0, 1):
        pos = _positions(R, layout)
        users, at = [], 0
        for k in (1, 2, 3, 5, 9):
            users.append(user([(r, 15) for r in pos[at:at + k]], f"15 x {k}"))
            at += k
        out.append(_map_call(shape, users, f"zero {shape} all 15 layout {layout}"))
    whole = _positions(R, 0)
    out.append(_map_call(shape, [user([(r, 15) for r in whole], f"15 x {R}")], f"zero {shape} all 15 whole band"))
    # one or two RBGs of CQI 14 (E = 1.8e-307) among RBGs of CQI 15: the mean is subnormal from 9 times as many PRBs; the same beside
    # an RBG of CQI 13
    for n14 in (1, 2):
        for with13 in (False, True):
            for where in ("lowest", "highest"):
                for k in sorted({3, 9, 10, 17, 18, R} - set(range(R + 1, 99))):
                    if k <= n14 + int(with13):
                        continue
                    for layout in ((0, 1) if k < R else (0,)):
                        mine = sorted(_positions(R, layout)[:k])
                        special = mine[:n14 + int(with13)] if where == "lowest" else mine[-(n14 + int(with13)):]
                        held = {r: 15 for r in mine}
                        for i, r in enumerate(special if where == "lowest" else special[::-1]):
                            held[r] = 14 if i < n14 else 13
                        tag = f"14 x {n14}{' + 13' if with13 else ''} {where} of {k}"
                        out.append(_map_call(shape, [user(held.items(), tag)], f"zero {shape} {tag} layout {layout}"))
    return out


def mixed_calls(shape):
    R, G = SHAPES[shape]
    specs = []
    for c in range(1, 16):
        near = c + 1 if c < 15 else 14
        far = 1 + (c + 6) % 15
        far = 2 if far == 1 else far
        for k in (1, 2, 3, 4, 7):
            for other, kind in ((near, "neighbour"), (far, "distant")):
                for where in ("lowest", "highest"):
                    for extra in (1, 2):
                        if k + extra <= R:
                            specs.append((c, k, other, kind, where, extra))
    out, users, at, n = [], [], 0, 0

    def flush():
        nonlocal users, at, n
        if users:
            out.append(_map_call(shape, users, f"mixed {shape} call {n}"))
            n += 1
        users, at = [], 0

    for c, k, other, kind, where, extra in specs:
        size = k + extra
        low = 1 in (c, other)      # (a call holds at most one user with an RBG of CQI 1)
        if at + size > R or len(users) == MAP_USERS - 1 or (low and any(1 in u.held.values() for u in users)):
            flush()
        layout = n % 2      # blocks, or a stride through the band
        pos = _positions(R, layout)
        mine = sorted(pos[at:at + size])
        special = mine[:extra] if where == "lowest" else mine[-extra:]
        users.append(User("mixed", {r: (other if r in special else c) for r in mine}, c=c, k=k,
                          tag=f"{k} x {c} + {extra} x {other} ({kind}, {where})"))
        at += size
    flush()
    return out


def prb_variant(call, noise):
    """the call through the per-PRB path: every RBG's report repeated, or (noise) the PRBs behind the first of every RBG moved to a
    neighbouring CQI by a fixed pattern; the metric reads the first PRB of an RBG, the link adaptation all of them"""
    R, G = call.R, call.G
    prb = []
    for i, row in enumerate(call.cqi):
        out = []
        for r in range(R):
            for j in range(G):
                c = row[r]
                if noise and j > 0:
                    c = min(15, max(1, c + (r + 2 * j + i) % 3 - 1))
                out.append(c)
        prb.append(out)
    users = [User("prb" if noise and u.family not in ("idle", "filler") else u.family, u.held, u.c, u.k, u.tag, u.data, u.side, u.takes)
             for u in call.users]
    name = call.name + (" per-PRB noise" if noise else " per-PRB")
    return Call(call.shape, call.kind, users, call.cqi, call.avg, call.data, prb, name=name)


def single_prb_calls(shape):
    """per-PRB only: ONE PRB of CQI 14 among PRBs of CQI 15 -- the mean is subnormal from 9 PRBs"""
    R, G = SHAPES[shape]
    out = []
    for k in sorted({(8 + G) // G, 5, 9, R}):
        for at in (1 % G, k * G - 1):       # not the first PRB of the first RBG, the last PRB
            base = _map_call(shape, [User("prb", {r: 15 for r in range(k)}, tag=f"one PRB of 14 among {k * G}")],
                             f"prb {shape} one PRB of CQI 14 at {at} of {k * G}")
            v = prb_variant(base, False)
            v.cqi_prb[0][at] = 14
            v.name = base.name
            out.append(v)
    return out


def flow_calls(shape, t):
    """flow_break: for every reachable (c, k) a flow whose data is the k-RBG block's bytes (it stops at the k-th RBG, on the == side
    where the block is a multiple of 8) and one with a byte more (it goes on); shrinking_block: for every unreachable (c, k) a flow
    with a byte more than the largest earlier block -- the k-th RBG's block is no larger, the flow must go on past it"""
    R, G = SHAPES[shape]
    bad = unreachable(t, R, G)
    flows = []
    for c in range(1, 16):
        top = 0
        for k in range(1, R + 1):
            b = uniform_tbs(t, G, c, k)
            if (c, k) in bad:
                flows.append(User("shrinking_block", {}, c=c, k=k, data=top // 8 + 1, side="goes on"))
            else:
                flows.append(User("flow_break", {}, c=c, k=k, data=b // 8, side="stops"))
                flows.append(User("flow_break", {}, c=c, k=k, data=b // 8 + 1, side="goes on"))
            top = max(top, b)
    # how many RBGs each takes when it has the band to itself
    for f in flows:
        f.takes = next((k for k in range(1, R + 1) if uniform_tbs(t, G, f.c, k) >= f.data * 8), R)
    # pack: large ones with small ones, at most 6 flows a call, the band never exhausted before the last flow is done
    flows.sort(key=lambda f: -f.takes)
    out, lo, hi = [], 0, len(flows) - 1
    while lo <= hi:
        group, room = [flows[lo]], R - flows[lo].takes
        lo += 1
        while lo <= hi and len(group) < 6 and flows[hi].takes <= room:
            group.append(flows[hi])
            room -= flows[hi].takes
            hi -= 1
        if len(out) % 2:
            group.reverse()
        while len(group) < MAP_USERS:       # idle flows behind the others: CQI 1, backlogged, the first of them takes what the cases leave
            group.append(User("idle", {}, c=1, tag="idle"))
        out.append(Call(shape, "flows", group, [[f.c] * R for f in group], [1000.0 * 64.0 ** i for i in range(len(group))],
                        [f.data for f in group], name=f"flows {shape} call {len(out)}"))
    return out


def gate_calls(shape):
    """Scheduler 7 with the m_requiredRBs gate as an input: rows uniform over the band, averages 64 times apart, required_rbs between
    (k - 1) G + 1 and k G (both ends, by turns) -- the users take k RBGs one after the other, every (c, k) exactly"""
    R, G = SHAPES[shape]
    out = []
    for pi, part in enumerate(partitions(R)):
        for t in range(15):
            users = [User("uniform", {}, c=1 + (t + 2 * j) % 15, k=k, tag="gate") for j, k in enumerate(part)]
            need = [(k - 1) * G + 1 if (pi + t + j) % 2 else k * G for j, k in enumerate(part)]
            while len(users) < MAP_USERS:
                users.append(User("idle", {}, c=1, tag="idle"))
                need.append(0)
            out.append(Call(shape, "gate", users, [[u.c] * R for u in users], [1000.0 * 64.0 ** i for i in range(len(users))], need,
                            name=f"gate {shape} {part} rotation {t}"))
    return out


def slice_partitions(shape):
    """quota vectors of one length per shape (zeros pad them) that hold every k of TRANSPORT_K"""
    R = SHAPES[shape][0]
    parts = {"A": [[1, 1, 2, 3, 4, 5, 9], [8, 8, 9], [25]],
             "B": [[1, 2, 3, 4, 5, 8, 9, 32], [16, 33, 15], [64], [1, 1, 2, 3, 4, 5, 9, 39]],
             "C": [[1, 2, 3, 4, 5, 8, 9], [32], [9, 1, 5, 17]],
             "D": [[1, 1, 2, 3, 4, 5, 8, 9], [33], [2, 9, 22]]}[shape]
    S = max(len(p) for p in parts)
    assert all(sum(p) == R for p in parts)
    return [p + [0] * (S - len(p)) for p in parts]


def slice_calls(shape):
    R, G = SHAPES[shape]
    out = []
    for part in slice_partitions(shape):
        S = len(part)
        w = [1.0 / S] * S
        offset = [k * G - (R * G) * w[s] + 0.5 for s, k in enumerate(part)]
        target, quota = qe.plain_quotas(R * G, G, w, offset, [True] * S, 0, 0)
        assert quota == part and target == [k * G for k in part], f"{shape} {part}: the offsets do not give the quotas"
        for t in range(15):
            users = [User("slices", {}, c=1 + (t + 2 * s) % 15, k=k) for s, k in enumerate(part)]
            avg = [BASE_AVG + 1000.0 * ((s * 7 + t) % 5) for s in range(S)]
            out.append(Call(shape, "slices", users, [[u.c] * R for u in users], avg, w=w, offset=offset,
                            name=f"slices {shape} {part} rotation {t}"))
    return out


def wide_population(t, shape, t0):
    """Scheduler 7 with the queue model: a queue_edges.Population of one slice of two users ('Q-' and 'B-', one CQI c over the band,
    equal averages: user 0 wins every race it is in) for every c whose wideband CQI over all R * G PRBs is not c, user 0's first
    bearer holding data for which m_requiredRBs (packet-scheduler.cpp:319-334: data * 8 / TBS(1 PRB, wideband CQI)) allows another
    number of RBGs than it would with CQI c; up to three such amounts per c, of different counts.  plan: per cell dict(c, wide,
    first, rbgs, rbgs_if_c)"""
    import numpy as np

    import queue_edges
    R, G = SHAPES[shape]
    tbs1 = lambda cqi: t.tbs[0][t.mcs_to_itbs[t.cqi_to_mcs[cqi - 1]]]     # noqa: E731
    cqis, bursts, plan = [], {}, []
    for c in range(1, 16):
        wide = plain_final_cqi(t.E, t.sinr, [c] * (R * G))
        if wide == c:
            continue
        counts = set()
        for first in range(16, 6000):
            k_wide, k_c = -(-((first * 8) // tbs1(wide)) // G), -(-((first * 8) // tbs1(c)) // G)
            if k_wide != k_c and 1 <= k_c and k_wide < R and k_wide not in counts:
                counts.add(k_wide)
                bursts[(len(cqis), 0, 0)] = queue_edges._burst_arrays([(t0, nf, la) for nf, la in queue_edges.shapes_for_data(first)])
                cqis.append([c, c])
                plan.append(dict(c=c, wide=wide, first=first, rbgs=k_wide, rbgs_if_c=k_c))
                if len(counts) == 3:
                    break
    return queue_edges.Population(f"wide-{shape}", 7, [2], R, G, ["Q-", "B-"], 3, np.array(cqis, np.uint8), bursts, plan=plan)


_cache = {}


def map_calls(shape):
    """uniform, zero and mixed, per-RBG reports"""
    if ("map", shape) not in _cache:
        _cache[("map", shape)] = uniform_calls(shape) + zero_calls(shape) + mixed_calls(shape)
    return _cache[("map", shape)]


def prb_calls(shape):
    """the uniform and zero calls through the per-PRB path, every third with reports that differ inside the RBGs, and the single-PRB
    users"""
    if ("prb", shape) not in _cache:
        base = uniform_calls(shape) + zero_calls(shape)
        _cache[("prb", shape)] = [prb_variant(c, i % 3 == 1) for i, c in enumerate(base)] + single_prb_calls(shape)
    return _cache[("prb", shape)]


def cached_flow_calls(shape, t):
    if ("flows", shape) not in _cache:
        _cache[("flows", shape)] = flow_calls(shape, t)
    return _cache[("flows", shape)]


def cached_gate_calls(shape):
    if ("gate", shape) not in _cache:
        _cache[("gate", shape)] = gate_calls(shape)
    return _cache[("gate", shape)]


def cached_slice_calls(shape):
    if ("slices", shape) not in _cache:
        _cache[("slices", shape)] = slice_calls(shape)
    return _cache[("slices", shape)]


def counts(calls):
    """cases per family; `tbs` counts, among them, the users who are to hold more than 110 PRBs"""
    n = {}
    for c in calls:
        for u in c.users:
            if u.family not in ("idle", "filler"):
                n[u.family] = n.get(u.family, 0) + 1
                if max(len(u.held), u.k, u.takes) * c.G > 110:
                    n["tbs"] = n.get("tbs", 0) + 1
    return n
