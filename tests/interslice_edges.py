"""Directed edge inputs for the inter-slice policies (GreedyByRow, SubOpt, MaximizeCell, VogelApproximate, UpperBound) and a plain
exact model of each.

Nothing here imports the kernels or the oracle; the models use Python ints, lists and floats (IEEE doubles, one rounding per
operation).  They are written from the reference's lines (downlink-transport-scheduler.cpp:223-451), not from the oracle:

  * GreedyByRow (:249-272): quota_edges.plain_greedy_by_row, imported.
  * SubOpt (:274-349): negative quotas clamped to 0 in place; every RBG to its first maximum from -1; the `slice_more` and
    `slice_fewer` maps; the least loss by strict '<' over the RBGs ascending and, within an RBG, over `slice_fewer` in its ITERATION
    order; both erase conditions.  The iteration order is `umap_order`, a model of libstdc++'s unordered_map<int, int>: identity
    hash, the prime rehash policy (13 buckets from the first insertion, then 29, 59 and 127 when the 14th, 30th and 60th key
    arrives), a node put at the head of the whole list when its bucket is empty and in front of its bucket's nodes otherwise (a
    rehash re-inserts the nodes in their current order by the same rule), and erase leaving the order of the rest alone.
    tests/csrc/umap_order_dump.cpp prints the real container's order; tests/test_interslice_edge_inputs.py compares the two.
  * VogelApproximate (:378-451), literally: the sentinel -1 compared by value; `continue` after a new best, so `second` is the
    largest value that was NOT a new best when it was met (a new best never demotes the old one); `max_diff` an int assigned
    from a double (truncated) and compared with the next double difference; the horizontal candidates (free RBGs ascending), then
    the vertical ones (open slices ascending), every accepted candidate replacing the one before; the model stops where the
    reference would read a coordinate it never assigned.
  * MaximizeCell (:362-369): `plain_maximize_cell(order, quota)` is the scan over a given order of the R * S records.  With at most
    16 records std::sort is one insertion sort (the introsort loop does nothing at or below its threshold of 16, and the final
    insertion sort moves a record only past records that compare strictly below it), so the order is the plain stable descending
    sort, `stable_order`; above that the order is the reference's own std::sort call, which the tests take from
    rso_maximize_cell_order (pinned `_ref` in tests/PINS.md).
  * UpperBound (:223-246): per slice with a positive quota the first `quota` RBGs of the column sorted by descending key.  Up to
    16 RBGs the sort is stable by the same argument and `plain_upper_bound` is whole; for more RBGs `upper_bound_facts` yields what
    does not depend on the order of ties: the multiset of the taken keys and every RBG strictly above the cut key.

Efficiencies are (bits / 0.001) / 180000. of the one-PRB transport block of the CQI's MCS (AMCModule.cpp:320-327), from
tests/golden/amc_tables.npz; key 0 (a slice without a listed user) is 0.0.  Two pairs of CQIs are exactly 2.0 apart, (11, 1) and
(14, 8); every other difference is no integer (`integral_differences`).

The mutant models exist only to prove that a case binds; nothing compares a kernel with them.  Three things they cannot show, by
arithmetic and not by omission:
  * SubOpt with negative quotas NOT clamped yields the same map as the reference on every input: `more` starts larger by -quota,
    and the reference's second erase condition, slice_rbgs[from] <= 0, then fires exactly when the clamped count reaches 0.  A
    slice that owns nothing and has a negative quota stays in `more` for ever, offers no RBG, and the loop ends at the reference's
    assert instead of at the loop condition, with the same map.  (`subopt_unclamped` is checked to EQUAL the model on every case.)
  * With the clamp in place that second erase condition never fires before `more <= 0`: more = owned - quota <= owned.
  * Through a TTI two inputs of Vogel cannot occur, because the quota step gives a slice without a listed user the quota 0 and
    makes the quotas sum to R: the 1.0 of a lone EMPTY slice (0 - (-1)), and all slices closed before the RBGs run out (where the
    reference reads coordinates it never assigned).  `bare_cases` holds both for the bare policy functions; the second is compared
    device-free, oracle == model, both stopping.

Case planting.  Keys are planted with one user per slice (the slice's winner is that user, its key the user's CQI; a slice without
a listed user has key 0); the [3, 2, 4, 3] shape has several users per slice and its keys are read from the oracle's slice_eff.
Quotas are planted through slice offsets that make every target a multiple of the RBG size summing to nb_rbs, so that extra_rbs ==
extra_rbgs == 0 and the rands cannot matter; `_mk` asserts quota_edges.quota_steps(...)["quota"] == planted and the setters' domain.
Shapes come from SHAPES only: one batch, one context or one run-time build serves a whole shape."""
import sys
import zlib
from pathlib import Path

import numpy as np

import quota_edges as qe
from quota_edges import Case, by_config, plain_greedy_by_row   # noqa: F401  (re-exported for the tests)

FAMILIES = ("gbr", "subopt", "vogel", "scan", "upper")
MIN_CASES = {"gbr": 15, "subopt": 24, "vogel": 24, "scan": 24, "upper": 10}
SCHED_OF = {"gbr": 8, "subopt": 101, "vogel": 103, "scan": 9, "upper": 10}
MAX_CASES = 150

# users per slice, RBGs, RBG size
SHAPES = dict(T4=([1] * 4, 4, 4), A20=([1] * 20, 25, 4), S32=([1] * 32, 32, 2), S33=([1] * 33, 33, 2), S64=([1] * 64, 64, 2),
              E8=([0, 1, 1, 0, 1, 1], 8, 4), M=([3, 2, 4, 3], 25, 4),
              R8S2=([1, 1], 8, 4), R2S8=([1] * 8, 2, 4), R16S1=([1], 16, 4), R1S16=([1] * 16, 1, 4))
JIT_SHAPES = ("A20", "S32", "S33")      # 20 users on 25 RBGs, 32 on 32, 33 on 33: the shapes that get run-time builds


def _eff_table():
    d = np.load(Path(__file__).resolve().parent / "golden" / "amc_tables.npz")
    out = [0.0]
    for cqi in range(1, 16):
        bits = int(d["tbs"][0][int(d["mcs_to_itbs"][int(d["cqi_to_mcs"][cqi - 1])])])
        out.append((bits / 0.001) / 180000.)
    return out


EFF = _eff_table()


def eff_of(keys):
    return [[EFF[k] for k in row] for row in keys]


def key_of(e):
    """the CQI key of an efficiency (exact: the 16 values are distinct)"""
    return EFF.index(e)


def integral_differences():
    return sorted((a, b) for a in range(16) for b in range(16) if a > b and EFF[a] - EFF[b] == int(EFF[a] - EFF[b]))


# ---------------------------------------------------------------------------------------------------------------------------
# libstdc++'s unordered_map<int, int>
# ---------------------------------------------------------------------------------------------------------------------------

_FAST_BKT = [2, 2, 2, 3, 5, 5, 7, 7, 11, 11, 11, 11, 13, 13]
_PRIMES = [17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 103, 109, 113, 127, 137, 139, 149, 157, 167,
           179, 193, 199, 211, 227, 241, 257]


class UMap:
    """Keys only, in iteration order (`order`).  max_load_factor 1, growth factor 2, the first allocation at least 11 buckets."""

    def __init__(self):
        self.n_bkt, self.next_resize, self.order, self.rehashes = 1, 0, [], 0

    def _next_bkt(self, n):
        if n < len(_FAST_BKT):
            p = _FAST_BKT[n]
        else:
            p = next(q for q in _PRIMES if q >= n)
        self.next_resize = p
        return p

    @staticmethod
    def _place(order, key, n_bkt):
        b = key % n_bkt
        for i, k in enumerate(order):
            if k % n_bkt == b:
                order.insert(i, key)      # after the bucket's before-node: in front of the bucket's nodes
                return
        order.insert(0, key)              # an empty bucket: the head of the whole list

    def insert(self, key):
        assert key >= 0 and key not in self.order
        n = len(self.order) + 1
        if n > self.next_resize:
            min_bkts = max(n, 0 if self.next_resize else 11)
            if min_bkts >= self.n_bkt:
                new = self._next_bkt(max(min_bkts + 1, self.n_bkt * 2))
                old, self.order = self.order, []
                for k in old:
                    self._place(self.order, k, new)
                self.n_bkt = new
                self.rehashes += 1
            else:
                self.next_resize = self.n_bkt
        self._place(self.order, key, self.n_bkt)

    def erase(self, key):
        self.order.remove(key)


def umap_order(keys_inserted_ascending):
    m = UMap()
    for k in keys_inserted_ascending:
        m.insert(k)
    return list(m.order)


def umap_rehashes(n_keys):
    m = UMap()
    for k in range(n_keys):
        m.insert(k)
    return m.rehashes - 1      # (the first allocation is no rehash of anything)


# ---------------------------------------------------------------------------------------------------------------------------
# the plain models and their mutants
# ---------------------------------------------------------------------------------------------------------------------------

def gbr_last_maximum(keys, quota):
    """mutant: '>=' -- the last maximum wins"""
    S = len(quota)
    got, out = [0] * S, []
    for row in keys:
        best, pick = -1, -1
        for s in range(S):
            if row[s] >= best and got[s] < quota[s]:
                best, pick = row[s], s
        out.append(pick)
        if pick >= 0:
            got[pick] += 1
    return out


def gbr_stale_pair(keys, quota):
    """mutant: both RBGs of a pair decided under the quotas at the start of the pair"""
    S = len(quota)
    got, out = [0] * S, []
    for r0 in range(0, len(keys), 2):
        start = list(got)
        for row in keys[r0:r0 + 2]:
            best, pick = -1, -1
            for s in range(S):
                if row[s] > best and start[s] < quota[s]:
                    best, pick = row[s], s
            out.append(pick)
            if pick >= 0:
                got[pick] += 1
    return out


def plain_subopt(eff, quota, fewer_order=umap_order, clamp=True, trace=None):
    """eff [R][S] -> rbg_to_slice [R].  trace (a dict, optional) receives the keys of slice_fewer as inserted, the erasures in the
    order they happen (erased_at: after how many moves) and the number of moves."""
    R, S = len(eff), len(quota)
    quota = [max(q, 0) for q in quota] if clamp else list(quota)
    got, m = [0] * S, []
    for i in range(R):
        best, pick = -1, -1
        for j in range(S):
            if eff[i][j] > best:
                best, pick = eff[i][j], j
        m.append(pick)
        got[pick] += 1
    more, need, inserted = {}, {}, []
    for j in range(S):
        if got[j] > quota[j]:
            more[j] = got[j] - quota[j]
        elif got[j] < quota[j]:
            need[j] = quota[j] - got[j]
            inserted.append(j)
    fewer = fewer_order(inserted)
    erased, erased_at, moves = [], [], 0
    while more and fewer:
        frm, to, rbg, least = -1, -1, -1, sys.float_info.max
        for i in range(R):
            own = m[i]
            if own not in more:
                continue
            for f in fewer:
                loss = eff[i][own] - eff[i][f]
                if loss < least:
                    least, frm, to, rbg = loss, own, f, i
        if frm < 0:
            break                      # the reference asserts
        got[frm] -= 1
        got[to] += 1
        m[rbg] = to
        more[frm] -= 1
        need[to] -= 1
        moves += 1
        if more[frm] <= 0 or got[frm] <= 0:
            del more[frm]
        if need[to] <= 0:
            fewer.remove(to)
            erased.append(to)
            erased_at.append(moves)
    if trace is not None:
        trace.update(inserted=inserted, erased=erased, erased_at=erased_at, moves=moves)
    return m


def subopt_ascending(eff, quota):
    """mutant: equal losses go to the lowest slice"""
    return plain_subopt(eff, quota, fewer_order=lambda ks: sorted(ks))


def subopt_descending(eff, quota):
    """mutant: equal losses go to the highest slice (what the container yields while every key has a bucket of its own and nothing
    was rehashed: at most 13 keys below 13)"""
    return plain_subopt(eff, quota, fewer_order=lambda ks: sorted(ks, reverse=True))


def subopt_unclamped(eff, quota):
    """no mutant at all (module docstring): equal to the model on every input"""
    return plain_subopt(eff, quota, clamp=False)


def plain_vogel(eff, quota, double_max=False, classical=False, first_wins=False, vertical_first=False, ge=False, trace=None):
    """eff [R][S] -> (rbg_to_slice [R], stopped).  stopped: the reference would read a coordinate it never assigned; the RBGs left
    then stay -1.  trace (a list, optional) receives (iteration, 'h' | 'v', index, d, second is -1, max_diff before, accepted)."""
    R, S = len(eff), len(quota)
    got, m = [0] * S, [-1] * R

    def search(items):
        e1 = e2 = -1
        a1 = None
        for idx, v in items:
            if e1 == -1 or v > e1:
                if classical and e1 != -1:
                    e2 = e1
                a1, e1 = idx, v
                continue
            if e2 == -1 or v > e2:
                e2 = v
                continue
        return e1, e2, a1

    for it in range(R):
        state = dict(max_diff=-1, coord=None)

        def candidate(kind, index, e1, e2, coord):
            d = e1 - e2
            md = state["max_diff"]
            ok = (d >= md) if ge else (int(d) > md) if first_wins else (d > md)
            if trace is not None:
                trace.append((it, kind, index, d, e2 == -1, md, ok))
            if ok:
                state["max_diff"] = d if double_max else int(d)
                state["coord"] = coord

        def horizontal():
            for j in range(R):
                if m[j] != -1:
                    continue
                e1, e2, s1 = search((k, eff[j][k]) for k in range(S) if got[k] < quota[k])
                candidate("h", j, e1, e2, (j, s1))

        def vertical():
            for k in range(S):
                if got[k] >= quota[k]:
                    continue
                e1, e2, r1 = search((j, eff[j][k]) for j in range(R) if m[j] == -1)
                candidate("v", k, e1, e2, (r1, k))

        for step in ((vertical, horizontal) if vertical_first else (horizontal, vertical)):
            step()
        c = state["coord"]
        if c is None or c[0] is None or c[1] is None:
            return m, True
        m[c[0]] = c[1]
        got[c[1]] += 1
    return m, False


VOGEL_MUTANTS = dict(double_max=dict(double_max=True), classical=dict(classical=True), first_wins=dict(first_wins=True),
                     vertical_first=dict(vertical_first=True), ge=dict(ge=True))


def vogel_tags(trace):
    """what a run of plain_vogel met, from its trace"""
    tags = set()
    by_it = {}
    for ev in trace:
        by_it.setdefault(ev[0], []).append(ev)
    for evs in by_it.values():
        accepted = [e for e in evs if e[6]]
        for (_, kind, _, d, lone, md, ok) in evs:
            if d == 2.0 and md == 2:
                tags.add("2.0 after 2")
            if d == 1.0 and lone:
                tags.add("1.0 of a lone empty slice")
            if lone and d != 1.0:
                tags.add("lone " + kind)
            if d == 0.0 and not lone:
                tags.add("equal second")
        for i, e in enumerate(accepted):
            if e[3] == 2.0 and any(2.0 < f[3] < 3.0 for f in accepted[i + 1:]):
                tags.add("2.0 then above")
            if any(f[3] > e[3] for f in accepted[:i]):
                tags.add("smaller wins")
        for lvl in {int(e[3]) for e in accepted}:
            if sum(1 for e in accepted if int(e[3]) == lvl) >= 3:
                tags.add("last of several")
        if accepted:
            tags.add("vertical overrides" if accepted[-1][1] == "v" else "vertical does not override")
    return tags


def stable_order(eff):
    """record indices rbg * S + slice by descending efficiency, ties in index order: std::sort's result for at most 16 records"""
    S = len(eff[0])
    return sorted(range(len(eff) * S), key=lambda x: -eff[x // S][x % S])


def plain_maximize_cell(order, quota, positions=None):
    """the scan of :362-369 over `order`; positions (a dict, optional) receives the sorted position of every grant, the position at
    which each slice reaches its quota, and the records still live (RBG free, slice open) behind the first 64"""
    S = len(quota)
    R = len(order) // S
    got, m = [0] * S, [-1] * R
    grants, closes, live_after = [], {}, None
    for pos, x in enumerate(order):
        if pos == 64:
            live_after = sum(1 for y in order[64:] if m[y // S] == -1 and got[y % S] < quota[y % S])
        r, s = x // S, x % S
        if got[s] < quota[s] and m[r] == -1:
            m[r] = s
            got[s] += 1
            grants.append(pos)
            if got[s] == quota[s]:
                closes[s] = pos
    if positions is not None:
        positions.update(grants=grants, closes=closes, live_after_first_vector=live_after)
    return m


def plain_upper_bound(eff, quota):
    """{slice: RBGs taken, in the order taken}; whole (R <= 16 only)"""
    R, S = len(eff), len(quota)
    assert R <= 16, "above 16 RBGs std::sort is not stable: use upper_bound_facts"
    out = {}
    for j in range(S):
        if quota[j] <= 0:
            continue
        col = sorted(range(R), key=lambda i: -eff[i][j])
        out[j] = col[:quota[j]]        # (beyond R the reference reads past its vector: the callers keep such cases apart)
    return out


def upper_bound_facts(eff, quota):
    """{slice: (the taken efficiencies, descending; the RBGs strictly above the cut, which every tie order takes)}"""
    R, S = len(eff), len(quota)
    out = {}
    for j in range(S):
        if quota[j] <= 0:
            continue
        col = sorted((eff[i][j] for i in range(R)), reverse=True)
        take = col[:quota[j]]
        out[j] = (take, {i for i in range(R) if eff[i][j] > take[-1]})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------

def _rng(name):
    return qe._Lcg(zlib.crc32(name.encode()))


def _mk(name, family, shape, keys, quota, listed=None, cqi=None, **plants):
    ues, R, G = SHAPES[shape]
    S, nb = len(ues), R * G
    w = [1.0 / S] * S
    u2s = [s for s, n in enumerate(ues) for _ in range(n)]
    ids = list(range(len(u2s))) if listed is None else list(listed)
    has = [False] * S
    for u in ids:
        has[u2s[u]] = True
    quota = list(quota)
    assert len(quota) == S and sum(quota) == R, name
    assert all(quota[s] == 0 for s in range(S) if not has[s]), name
    state = []
    for s in range(S):
        if not has[s]:
            state.append(0.0)
            continue
        t, p = quota[s] * G, nb * w[s]
        x = t - p
        for k in range(1, 5):              # (nb * w is inexact on some shapes: the sum must still truncate to the target)
            if int(p + x) == t:
                break
            x = np.nextafter(t - p, np.inf if p + (t - p) < t else -np.inf).item() if k == 1 else np.nextafter(x, np.inf if p + x < t else -np.inf).item()
        state.append(x)
    g = _rng(name)
    c = Case(name, family, list(ues), w, R, G, state, listed=listed, r0=g.next() % 1000, r1=g.next() % 1000,
             plants=dict(keys=keys, quota=quota, shape=shape, **plants))
    if cqi is None:
        assert max(ues) == 1 and len(keys) == R and all(len(row) == S for row in keys), name
        for r in range(R):
            for s in range(S):
                assert (1 <= keys[r][s] <= 15) if has[s] else keys[r][s] == 0, (name, r, s)
        cqi = [[keys[r][u2s[u]] if u in ids else 15 for r in range(R)] for u in range(len(u2s))]
    c.cqi = cqi
    c.avg = [1000.0 + 37 * u + g.next() % 4000 for u in range(len(u2s))]
    st = c.steps()
    assert st["quota"] == quota and st["extra_rbs"] == 0 and st["extra_rbgs"] == 0, (name, st)
    assert 5 * nb * (1 + sum(w)) + sum(abs(x) for x in state) < 2**15, name      # the setters' domain (include/radiosaber_hip.h)
    return c


def _has(shape, listed=None):
    ues = SHAPES[shape][0]
    if listed is None:
        return [n > 0 for n in ues]
    u2s = [s for s, n in enumerate(ues) for _ in range(n)]
    return [any(u2s[u] == s for u in listed) for s in range(len(ues))]


def _rand_keys(g, shape, palette, listed=None):
    ues, R, _ = SHAPES[shape]
    has = _has(shape, listed)
    return [[palette[g.next() % len(palette)] if has[s] else 0 for s in range(len(ues))] for _ in range(R)]


def _rand_quota(g, shape, listed=None, negatives=0):
    """R units dealt over the slices with a listed user; `negatives` of them pushed to -1 .. -3 and the units given to another"""
    ues, R, _ = SHAPES[shape]
    has = _has(shape, listed)
    on = [s for s in range(len(ues)) if has[s]]
    q = [0] * len(ues)
    for _ in range(R):
        q[on[g.next() % len(on)]] += 1
    for _ in range(negatives):
        a, b = on[g.next() % len(on)], on[g.next() % len(on)]
        if a != b:
            d = q[a] + 1 + g.next() % 3
            q[a] -= d
            q[b] += d
    return q


def _m_cqi(g, palette):
    ues, R, _ = SHAPES["M"]
    return [[palette[g.next() % len(palette)] for _ in range(R)] for _ in range(sum(ues))]


TIES = [9, 9, 11, 14]


def _random_case(family, shape, k, palette=TIES, negatives=0, listed=None, **plants):
    name = f"{family} random {shape} #{k}" + (" subset" if listed is not None else "")
    g = _rng(name)
    if shape == "M":
        return _mk(name, family, shape, None, _rand_quota(g, shape, negatives=negatives), cqi=_m_cqi(g, palette), **plants)
    return _mk(name, family, shape, _rand_keys(g, shape, palette, listed), _rand_quota(g, shape, listed, negatives), listed=listed, **plants)


def _all_but(shape, user):
    return [u for u in range(sum(SHAPES[shape][0])) if u != user]


# ---- GreedyByRow ------------------------------------------------------------------------------------------------------------

def _gbr_pairs(name, shape, slices, quota):
    """pair p (RBGs 2p, 2p + 1) belongs to slices[p], a slice of quota 1: key 15 on both RBGs and key 1 everywhere else, so that the
    slice takes the even RBG, is closed, and still holds the odd RBG's maximum"""
    ues, R, _ = SHAPES[shape]
    g = _rng(name)
    keys = [[2 + g.next() % 11 for _ in ues] for _ in range(R)]
    for p, s in enumerate(slices):
        assert quota[s] == 1
        for r in range(R):
            keys[r][s] = 15 if r in (2 * p, 2 * p + 1) else 1
    return _mk(name, "gbr", shape, keys, quota, pairs=[(2 * p, s) for p, s in enumerate(slices)])


def gbr_cases():
    out = [
        _mk("gbr two pairs close on the even RBG", "gbr", "T4", [[15, 5, 4, 3], [15, 5, 4, 3], [1, 1, 15, 8], [1, 1, 15, 8]], [1] * 4,
            pairs=[(0, 0), (2, 2)]),
        _mk("gbr identical rows, quota 1 each", "gbr", "T4", [[9] * 4] * 4, [1] * 4),
        _gbr_pairs("gbr five pairs on 25 RBGs", "A20", [0, 3, 7, 11, 14], [1] * 15 + [2] * 5),
        _gbr_pairs("gbr eight pairs on 32 x 32", "S32", [31, 0, 5, 9, 16, 17, 30, 2], [1] * 32),
        _gbr_pairs("gbr eight pairs on 33 x 33", "S33", [32, 31, 1, 0, 15, 16, 17, 8], [1] * 33),
        _gbr_pairs("gbr pairs on 64 x 64, lane 63 first", "S64", [63, 62, 0, 32, 31, 33], [1] * 64),
        _mk("gbr identical rows on 64 x 64, quota 1 each", "gbr", "S64", [[9] * 64] * 64, [1] * 64),
        _mk("gbr the winner in lane 63", "gbr", "S64", [[3 + (r + s) % 7 for s in range(63)] + [15] for r in range(64)], [1] * 32 + [0] * 31 + [32]),
        _mk("gbr one RBG, sixteen slices", "gbr", "R1S16", [[9] * 16], [0] * 5 + [1] + [0] * 10),
        _mk("gbr one RBG, a negative quota beside it", "gbr", "R1S16", [[3] * 15 + [15]], [2, -1] + [0] * 14),
        _mk("gbr equal keys everywhere on 25 RBGs", "gbr", "A20", [[9] * 20] * 25, [2, 0, 1, 1, 3] * 3 + [1, 1, 1, 0, 1]),
        _mk("gbr negative, zero, above R on 4 RBGs", "gbr", "T4", [[9, 9, 9, 9], [12, 9, 7, 12], [9, 9, 9, 9], [5, 15, 5, 15]], [-2, 0, 8, -2]),
        _mk("gbr negative, zero, above R on 25 RBGs", "gbr", "A20", _rand_keys(_rng("gbr nz"), "A20", TIES), [-3, 0, 30, -2] + [0] * 16),
        _mk("gbr negative, zero, above R on 64 RBGs", "gbr", "S64", _rand_keys(_rng("gbr nz64"), "S64", TIES), [0] * 62 + [-6, 70]),
        _mk("gbr empty slices on 8 RBGs", "gbr", "E8", _rand_keys(_rng("gbr e8"), "E8", TIES), [0, 2, 1, 0, 4, 1]),
    ]
    out += [_random_case("gbr", "A20", k) for k in range(3)]
    out += [_random_case("gbr", "S33", k) for k in range(2)]
    out += [_random_case("gbr", "M", k) for k in range(2)]
    out += [_random_case("gbr", "A20", 0, listed=_all_but("A20", 7)), _random_case("gbr", "S32", 0, negatives=3)]
    return out


# ---- SubOpt -----------------------------------------------------------------------------------------------------------------

def _subopt_ties(name, shape, need, owners=None, neither=None, bump=None, listed=None):
    """Every RBG starts with an owner slice (key 15, or 14 for a second owner on the odd RBGs); the slices of `need` (slice ->
    units below quota) hold key 9 on every RBG, so that every move to any of them from one owner loses the same; the rest hold
    key 3 and own nothing (`neither`: their quotas, zero or negative).  bump = (RBG, slice): key 12 there, a smaller loss on a later
    RBG."""
    ues, R, _ = SHAPES[shape]
    S = len(ues)
    has = _has(shape, listed)
    on = [s for s in range(S) if has[s]]
    owners = [next(s for s in on if s not in need)] if owners is None else owners
    keys = [[0] * S for _ in range(R)]
    for r in range(R):
        for s in on:
            keys[r][s] = 9 if s in need else 3
        o = owners[r % len(owners)]
        keys[r][o] = 15 if o == owners[0] else 14
    if bump:
        keys[bump[0]][bump[1]] = 12
    quota = [0] * S
    for s, n in need.items():
        quota[s] = n
    for s, q in (neither or {}).items():
        assert s in on and s not in need and s not in owners
        quota[s] = q
    left = R - sum(quota)
    for i, o in enumerate(owners):
        quota[o] = left // len(owners) + (left % len(owners) if i == 0 else 0)
    return _mk(name, "subopt", shape, keys, quota, listed=listed, fewer=sorted(need))


def subopt_cases():
    ones = lambda slices: {s: 1 for s in slices}
    out = [
        _subopt_ties("subopt three fewer slices on 4 RBGs", "T4", ones([1, 2, 3])),
        _subopt_ties("subopt chain longer than S, empty slice 0", "E8", {2: 3, 4: 2, 5: 2}),
        _subopt_ties("subopt keys that share a bucket of 13", "A20", ones([2, 5, 15, 18])),
        _subopt_ties("subopt 13 fewer slices: no rehash", "A20", ones(range(1, 14))),
        _subopt_ties("subopt 14 fewer slices: one rehash", "A20", ones(range(1, 15))),
        _subopt_ties("subopt 19 fewer slices", "A20", ones(range(1, 20))),
        _subopt_ties("subopt 24 moves on 20 slices", "A20", {s: (2 if s <= 10 else 1) for s in range(1, 15)}),
        _subopt_ties("subopt a fewer slice erased in mid-run", "A20", {3: 2, 17: 1, 4: 3, 16: 1, 9: 2, 13: 4, 14: 1}),
        _subopt_ties("subopt two owners, the cheaper one runs out", "A20", {s: 1 for s in range(4, 19)}, owners=[0, 1]),
        _subopt_ties("subopt a smaller loss on a later RBG", "A20", ones(range(2, 17)), bump=(19, 7)),
        _subopt_ties("subopt negative quotas beside the fewer slices", "A20", {s: 2 for s in range(1, 15)}, neither={15: -1, 16: -2, 19: -1}),
        _subopt_ties("subopt a negative quota on an owner's neighbour", "T4", {1: 2, 3: 3}, neither={2: -2}),
        _subopt_ties("subopt a slice with users but none listed", "A20", ones([1, 2, 3, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18]),
                     listed=_all_but("A20", 7)),
        _subopt_ties("subopt 31 fewer slices of 32: two rehashes", "S32", ones(range(1, 32))),
        _subopt_ties("subopt 29 fewer slices of 32", "S32", ones(range(3, 32))),
        _subopt_ties("subopt 30 fewer slices of 32", "S32", ones(range(2, 32))),
        _subopt_ties("subopt 32 fewer slices of 33", "S33", ones(range(1, 33))),
        _subopt_ties("subopt 25 fewer slices of 33, two owners", "S33", ones(range(8, 33)), owners=[0, 4]),
        _subopt_ties("subopt 63 fewer slices of 64: three rehashes", "S64", ones(range(1, 64))),
        _subopt_ties("subopt 60 fewer slices of 64", "S64", ones(range(4, 64))),
        _subopt_ties("subopt 59 fewer slices of 64", "S64", ones(range(5, 64))),
        _subopt_ties("subopt 30 fewer slices of 64, needs of 2", "S64", {s: 2 for s in range(1, 60, 2)}),
    ]
    out += [_random_case("subopt", "A20", k, negatives=k % 2) for k in range(3)]
    out += [_random_case("subopt", "S32", k) for k in range(2)]
    out += [_random_case("subopt", "S33", k, negatives=k) for k in range(2)]
    out += [_random_case("subopt", "T4", k) for k in range(2)]
    out += [_random_case("subopt", "S64", 0), _random_case("subopt", "E8", 0)]
    out += [_random_case("subopt", "M", k) for k in range(2)]
    return out


# ---- VogelApproximate -------------------------------------------------------------------------------------------------------

VOGEL_PALETTE = [1, 1, 8, 11, 11, 14, 12, 5, 13, 9]
# (shape, number): picked by search so that the tags below and every mutant are met several times; the CPU tests check that they do
VOGEL_RANDOM = [("T4", k) for k in (0, 1, 2, 3, 4, 5)] + [("E8", k) for k in (0, 1, 2)] + [("A20", k) for k in (0, 1, 2, 3)] + \
               [("S32", k) for k in (0, 1, 2)] + [("S33", k) for k in (0, 1, 2)] + [("S64", k) for k in (0, 1)] + [("M", k) for k in (0, 1)]
VOGEL_TAGS = ("2.0 after 2", "2.0 then above", "smaller wins", "equal second", "lone h", "lone v", "last of several",
              "vertical overrides", "vertical does not override")


def vogel_cases():
    low = [3, 3, 3, 3]
    out = [
        _mk("vogel 2.0 after the maximum is 2", "vogel", "T4", [[12, 1, 1, 1], [11, 1, 1, 1], low, low], [1] * 4, tags=["2.0 after 2"]),
        _mk("vogel 2.0 first, then 2.2", "vogel", "T4", [[11, 1, 1, 1], [13, 5, 5, 5], low, low], [1] * 4, tags=["2.0 then above"]),
        _mk("vogel 2.0 twice, (14, 8) after (11, 1)", "vogel", "T4", [[11, 1, 1, 1], [14, 8, 8, 8], low, low], [1] * 4, tags=["2.0 after 2"]),
        _mk("vogel a smaller difference wins", "vogel", "T4", [[12, 1, 1, 1], [15, 10, 10, 10], low, low], [1] * 4, tags=["smaller wins"]),
        _mk("vogel an equal earlier value is second", "vogel", "T4", [[9, 9, 3, 3], [9, 3, 9, 3], [12, 12, 12, 12], [7, 7, 7, 9]], [1] * 4,
            tags=["equal second"]),
        _mk("vogel a new best does not demote the old one", "vogel", "T4", [[5, 12, 1, 1], [9, 9, 9, 9], [9, 9, 9, 9], [9, 9, 9, 9]], [1] * 4),
        _mk("vogel a single open slice", "vogel", "T4", [[5, 9, 9, 9], [12, 9, 9, 9], [15, 9, 9, 9], [14, 9, 9, 9]], [4, 0, 0, 0],
            tags=["lone h", "smaller wins"]),
        _mk("vogel the last accepted of three", "vogel", "T4", [[12, 1, 1, 1], [12, 2, 2, 2], [13, 5, 5, 5], low], [1] * 4, tags=["last of several"]),
        _mk("vogel a column overrides the rows", "vogel", "T4", [[15, 15, 15, 15], [15, 1, 15, 15], [15, 1, 15, 15], [15, 1, 15, 15]], [1] * 4,
            tags=["vertical overrides"]),
        _mk("vogel negative, zero, above R", "vogel", "T4", [[11, 1, 14, 8], [1, 11, 8, 14], [12, 1, 15, 10], [11, 1, 1, 1]], [-2, 0, 8, -2]),
        _mk("vogel negative, zero, above R on 25 RBGs", "vogel", "A20", _rand_keys(_rng("vogel nz"), "A20", VOGEL_PALETTE), [-3, 12, 18, -2] + [0] * 16),
        _mk("vogel one RBG, sixteen slices", "vogel", "R1S16", [[11] + [1] * 15], [0] * 3 + [1] + [0] * 12, tags=["lone h", "lone v"]),
        _mk("vogel sixteen RBGs, one slice", "vogel", "R16S1", [[1 + (5 * r) % 15] for r in range(16)], [16], tags=["lone h"]),
    ]
    out += [_random_case("vogel", shape, k, palette=VOGEL_PALETTE) for shape, k in VOGEL_RANDOM]
    out += [_random_case("vogel", "A20", 0, palette=VOGEL_PALETTE, listed=_all_but("A20", 7))]
    return out


def bare_cases():
    """(name, policy, keys [R][S], quota): inputs of the bare policy functions that no TTI can produce (module docstring).  With one
    slice open the order of the picks cannot change the map, so the lone 1.0 pins the arithmetic of the event and nothing else."""
    return [
        ("vogel the 1.0 of a lone empty slice", "vogel", [[0, 9], [0, 9], [0, 9]], [3, 0]),
        ("vogel the 1.0 of a lone empty slice after a 1.09", "vogel", [[1, 9], [0, 9], [0, 9]], [3, 0]),
        ("vogel all slices closed before the RBGs run out", "vogel", [[11, 1, 5], [14, 8, 5], [9, 9, 9], [12, 3, 7]], [1, 1, 0]),
        ("vogel no slice open at all", "vogel", [[11, 1], [14, 8]], [0, -1]),
    ]


# ---- MaximizeCell's scan ----------------------------------------------------------------------------------------------------

SCAN_RANDOM = [("A20", k) for k in (0, 1, 2, 3)] + [("S32", k) for k in (0, 1, 2)] + [("S33", k) for k in (0, 1)] + \
              [("S64", k) for k in (0, 1)] + [("M", k) for k in (0, 1)] + [("E8", 0)]
TINY = ("T4", "R8S2", "R2S8", "R16S1", "R1S16")


def _block_keys(shape, g, blocks, rest=(1, 5)):
    """blocks: {slice: (key, RBGs or None for all)}; everything else a key of rest[0] .. rest[1]"""
    ues, R, _ = SHAPES[shape]
    keys = [[rest[0] + g.next() % (rest[1] - rest[0] + 1) for _ in ues] for _ in range(R)]
    for s, (k, rbgs) in blocks.items():
        for r in (range(R) if rbgs is None else rbgs):
            keys[r][s] = k
    return keys


def scan_cases():
    g = _rng("scan blocks")
    q32 = lambda d: [d.get(s, 0) for s in range(32)]
    out = [
        # 32 records of key 15 whose slice has quota 0, then the 32 of slice 1: its last grant is the record at position 63
        _mk("scan a slice closes at position 63", "scan", "S32", _block_keys("S32", g, {0: (15, None), 1: (14, None)}), q32({1: 32}),
            close=(1, 63)),
        _mk("scan a slice closes at position 64", "scan", "S32", _block_keys("S32", g, {0: (15, None), 2: (15, [0]), 1: (14, None)}), q32({1: 32}),
            close=(1, 64)),
        _mk("scan a slice closes at position 63, 20 slices", "scan", "A20", _block_keys("A20", g, {0: (15, None), 5: (15, range(14)), 1: (14, None)}),
            [0, 25] + [0] * 18, close=(1, 63)),
        _mk("scan a slice closes at position 64, 20 slices", "scan", "A20", _block_keys("A20", g, {0: (15, None), 5: (15, range(15)), 1: (14, None)}),
            [0, 25] + [0] * 18, close=(1, 64)),
        _mk("scan the R-th grant at position 31", "scan", "S32", [[15 if s == r else 1 + (r * 7 + s) % 9 for s in range(32)] for r in range(32)],
            [1] * 32, last_grant_below=64),
        _mk("scan the R-th grant inside the first vector, 20 slices", "scan", "A20",
            [[15 if s == r % 20 else 1 + (r * 7 + s) % 9 for s in range(20)] for r in range(25)], [2] * 5 + [1] * 15, last_grant_below=64),
        _mk("scan the last RBG is granted behind every other record", "scan", "A20", [[2 + (r * 3 + s) % 13 for s in range(20)] for r in range(24)] + [[1] * 20],
            _rand_quota(g, "A20"), last_grant_above=128),
        _mk("scan the last RBG is granted behind every other record, 32 x 32", "scan", "S32",
            [[2 + (r * 3 + s) % 13 for s in range(32)] for r in range(31)] + [[1] * 32], [1] * 32, last_grant_above=128),
        _mk("scan negative, zero, above R", "scan", "A20", _rand_keys(g, "A20", TIES), [-3, 0, 30, -2] + [0] * 16),
        _mk("scan negative, zero, above R on 32 x 32", "scan", "S32", _rand_keys(g, "S32", TIES), q32({0: -4, 7: 40, 31: -4})),
        _mk("scan negative, zero, above R on 64 x 64", "scan", "S64", _rand_keys(g, "S64", TIES), [0] * 62 + [-6, 70]),
    ]
    out += [_random_case("scan", shape, k, live_after_first_vector=65 if shape == "S32" else None) for shape, k in SCAN_RANDOM]
    for shape in TINY:
        out += [_random_case("scan", shape, k, negatives=k) for k in range(2)]
    return out


# ---- UpperBound -------------------------------------------------------------------------------------------------------------

def upper_cases():
    g = _rng("upper")
    out = [
        _mk("upper ties at the cut key", "upper", "T4", [[9, 12, 9, 9], [9, 9, 14, 9], [9, 12, 9, 9], [9, 9, 14, 9]], [2, 1, 1, 0], cut_ties=True),
        _mk("upper one slice takes exactly R", "upper", "T4", [[9, 1, 1, 1], [11, 1, 1, 1], [9, 1, 1, 1], [14, 1, 1, 1]], [4, 0, 0, 0]),
        _mk("upper negative and zero quotas", "upper", "T4", _rand_keys(g, "T4", TIES), [-1, 0, 3, 2], cut_ties=True),
        _mk("upper a quota above R", "upper", "T4", _rand_keys(g, "T4", TIES), [6, -1, -1, 0], oracle_only=True),
        _mk("upper empty slices, ties at the cut", "upper", "E8", _rand_keys(g, "E8", TIES), [0, 3, 2, 0, 2, 1], cut_ties=True),
        _mk("upper empty slices, a negative quota", "upper", "E8", _rand_keys(g, "E8", TIES), [0, 7, -2, 0, 2, 1]),
        _mk("upper two slices on 8 RBGs", "upper", "R8S2", _rand_keys(g, "R8S2", TIES), [5, 3], cut_ties=True),
        _mk("upper two slices, one takes all 8", "upper", "R8S2", _rand_keys(g, "R8S2", TIES), [8, 0]),
        _mk("upper sixteen RBGs, one slice", "upper", "R16S1", _rand_keys(g, "R16S1", TIES), [16]),
        _mk("upper two RBGs, eight slices", "upper", "R2S8", [[9, 11, 11, 11, 11, 14, 9, 9], [9, 9, 11, 9, 11, 14, 9, 9]], [1, 0, 2, -1, 0, 0, 0, 0], cut_ties=True),
        _mk("upper one RBG, sixteen slices", "upper", "R1S16", _rand_keys(g, "R1S16", TIES), [0] * 9 + [1] + [0] * 6),
        _mk("upper ties at the cut key on 25 RBGs", "upper", "A20", _rand_keys(g, "A20", TIES), _rand_quota(g, "A20"), cut_ties=True),
        _mk("upper 25 RBGs, negative, zero, exactly R", "upper", "A20", _rand_keys(g, "A20", TIES), [-3, 25, 5, -2] + [0] * 16),
    ]
    out += [_random_case("upper", "M", 0)]
    return out


_BUILDERS = dict(gbr=gbr_cases, subopt=subopt_cases, vogel=vogel_cases, scan=scan_cases, upper=upper_cases)
_cache = {}


def cases(family):
    if family not in _cache:
        got = _BUILDERS[family]()
        assert len({c.name for c in got}) == len(got), f"{family}: duplicate names"
        for c in got:
            assert c.family == family and c.U <= 64 and c.R <= 64 and c.plants["shape"] in SHAPES, c.name
        _cache[family] = got
    return _cache[family]


def all_cases():
    return [c for f in FAMILIES for c in cases(f)]


def whole(c):
    """True where the model of the case's policy is whole without the oracle's sort order"""
    if c.family == "scan":
        return c.R * c.S <= 16
    if c.family == "upper":
        return c.R <= 16
    return True
