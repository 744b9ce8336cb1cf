"""Directed edge inputs for the quota step (P2) and for scheduler 7's slice pick, and a plain exact model of both.

Nothing here imports the kernels or the oracle; the model uses Python ints, floats (IEEE doubles, one rounding per operation, never
fused) and fractions.Fraction.  It is written from the behaviour of the reference at the cited lines, not from the oracle:

  * quotas (downlink-transport-scheduler.cpp:463-521).  A slice counts when one of the call's users belongs to it.  Its target is
    (int)(nb_rbs * weight + offset): one rounded product, one rounded sum, truncation toward zero.  extra_rbs = nb_rbs minus the
    targets; every counted slice receives extra_rbs / n (C division: toward zero), and the first counted slice of the rotation
    k = (i + rand()) % S, i = 0 .. S-1, receives extra_rbs % n (C remainder: the sign of the dividend).  quota = target / rbg_size
    for every slice (C division again), and the same distribution of extra_rbgs = nb_rbgs minus the quotas with a second rand().
  * offsets afterwards (:618-620): target - granted RBGs * rbg_size, stored as a double.
  * GreedyByRow (:249-272): RBG ascending; strict '>' from -1 over the slices under their quota, so the first maximum wins.
  * SelectSliceToServe (downlink-nvs-scheduler.cpp:94-142): slices with data ascending; a zero EWMA ends the scan and wins; else
    score = weight / ewma and '>=' from 0, so the LAST maximum wins; then ewma = (1 - 0.01) * ewma for every slice with data and
    += 0.01 * 1 for the picked one, each operation rounded.

`fused_target` / `fused_ewma` evaluate product-and-sum with ONE rounding (what a fused multiply-add does), through Fraction.  They
exist only to prove that a case would expose a contracted evaluation; nothing compares a kernel with them.

Two things the case families cannot contain, by arithmetic and not by omission:
  * `product` triples on a grid whose nb_rbs is a power of two ((8, 4), (4, 2), (64, 8): nb = 32, 8, 512).  nb * w is then exact
    (a change of exponent), so the rounded sum IS the once-rounded value and no input separates the two evaluations
    (`no_product_triples_on` checks it by search).  The family uses the three grids of 25 RBGs instead: nb = 100, 50, 25.
  * |extra_rbgs| >= n.  The targets sum to nb_rbs = nb_rbgs * rbg_size exactly, so extra_rbgs = sum of the targets' C remainders
    / rbg_size, of magnitude below n: extra_rbgs / n is always 0 and the whole of it is the remainder.  `negdiv` plants extra_rbgs
    at what can occur, -(n - 2) ... n - 1, and the full range on extra_rbs.

Rands stay at or below 2^31 - 1 - S: above that the reference's own `i + rand()` overflows an int (undefined behaviour)."""
import math
import struct
import zlib
from dataclasses import dataclass, field
from fractions import Fraction

BETA = 0.01          # downlink-nvs-scheduler.h:42
RAND_MAX = 2**31 - 1
FAMILIES = ("trunc", "product", "negdiv", "rotate", "policy", "chain", "nvs")
MIN_CASES = {"trunc": 6, "product": 6, "negdiv": 30, "rotate": 12, "policy": 4, "chain": 3, "nvs": 20}
TRANSPORT = (8, 9, 10, 101, 103)
CHAIN_TTIS = 8


# ---------------------------------------------------------------------------------------------------------------------------
# the plain model
# ---------------------------------------------------------------------------------------------------------------------------

def c_div(a, b):
    """C's a / b on ints: the quotient truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def c_mod(a, b):
    """C's a % b: a - (a / b) * b, the sign of the dividend"""
    return a - c_div(a, b) * b


def reference_target(nb_rbs, w, offset):
    product = nb_rbs * w          # one rounding
    total = product + offset      # one rounding
    return int(total)             # toward zero


def fused_target(nb_rbs, w, offset):
    return int(float(Fraction(nb_rbs) * Fraction(w) + Fraction(offset)))   # one rounding in all


def first_of_rotation(has, r):
    S = len(has)
    for i in range(S):
        k = (i + r) % S
        if has[k]:
            return k
    raise ValueError("no slice with a listed user: the reference asserts (:487)")


def quota_steps(nb_rbs, G, w, offset, has, r0, r1, target_of=reference_target, div=c_div, mod=c_mod):
    """Every intermediate of :463-521 as a dict (the tests read the extras, remainders and rotation heads from it)."""
    S = len(w)
    n = sum(1 for h in has if h)
    raw = [target_of(nb_rbs, w[s], offset[s]) if has[s] else 0 for s in range(S)]
    extra = nb_rbs - sum(raw)
    first0 = first_of_rotation(has, r0)
    target = list(raw)
    for s in range(S):
        if has[s]:
            target[s] += div(extra, n)
    target[first0] += mod(extra, n)
    nb_rbgs = div(nb_rbs, G)
    quota0 = [div(t, G) for t in target]
    extra_g = nb_rbgs - sum(quota0)
    first1 = first_of_rotation(has, r1)
    quota = list(quota0)
    for s in range(S):
        if has[s]:
            quota[s] += div(extra_g, n)
    quota[first1] += mod(extra_g, n)
    return dict(n=n, raw=raw, extra_rbs=extra, share=div(extra, n), rem=mod(extra, n), first0=first0, target=target,
                quota0=quota0, extra_rbgs=extra_g, share_g=div(extra_g, n), rem_g=mod(extra_g, n), first1=first1, quota=quota)


def plain_quotas(nb_rbs, G, w, offset, has, r0, r1):
    st = quota_steps(nb_rbs, G, w, offset, has, r0, r1)
    return st["target"], st["quota"]


def plain_offsets_after(target, granted_rbgs, G):
    return [float(t - g * G) for t, g in zip(target, granted_rbgs)]


def plain_greedy_by_row(keys, quota):
    """keys [R][S] -> rbg_to_slice [R] (-1 where the reference would assert: no slice under its quota)"""
    S = len(quota)
    got = [0] * S
    out = []
    for row in keys:
        best, pick = -1, -1
        for s in range(S):
            if row[s] > best and got[s] < quota[s]:
                best, pick = row[s], s
        out.append(pick)
        if pick >= 0:
            got[pick] += 1
    return out


def plain_nvs_pick(w, ewma, has):
    pick, best = 0, 0.0
    for i in range(len(w)):
        if not has[i]:
            continue
        if ewma[i] == 0:
            pick = i
            break
        score = w[i] / ewma[i]
        if score >= best:
            best, pick = score, i
    after = list(ewma)
    for i in range(len(w)):
        if not has[i]:
            continue
        after[i] = (1 - BETA) * ewma[i]
        if i == pick:
            after[i] = after[i] + BETA * 1
    return pick, after


def fused_ewma(e, picked=True):
    """the picked slice's update with the product and the sum rounded once"""
    if not picked:
        return (1 - BETA) * e
    return float(Fraction(1 - BETA) * Fraction(e) + Fraction(BETA * 1))


def bits(x):
    """(high word, low word) of a double, from struct.pack"""
    q = struct.unpack("<Q", struct.pack("<d", x))[0]
    return q >> 32, q & 0xFFFFFFFF


def from_bits(hi, lo):
    return struct.unpack("<d", struct.pack("<Q", (hi << 32) | lo))[0]


def _step(x, k):
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    family: str
    ues: list            # users per slice
    w: list              # slice weights
    R: int
    G: int
    state: list          # slice_rbs_offset_ before the call (nvs: slice_ewma_time_)
    listed: object = None   # ascending user ids of the call; None = every user
    r0: int = 0
    r1: int = 0
    plants: dict = field(default_factory=dict)
    cqi: list = None     # [U][R], 1..15
    avg: list = None     # [U]
    rands: list = None   # chain: CHAIN_TTIS pairs

    @property
    def S(self):
        return len(self.ues)

    @property
    def U(self):
        return sum(self.ues)

    @property
    def nb(self):
        return self.R * self.G

    @property
    def u2s(self):
        return [s for s, n in enumerate(self.ues) for _ in range(n)]

    @property
    def ids(self):
        return list(range(self.U)) if self.listed is None else list(self.listed)

    @property
    def has(self):
        u2s, h = self.u2s, [False] * self.S
        for u in self.ids:
            h[u2s[u]] = True
        return h

    @property
    def shape(self):
        return (tuple(self.ues), self.R, self.G)

    def steps(self, **kw):
        return quota_steps(self.nb, self.G, self.w, self.state, self.has, self.r0, self.r1, **kw)


class _Lcg:
    def __init__(self, seed):
        self.x = seed & 0x7FFFFFFF

    def next(self):
        self.x = (self.x * 1103515245 + 12345) & 0x7FFFFFFF
        return self.x >> 8


def _fill(c, equal_columns=False):
    """reports and averages of a case, drawn from its name; equal_columns: on every even RBG all users report CQI 9, so that the
    keys of the slices are equal there"""
    g = _Lcg(zlib.crc32(c.name.encode()))
    c.cqi = [[(9 if equal_columns and r % 2 == 0 else 1 + g.next() % 15) for r in range(c.R)] for _ in range(c.U)]
    c.avg = [1000.0 + g.next() % 4000000 for _ in range(c.U)]
    if c.family == "chain":
        c.rands = [[g.next() % (RAND_MAX - 64), g.next() % (RAND_MAX - 64)] for _ in range(CHAIN_TTIS)]
    return c


A = ([3, 2, 4, 3], 25, 4)     # nb = 100: the shape most cases share (one run-time build serves them)
B = ([3, 2, 3], 8, 4)         # nb = 32
W4 = [0.25] * 4


def _mk(name, family, shape, w, state, **kw):
    ues, R, G = shape
    eq = kw.pop("equal_columns", False)
    c = Case(name, family, list(ues), [float(x) for x in w], R, G, [float(x) for x in state], **kw)
    assert len(c.w) == c.S and len(c.state) == c.S, name
    return _fill(c, eq)


def _users_of(ues, slices):
    first = [0]
    for n in ues:
        first.append(first[-1] + n)
    return [u for s in slices for u in range(first[s], first[s + 1])]


def trunc_cases():
    below = math.nextafter(-25.0, -math.inf)
    out = [
        _mk("trunc sums -1.5 -1.0 -0.5 -0", "trunc", A, W4, [-26.5, -26.0, -25.5, below],
            plants=dict(sums=[-1.5, -1.0, -0.5, 25.0 + below], raw=[-1, -1, 0, 0])),
        _mk("trunc sums 0.5 0 3 21.75", "trunc", A, W4, [-24.5, -25.0, -22.0, -3.25],
            plants=dict(sums=[0.5, 0.0, 3.0, 21.75], raw=[0, 0, 3, 21])),
        _mk("trunc fractional offsets", "trunc", A, W4, [0.75, -0.75, 1e-9, -1e-9],
            plants=dict(sums=[25.75, 24.25, 25.0 + 1e-9, 25.0 - 1e-9], raw=[25, 24, 25, 24])),
        _mk("trunc sums 2.5 -2.5 on 8x4", "trunc", B, [0.5, 0.25, 0.25], [-13.5, -10.5, 0.0],
            plants=dict(sums=[2.5, -2.5, 8.0], raw=[2, -2, 8])),
        _mk("trunc sums -0.5 4.5 on 4x2", "trunc", ([2, 3], 4, 2), [0.5, 0.5], [-4.5, 0.5], plants=dict(sums=[-0.5, 4.5], raw=[0, 4])),
        # final targets whose division by the RBG size must truncate toward zero: -1 / 4 = 0, -3 / 4 = 0, -4 / 4 = -1, -5 / 4 = -1
        _mk("trunc targets -1 -3 -4 108", "trunc", A, W4, [-26, -28, -29, 83], plants=dict(target=[-1, -3, -4, 108], quota0=[0, 0, -1, 27])),
        _mk("trunc targets -5 -4 -3 112", "trunc", A, W4, [-30, -29, -28, 87], plants=dict(target=[-5, -4, -3, 112], quota0=[-1, -1, 0, 28])),
        _mk("trunc targets -1 -7 -8 -9 on 8x4", "trunc", ([2, 2, 2, 2], 8, 4), W4, [-9, -15, -16, 40],
            plants=dict(target=[-1, -7, -8, 48], quota0=[0, -1, -2, 12])),
    ]
    return out


def product_triples(nb, weights=None, offsets=None):
    """(w, offset, reference target, fused target) wherever the two evaluations truncate differently"""
    weights = [k / 100 for k in range(1, 100)] if weights is None else weights
    offsets = [float(x) for x in range(-nb, nb + 1)] if offsets is None else offsets
    out = []
    for w in weights:
        if Fraction(nb) * Fraction(w) == Fraction(nb * w):
            continue     # the product is exact: both evaluations round the same number once
        for off in offsets:
            a, b = reference_target(nb, w, off), fused_target(nb, w, off)
            if a != b:
                out.append((w, off, a, b))
    return out


def no_product_triples_on(nb):
    """True when nb * w is exact for every weight searched (nb a power of two): the two evaluations cannot differ"""
    return not product_triples(nb)


PRODUCT_GRIDS = [(25, 4), (25, 2), (25, 1)]


def _separating(nb, G, w4, sl, r0, triples):
    """offsets (a binding one for slice sl, plain ones elsewhere) at which the final targets or quotas of the two evaluations differ:
    a difference of one PRB in one slice can vanish again in the shares, above all when that slice also receives the remainder"""
    for t in triples:
        for filler in ([0.5, 0.5, -1.25, 2.0], [0.5, 1.5, -1.25, 2.0], [1.5, 0.5, 0.75, 2.0], [0.5, 2.5, -2.25, 3.0]):
            state = list(filler)
            state[sl] = t[0]
            ref = quota_steps(nb, G, w4, state, [True] * 4, r0, 5)
            fus = quota_steps(nb, G, w4, state, [True] * 4, r0, 5, target_of=fused_target)
            if (ref["target"], ref["quota"]) != (fus["target"], fus["quota"]):
                return state, t
    raise AssertionError(f"nb {nb} w {w4[sl]}: no offsets separate the two evaluations in the final targets")


def product_cases():
    out = []
    for R, G in PRODUCT_GRIDS:
        nb = R * G
        by_w = {}
        for w, off, a, b in product_triples(nb):
            by_w.setdefault(w, []).append((off, a, b))
        ws = sorted(w for w in by_w if len(by_w[w]) >= 2 and w <= 0.3)
        if nb == 100:
            assert (-6.0, -1, 0) in by_w[0.05]
            ws = [0.05] + [w for w in ws if w != 0.05]
        if len(ws) < 2:
            raise AssertionError(f"no two weights with two binding offsets on nb = {nb}")
        shape = ([3, 2, 4, 3], R, G)
        w4 = [ws[0], ws[1], 0.3, 0.25]
        for j in range(2):
            # case 0: slice 0 binds and heads the first rotation (it also receives the remainder); case 1: slice 1 binds, slice 2 heads
            sl, head = j, (0 if j == 0 else 2)
            pick = by_w[w4[sl]]
            if nb == 100 and j == 0:
                pick = [t for t in pick if t[0] == -6.0]
            state, (off, a, b) = _separating(nb, G, w4, sl, 4 * 1000 + head, pick)
            out.append(_mk(f"product nb {nb} w {w4[sl]} offset {off}", "product", shape, w4, state, r0=4 * 1000 + head, r1=5,
                           plants=dict(slice=sl, reference=a, fused=b, head=head)))
        # a third case per grid: two slices bind at once, in a subset call that lists no user of slice 3
        (o0, a0, b0), (o1, a1, b1) = by_w[w4[0]][0], by_w[w4[1]][0]
        out.append(_mk(f"product nb {nb} two slices", "product", shape, w4, [o0, o1, 0.0, 7.0], listed=_users_of(shape[0], [0, 1, 2]),
                       r0=3, r1=RAND_MAX - 4, plants=dict(slice=0, reference=a0, fused=b0, also=(1, a1, b1), head=0)))
    return out


NEGDIV_UES = {4: [3, 2, 4, 3], 3: [3, 0, 4, 3], 2: [3, 0, 4, 0], 1: [0, 0, 4, 0]}


def negdiv_cases():
    """extra_rbs planted through the offset of the first counted slice (every counted slice has nb * w = 25); extra_rbgs through targets
    that are no multiple of the RBG size"""
    out = []
    for n, ues in NEGDIV_UES.items():
        shape = (ues, 25, 4)
        counted = [s for s in range(4) if ues[s]]
        wanted = []
        for e in (-1, -(n - 1), -n, -(n + 1), 1, n - 1, n, n + 1, -300 - n - 1, 300 + n + 1, -217, 214):
            if e != 0 and e not in wanted:
                wanted.append(e)
        for j, e in enumerate(wanted):
            state = [0.0] * 4
            state[counted[0]] = float((100 - 25 * n) - e)
            r0 = counted[j % n] + 4 * j      # the remainder's slice moves through the counted ones
            out.append(_mk(f"negdiv n {n} extra_rbs {e}", "negdiv", shape, W4, state, r0=r0, r1=r0 + 1,
                           plants=dict(n=n, extra_rbs=e, rem=c_mod(e, n), first0=counted[j % n])))
    # extra_rbgs: the targets already sum to 100 (extra_rbs = 0), their C remainders by 4 sum to 4 * extra_rbgs
    for name, ues, targets, eg in [("-2 of n 4", NEGDIV_UES[4], [-3, -3, -3, 109], -2), ("3 of n 4", NEGDIV_UES[4], [3, 3, 3, 91], 3),
                                   ("1 of n 4", NEGDIV_UES[4], [29, 24, 24, 23], 1), ("-1 of n 4", NEGDIV_UES[4], [-1, -3, 4, 100], -1),
                                   ("-1 of n 3", NEGDIV_UES[3], [-3, 0, -3, 106], -1), ("2 of n 3", NEGDIV_UES[3], [3, 0, 3, 94], 2),
                                   ("0 of n 2, remainders -1 and 1", NEGDIV_UES[2], [-1, 0, 101, 0], 0), ("1 of n 2", NEGDIV_UES[2], [27, 0, 73, 0], 1)]:
        state = [t - 25 if ues[s] else 0 for s, t in enumerate(targets)]
        counted = [s for s in range(4) if ues[s]]
        out.append(_mk(f"negdiv extra_rbgs {name}", "negdiv", (ues, 25, 4), W4, state, r0=1, r1=counted[-1],
                       plants=dict(n=len(counted), extra_rbs=0, extra_rbgs=eg, rem_g=eg, first1=counted[-1])))
    return out


S64_UES = [0 if s % 4 == 3 else 1 for s in range(64)]      # 48 users; slices 3, 7, ... are empty


def rotate_cases():
    out = []
    top = RAND_MAX
    # S = 1
    one = ([4], 8, 4)
    for r0, r1 in [(0, 1), (top - 1, top - 1)]:
        out.append(_mk(f"rotate S 1 rands {r0} {r1}", "rotate", one, [1.0], [-1.5], r0=r0, r1=r1, plants=dict(first0=0, first1=0)))
    # S = 3: every slice has users; rand % S in {0, 1, S - 1}, small and near the top of rand()'s range
    for m0, m1 in [(0, 1), (1, 2), (2, 0)]:
        big = (top - 3) - ((top - 3) % 3)       # a multiple of 3 at most 2^31 - 1 - S
        for base in (0, big - 3):
            r0, r1 = base + m0, base + m1
            out.append(_mk(f"rotate S 3 rands {r0} {r1}", "rotate", B, [0.5, 0.25, 0.25], [-2.0, 0.0, 3.0], r0=r0, r1=r1,
                           plants=dict(first0=m0, first1=m1)))
    # S = 5: slice 2 is empty; subset calls leave slice 1 (and 4) with users but none listed
    five = ([2, 3, 0, 2, 2], 8, 4)
    w5 = [0.25, 0.25, 0.125, 0.125, 0.25]
    off5, off5b = [-2.0, 1.0, 0.0, 0.0, 2.0], [-3.0, 1.0, 0.0, 0.0, 2.0]   # (both remainders must be non-zero for the head to show)
    big5 = (top - 5) - ((top - 5) % 5)
    for name, listed, off, r0, r1, f0, f1 in [
            ("starts on the empty slice", None, off5, 2, big5 - 5 + 2, 3, 3),
            ("starts on a slice with no listed user", [0, 1, 5, 6, 7, 8], off5b, 1, 4, 3, 4),
            ("wraps past the last slice", [0, 1, 2, 3, 4], off5, 4, big5 - 5 + 2, 0, 0),
            ("the last slice is first", None, off5, big5 - 1, 4, 4, 4),
            ("two rands two slices", None, off5, 0, 1, 0, 1),
            ("wraps over two skipped slices", [0, 1, 5, 6], off5b, big5 - 1, 1, 0, 3)]:
        out.append(_mk(f"rotate S 5 {name}", "rotate", five, w5, off, listed=listed, r0=r0, r1=r1, plants=dict(first0=f0, first1=f1)))
    # S = 64 on R = 8: the whole wave; the rotation starts on an empty slice and on the last slice
    out.append(_mk("rotate S 64", "rotate", (S64_UES, 8, 4), [1.0 / 64] * 64, [3.0 if s in (4, 62) else (1.75 if s == 9 else 0.0) for s in range(64)],
                   r0=64 * 1000 + 3, r1=64 * 33554430 + 63, plants=dict(first0=4, first1=0)))
    return out


def policy_cases():
    out = []
    for name, targets, r1 in [("negative zero above R", [-8, 2, 0, 106], 1), ("one slice holds all R", [0, 0, 100, 0], 0),
                              ("two negative entries", [-4, -9, 60, 53], 2), ("above R twice over", [-104, 0, 2, 202], 3),
                              ("zeros and one RBG each", [4, 0, 4, 92], 0)]:
        st = [t - 25 for t in targets]
        q = quota_steps(100, 4, W4, [float(x) for x in st], [True] * 4, 0, r1)["quota"]
        out.append(_mk(f"policy {name}", "policy", A, W4, st, r0=0, r1=r1, equal_columns=True, plants=dict(quota=q)))
    return out


def chain_cases():
    return [_mk("chain 0.3 0.3 0.2 0.2", "chain", A, [0.3, 0.3, 0.2, 0.2], [-6.0, 3.5, 0.0, 2.5]),
            _mk("chain quarter weights", "chain", A, W4, [-26.5, 30.25, -3.0, 0.0]),
            _mk("chain bench weight 0.05", "chain", A, [0.05, 0.45, 0.25, 0.25], [-6.0, 2.0, 3.0, 1.0]),
            _mk("chain 8x4", "chain", B, [0.5, 0.25, 0.25], [-17.0, 9.0, 8.5])]


N3 = ([2, 2, 2], 8, 4)
N4 = ([2, 0, 3, 2], 8, 4)


def _ulp_pair(w, e):
    """an EWMA near e whose score is exactly one ulp below e's"""
    s = w / e
    for k in range(1, 200):
        e2 = _step(e, k)
        if w / e2 == math.nextafter(s, 0.0):
            return e2
    raise AssertionError("no EWMA one ulp of the score away")


def _straddle(w, hi):
    """two EWMAs whose scores share the high word `hi`, one with a low word just below 0x80000000 and one at or above it"""
    e0 = w / from_bits(hi, 0x80000000)
    under = over = None
    for k in range(-60, 61):
        e = _step(e0, k)
        h, lo = bits(w / e)
        if h != hi:
            continue
        if lo < 0x80000000 and (under is None or lo > under[1]):
            under = (e, lo)
        if lo >= 0x80000000 and (over is None or lo < over[1]):
            over = (e, lo)
    if under is None or over is None:
        raise AssertionError("no pair of scores around the low word's sign bit")
    return under[0], over[0]


def fused_ewma_values(count=3):
    out = []
    for k in range(1, 1000):
        e = k / 1000
        if (1 - BETA) * e + BETA * 1 != fused_ewma(e):
            out.append(e)
            if len(out) == count:
                return out
    raise AssertionError("no EWMA separates the two evaluations")


def nvs_cases():
    out = []

    def mk(name, shape, w, ewma, **plants):
        out.append(_mk("nvs " + name, "nvs", shape, w, ewma, plants=plants))

    third = [1.0 / 3] * 3
    mk("two equal scores", N3, third, [0.5, 0.25, 0.25], pick=2, equal=(1, 2))
    mk("three equal scores", N3, third, [0.25, 0.25, 0.25], pick=2, equal=(0, 1, 2))
    mk("equal scores from different weights", N3, [0.5, 0.25, 0.25], [1.0, 0.5, 0.75], pick=1, equal=(0, 1))
    mk("a zero after a larger score", N3, third, [1e-9, 0.0, 0.5], pick=1)
    mk("two zeros", N3, third, [0.5, 0.0, 0.0], pick=1)
    mk("all zero: a fresh cell", N3, third, [0.0, 0.0, 0.0], pick=0)
    e = 1.4
    e2 = _ulp_pair(0.25, e)
    mk("scores an ulp apart, larger first", N3, [0.25, 0.25, 0.25], [e, e2, 3.0], pick=0, ulp=(0, 1))
    mk("scores an ulp apart, larger last", N3, [0.25, 0.25, 0.25], [e2, e, 3.0], pick=1, ulp=(1, 0))
    hi = bits(0.2)[0]
    under, over = _straddle(0.25, hi)
    mk("low words around the sign bit, larger first", N3, [0.25, 0.25, 0.25], [over, under, 3.0], pick=0, straddle=(0, 1))
    mk("low words around the sign bit, larger last", N3, [0.25, 0.25, 0.25], [under, over, 3.0], pick=1, straddle=(1, 0))
    hi2 = bits(0.7)[0]
    under2, over2 = _straddle(0.5, hi2)
    mk("low words around the sign bit, three slices", N3, [0.5, 0.5, 0.5], [under2, over2, under2], pick=1, straddle=(1, 0))
    mk("larger high word, smaller low word", N3, [0.25, 0.25, 0.25], [1.1, 0.5, 1.3], pick=1, hilo=(1, 0))
    mk("larger high word, smaller low word, first", N3, [0.25, 0.25, 0.25], [0.5, 1.1, 1.3], pick=0, hilo=(0, 1))
    mk("an infinite score against 1e308", N3, [0.25, 0.25, 0.25], [0.25 / 1e308, 5e-324, 1.0], pick=1, infinite=1, finite=0)
    mk("an infinite score first", N3, [0.25, 0.25, 0.25], [5e-324, 0.25 / 1e308, 1.0], pick=0, infinite=0, finite=1)
    mk("the empty slice holds the best score", N4, W4, [1.0, 1e-6, 2.0, 4.0], pick=0, ignored=1)
    mk("the empty slice holds a zero", N4, W4, [1.0, 0.0, 0.5, 4.0], pick=2, ignored=1)
    mk("the empty slice holds the last equal score", ([2, 2, 3, 0], 8, 4), W4, [0.5, 0.5, 1.0, 0.5], pick=1, ignored=3)
    mk("one slice with users, not slice 0", ([0, 0, 3, 0], 8, 4), W4, [0.0, 0.0, 0.5, 0.0], pick=2)
    mk("one slice with users, zero EWMA", ([0, 3, 0], 8, 4), third, [0.5, 0.0, 0.0], pick=1)
    ew64 = [0.5] * 64
    ew64[63] = 1e-3      # (empty)
    mk("S 64, every score equal", (S64_UES, 8, 4), [1.0 / 64] * 64, ew64, pick=62)
    for e in fused_ewma_values(3):
        mk(f"fused update differs at {e}", N3, [0.6, 0.2, 0.2], [e, 5.0, 7.0], pick=0, fused=e)
    mk("fused update differs on the last slice", N3, [0.2, 0.2, 0.6], [5.0, 7.0, fused_ewma_values(2)[1]], pick=2, fused=fused_ewma_values(2)[1])
    return out


_BUILDERS = dict(trunc=trunc_cases, product=product_cases, negdiv=negdiv_cases, rotate=rotate_cases, policy=policy_cases,
                 chain=chain_cases, nvs=nvs_cases)
_cache = {}


def cases(family):
    if family not in _cache:
        got = _BUILDERS[family]()
        assert len({c.name for c in got}) == len(got), f"{family}: duplicate names"
        for c in got:
            assert c.family == family and c.U <= 48 and c.R in (4, 8, 25) and (c.S <= 8 or c.S == 64), c.name
        _cache[family] = got
    return _cache[family]


def all_cases():
    return [c for f in FAMILIES for c in cases(f)]


def by_config(cs):
    """cases grouped by what one batch or one context fixes: (users per slice, weights, R, G)"""
    groups = {}
    for c in cs:
        groups.setdefault((tuple(c.ues), tuple(c.w), c.R, c.G), []).append(c)
    return list(groups.values())
