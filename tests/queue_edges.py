"""Directed edge populations for the batch queue model (finite MAC queues, two bearers per user) and a plain per-packet model of it.

Nothing here imports the kernels.  The oracle module is an argument where a builder needs it: a population's grants are read from a
backlogged oracle run of the same cell, the link tables (`rso_tbs_bits`, `rso_cqi_to_mcs`: `_ref`-pinned in tests/PINS.md) through it.

The plain model (`plain_user`, `plain_cell`): one user's two bearers as lists of packets [size, time stamp, bytes already sent].
  * a packet bears 8 bytes of overhead (RLC 2, MAC 3, CRC 3) whenever it or a piece of it is sent; a bearer's data to transmit is its
    queued bytes + 8 per queued packet, 0 without packets (ref: flows/MacQueue.cpp:86-99); a backlogged bearer's is 100 000 000;
  * a dequeue with `room` bytes (MacQueue.cpp:126-200, um-rlc-entity.cpp:126-196) goes on while room is left and packets wait: room of
    at most 8 sends nothing and ends it; a packet whose remaining bytes + 8 exceed the room leaves a fragment of room - 8 bytes and
    ends it; otherwise the packet leaves whole and the room shrinks by its remaining bytes + 8;
  * a transport scheduler (downlink-transport-scheduler.cpp:170-221) offers the user's grant to bearer 1, then what is left to bearer
    0; each takes min(offer, its data) and is credited that; scheduler 1 (dl-pf-packet-scheduler.cpp:60-125) credits every flow its
    own block in full;
  * the head-of-line delay (flows/radio-bearer.cpp:281-308) is read before the dequeue: 0 with no queued bytes, else now minus the
    head packet's time stamp, at least 1e-5;
  * a burst arrives in the first TTI whose clock value is not below its time; it is complete in the TTI in which its last packet
    leaves, whole or as its last fragment.
The model returns an event log that names the edge every dequeue took (`CLASSES`)."""
import collections
import math
from dataclasses import dataclass, field

import numpy as np

FULL = 1495        # bytes of a full packet in the MAC queue
OVERHEAD = 8
BACKLOG = 100000000
KIND = {"-": 0, "B": 1, "Q": 2}
SEED0 = 100        # cell c of every population draws from seed SEED0 + c

CLASSES = (["whole-exact"] + [f"whole-with-room-{r}" for r in range(1, 9)] + [f"fragment-leaves-{r}" for r in range(1, 10)]
           + ["fragment-continues", "run-of-k-full", "run-ends-at-burst-end", "head-advances-h", "queue-emptied", "nothing-sent"]
           + [f"second-bearer-offered-{r}" for r in range(0, 10)]
           + ["arrival-on-tick", "arrival-ulp-late", "arrival-into-empty", "arrival-into-nonempty"])


# ---------------------------------------------------------------------------------------------------------------------------
# the plain model
# ---------------------------------------------------------------------------------------------------------------------------

class _Bearer:
    def __init__(self, kind, bursts):
        self.kind = kind
        t, nf, la = bursts if bursts is not None else ((), (), ())
        self.t, self.nf, self.la = [float(x) for x in t], [int(x) for x in nf], [int(x) for x in la]
        self.next = 0
        self.q = collections.deque()    # [size, time stamp, bytes sent, burst, last of its burst, TTIs it was sent in, last such TTI]
        self.bytes = 0
        self.done = np.full(len(self.t), -1, np.int32)
        self.emptied_in = -2

    def data(self):
        if self.kind == KIND["B"]:
            return BACKLOG
        return self.bytes + OVERHEAD * len(self.q) if self.q else 0

    def hol(self, now):
        if self.kind != KIND["Q"] or self.bytes == 0:
            return 0.0
        h = now - self.q[0][1]
        return h if h >= 0.00001 else 0.00001

    def arrive(self, n, ticks, ev):
        now = ticks[n]
        while self.next < len(self.t) and self.t[self.next] <= now:
            i, ts = self.next, self.t[self.next]
            if ts == now:
                ev["arrival-on-tick"] += 1
            elif ts == math.nextafter(now, -math.inf):
                ev["arrival-ulp-early"] += 1
            elif n > 0 and ts == math.nextafter(ticks[n - 1], math.inf):
                ev["arrival-ulp-late"] += 1
            ev["arrival-into-nonempty" if self.q else "arrival-into-empty"] += 1
            if not self.q and self.emptied_in == n - 1:
                ev["arrival-right-after-emptied"] += 1
            sizes = [FULL] * self.nf[i] + ([self.la[i]] if self.la[i] > 0 else [])
            for j, s in enumerate(sizes):
                self.q.append([s, ts, 0, i, j == len(sizes) - 1, 0, -1])
                self.bytes += s
            self.next += 1

    def dequeue(self, room, n, ev, frag_ge=False, ignore_min_room=False):
        sent_any, heads = False, 0
        run, run_burst = 0, -1

        def end_run(at_burst_end, by):
            nonlocal run
            if run >= 2:
                ev["run-of-k-full"] += 1
                ev[f"run-capped-by-{by}"] += 1
                if at_burst_end:
                    ev["run-ends-at-burst-end"] += 1
            run = 0

        while room > 0 and self.q:
            if not ignore_min_room and OVERHEAD >= room:
                ev[f"whole-with-room-{room}" if sent_any else "nothing-sent"] += 1
                break
            p = self.q[0]
            left = p[0] - p[2]
            if p[6] != n:
                p[5], p[6] = p[5] + 1, n
            if (left + OVERHEAD >= room) if frag_ge else (left + OVERHEAD > room):
                f = room - OVERHEAD
                p[2] += f
                self.bytes -= f
                room = 0
                ev[f"fragment-leaves-{left - f}"] += 1
                if f == 1:
                    ev["fragment-of-1-byte"] += 1
                if p[5] >= 3:
                    ev["fragment-continues"] += 1
                end_run(False, "grant")
                sent_any = True
                break
            if left + OVERHEAD == room:
                ev["whole-exact"] += 1
            if p[5] >= 3:
                ev["fragment-continues"] += 1
            room -= left + OVERHEAD
            self.bytes -= left
            self.q.popleft()
            sent_any = True
            if p[0] == FULL and (run == 0 or p[3] == run_burst):
                run, run_burst = run + 1, p[3]
            else:
                end_run(False, "burst")
                run, run_burst = (1, p[3]) if p[0] == FULL else (0, -1)
            if p[4]:
                self.done[p[3]] = n
                heads += 1
                end_run(p[0] == FULL, "burst")
        end_run(False, "grant")
        if heads >= 3:
            ev["head-advances-h"] += 1
        ev[f"heads-{heads}"] += 1
        if sent_any and not self.q:
            ev["queue-emptied"] += 1
            self.emptied_in = n


def plain_user(kinds, bursts, ticks, grants, per_flow=False, frag_ge=False, ignore_min_room=False, events=None):
    """One user.  kinds: two letters of 'BQ-' (bearer 0, bearer 1; the index is the priority).  bursts: {bearer: (time, n_full, last)}.
    grants [T]: (bytes, PRBs) of the user, or with per_flow (scheduler 1) ((bytes, PRBs) of bearer 0, of bearer 1).
    Returns dict: credited, rbs, queue_bytes, queue_packets [T][2] (after the TTI), hol [T][2] (before the dequeue, in the rows that
    credit something), done {bearer: completion TTI per burst}; events (a Counter) collects the edges taken."""
    ev = events if events is not None else collections.Counter()
    T = len(ticks)
    br = [_Bearer(KIND[kinds[b]], bursts.get(b)) for b in range(2)]
    out = {k: np.zeros((T, 2), np.int64) for k in ("credited", "rbs", "queue_bytes", "queue_packets")}
    out["hol"] = np.zeros((T, 2), np.float64)
    kw = dict(frag_ge=frag_ge, ignore_min_room=ignore_min_room)
    for n in range(T):
        now = float(ticks[n])
        for b in br:
            if b.kind == KIND["Q"]:
                b.arrive(n, ticks, ev)
        data = [b.data() for b in br]

        def credit(i, amount, nprb):
            out["credited"][n, i], out["rbs"][n, i], out["hol"][n, i] = amount, nprb, br[i].hol(now)
            if br[i].kind == KIND["Q"]:
                br[i].dequeue(amount, n, ev, **kw)

        if per_flow:
            for i in (0, 1):
                if grants[n][i][0] > 0:
                    credit(i, grants[n][i][0], grants[n][i][1])
        elif grants[n][0] > 0:
            room, nprb = grants[n]
            for i in (1, 0):
                if i == 0 and data[0] > 0 and data[1] > 0:
                    ev[f"second-bearer-offered-{room}"] += 1
                if room <= 0:
                    break
                if data[i] > 0:
                    sent = min(room, data[i])
                    room -= sent
                    credit(i, sent, nprb)
        for i in (0, 1):
            out["queue_bytes"][n, i], out["queue_packets"][n, i] = br[i].bytes, len(br[i].q)
    out["done"] = {b: br[b].done for b in range(2) if b in bursts}
    return out


# the two gates (tbs_bits(mcs, prbs) and cqi_to_mcs[cqi - 1] are the oracle's link tables)

def required_prbs(data_bytes, wide_cqi, tbs_bits, cqi_to_mcs):
    """Scheduler 7 (packet-scheduler.cpp:319-334): the user competes for an RBG while it holds fewer PRBs than its first bearer's data
    in bits divided (integer) by the one-PRB transport block of its wideband CQI."""
    return (data_bytes * 8) // tbs_bits(int(cqi_to_mcs[wide_cqi - 1]), 1)


def block_carries(n_rbgs, rbg_size, final_cqi, data_bytes, tbs_bits, cqi_to_mcs):
    """Scheduler 1 (downlink-packet-scheduler.cpp:253-265): the flow leaves the TTI's competition once the transport block of the PRBs
    it holds is at least its data in bits."""
    return tbs_bits(int(cqi_to_mcs[final_cqi - 1]), n_rbgs * rbg_size) >= data_bytes * 8


def rbgs_until_left(data_bytes, sched, R, G, cqi, tbs_bits, cqi_to_mcs):
    """How many RBGs a user (scheduler 7: cqi = wideband) / flow (scheduler 1: cqi = final) that wins every race takes."""
    if sched == 7:
        need = required_prbs(data_bytes, cqi, tbs_bits, cqi_to_mcs)
        return min(R, -(-need // G))
    return next((k for k in range(1, R + 1) if block_carries(k, G, cqi, data_bytes, tbs_bits, cqi_to_mcs)), R)


# ---------------------------------------------------------------------------------------------------------------------------
# populations
# ---------------------------------------------------------------------------------------------------------------------------

@dataclass
class Population:
    name: str
    sched: int
    ues: list
    R: int
    G: int
    kinds: list              # per user: two letters
    n_ttis: int
    cqi: np.ndarray          # [cells][U]: uniform over RBGs and TTIs
    bursts: dict             # {(cell, user, bearer): (time f64[n], n_full i32[n], last i32[n])}
    alpha: list = None
    beta: list = None
    plan: list = field(default_factory=list)   # per cell: what was planted (for the messages; the tests measure)

    @property
    def n_cells(self):
        return self.cqi.shape[0]

    @property
    def n_users(self):
        return int(sum(self.ues))

    def kind_codes(self):
        return np.array([[KIND[k[0]], KIND[k[1]]] for k in self.kinds], np.uint8)

    def grids(self):
        e = (self.n_ttis + 39) // 40
        return np.ascontiguousarray(np.broadcast_to(self.cqi[:, None, :, None], (self.n_cells, e, self.n_users, self.R)), np.uint8)

    def seeds(self):
        return np.arange(self.n_cells, dtype=np.uint32) + SEED0


def _burst_arrays(items):
    """[(time, n_full, last)] -> the three arrays"""
    return (np.array([i[0] for i in items], np.float64), np.array([i[1] for i in items], np.int32), np.array([i[2] for i in items], np.int32))


def shapes_for_data(data):
    """[(n_full, last)] whose bytes + 8 per packet are `data` (>= 9): one burst, or two where the rest after the full packets is 1..8."""
    assert data > OVERHEAD
    nf, rem = divmod(data, FULL + OVERHEAD)
    if rem == 0:
        return [(nf, 0)]
    if rem > OVERHEAD:
        return [(nf, rem - OVERHEAD)]
    rest = rem + FULL + OVERHEAD - 2 * OVERHEAD   # one full packet less, its bytes and the rest in two packets
    return ([(nf - 1, 700)] if nf > 1 else [(0, 700)]) + [(0, rest - 700)]


def backlogged_grant(oracle, sched, ues, R, G, cqi_row):
    """(bytes, final CQI) per user of one TTI of the cell with every user backlogged: the grant as the oracle's link adaptation gives it."""
    cell = oracle.Cell(ues, R, G, sched)
    U = int(sum(ues))
    cell.enable_queues(np.array([[KIND["B"], KIND["-"]]] * U, np.uint8))
    cell.set_cqi(np.broadcast_to(np.asarray(cqi_row, np.uint8)[:, None], (U, R)))
    out = cell.new_out()
    assert cell.step_queues(float(oracle.clock_ticks(100, 1)[0]), oracle.Rng(SEED0), out) == 0
    return out.user_tbs_bits // 8, out.user_final_cqi.copy()


def fit_family(oracle):
    """1 x 1, 6 RBGs of 2 PRBs, 'Q-': a first packet of B - 8 + d bytes, d = -9 .. 9, and a full packet queued behind it."""
    t0 = float(oracle.clock_ticks(100, 1)[0])
    cqis, bursts, plan = [], {}, []
    for cqi in (1, 9, 15):
        B = int(backlogged_grant(oracle, 9, [1], 6, 2, [cqi])[0][0])
        for d in range(-9, 10):
            c = len(cqis)
            cqis.append([cqi])
            bursts[(c, 0, 0)] = _burst_arrays([(t0, 0, B - 8 + d), (t0, 1, 0)])
            plan.append(dict(B=B, d=d))
    return Population("fit", 9, [1], 6, 2, ["Q-"], 48, np.array(cqis, np.uint8), bursts, plan=plan)


def runs_family(oracle):
    """1 x 1, 25 RBGs of 4 PRBs, 'Q-': bursts of k full packets and a last one around what one grant carries, alone and with a burst behind."""
    t0 = float(oracle.clock_ticks(100, 1)[0])
    cqis, bursts, plan = [], {}, []
    for cqi in (15, 9):
        B = int(backlogged_grant(oracle, 9, [1], 25, 4, [cqi])[0][0])
        K = B // (FULL + OVERHEAD)
        shapes = [(k, last) for k in (K - 1, K, K + 1) if k >= 1 for last in (0, 1, FULL)]
        for d in (-1, 0, 1):
            k = K if B + d - OVERHEAD - K * (FULL + OVERHEAD) >= 1 else K - 1
            shapes.append((k, B + d - OVERHEAD - k * (FULL + OVERHEAD)))
        for k, last in shapes:
            assert k >= 0 and 0 <= last <= FULL and k + last > 0
            for behind in (False, True):
                c = len(cqis)
                cqis.append([cqi])
                bursts[(c, 0, 0)] = _burst_arrays([(t0, k, last)] + ([(t0, 2, 100)] if behind else []))
                plan.append(dict(B=B, K=K, shape=(k, last), behind=behind))
    return Population("runs", 9, [1], 25, 4, ["Q-"], 6, np.array(cqis, np.uint8), bursts, plan=plan)


def _sizes_filling(total, n, seed):
    """n packet sizes in 1 .. 40, the first of them 1, whose bytes + 8 each are `total`"""
    rng = np.random.default_rng(seed)
    s = [1] + [int(x) for x in rng.integers(1, 41, n - 1)]
    i = 1
    while sum(s) + OVERHEAD * n != total:
        step = 1 if sum(s) + OVERHEAD * n < total else -1
        if 1 <= s[i] + step <= 40:
            s[i] += step
        i = 1 + i % (n - 1)
    return s


def many_heads_family(oracle):
    """1 x 1, 6 x 2, 'Q-': 30 bursts of one packet of 1 .. 40 bytes; the first 12 leave room of exactly 8 (stop) or 9 (a one-byte
    fragment) in the first grant; all in one TTI, or 15 in each of two consecutive TTIs."""
    ticks = oracle.clock_ticks(100, 2)
    B = int(backlogged_grant(oracle, 9, [1], 6, 2, [9])[0][0])
    cqis, bursts, plan = [], {}, []
    for room in (8, 9):
        for spread in (False, True):
            sizes = _sizes_filling(B - room, 12, 10 + room) + [2 + (7 * j + room) % 39 for j in range(18)]
            c = len(cqis)
            cqis.append([9])
            bursts[(c, 0, 0)] = _burst_arrays([(float(ticks[1 if spread and j >= 15 else 0]), 0, s) for j, s in enumerate(sizes)])
            plan.append(dict(B=B, room=room, spread=spread))
    return Population("many-heads", 9, [1], 6, 2, ["Q-"], 8, np.array(cqis, np.uint8), bursts, plan=plan)


def instants_family(oracle):
    """2 slices x 1 user, 6 x 2, 'Q-' both, slice 1 with alpha = beta = 1 (its metric reads the head-of-line delay): burst times on a
    tick, one ulp above and below; two bursts with one time stamp; arrivals right after the queue emptied and into a queue that is
    not empty; a stretch without any data in the cell (no rand() drawn), then a return."""
    T = 24
    tk = [float(x) for x in oracle.clock_ticks(100, T)]
    up, dn = (lambda x: math.nextafter(x, math.inf)), (lambda x: math.nextafter(x, -math.inf))
    cells = [
        # on the tick, an ulp late, an ulp early; user 1 the same a TTI later
        {0: [(tk[0], 0, 300), (up(tk[2]), 0, 300), (dn(tk[5]), 0, 300), (tk[9], 1, 0)],
         1: [(tk[1], 0, 200), (up(tk[3]), 0, 200), (dn(tk[6]), 0, 200)]},
        # two bursts with one time stamp; a large burst, and arrivals while it drains (into a queue that is not empty)
        {0: [(tk[0], 0, 100), (tk[0], 0, 120), (tk[4], 3, 0), (tk[5], 0, 50), (up(tk[5]), 0, 60)],
         1: [(tk[2], 2, 7), (tk[2], 0, 1), (tk[3], 0, 9)]},
        # the queue empties in TTI k, a burst arrives in TTI k + 1 (one grant of 389 bytes or half of it carries 100 bytes)
        {0: [(tk[0], 0, 100), (tk[1], 0, 100), (tk[2], 0, 100), (up(tk[2]), 0, 100)],
         1: [(tk[0], 0, 40), (tk[1], 0, 40), (dn(tk[2]), 0, 40)]},
        # nobody has data in TTIs 3 .. 11, then both return; a second silence, one returns
        {0: [(tk[0], 0, 500), (tk[12], 0, 500), (tk[20], 0, 30)],
         1: [(tk[0], 0, 300), (up(tk[11]), 1, 1)]},
    ]
    bursts = {(c, u, 0): _burst_arrays(items) for c, cell in enumerate(cells) for u, items in cell.items()}
    return Population("instants", 9, [1, 1], 6, 2, ["Q-", "Q-"], T, np.full((len(cells), 2), 9, np.uint8), bursts,
                      alpha=[0, 1], beta=[0, 1], plan=[dict(cell=c) for c in range(len(cells))])


def split_family(oracle, kinds):
    """1 x 1, 6 x 2, kinds 'QQ', 'BQ' or 'QB': bearer 1's data is B + d, d = -9 .. 1, so bearer 0 is offered 0 .. 9 bytes."""
    t0 = float(oracle.clock_ticks(100, 1)[0])
    B = int(backlogged_grant(oracle, 9, [1], 6, 2, [9])[0][0])
    cqis, bursts, plan = [], {}, []
    for d in range(-9, 2):
        c = len(cqis)
        cqis.append([9])
        for b in (0, 1):
            if kinds[b] == "Q":
                items = [(t0, 0, B + d - OVERHEAD)] if b == 1 else [(t0, 0, 100), (t0, 0, 50)]
                if b == 1 and kinds[0] == "Q":
                    items.append((float(oracle.clock_ticks(100, 3)[2]), 0, 20))   # (bearer 1 returns while bearer 0 still drains)
                bursts[(c, 0, b)] = _burst_arrays(items)
        plan.append(dict(B=B, d=d))
    return Population(f"split-{kinds}", 9, [1], 6, 2, [kinds], 4, np.array(cqis, np.uint8), bursts, plan=plan)


def gate7_family(oracle, R, G):
    """Scheduler 7, one slice of two users ('Q-' and 'B-', equal CQI and averages: user 0 wins every race it is in): user 0's data
    `first` with first * 8 = m * tbs1(wide) + e, m in {G k - 1, G k, G k + 1}, k = 1 .. 3, e in {-8, 0, 8}."""
    t0 = float(oracle.clock_ticks(100, 1)[0])
    L, tab = oracle.lib(), oracle.tables()
    cqi = 9 if G == 2 else 15
    wide = oracle.final_cqi([cqi] * (R * G))
    tbs1 = L.rso_tbs_bits(int(tab["cqi_to_mcs"][wide - 1]), 1)
    assert tbs1 % 8 == 0 and tbs1 > 8
    cqis, bursts, plan = [], {}, []
    for k in (1, 2, 3):
        for dm in (-1, 0, 1):
            for e in (-8, 0, 8):
                m = G * k + dm
                first = (m * tbs1 + e) // 8
                c = len(cqis)
                cqis.append([cqi, cqi])
                bursts[(c, 0, 0)] = _burst_arrays([(t0, nf, la) for nf, la in shapes_for_data(first)])
                plan.append(dict(k=k, dm=dm, e=e, first=first, wide=wide))
    return Population(f"gate7-{R}x{G}", 7, [2], R, G, ["Q-", "B-"], 3, np.array(cqis, np.uint8), bursts, plan=plan)


def gate1_family(oracle):
    """Scheduler 1, one slice of two users ('QQ' and 'B-', 25 x 4, equal CQI and averages: the flows are served in order): a flow's
    data is TBS(k RBGs, final CQI) / 8 + d, k = 1 .. 3, d in {-1, 0, 1}; flow 0 holds case i, flow 1 case i + 4."""
    R, G, cqi = 25, 4, 9
    t0 = float(oracle.clock_ticks(100, 1)[0])
    L, tab = oracle.lib(), oracle.tables()
    fc = int(backlogged_grant(oracle, 1, [2], R, G, [cqi, cqi])[1][0])
    cases = [(k, d) for k in (1, 2, 3) for d in (-1, 0, 1)]
    cqis, bursts, plan = [], {}, []
    for i in range(len(cases)):
        c = len(cqis)
        cqis.append([cqi, cqi])
        mine = []
        for b in (0, 1):
            k, d = cases[(i + 4 * b) % len(cases)]
            tbs = L.rso_tbs_bits(int(tab["cqi_to_mcs"][fc - 1]), k * G)
            assert tbs % 8 == 0
            data = tbs // 8 + d
            bursts[(c, 0, b)] = _burst_arrays([(t0, nf, la) for nf, la in shapes_for_data(data)])
            mine.append(dict(k=k, d=d, data=data))
        plan.append(dict(flows=mine, final_cqi=fc))
    return Population("gate1-25x4", 1, [2], R, G, ["QQ", "B-"], 3, np.array(cqis, np.uint8), bursts, plan=plan)


FAMILY_CELLS = {"fit": 57, "runs": 48, "many-heads": 4, "instants": 4, "split-QQ": 11, "split-BQ": 11, "split-QB": 11,
                "gate7-6x2": 27, "gate7-25x4": 27, "gate1-25x4": 9}


def all_populations(oracle):
    return [fit_family(oracle), runs_family(oracle), many_heads_family(oracle), instants_family(oracle)] \
        + [split_family(oracle, k) for k in ("QQ", "BQ", "QB")] + [gate7_family(oracle, 6, 2), gate7_family(oracle, 25, 4), gate1_family(oracle)]


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle, stepped TTI by TTI, and the plain model on the oracle's grants
# ---------------------------------------------------------------------------------------------------------------------------

def oracle_run(oracle, pop):
    """Every cell of the population through rso_cell_step_queues.  Returns dict of arrays with a leading cell axis: maps [T][R], tbs,
    nprb, final_cqi [T][U], cum_bytes, cum_rbs, queue_bytes, queue_packets [T][U][2] (after the TTI), avg_rate [U][2], slice_state [S],
    bearer_bytes [T][U][2] (credited per TTI), bearer_hol [T][U][2] and done {(cell, user, bearer): (tti, time)}: the last three are
    what the oracle's per-TTI state implies, derived like tests/test_gpu_flow_log.py does."""
    T, U, R = pop.n_ttis, pop.n_users, pop.R
    ticks = oracle.clock_ticks(100, T)
    grids, seeds, kinds = pop.grids(), pop.seeds(), pop.kind_codes()
    keys = dict(maps=(T, R), tbs=(T, U), nprb=(T, U), final_cqi=(T, U), cum_bytes=(T, U, 2), cum_rbs=(T, U, 2), queue_bytes=(T, U, 2),
                queue_packets=(T, U, 2))
    res = {k: np.zeros((pop.n_cells,) + s, np.int64) for k, s in keys.items()}
    res["avg_rate"] = np.zeros((pop.n_cells, U, 2))
    res["slice_state"] = np.zeros((pop.n_cells, len(pop.ues)))
    for c in range(pop.n_cells):
        cell = oracle.Cell(pop.ues, R, pop.G, pop.sched, alpha=pop.alpha, beta=pop.beta)
        cell.enable_queues(kinds)
        for (cc, u, k), (t, nf, la) in pop.bursts.items():
            if cc == c:
                cell.set_arrivals(u, k, t, nf, la)
        rng, out = oracle.Rng(int(seeds[c])), cell.new_out()
        for n in range(T):
            if n % 40 == 0:
                cell.set_cqi(grids[c, n // 40])
            assert cell.step_queues(float(ticks[n]), rng, out) == 0
            st = cell.bearer_state()
            res["maps"][c, n], res["tbs"][c, n], res["nprb"][c, n] = out.rbg_to_user, out.user_tbs_bits, out.user_nprb
            res["final_cqi"][c, n] = out.user_final_cqi
            for k in ("cum_bytes", "cum_rbs", "queue_bytes", "queue_packets"):
                res[k][c, n] = st[k]
        res["avg_rate"][c], res["slice_state"][c] = cell.bearer_state()["avg_rate"], cell.state()["slice_state"]
    res["bearer_bytes"] = np.diff(np.concatenate([np.zeros_like(res["cum_bytes"][:, :1]), res["cum_bytes"]], axis=1), axis=1)
    res["bearer_hol"] = np.zeros((pop.n_cells, T, U, 2))
    res["done"] = {}
    for (c, u, k), (t, nf, la) in pop.bursts.items():
        pk = np.cumsum(np.asarray(nf, np.int64) + (np.asarray(la) > 0))
        n_arr = np.searchsorted(t, ticks, side="right")
        arrived = np.where(n_arr > 0, pk[np.maximum(n_arr - 1, 0)], 0)
        dequeued = arrived - res["queue_packets"][c, :, u, k]
        before = np.concatenate([[0], dequeued[:-1]])
        tti = np.searchsorted(dequeued, pk, side="left")
        tti = np.where(tti < T, tti, -1).astype(np.int32)
        res["done"][(c, u, k)] = (tti, np.where(tti >= 0, ticks[np.maximum(tti, 0)], -1.0))
        for n in np.flatnonzero(res["bearer_bytes"][c, :, u, k] > 0):
            if arrived[n] - before[n] > 0:
                hol = ticks[n] - t[int(np.searchsorted(pk, before[n], side="right"))]
                res["bearer_hol"][c, n, u, k] = hol if hol >= 0.00001 else 0.00001
    return res


def grants_of(oracle, pop, run, c, u):
    """The plain model's input: user u's grant per TTI from the oracle's allocation (scheduler 1: per flow, from the RBG map, the final
    CQI and the link tables)."""
    if pop.sched != 1:
        return [(int(run["tbs"][c, n, u]) // 8, int(run["nprb"][c, n, u])) for n in range(pop.n_ttis)]
    L, mcs = oracle.lib(), oracle.tables()["cqi_to_mcs"]
    out = []
    for n in range(pop.n_ttis):
        row = []
        for b in (0, 1):
            nprb = int((run["maps"][c, n] == 2 * u + b).sum()) * pop.G
            row.append((L.rso_tbs_bits(int(mcs[int(run["final_cqi"][c, n, u]) - 1]), nprb) // 8 if nprb else 0, nprb))
        out.append(tuple(row))
    return out


def plain_cell(oracle, pop, run, c, events=None, **variant):
    """[per user: plain_user's result] of cell c on the oracle's grants"""
    ticks = oracle.clock_ticks(100, pop.n_ttis)
    return [plain_user(pop.kinds[u], {k: v for (cc, uu, k), v in pop.bursts.items() if cc == c and uu == u}, ticks,
                       grants_of(oracle, pop, run, c, u), per_flow=pop.sched == 1, events=events, **variant) for u in range(pop.n_users)]


def disagreements(oracle, pop, run, **variant):
    """[(cell, user, what)] where the plain model (or a variant of it) and the stepped oracle differ; events of the run as second value"""
    ev = collections.Counter()
    ticks = oracle.clock_ticks(100, pop.n_ttis)
    bad = []
    for c in range(pop.n_cells):
        for u, m in enumerate(plain_cell(oracle, pop, run, c, events=ev, **variant)):
            checks = [("credited", m["credited"], run["bearer_bytes"][c, :, u]), ("cum_rbs", np.cumsum(m["rbs"], axis=0), run["cum_rbs"][c, :, u]),
                      ("queue_bytes", m["queue_bytes"], run["queue_bytes"][c, :, u]), ("queue_packets", m["queue_packets"], run["queue_packets"][c, :, u])]
            bad += [(c, u, what) for what, a, b in checks if not np.array_equal(a, b)]
            if m["hol"].tobytes() != run["bearer_hol"][c, :, u].tobytes():
                bad.append((c, u, "hol"))
            for k, tti in m["done"].items():
                want_tti, want_time = run["done"][(c, u, k)]
                if not np.array_equal(tti, want_tti) or np.where(tti >= 0, ticks[np.maximum(tti, 0)], -1.0).tobytes() != want_time.tobytes():
                    bad.append((c, u, f"done of bearer {k}"))
    return bad, ev
