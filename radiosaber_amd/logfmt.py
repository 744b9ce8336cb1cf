"""Log-compatible text output and the per-slice throughput reducer.

The reference's experiments are evaluated by parsing the simulator's output streams:

  stderr, one line per (TTI, transmitting bearer), DoStopSchedule
      (downlink-transport-scheduler.cpp:192-199, same in the NVS and PF schedulers):
      "<ts> app: <A> cumu_bytes: <B> cumu_rbs: <K> hol_delay: <H> user: <U> slice: <S>"
  stdout, per TTI, RBsAllocation (downlink-transport-scheduler.cpp:523-527, 631-649):
      "slice_id, target_rbs, quota_rbgs: (0, t, q) (1, t, q) ... "
      "<ts>"
      "User(<id>) allocated RBGS: <rbg>(<cqi>) ... final_cqi: <c>"

These helpers rebuild those lines from the per-TTI decision log of one cell (BatchScheduler.run_logged
or the oracle) so the reference's own scripts (NSDI23-radiosaber-experiments/*/plot_*.py) keep working,
and reimplement the reducer of plot_throughput.py:26-56.  InfiniteBuffer bearers have an empty MAC
queue, so hol_delay prints as 0 (src/flows/radio-bearer.cpp:281-289); app id == user id for the
one-bearer-per-UE backlogged configs.
"""
from typing import Iterable, List, Sequence

import numpy as np


def stderr_lines(tbs_bits, rbg_to_user, user_to_slice: Sequence[int], rbg_size: int, first_ts: int = 100,
                 cum_bytes0=None, cum_rbs0=None, nprb=None, pf_format: bool = False) -> List[str]:
    """tbs_bits [n_ttis][U], rbg_to_user [n_ttis][R] of ONE cell -> the reference's stderr lines.
    nprb [n_ttis][U] (run_logged's "nprb"): the per-user PRB counts, needed for UpperBound where several users hold one
    RBG; derived from rbg_to_user otherwise.  pf_format: the "flow:" line of the PF scheduler
    (downlink-packet-scheduler.cpp:140-145) instead of the "app: .. user: .. slice: .." line."""
    tbs_bits = np.asarray(tbs_bits)
    rbg_to_user = np.asarray(rbg_to_user)
    n_ttis, U = tbs_bits.shape
    cb = np.zeros(U, np.int64) if cum_bytes0 is None else np.array(cum_bytes0, np.int64)
    cr = np.zeros(U, np.int64) if cum_rbs0 is None else np.array(cum_rbs0, np.int64)
    out = []
    for n in range(n_ttis):
        prbs = np.asarray(nprb[n]) if nprb is not None else \
            np.bincount(rbg_to_user[n][rbg_to_user[n] >= 0], minlength=U) * rbg_size
        for u in np.flatnonzero(tbs_bits[n] // 8 > 0):
            cb[u] += min(int(tbs_bits[n, u]) // 8, 100000000)
            cr[u] += int(prbs[u])
            if pf_format:
                out.append(f"{first_ts + n} flow: {u} cumu_bytes: {cb[u]} cumu_rbs: {cr[u]} hol_delay: 0")
            else:
                out.append(f"{first_ts + n} app: {u} cumu_bytes: {cb[u]} cumu_rbs: {cr[u]} hol_delay: 0 "
                           f"user: {u} slice: {user_to_slice[u]}")
    return out


def run_record_lines(records, user_to_slice: Sequence[int], first_ts: int = 100, pf_format: bool = False) -> List[str]:
    """records[t]: the grant records of ONE cell's TTI t (GroupScheduler.run_counted_at(..., records=True)[1][k]: a sequence of
    arrays of api.GRANT_RECORD) -> the lines stderr_lines writes for the same run
    with the same starting counters.  A record carries the user's counters after the TTI's credit, so nothing is summed here; the
    records of a TTI come in DoStopSchedule's order.  user_to_slice is by user id; pf_format as in stderr_lines."""
    out = []
    for t, recs in enumerate(records):
        for r in recs:
            u, cb, cr = int(r["user_id"]), int(r["cum_bytes"]), int(r["cum_rbs"])
            if pf_format:
                out.append(f"{first_ts + t} flow: {u} cumu_bytes: {cb} cumu_rbs: {cr} hol_delay: 0")
            else:
                out.append(f"{first_ts + t} app: {u} cumu_bytes: {cb} cumu_rbs: {cr} hol_delay: 0 user: {u} slice: {user_to_slice[u]}")
    return out


def grant_record_lines(records, user_to_slice: Sequence[int], first_ts: int = 100, cum_bytes0=None, cum_rbs0=None,
                       pf_format: bool = False) -> List[str]:
    """records: the grant records of ONE cell (BatchScheduler.run_grant_records(...)[c], api.BATCH_GRANT_RECORD; the lists of
    consecutive launches concatenated) -> the lines stderr_lines writes for the same run.  A record's tti counts from the batch's first
    TTI, so first_ts is the time stamp of that TTI whichever launch the records come from.  The counters are summed here from the
    starting values (cum_bytes0 / cum_rbs0 [U]: BatchScheduler.state() before the first of these launches; None: zero), a record
    carries the TTI's credit alone.  The records come in DoStopSchedule's order.  pf_format as in stderr_lines."""
    records = np.asarray(records)
    U = len(user_to_slice)
    cb = np.zeros(U, np.int64) if cum_bytes0 is None else np.array(cum_bytes0, np.int64)
    cr = np.zeros(U, np.int64) if cum_rbs0 is None else np.array(cum_rbs0, np.int64)
    out = []
    for r in records:
        u, ts = int(r["user"]), first_ts + int(r["tti"])
        cb[u] += int(r["bytes"])
        cr[u] += int(r["nprb"])
        if pf_format:
            out.append(f"{ts} flow: {u} cumu_bytes: {cb[u]} cumu_rbs: {cr[u]} hol_delay: 0")
        else:
            out.append(f"{ts} app: {u} cumu_bytes: {cb[u]} cumu_rbs: {cr[u]} hol_delay: 0 user: {u} slice: {user_to_slice[u]}")
    return out


def _grant_record_dtype():
    from .api import BATCH_GRANT_RECORD  # (api imports nothing from here; the dtype has one home)
    return BATCH_GRANT_RECORD


def rows_from_grant_records(records, n_ttis: int, U: int, R: int, first_tti: int = 0, with_map: bool = True):
    """The dense rows of ONE cell's n_ttis TTIs from first_tti on, rebuilt from its grant records: dict(tbs_bits [n_ttis][U], uinfo
    [n_ttis][U] -- nprb | final_cqi << 16 | mcs << 24, run_logged's word -- and, with_map, rbg_to_user [n_ttis][R], -1 where no record
    has the RBG).  with_map=False for scheduler 10, where two users of different slices may hold one RBG and the map (the lowest
    slice's user) cannot be told from the masks."""
    records = np.asarray(records)
    tbs = np.zeros((n_ttis, U), np.int32)
    uinfo = np.zeros((n_ttis, U), np.int32)
    out = {"tbs_bits": tbs, "uinfo": uinfo}
    n = records["tti"].astype(np.int64) - first_tti
    u = records["user"].astype(np.int64)
    if len(records) and (n.min() < 0 or n.max() >= n_ttis or u.min() < 0 or u.max() >= U):
        raise ValueError("a grant record outside the asked TTIs or users")
    tbs[n, u] = records["tbs_bits"]
    uinfo[n, u] = records["nprb"].astype(np.int32) | (records["final_cqi"].astype(np.int32) << 16) | (records["mcs"].astype(np.int32) << 24)
    if with_map:
        m = np.full((n_ttis, R), -1, np.int16)
        bits = (records["rbg_mask"][:, None] >> np.arange(R, dtype=np.uint64)[None, :]) & np.uint64(1)
        k, r = np.nonzero(bits)
        m[n[k], r] = u[k]
        out["rbg_to_user"] = m
    return out


def grant_records_from_rows(tbs_bits, uinfo, rbg_to_user, first_tti: int = 0):
    """The inverse, host only: the grant records (api.BATCH_GRANT_RECORD, ascending in TTI, then in user) that a launch with these dense
    rows of ONE cell would return -- one per (TTI, user) with tbs_bits // 8 > 0, rbg_mask from rbg_to_user (None: masks of 0)."""
    tbs_bits, uinfo = np.asarray(tbs_bits), np.asarray(uinfo)
    n, u = np.nonzero(tbs_bits // 8 > 0)  # (row-major: TTI, then user)
    recs = np.zeros(len(n), _grant_record_dtype())
    recs["tti"] = n + first_tti
    recs["user"] = u
    recs["tbs_bits"] = tbs_bits[n, u]
    recs["bytes"] = np.minimum(tbs_bits[n, u] // 8, 100000000)
    w = uinfo[n, u].astype(np.int64)
    recs["nprb"] = w & 0xFFFF
    recs["final_cqi"] = (w >> 16) & 0xFF
    recs["mcs"] = (w >> 24) & 0xFF
    if rbg_to_user is not None:
        m = np.asarray(rbg_to_user)
        R = m.shape[1]
        weights = np.uint64(1) << np.arange(R, dtype=np.uint64)
        recs["rbg_mask"] = ((m[n] == u[:, None]).astype(np.uint64) * weights[None, :]).sum(axis=1, dtype=np.uint64)
    return recs


def stdout_lines(rbg_to_user, final_cqi, target, quota, cqi_of, first_ts: int = 100, transport: bool = True) -> List[str]:
    """The reference's allocation map.  cqi_of(n, user, rbg) -> CQI the user reported on that RBG."""
    rbg_to_user = np.asarray(rbg_to_user)
    n_ttis, R = rbg_to_user.shape
    out = []
    for n in range(n_ttis):
        if transport:
            out.append("slice_id, target_rbs, quota_rbgs: " +
                       "".join(f"({i}, {int(target[n][i])}, {int(quota[n][i])}) " for i in range(len(quota[n]))))
        out.append(str(first_ts + n))
        for u in np.unique(rbg_to_user[n][rbg_to_user[n] >= 0]):
            rb = np.flatnonzero(rbg_to_user[n] == u)
            out.append(f"User({u}) allocated RBGS:" + "".join(f" {r}({cqi_of(n, int(u), int(r))})" for r in rb) +
                       f" final_cqi: {int(final_cqi[n][u])}")
    return out


def _parse_counter_lines(lines: Iterable[str]):
    """The numeric columns of every counter line, looked up by their labels: a line is "<ts> app: <A> cumu_bytes: <B> cumu_rbs: <K>
    hol_delay: <H> user: <U> slice: <S>"; anything that does not start with a TTI stamp or lacks a label is not a counter line."""
    want = ("app:", "cumu_bytes:", "cumu_rbs:", "slice:")
    rows = []
    for line in lines:
        tok = line.split()
        if not tok or not tok[0].isdigit():
            continue
        try:
            rows.append([int(tok[0])] + [int(tok[tok.index(k) + 1]) for k in want])
        except (ValueError, IndexError):
            continue
    return np.asarray(rows, np.int64).reshape(-1, 1 + len(want))


def slice_throughput_from_log(lines: Iterable[str], n_users: int, n_slices: int, begin_ts: int = 0,
                              end_ts: int = 10000):
    """Per-slice throughput of one run's stderr, as the reference's evaluation defines it (what plot_throughput.py:26-56 computes):
    for every flow the LAST cumu_bytes / cumu_rbs it printed at a stamp in (begin_ts, end_ts], over end_ts milliseconds in seconds,
    summed over the flows of a slice; bytes as Mbit/s (x 8 / 1e6).  A flow that printed nothing in the window counts for nothing.
    Returns (mbps[n_slices], rbs_per_s[n_slices]).  The stamps of a log ascend, so "the last line" is the row with the largest index."""
    tab = _parse_counter_lines(lines)
    mbps, rbs = np.zeros(n_slices), np.zeros(n_slices)
    if tab.size:
        ts, flow = tab[:, 0], tab[:, 1]
        tab = tab[(ts > begin_ts) & (ts <= end_ts) & (flow >= 0) & (flow < n_users)]
    if tab.size:
        # the last row of each flow: first occurrence in the reversed table
        flows, first_rev = np.unique(tab[::-1, 1], return_index=True)
        last = tab[len(tab) - 1 - first_rev]
        seconds = end_ts / 1000
        np.add.at(mbps, last[:, 4], last[:, 2] / seconds)
        np.add.at(rbs, last[:, 4], last[:, 3] / seconds)
    return list(mbps * 8 / 1e6), list(rbs)


# ---- the queue model's per-bearer lines and the customised-slice experiment's outputs (exp-customization) ----
#
#   stderr, DoStopSchedule, one line per bearer credited with bytes (downlink-transport-scheduler.cpp:179-199,
#   dl-pf-packet-scheduler.cpp:77-96) -- the line above, with the bearer's own application id and GetHeadOfLinePacketDelay;
#   "ipflow start app: <A> flow: <F> flowsize: <Z>"                            (radio-bearer.cpp:335, MacQueue enqueue of a flow)
#   "ipflow end app: <A> flow: <F> fct: <T> flowsize: <Z> priority: <P>"      (um-rlc-entity.cpp:154-160, its last packet sent)


def fmt_double(x: float) -> str:
    """A double as std::ostream prints it by default (%g: 6 significant digits, e.g. 0.003, 1e-05, 0)."""
    return f"{float(x):g}"


def app_ids(slices) -> np.ndarray:
    """[U][2] application id of the bearer (user, priority), -1 = no bearer: the scenario's creation order
    (single-cell-with-interference.h:206, 308-440) -- one global counter from 0; per UE its video applications, then its backlogged
    flows, then InternetFlow j (priority j).  The bearer that SliceConfig.bearer_kinds() gives an application: InternetFlow j at
    priority j; else the first video application, else the first backlogged flow at priority 0.  No traffic section: one backlogged
    flow per UE, app id == user id."""
    U = slices.n_users
    out = np.full((U, 2), -1, np.int64)
    nxt = 0
    for u, s in enumerate(slices.user_to_slice):
        t = slices.traffic[s] if slices.traffic else {}
        n_vid, n_if = int(t.get("video_app", 0)), int(t.get("internet_flow", 0))
        n_bl = int(t.get("backlog_flow", 0)) if t else 1
        vid = list(range(nxt, nxt + n_vid))
        bl = list(range(nxt + n_vid, nxt + n_vid + n_bl))
        ipf = list(range(nxt + n_vid + n_bl, nxt + n_vid + n_bl + n_if))
        nxt += n_vid + n_bl + n_if
        if ipf:
            out[u, :len(ipf)] = ipf
        elif vid:
            out[u, 0] = vid[0]
        elif bl:
            out[u, 0] = bl[0]
    return out


def internet_flow_bearers(slices) -> np.ndarray:
    """[U][2] bool: the bearer carries an InternetFlow application (the ones that print ipflow lines; video bearers do not)."""
    out = np.zeros((slices.n_users, 2), bool)
    for u, s in enumerate(slices.user_to_slice):
        t = slices.traffic[s] if slices.traffic else {}
        out[u, :int(t.get("internet_flow", 0))] = True
    return out


def bearer_rows_from_users(tbs_bits):
    """The bearer rows of a batch without the queue model (one backlogged bearer per UE, priority 0): what DoStopSchedule credits,
    min(tbs / 8, 1e8) bytes, and hol_delay 0 (an InfiniteBuffer bearer has an empty MAC queue).  -> (bytes, hol) [n_ttis][U][2]."""
    tbs_bits = np.asarray(tbs_bits)
    by = np.zeros(tbs_bits.shape + (2,), np.int64)
    by[..., 0] = np.minimum(tbs_bits // 8, 100000000)
    return by, np.zeros(by.shape, np.float64)


def bearer_prbs(rbg_to_user, nprb, rbg_size: int, pf_flows: bool = False):
    """[n_ttis][U][2] PRBs that UpdateCumulateRBs adds to a bearer that transmitted: the user's PRB count (transport and NVS schedulers,
    downlink-transport-scheduler.cpp:189-191), or with DL_PF on flows (pf_flows: the queue model's scheduler 1, whose rbg_to_user
    holds flow ids 2 * user + priority) the flow's own PRBs (dl-pf-packet-scheduler.cpp:81)."""
    rbg_to_user = np.asarray(rbg_to_user)
    n = rbg_to_user.shape[0]
    if pf_flows:
        U = np.asarray(nprb).shape[1]
        out = np.zeros((n, U * 2), np.int64)
        for k in range(n):
            m = rbg_to_user[k]
            out[k] = np.bincount(m[m >= 0], minlength=U * 2)[:U * 2] * rbg_size
        return out.reshape(n, U, 2)
    p = np.asarray(nprb, np.int64)
    return np.repeat(p[:, :, None], 2, axis=2)


class BearerLogWriter:
    """The reference's stderr lines of one cell of a queue-model batch, launch after launch: the per-bearer counter lines of every
    scheduler (scheduler 1 included: DL_PF_PacketScheduler::DoStopSchedule prints the same "app: .. user: .. slice:" line) and the
    ipflow lines of the InternetFlow bearers.

    Within a TTI: first the "ipflow start" lines of the flows enqueued since the previous TTI (time in (t_{k-1}, t_k], by time, app,
    flow), then the users ascending, each user's bearers in the reference's loop order -- priority 1 before 0 (transport and NVS
    schedulers, downlink-transport-scheduler.cpp:179), 0 before 1 for DL_PF's FlowsToSchedule -- and right after a bearer's counter
    line the "ipflow end" lines of its flows whose last packet left in that TTI, in flow order.  A flow is numbered by its burst index
    on its bearer; flowsize = n_full * 1490 + last; fct = t_k - time in double.

    app_of [U][2] (app_ids), flows {(user, prio): (time, n_full, last)} of the InternetFlow bearers of this cell (set_arrivals'
    bursts), pf_flows: scheduler 1 (bearer order 0, 1).  Stamps are first_ts + the TTI's index in the batch.  flow_format: the
    base class's "<ts> flow: <A> cumu_bytes: .. cumu_rbs: .. hol_delay: .." line (downlink-packet-scheduler.cpp:140-145, what
    stderr_lines(pf_format=True) writes) instead of the "app: .. user: .. slice:" line."""

    def __init__(self, app_of, user_to_slice, pf_flows: bool = False, flows=None, first_ts: int = 100,
                 cum_bytes0=None, cum_rbs0=None, flow_format: bool = False):
        self.app_of = np.asarray(app_of)
        U = self.app_of.shape[0]
        self.u2s = np.asarray(user_to_slice)
        self.order = (0, 1) if pf_flows else (1, 0)
        self.first_ts = first_ts
        self.flow_format = flow_format
        self.cb = np.zeros((U, 2), np.int64) if cum_bytes0 is None else np.array(cum_bytes0, np.int64)
        self.cr = np.zeros((U, 2), np.int64) if cum_rbs0 is None else np.array(cum_rbs0, np.int64)
        self.tti = 0  # index in the batch of the next TTI
        self.flows = {}
        starts = []
        for (u, k), (t, nf, la) in (flows or {}).items():
            t, nf, la = np.asarray(t, np.float64), np.asarray(nf, np.int64), np.asarray(la, np.int64)
            self.flows[(u, k)] = (t, nf * 1490 + la)
            starts += [(float(t[i]), int(self.app_of[u, k]), i, u, k) for i in range(len(t))]
        starts.sort()
        self.starts = starts
        self.next_start = 0

    @staticmethod
    def counter_line(ts, app, cum_bytes, cum_rbs, hol, user, slice_id, flow_format: bool = False) -> str:
        """DoStopSchedule's line of one credited bearer, counters as they are after the credit."""
        line = (f"{ts} {'flow' if flow_format else 'app'}: {app} cumu_bytes: {cum_bytes} "
                f"cumu_rbs: {cum_rbs} hol_delay: {fmt_double(hol)}")
        return line if flow_format else f"{line} user: {user} slice: {slice_id}"

    def lines(self, bearer_bytes, bearer_hol, bearer_rbs, t_first: float, done=None) -> List[str]:
        """One launch: bearer_bytes / bearer_hol / bearer_rbs [n_ttis][U][2] (run_logged(bearers=True), bearer_prbs), t_first = the
        batch clock before the launch (BatchScheduler.clock()[0][cell]; t_{k+1} = t_k + 0.001), done = {(user, prio): (done_tti,
        done_time)} of this cell (BatchScheduler.flow_record())."""
        bearer_bytes = np.asarray(bearer_bytes)
        n = bearer_bytes.shape[0]
        credits = [{} for _ in range(n)]
        for j in range(n):
            for u in np.flatnonzero(bearer_bytes[j].any(1)):
                credits[j][int(u)] = {k: (int(bearer_bytes[j, u, k]), int(bearer_rbs[j, u, k]), bearer_hol[j, u, k])
                                      for k in (0, 1) if bearer_bytes[j, u, k] > 0}
        return self._launch_lines(credits, t_first, done)

    def record_lines(self, records, t_first: float, n_ttis: int, done=None) -> List[str]:
        """The same launch from its bearer records alone (BatchScheduler.run_records, one cell's BEARER_RECORD array): the lines
        lines() writes from the dense rows and the PRB counts of a logged launch of the same n_ttis TTIs.  t_first and done as there.
        A record's tti counts from the batch's first TTI, like this writer's; a TTI without a record still advances the clock and
        prints the ipflow start lines that fall into it."""
        g0 = self.tti
        credits = [{} for _ in range(n_ttis)]
        for r in np.asarray(records):
            j = int(r["tti"]) - g0
            if not 0 <= j < n_ttis:
                raise ValueError(f"record of TTI {int(r['tti'])} outside this launch's TTIs {g0} .. {g0 + n_ttis - 1}")
            credits[j].setdefault(int(r["user"]), {})[int(r["bearer"])] = (int(r["bytes"]), int(r["nprb"]), r["hol_delay"])
        return self._launch_lines(credits, t_first, done)

    def _launch_lines(self, credits, t_first: float, done) -> List[str]:
        """credits[j] = {user: {prio: (bytes, PRBs, hol_delay)}} of the launch's TTI j, credited bearers only."""
        n = len(credits)
        g0 = self.tti
        ends = {}
        for key, (dt, dtime) in (done or {}).items():
            if key not in self.flows:
                continue
            dt = np.asarray(dt)
            for i in np.flatnonzero((dt >= g0) & (dt < g0 + n)):
                ends.setdefault((int(dt[i]) - g0, key[0], key[1]), []).append((int(i), float(dtime[i])))
        out = []
        tk = t_first
        for j in range(n):
            if j:
                tk = tk + 0.001
            ts = self.first_ts + g0 + j
            while self.next_start < len(self.starts) and self.starts[self.next_start][0] <= tk:
                t, app, i, u, k = self.starts[self.next_start]
                out.append(f"ipflow start app: {app} flow: {i} flowsize: {int(self.flows[(u, k)][1][i])}")
                self.next_start += 1
            for u in sorted(credits[j]):
                for k in self.order:
                    if k in credits[j][u]:
                        by, rbs, hol = credits[j][u][k]
                        self.cb[u, k] += by
                        self.cr[u, k] += rbs
                        out.append(self.counter_line(ts, self.app_of[u, k], self.cb[u, k], self.cr[u, k], hol, u,
                                                     self.u2s[u], self.flow_format))
                    for i, dtime in sorted(ends.get((j, int(u), k), [])):
                        t, size = self.flows[(int(u), k)]
                        out.append(f"ipflow end app: {self.app_of[u, k]} flow: {i} fct: {fmt_double(dtime - t[i])} "
                                   f"flowsize: {int(size[i])} priority: {k}")
        self.tti = g0 + n
        return out


def counted_call_lines(ts: int, ids, sent, hol_delay, cum_bytes, cum_rbs, app_of, user_to_slice) -> List[str]:
    """The reference's "app:" lines of ONE cell's slot of a counted group call (GroupScheduler.schedule_tti_counted): one line per
    bearer the call credited, in DoStopSchedule's order -- users ascending by id, bearer 1 before 0 -- in BearerLogWriter's format.
    ts: the TTI's stamp; ids [n]: the call's user ids in call order (None: 0..n-1); sent [n][2]: the result's .sent; hol_delay: the
    bearers' GetHeadOfLinePacketDelay as the caller knows them, [n][2], or [n] (one value per position, printed for either bearer),
    or None (0: InfiniteBuffer bearers); cum_bytes / cum_rbs [U][2] by user id: the cell's counters AFTER the call, read back
    (get_counters) or tracked from .sent and user_nprb; app_of: app_ids(slices); user_to_slice: the slice map."""
    sent = np.asarray(sent).reshape(-1, 2)
    n = sent.shape[0]
    ids = np.arange(n) if ids is None else np.asarray(ids)
    assert ids.shape == (n,)
    hol = np.zeros((n, 2)) if hol_delay is None else np.asarray(hol_delay, np.float64)
    if hol.ndim == 1:
        hol = np.repeat(hol[:, None], 2, axis=1)
    assert hol.shape == (n, 2)
    cum_bytes, cum_rbs, app_of = np.asarray(cum_bytes), np.asarray(cum_rbs), np.asarray(app_of)
    out = []
    for i in np.argsort(ids, kind="stable"):
        u = int(ids[i])
        for k in (1, 0):
            if sent[i, k] > 0:
                out.append(BearerLogWriter.counter_line(ts, app_of[u, k], int(cum_bytes[u, k]), int(cum_rbs[u, k]), hol[i, k], u,
                                                        user_to_slice[u]))
    return out


def flows_call_lines(ts: int, ids, flow_bearer, tbs_bits, hol_delay, cum_bytes, cum_rbs, app_of, user_to_slice) -> List[str]:
    """The reference's "app:" lines of ONE cell's slot of a flows group call (GroupScheduler.schedule_tti_flows; scheduler 1,
    dl-pf-packet-scheduler.cpp:89-96): one line per flow the call credited -- a position whose block holds a byte,
    user_tbs_bits // 8 > 0 -- in FlowsToSchedule order, which is the call's: users ascending, bearer 0 before 1.
    ts: the TTI's stamp; ids [n]: the positions' user ids (None: 0..n-1); flow_bearer [n]: their bearer words; tbs_bits [n]: the
    result's user_tbs_bits; hol_delay [n]: the flows' GetHeadOfLinePacketDelay as the caller knows them, or None (0: InfiniteBuffer
    flows); cum_bytes / cum_rbs [U][2] by user id: the cell's counters AFTER the call (get_flows); app_of: app_ids(slices);
    user_to_slice: the slice map."""
    tbs_bits = np.asarray(tbs_bits).reshape(-1)
    n = tbs_bits.shape[0]
    ids = np.arange(n) if ids is None else np.asarray(ids)
    fb = np.asarray(flow_bearer).reshape(-1)
    hol = np.zeros(n) if hol_delay is None else np.asarray(hol_delay, np.float64)
    assert ids.shape == (n,) and fb.shape == (n,) and hol.shape == (n,)
    cum_bytes, cum_rbs, app_of = np.asarray(cum_bytes), np.asarray(cum_rbs), np.asarray(app_of)
    out = []
    for i in range(n):
        if int(tbs_bits[i]) // 8 > 0:
            u, k = int(ids[i]), int(fb[i])
            out.append(BearerLogWriter.counter_line(ts, app_of[u, k], int(cum_bytes[u, k]), int(cum_rbs[u, k]), hol[i], u, user_to_slice[u]))
    return out


# reducers of the customised-slice experiment (what exp-customization/plot_fctdelay.py computes from a run's stderr)
def _words(line: str):
    return line.split()


def fct_from_log(lines: Iterable[str], slice_begin: int, slice_end: int, priority_only: bool = False, ts_shoot: int = 10000):
    """Flow completion times (get_fct): an app's slice is the slice: field of its counter lines; flows of apps whose slice lies outside
    [slice_begin, slice_end] are skipped (apps without a counter line are kept).  A flow counts when its "ipflow start" line comes
    before the first counter line stamped after ts_shoot, and its fct is that of its "ipflow end" line; priority_only keeps end lines
    of non-zero priority only.  Returns the fcts in the order the flows started."""
    lines = list(lines)
    slice_of = {}
    for line in lines:
        w = _words(line)
        if w and w[0].isdigit():
            slice_of[int(w[2])] = int(w[12])
    captured = {}
    after = False
    for line in lines:
        w = _words(line)
        if not w:
            continue
        if w[0].isdigit() and int(w[0]) > ts_shoot:
            after = True
        if w[0] != "ipflow":
            continue
        app = int(w[3])
        if app in slice_of and not (slice_begin <= slice_of[app] <= slice_end):
            continue
        if w[1] == "start" and not after:
            captured[(app, int(w[5]))] = -1
        if w[1] == "end":
            if priority_only and int(w[11]) == 0:
                continue
            if (app, int(w[5])) in captured:
                captured[(app, int(w[5]))] = float(w[7])
    return [v for v in captured.values() if v != -1]


def hol_from_log(lines: Iterable[str], slice_begin: int, slice_end: int):
    """Head-of-line delays (get_hol): the hol_delay: of every counter line of a slice in [slice_begin, slice_end], in log order."""
    out = []
    for line in lines:
        w = _words(line)
        if w and w[0].isdigit() and slice_begin <= int(w[12]) <= slice_end:
            out.append(float(w[8]))
    return out


def slice_throughput_window(lines: Iterable[str], slice_begin: int, slice_end: int, begin_ts: int = 20000, end_ts: int = 22000):
    """Per-slice throughput (get_throughput) of the slices in [slice_begin, slice_end) -- end exclusive here: for every app the
    cumu_bytes of its last counter line stamped in (begin_ts, end_ts], over end_ts milliseconds, in Mbit/s, summed per slice in the
    order the apps first appear; lines after the first stamp beyond end_ts are not read."""
    per_app = {s: {} for s in range(slice_begin, slice_end)}
    for line in lines:
        w = _words(line)
        if not w or not w[0].isdigit():
            continue
        if int(w[0]) > end_ts:
            break
        if int(w[0]) > begin_ts:
            sid = int(w[12])
            if slice_begin <= sid < slice_end:
                per_app[sid][int(w[2])] = int(w[4]) / (end_ts / 1000) * 8 / (1000 * 1000)
    out = []
    for s in range(slice_begin, slice_end):
        acc = 0
        for v in per_app[s].values():
            acc += v
        out.append(acc)
    return out
