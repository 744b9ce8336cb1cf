"""What a batch's setters leave behind (gpu): a setter that REPLACES device arrays -- a CQI source by another of any kind, bearers and
arrival lists by later ones, per-cell rows by later rows -- leaves a batch that cannot be told from one that was given the last of
them only, and the checkpoint block keeps its bytes.  Host paths of rs_api.cpp (the batch's device memory, csrc/rs_devmem.h); the
kernels are the built-in ones (jit=False: the host paths are the same with run-time builds, which the rest of the suite runs).

The smallest shapes at which the arrays differ from each other: 3 cells, slices of 5 and 4 users (U = 9: the [R][Upad] image has a
padded tail and a partial group of 8), R = 5, G = 2 (a per-PRB twin differs from its grid), scheduler 9.

tests/golden/batch_checkpoints.npz holds two checkpoint blocks as the commit BEFORE the batch's buffers became owned ones wrote them:
the plain batch and the queue-model batch below, each after 12 TTIs.  Recording (only ever from a library whose checkpoints are known
to be right, on an MI355X):
    python tests/test_gpu_batch_memory.py tests/golden/batch_checkpoints.npz
A checkpoint carries every cell's scalar record verbatim, and the record's last 32 bytes are the last launch's first and last
instruction on the shader clock and on the 100 MHz clock (rs_batch_debug_clocks): no two launches share them -- two runs of one
library differ there -- so they are left out of the comparison (_without_clocks, as tests/test_gpu_batch_records.py does), and
nothing else is."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch  # noqa: F401  (before the product library first touches HIP: one HIP runtime serves both, and torch's must come first)

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
GOLDEN_FILE = ROOT / "tests" / "golden" / "batch_checkpoints.npz"

pytestmark = pytest.mark.gpu

CELLS, UES, R, G, SCHED, N_TTIS = 3, [5, 4], 5, 2, 9, 12
U, S = sum(UES), len(UES)
SEEDS = np.array([11, 12, 13], np.uint32)
SETTERS = ("upload", "upload_prb", "synthesize", "device", "trace", "trace_prb")
EPOCH_SETTERS = ("upload", "upload_prb", "synthesize", "device")
TWIN_MESSAGE = "the batch has a per-PRB twin of its grids, which a write would leave behind"


def _cqi(seed, shape):
    return np.random.default_rng(seed).integers(1, 16, size=shape, dtype=np.uint8)


def _source(kind, second):
    """The arguments of setter `kind` in its role: the first of a pair has 3 epochs (5 traces of 6 rows), the second 2 (4 of 4)."""
    E, traces, rows = (2, 4, 4) if second else (3, 5, 6)
    seed = 100 * SETTERS.index(kind) + (50 if second else 0)
    if kind in ("upload", "device"):
        return _cqi(seed, (CELLS, E, U, R))
    if kind == "upload_prb":
        return _cqi(seed, (CELLS, E, U, R * G))
    if kind == "synthesize":
        return seed, E
    user_trace = (np.arange(CELLS * U, dtype=np.int32).reshape(CELLS, U) * 3 + seed) % traces
    return _cqi(seed, (traces, rows, R * G if kind == "trace_prb" else R)), user_trace.astype(np.int32), rows


def _apply(b, kind, second):
    src = _source(kind, second)
    if kind == "upload":
        b.upload_cqi_epochs(src)
    elif kind == "upload_prb":
        b.upload_cqi_epochs_prb(src)
    elif kind == "synthesize":
        b.synthesize_cqi(*src)
    elif kind == "device":
        import torch
        b.set_cqi_epochs_device(torch.from_numpy(src).cuda())
    elif kind == "trace":
        b.set_trace(src[0], src[1], row_modulus=src[2])
    else:
        b.set_trace_prb(src[0], src[1], row_modulus=src[2])


def _batch(rs):
    # (cqi_refresh = 4 with wrap: 12 TTIs read three grids in turn, whichever epoch count the source has)
    b = rs.BatchScheduler(rs.SliceConfig(UES, weight=[0.6, 0.4]), R, G, CELLS, sched=SCHED, jit=False, cqi_refresh=4, cqi_epoch_wrap=True)
    b.seed(SEEDS)
    return b


def _logged_run(b):
    """12 logged TTIs and everything they leave, as bytes"""
    got = b.run_logged(N_TTIS)
    out = {k: got[k].tobytes() for k in ("rbg_to_user", "tbs_bits", "quota")}
    out.update({"state." + k: v.tobytes() for k, v in b.state().items()})
    t, last = b.clock()
    out["clock.t"], out["clock.last_update"] = t.tobytes(), last.tobytes()
    return out


def _grids(b):
    return np.stack([b.download_cqi_epochs(c) for c in range(CELLS)])


_alone = {}


def _second_alone(rs, kind):
    """batch B of a pair -- the second setter only --, computed once per setter and left unchanged: (its run, its grids or None)"""
    if kind not in _alone:
        b = _batch(rs)
        _apply(b, kind, True)
        grids = _grids(b) if kind in EPOCH_SETTERS else None
        _alone[kind] = (_logged_run(b), grids)
        b.close()
    return _alone[kind]


@pytest.mark.parametrize("second", SETTERS)
@pytest.mark.parametrize("first", SETTERS)
def test_replacing_a_cqi_source(rs, first, second):
    import torch
    want, want_grids = _second_alone(rs, second)
    a = _batch(rs)
    _apply(a, first, False)
    _apply(a, second, True)
    if second in EPOCH_SETTERS:
        grids = _grids(a)
        assert grids.shape == want_grids.shape and (grids == want_grids).all(), "download_cqi_epochs: not the second's grids"
        src = _source(second, True)
        if second in ("upload", "device"):
            assert (grids == src).all()
        elif second == "upload_prb":
            assert (grids == src[..., ::G]).all()  # (the first PRB of every RBG)
        # a write of epoch 0 with the values it holds: accepted unless the grids have a per-PRB twin
        t = torch.from_numpy(np.ascontiguousarray(grids[:, :1])).cuda()
        if second == "upload_prb":
            with pytest.raises(rs.RadioSaberError) as e:
                a.write_cqi_epochs_device(0, t)
            assert TWIN_MESSAGE in str(e.value)
        else:
            a.write_cqi_epochs_device(0, t)
    got = _logged_run(a)
    a.close()
    for k in want:
        assert got[k] == want[k], f"{first} then {second}: {k} differs from a batch given {second} only"


# ---- the queue model ----
KINDS_FIRST = np.array([[1, 0], [2, 0], [1, 2], [2, 2], [0, 2], [1, 0], [2, 1], [1, 2], [2, 0]], np.uint8)
KINDS_LAST = np.array([[2, 0], [1, 0], [2, 2], [1, 2], [1, 0], [0, 2], [1, 2], [2, 1], [1, 0]], np.uint8)


def _bursts(kinds, per_bearer, seed):
    """`per_bearer` bursts inside the 12 TTIs (the clock starts at 0.1 s) for every finite-queue bearer of `kinds`"""
    rng = np.random.default_rng(seed)
    out = {}
    for c in range(CELLS):
        for u in range(U):
            for k in range(2):
                if kinds[u, k] == 2 and per_bearer:
                    t = 0.1 + np.sort(rng.integers(0, 10, per_bearer)) * 0.001
                    out[(c, u, k)] = (t, rng.integers(0, 3, per_bearer).astype(np.int32), rng.integers(1, 1400, per_bearer).astype(np.int32))
    return out


ARRIVALS = {"longer": (4, 5), "shorter": (2, 6), "none": (0, 7)}


def _queue_batch(rs, kinds_seq, arrivals_seq):
    b = _batch(rs)
    b.upload_cqi_epochs(_source("upload", True))
    for kinds in kinds_seq:
        b.set_bearers(kinds)
    for name in arrivals_seq:
        b.set_arrivals(_bursts(kinds_seq[-1], *ARRIVALS[name]))
    return b


def _queue_run(b):
    b.run(N_TTIS)
    out = {"state." + k: v.tobytes() for k, v in b.state().items()}
    out.update({"bearers." + k: v.tobytes() for k, v in b.bearer_state().items()})
    rec = b.flow_record()
    out["flow_record.keys"] = sorted(rec)
    out["flow_record.bursts"] = b._n_bursts  # (the binding's own count, from the offsets it was given: not read from the library)
    for key in sorted(rec):
        out[f"flow_record.{key}"] = rec[key][0].tobytes() + rec[key][1].tobytes()
    return out


@pytest.mark.parametrize("lists", [("longer", "shorter", "none"), ("longer", "shorter")], ids=["ending-without-bursts", "ending-shorter"])
def test_replacing_bearers_and_arrivals(rs, lists):
    a = _queue_batch(rs, [KINDS_FIRST, KINDS_LAST], lists)
    b = _queue_batch(rs, [KINDS_LAST], lists[-1:])
    got, want = _queue_run(a), _queue_run(b)
    # the record is returned in the binding's slots of the LAST list (the library's own length shows in the contents compared below:
    # "ending-shorter" reads every entry of the shorter record; without bursts there is nothing to read)
    n_last = sum(len(v[0]) for v in _bursts(KINDS_LAST, *ARRIVALS[lists[-1]]).values())
    assert got["flow_record.bursts"] == n_last == want["flow_record.bursts"]
    if lists[-1] == "shorter":  # (the traffic arrived and was sent: the comparison is of something)
        assert any(np.frombuffer(v, np.int32, 2).max() >= 0 for k, v in want.items() if k.startswith("flow_record.("))
        assert np.frombuffer(want["bearers.queue_packets"], np.int32).any() or np.frombuffer(want["bearers.cum_bytes"], np.int64).any()
    a.close()
    b.close()
    for k in want:
        assert got[k] == want[k], f"{k} differs from a batch given the last bearers and the last arrival list only"


# ---- per-cell configurations ----
def test_replacing_cell_configs(rs):
    first = [rs.SliceConfig([5, 4], weight=[0.3, 0.7]), rs.SliceConfig([4, 5], weight=[0.5, 0.5]), rs.SliceConfig([3, 6], weight=[0.8, 0.2])]
    second = [rs.SliceConfig([4, 5], weight=[0.7, 0.3]), rs.SliceConfig([5, 2], weight=[0.4, 0.6]), rs.SliceConfig([6, 3], weight=[0.2, 0.8])]
    runs = []
    for seq in ((first, second), (second,)):
        b = _batch(rs)
        for configs in seq:
            b.set_cell_configs(configs)
        assert list(b.cell_users()) == [9, 7, 9]  # (the second's middle cell: an absent-user suffix)
        b.upload_cqi_epochs(_source("upload", True))
        runs.append(_logged_run(b))
        totals = b.slice_totals()
        runs[-1].update({"totals." + k: v.tobytes() for k, v in totals.items()})
        b.close()
    for k in runs[1]:
        assert runs[0][k] == runs[1][k], f"{k} differs from a batch given the second rows only"


# ---- the checkpoint's bytes ----
def _without_clocks(blob, queues):
    """The block without the four clock words of every cell's scalar record (the module's docstring); the layout is a 64-byte
    header, [cells][U] averages (8), pending grants (4), bytes and RBs (8 each), [cells][S] slice state (8), the 240-byte scalar records,
    then the queue model's parts: 7 + 2 + 4 words of 4 bytes per bearer, 1 + 8 bytes per user."""
    blob = bytearray(blob)
    scal = 64 + 28 * CELLS * U + 8 * CELLS * S
    assert len(blob) == scal + 240 * CELLS + (52 * 2 * CELLS * U + 9 * CELLS * U if queues else 0), "not the layout this helper masks"
    for c in range(CELLS):
        blob[scal + 240 * c + 208:scal + 240 * (c + 1)] = bytes(32)
    return bytes(blob)


def _plain(rs):
    b = _batch(rs)
    b.upload_cqi_epochs(_source("upload", True))
    return b


def _queued(rs):
    return _queue_batch(rs, [KINDS_FIRST, KINDS_LAST], ("longer", "shorter", "none"))


def _final(b, queues):
    out = {"state." + k: v.tobytes() for k, v in b.state().items()}
    if queues:
        out.update({"bearers." + k: v.tobytes() for k, v in b.bearer_state().items()})
    t, last = b.clock()
    out["clock.t"], out["clock.last_update"] = t.tobytes(), last.tobytes()
    return out


@pytest.mark.parametrize("which", ["plain", "queued"])
def test_checkpoint_bytes_are_the_recorded_ones(rs, which):
    queues, make = which == "queued", {"plain": _plain, "queued": _queued}[which]
    recorded = np.load(GOLDEN_FILE)[which].tobytes()
    a = make(rs)
    a.run(N_TTIS)
    blob = a.checkpoint()
    assert len(blob) == len(recorded)
    differ = [i for i in range(len(blob)) if blob[i] != recorded[i]]
    print(f"{which}: {len(blob)} bytes, {len(differ)} differ from the recording, at {differ[:4]} .. {differ[-4:]}")
    assert len(differ) <= 32 * CELLS, "more bytes differ than the cells have clock bytes"
    assert _without_clocks(blob, queues) == _without_clocks(recorded, queues), f"first difference at byte {differ[0] if differ else None}"
    a.run(8)
    want = _final(a, queues)
    a.close()
    b = make(rs)  # (the CQI source and the queue model's lists are configuration: set again on the batch that resumes)
    b.restore(recorded)
    b.run(8)
    got = _final(b, queues)
    b.close()
    for k in want:
        assert got[k] == want[k], f"{which}: {k} after restore + 8 TTIs differs from the uninterrupted 20"


if __name__ == "__main__":
    import radiosaber_amd
    blobs = {}
    for name, make_ in (("plain", _plain), ("queued", _queued)):
        batch = make_(radiosaber_amd)
        batch.run(N_TTIS)
        blobs[name] = np.frombuffer(batch.checkpoint(), np.uint8)
        batch.close()
    np.savez(sys.argv[1], **blobs)
    print({k: v.size for k, v in blobs.items()})
