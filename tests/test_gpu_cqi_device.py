"""CQI epoch grids from device memory (gpu): rs_batch_set_cqi_epochs_device / rs_batch_write_cqi_epochs_device pack a torch tensor
[n_cells][E][U][R] into the kernels' image [R][Upad] with rs_pack_cqi_kernel on the batch's stream.  A batch fed this way must be
indistinguishable from one given the same values through upload_cqi_epochs: image bytes (padding and tail included), downloads, runs.

Shapes (U, R), the smallest at which each branch of the pack can go wrong: 1 x 1 a single byte; 7 x 25 U < 8, grids of 175 bytes, so
grid starts take every alignment; 8 x 25 no padding in a row; 9 x 25 Upad = 24; 33 x 33 odd R; 500 x 25 the 12 500-byte grid;
100 x 64 the shipped wide grid; 1000 x 64 the largest tile count.  3 cells and 5 epochs each; built-in kernels."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the product library first touches HIP: one HIP runtime serves both, and torch's must come first)

pytestmark = pytest.mark.gpu

N_CELLS, E, G = 3, 5, 2
SHAPES = [(1, 1), (7, 25), (8, 25), (9, 25), (33, 33), (500, 25), (100, 64), (1000, 64)]
RUN_SHAPES = [(7, 25), (500, 25), (100, 64)]
OFFSETS = (0, 1, 5, 15)
SEEDS = np.arange(N_CELLS, dtype=np.uint32) * 104729 + 20250101


def _upad(U):
    k = (U + 7) // 8
    return 8 * (k if k & 1 else k + 1)


def _slices(rs, U):
    S = min(3, U)
    return rs.SliceConfig([U // S + (1 if s < U % S else 0) for s in range(S)])


@functools.lru_cache(maxsize=None)
def _values(U, R, n_epochs=E, seed=0):
    v = np.random.default_rng(1000 * U + R + seed).integers(1, 16, (N_CELLS, n_epochs, U, R)).astype(np.uint8)
    v.setflags(write=False)
    return v


def _image(grid):
    """the stored form of one grid [U][R]: [R][Upad], zeros behind the last user and up to the next multiple of 16"""
    U, R = grid.shape
    img = np.zeros((_upad(U) * R + 15) // 16 * 16, np.uint8)
    img[:R * _upad(U)].reshape(R, _upad(U))[:, :U] = grid.T
    return img


def _view(values, offset):
    """the values as a device tensor that begins `offset` bytes into a larger one"""
    flat = torch.from_numpy(np.array(values, np.uint8)).reshape(-1)   # (a copy: the cached values are read-only)
    big = torch.full((flat.numel() + 16,), 99, dtype=torch.uint8, device="cuda")   # (99: a byte of the surroundings read as a value shows)
    big[offset:offset + flat.numel()] = flat.cuda()
    t = big[offset:offset + flat.numel()].view(values.shape)
    assert t.data_ptr() % 16 == offset and t.is_contiguous()
    return t


def _batch(rs, U, R, sched=1, wrap=True, refresh=2):
    b = rs.BatchScheduler(_slices(rs, U), R, G, N_CELLS, sched=sched, cqi_refresh=refresh, cqi_epoch_wrap=wrap)
    b.seed(SEEDS)
    return b


def _images(b, n_epochs=E):
    return [[b.debug_cqi_image(c, e) for e in range(n_epochs)] for c in range(N_CELLS)]


def _assert_same_state(a, b):
    sa, sb = a.state(), b.state()
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    assert sa["cum_bytes"].sum() > 0


_HOST = {}


def _host_twin(rs, U, R):
    """the batch uploaded from the host, its images and the expected ones: once per shape"""
    if (U, R) not in _HOST:
        b = _batch(rs, U, R)
        b.upload_cqi_epochs(_values(U, R))
        imgs = _images(b)
        for c in range(N_CELLS):
            for e in range(E):
                assert imgs[c][e].tobytes() == _image(_values(U, R)[c, e]).tobytes()
        _HOST[(U, R)] = imgs
        b.close()
    return _HOST[(U, R)]


@pytest.mark.parametrize("U,R", SHAPES)
def test_a_set_from_the_device_stores_what_an_upload_stores(rs, U, R):
    want = _host_twin(rs, U, R)
    b = _batch(rs, U, R)
    for off in OFFSETS:
        # (what the buffer held before must not show: the first round meets fresh memory, the later ones the round before)
        b.set_cqi_epochs_device(_view(_values(U, R), off))
        got = _images(b)
        for c in range(N_CELLS):
            for e in range(E):
                assert got[c][e].tobytes() == want[c][e].tobytes(), (off, c, e, np.flatnonzero(got[c][e] != want[c][e])[:8])
            np.testing.assert_array_equal(b.download_cqi_epochs(c), _values(U, R)[c])
        assert b.cqi_write_status() is None
    b.close()


@pytest.mark.parametrize("sched", [9, 1, 7])
@pytest.mark.parametrize("U,R", RUN_SHAPES)
def test_a_batch_set_from_the_device_runs_like_one_uploaded(rs, U, R, sched):
    host, dev = _batch(rs, U, R, sched), _batch(rs, U, R, sched)
    host.upload_cqi_epochs(_values(U, R))
    dev.set_cqi_epochs_device(_view(_values(U, R), 5))
    for b in (host, dev):
        b.run(2 * 2 * E)
    _assert_same_state(host, dev)
    host.close(), dev.close()


@pytest.mark.parametrize("U,R", [(9, 25), (100, 64)])
def test_the_ring(rs, U, R):
    """E = 4 with wrap and cqi_refresh = 2: run 4 TTIs, rewrite the two epochs just consumed -- sync and async in turn -- over 16
    epochs of values; the twin has no wrap and all 16 epochs from the host"""
    v = _values(U, R, 16, seed=7)
    twin = _batch(rs, U, R, sched=9, wrap=False)
    twin.upload_cqi_epochs(v)
    twin.run(32)
    ring = _batch(rs, U, R, sched=9, wrap=True)
    ring.set_cqi_epochs_device(_view(v[:, :4], 1))
    for step in range(8):
        ring.run_async(4)
        nxt = 2 * step + 4
        if nxt < 16:
            ring.write_cqi_epochs_device((2 * step) % 4, _view(v[:, nxt:nxt + 2], 1 + step), sync=step % 2 == 0)
    ring.sync()
    assert ring.cqi_write_status() is None
    _assert_same_state(twin, ring)
    # the ring now holds epochs 12..15 in places 0..3
    for c in range(N_CELLS):
        for e in range(4):
            assert ring.debug_cqi_image(c, e).tobytes() == _image(v[c, 12 + e]).tobytes()
    # a window across the end: epochs 3 and 0 with wrap, the others keep their bytes
    w = _values(U, R, 2, seed=8)
    ring.write_cqi_epochs_device(3, _view(w, 15))
    for c in range(N_CELLS):
        assert ring.debug_cqi_image(c, 3).tobytes() == _image(w[c, 0]).tobytes()
        assert ring.debug_cqi_image(c, 0).tobytes() == _image(w[c, 1]).tobytes()
        assert ring.debug_cqi_image(c, 1).tobytes() == _image(v[c, 13]).tobytes()
        assert ring.debug_cqi_image(c, 2).tobytes() == _image(v[c, 14]).tobytes()
    # a second write of other values into the same epochs: the padding stays zero (the expected image has it so)
    w2 = _values(U, R, 2, seed=9)
    ring.write_cqi_epochs_device(3, _view(w2, 5), sync=False)
    for c in range(N_CELLS):
        assert ring.debug_cqi_image(c, 3).tobytes() == _image(w2[c, 0]).tobytes()
        assert ring.debug_cqi_image(c, 0).tobytes() == _image(w2[c, 1]).tobytes()
    # ... and without wrap the same window is refused, with nothing written
    flat = _batch(rs, U, R, sched=9, wrap=False)
    flat.set_cqi_epochs_device(_view(v[:, :4], 0))
    with pytest.raises(rs.RadioSaberError) as err:
        flat.write_cqi_epochs_device(3, _view(w, 0))
    assert err.value.code == -5
    for c in range(N_CELLS):
        for e in range(4):
            assert flat.debug_cqi_image(c, e).tobytes() == _image(v[c, e]).tobytes()
    flat.write_cqi_epochs_device(2, _view(w, 0))  # epochs 2 and 3 end at the end
    assert flat.debug_cqi_image(1, 3).tobytes() == _image(w[1, 1]).tobytes()
    for b in (twin, ring, flat):
        b.close()


def _spoiled(U, R, places):
    v = _values(U, R).copy()
    flat = v.reshape(-1)
    for at, value in places.items():
        flat[at % flat.size] = value
    clamped = v.copy()
    clamped.reshape(-1)[[at % flat.size for at in places]] = 1
    return v, clamped


# byte -> value (negative: from the end); the view begins at byte 1 of its buffer, so bytes 0..2 are the unaligned head
BAD = [({0: 0, -1: 16}, (0, 0)), ({2: 16, -1: 0}, (2, 16)), ({-1: 16}, (-1, 16)), ({-1: 0, -40: 16}, (-40, 16))]


@pytest.mark.parametrize("places,first", BAD)
def test_values_outside_1_to_15(rs, places, first):
    U, R = 7, 25
    total = N_CELLS * E * U * R
    byte, value = first[0] % total, first[1]
    v, clamped = _spoiled(U, R, places)
    good = _view(_values(U, R), 1)
    b = _batch(rs, U, R, sched=9)
    # synchronous: the call names the lowest byte, and the batch is left without a source until a good call
    with pytest.raises(rs.RadioSaberError, match=f"CQI {value} at byte {byte} outside 1..15") as err:
        b.set_cqi_epochs_device(_view(v, 1))
    assert err.value.code == -1
    with pytest.raises(rs.RadioSaberError, match="no CQI source") as err:
        b.run(2)
    assert err.value.code == -4
    assert b.cqi_write_status() is None   # the failing call was the report
    b.set_cqi_epochs_device(good)
    b.run(2)
    with pytest.raises(rs.RadioSaberError, match=f"CQI {value} at byte {byte} outside 1..15"):
        b.write_cqi_epochs_device(0, _view(v, 1))
    with pytest.raises(rs.RadioSaberError, match="no CQI source"):
        b.run(2)
    b.set_cqi_epochs_device(good)
    # asynchronous: the values run as CQI 1 and the status names the byte; no launch sees the raw value
    b.write_cqi_epochs_device(0, _view(v, 1), sync=False)
    b.run(2)
    for c in range(N_CELLS):
        for e in range(E):
            assert b.debug_cqi_image(c, e).tobytes() == _image(clamped[c, e]).tobytes()
    assert b.cqi_write_status() == (byte, value)
    assert b.cqi_write_status() is None
    with pytest.raises(rs.RadioSaberError, match="no CQI source"):
        b.run(2)
    b.set_cqi_epochs_device(good)
    b.run(2)
    b.close()


def test_refusals_come_before_any_enqueue(rs):
    U, R = 9, 25
    L = rs.lib()
    grid = U * R
    v = _values(U, R)
    t = _view(v, 0)
    two = _view(v[:, :2], 0)
    err = lambda: L.rs_last_error().decode()
    b = _batch(rs, U, R, sched=9)
    # a write on a batch without a source
    assert L.rs_batch_write_cqi_epochs_device(b._h, 0, 2, two.data_ptr(), N_CELLS * 2 * grid, 0) == -4
    with pytest.raises(rs.RadioSaberError) as e:
        b.write_cqi_epochs_device(0, two)
    assert e.value.code == -4
    # d_bytes off by one, either way, in both calls
    for d in (-1, 1):
        assert L.rs_batch_set_cqi_epochs_device(b._h, t.data_ptr(), N_CELLS * E * grid + d, E) == -1 and "d_bytes" in err()
    with pytest.raises(rs.RadioSaberError, match="no CQI source"):
        b.run(2)   # nothing was stored
    b.set_cqi_epochs_device(t)
    before = _images(b)
    for d in (-1, 1):
        assert L.rs_batch_write_cqi_epochs_device(b._h, 0, 2, two.data_ptr(), N_CELLS * 2 * grid + d, 0) == -1 and "d_bytes" in err()
    assert L.rs_batch_write_cqi_epochs_device(b._h, 0, 0, two.data_ptr(), 0, 0) == -1
    assert L.rs_batch_write_cqi_epochs_device(b._h, 0, E + 1, two.data_ptr(), N_CELLS * (E + 1) * grid, 0) == -1
    assert L.rs_batch_write_cqi_epochs_device(b._h, E, 1, two.data_ptr(), N_CELLS * grid, 0) == -1
    assert L.rs_batch_write_cqi_epochs_device(b._h, -1, 1, two.data_ptr(), N_CELLS * grid, 0) == -1
    assert L.rs_batch_set_cqi_epochs_device(b._h, t.data_ptr(), 0, 0) == -1
    assert L.rs_batch_write_cqi_epochs_device(b._h, 0, 2, two.data_ptr(), N_CELLS * 2 * grid, 2) == -1   # an unknown flag
    # pinned host memory is refused by the attribute check, in words
    pinned = torch.from_numpy(np.array(v[:, :2])).pin_memory()
    assert pinned.is_pinned() and not pinned.is_cuda
    assert L.rs_batch_write_cqi_epochs_device(b._h, 0, 2, pinned.data_ptr(), N_CELLS * 2 * grid, 0) == -1
    assert "host memory" in err()
    assert L.rs_batch_set_cqi_epochs_device(b._h, pinned.data_ptr(), N_CELLS * 2 * grid, 2) == -1 and "host memory" in err()
    # in Python, before the C call
    strided = torch.ones((N_CELLS, E, U, 2 * R), dtype=torch.uint8, device="cuda")[..., ::2]
    assert tuple(strided.shape) == tuple(t.shape) and not strided.is_contiguous()
    for bad in (t.to(torch.int8), t[:, :, :, :R - 1], t[:2], t.permute(0, 1, 3, 2), strided, t.cpu(), pinned, v):
        with pytest.raises(ValueError):
            b.set_cqi_epochs_device(bad)
        with pytest.raises(ValueError):
            b.write_cqi_epochs_device(0, bad, sync=False)
    with pytest.raises(ValueError):
        b.write_cqi_epochs_device(0, t[:, :0])
    # none of this wrote a byte or dropped the source
    assert b.cqi_write_status() is None
    after = _images(b)
    assert all(after[c][e].tobytes() == before[c][e].tobytes() for c in range(N_CELLS) for e in range(E))
    b.run(2)
    # a batch with a per-PRB twin: a write would leave the twin behind
    p = _batch(rs, U, R, sched=9)
    p.upload_cqi_epochs_prb(np.repeat(v, G, axis=3))
    assert L.rs_batch_write_cqi_epochs_device(p._h, 0, 2, two.data_ptr(), N_CELLS * 2 * grid, 0) == -4 and "per-PRB" in err()
    p.set_cqi_epochs_device(t)   # the setter replaces both
    p.write_cqi_epochs_device(0, two)
    b.close(), p.close()


@pytest.mark.parametrize("sched", [9, 1])
def test_a_ragged_batch_set_from_the_device(rs, sched):
    """per-cell rows with absent users: their columns are stored and ignored, as with an upload"""
    U, R = 33, 33
    full = rs.SliceConfig([11, 11, 11])
    rows = [full, rs.SliceConfig([7, 9, 4]), rs.SliceConfig([1, 0, 0])]
    out = []
    for device in (False, True):
        b = rs.BatchScheduler(full, R, G, N_CELLS, sched=sched, cqi_refresh=2, cqi_epoch_wrap=True)
        b.set_cell_configs(rows)
        b.seed(SEEDS)
        if device:
            b.set_cqi_epochs_device(_view(_values(U, R), 5))
        else:
            b.upload_cqi_epochs(_values(U, R))
        b.run(20)
        out.append(b)
    assert list(out[1].cell_users()) == [33, 20, 1]
    _assert_same_state(*out)
    assert [x.tobytes() for row in _images(out[0]) for x in row] == [x.tobytes() for row in _images(out[1]) for x in row]
    for b in out:
        b.close()
