"""A batch's table of run-time builds (`rs_api.cpp`: BatchBuilds): a trial launch names the kernel it runs, and one
reset starts every build over when the general build changes.  Two corners the table closed:

* the self-check of the lean build ran min(n, 256) TTIs and left the choice of kernel to the launch, which compares the TTI count with
  RS_JIT_LEAN_MIN_TTIS: above 256 the "lean" trial ran the general build and the lean build was marked verified without running;
* a batch prepared (and so checked) before rs_batch_set_bearers kept the mark of the check when the queue-model build, another code
  object, took the general build's place.

Both use the value-only fault injection -DRS_FAULT_INJECT_LEAN (one byte more per grant in the lean build; no address changes) or none."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UES, R, G, N_CELLS = [6, 5, 4], 13, 4, 2


def test_the_lean_build_is_checked_by_running_it(rs, oracle, monkeypatch):
    """RS_JIT_LEAN_MIN_TTIS above the self-check's 256-TTI trial: the 400-TTI launch wants the lean build, the trial must run THAT build
    -- which the injection makes wrong -- and drop it; the general build serves and the run ends where the oracle ends."""
    monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "300")
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_LEAN")
    b = rs.BatchScheduler(rs.SliceConfig(UES), R, G, N_CELLS, sched=9, jit=True, selfcheck=1)
    seeds = np.arange(N_CELLS, dtype=np.uint32) + 5
    b.seed(seeds)
    b.synthesize_cqi(11, 12)
    grids = [b.download_cqi_epochs(c) for c in range(N_CELLS)]
    b.run(30)
    assert b.jit_status()[0] == 1, b.jit_status()
    b.run(400)
    code, msg = b.jit_status()
    assert code == 1 and "lean build" in msg and "dropped" in msg, (code, msg)
    assert b.kernel_name == "rs_cell_kernel_jit"
    st = b.state()
    b.close()
    for c in range(N_CELLS):
        cell = oracle.Cell(UES, R, G, 9)
        cell.run_synth(grids[c], int(seeds[c]), 430, log=False)
        ost = cell.state()
        np.testing.assert_array_equal(st["cum_bytes"][c], ost["cum_bytes"])
        np.testing.assert_array_equal(st["cum_rbs"][c], ost["cum_rbs"])
        assert st["avg_rate"][c].tobytes() == ost["avg_rate"].tobytes()


def test_bearers_after_prepare_launch_get_their_build_checked(rs):
    """prepare_launch checks the general build while no TTI has run, so rs_batch_set_bearers is still allowed afterwards and replaces
    it by the queue-model build: that build is checked at the first launch (over ITS 32 TTIs, not the 64 of the earlier check), and the
    batch ends, byte for byte, where the same batch ends without the prepare_launch."""
    sc = rs.SliceConfig(UES)
    U = sc.n_users
    kinds = np.zeros((U, 2), np.uint8)
    kinds[:, 0] = rs.BEARER_QUEUE
    bursts = {}
    for c in range(N_CELLS):
        for u in range(U):
            k = np.arange(4)
            t = np.full(4, 0.1)
            for i in range(1, 4):  # (the applications' millisecond grid, by repeated addition)
                t[i] = t[i - 1] + (3 + (u + c) % 4) / 1000.0
            bursts[(c, u, 0)] = (t, ((k + u) % 3).astype(np.int32), (200 + 37 * u + 11 * k + c).astype(np.int32))

    def run(prepare):
        b = rs.BatchScheduler(sc, R, G, N_CELLS, sched=8, jit=True, selfcheck=1)
        b.seed(np.arange(N_CELLS, dtype=np.uint32) + 21)
        b.synthesize_cqi(13, 2)
        if prepare:
            b.prepare_launch(64)
        b.set_bearers(kinds)
        b.set_arrivals(bursts)
        b.run(32)
        out = (b.jit_status(), b.state(), b.bearer_state())
        b.close()
        return out

    (code, msg), st, bst = run(True)
    assert code == 1 and "selfcheck over 32 TTIs" in msg, (code, msg)
    _, st0, bst0 = run(False)
    for key in st0:
        assert st[key].tobytes() == st0[key].tobytes(), key
    for key in bst0:
        assert bst[key].tobytes() == bst0[key].tobytes(), key
    assert bst["cum_bytes"].sum() > 0
