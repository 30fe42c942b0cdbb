"""GPU: crr_checksum (the Load verify path) on states that no replay of the same buffers just wrote.

crr_checksum reads the five pending-ID lists from the live-ID sidecar (crr_outputs.live_ids) when it is set, and
from the rows otherwise.  Both paths are checked here -- the sidecar path is engine.checksum(db), the rows path the
same call with the sidecar pointers NULL -- against values that neither of them produced: the independent encoder
oracle/checksum_py over rows the CPU holds (result.allocate_host for uploaded states, engine.download for states in
HBM, the oracle's prefix replay for prefix states).  test_checksum_states.py checks those references against each
other and pins the counts stated below on the CPU.

The states: loaded rows uploaded from the host before any launch; a passive-replication state after setup, after a
step, after restore() and after a second step; and, in each, the workflows whose step ended in an error, which get
new counts but no sidecar slots.
"""
import ctypes

import numpy as np
import pytest

from cadence_amd import abi

import checksum_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


def both_paths(eng, db):
    """(crr_checksum reading the sidecar, crr_checksum reading the rows) for every workflow of ``db``."""
    import torch
    assert db.c_out.live_ids[0], "the batch keeps no sidecar"
    side = eng.checksum(db)
    co = abi.COutputs.from_buffer_copy(db.c_out)
    for t in range(len(abi.ID_TABLES)):
        co.live_ids[t] = None
    out = torch.zeros(max(db.n_wf, 1), dtype=torch.int32, device=eng.dev)
    s = torch.cuda.current_stream(eng.dev)
    assert eng.lib.crr_checksum(ctypes.byref(db.c_in), ctypes.byref(co), ctypes.c_void_p(out.data_ptr()),
                                ctypes.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize(eng.dev)
    return side, out.cpu().numpy().view(np.uint32)[:db.n_wf].copy()


def _equal(got, want, sel, what):
    bad = np.nonzero((got != want) & sel)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {int(sel.sum())} checksums differ, first positions {bad[:5]}"


def _both_equal(eng, db, want, sel, what):
    side, rows = both_paths(eng, db)
    _equal(rows, want, sel, what + ", rows path")
    _equal(side, want, sel, what + ", sidecar path")
    return side, rows


@pytest.mark.parametrize("kind,layout", [("mixed", "interleaved"), ("mixed", "canonical"), ("mixed", "lanes"),
                                         ("long", "interleaved")])
def test_uploaded_loaded_rows_before_any_launch_and_after_a_failing_step(eng, kind, layout):
    """engine.upload of a batch with loaded states, no launch: both paths give the independent encoder's value over
    the uploaded rows, which is the prefix replay's checksum, for every loaded workflow (positions mapped through
    the layout's perm).  Then the suffix is replayed: both paths give the encoder's value over the downloaded rows
    for every workflow that ended OK, and the sidecar path equals the rows path for every workflow of the batch,
    the failing ones included.

    mixed (600 histories, 605 workflows with new runs; the same in the three layouts): 582 loaded, 420 with a
    pending ID; the suffix changes the ID lists of 470 loaded workflows and 66 workflows fail in it, 57 of them
    loaded and 39 with a pending ID before it.  long (40 long-tail histories, 60 workflows): 50 loaded, 41 with a
    pending ID, 26 loaded ones in the wave tail (24 with a pending ID), none failing."""
    b, rows, want, loaded, prefix = cc.loaded_reference(kind, layout)
    pending = cc.has_pending(cc.id_lists(b, rows)) & loaded
    if kind == "mixed":
        assert loaded.sum() >= 500 and pending.sum() >= 350
    else:
        assert 0 < b.wave_begin < b.n_wf
        assert (loaded[b.wave_begin:]).sum() >= 10 and (pending[b.wave_begin:]).sum() >= 5
    assert (want[loaded] == prefix[loaded]).all()
    db = eng.upload(b)
    side, from_rows = _both_equal(eng, db, want, loaded, "uploaded rows")
    assert (side == from_rows).all()                    # the workflows that are not loaded: empty rows, both paths
    # the step: some workflows fail, and keep the sidecar slots of the state before
    eng.launch(db)
    after = eng.download(db)
    ok = after.exec["status"] == 0
    if kind == "mixed":
        assert (~ok).sum() >= 30 and (~ok & pending).sum() >= 10
    side, from_rows = _both_equal(eng, db, cc.expected_checksums(b, after), ok, "after the step")
    _equal(side, from_rows, np.ones(b.n_wf, bool), "after the step, sidecar path against rows path")


@pytest.mark.parametrize("kind", ["as_generated", "trimmed"])
def test_passive_replication_setup_step_restore_step(eng, kind):
    """PassiveReplication over 1500 histories cut before their last batch.  After setup() both paths give the
    encoder's value over the oracle's prefix replay (and over the downloaded prefix rows); after step() the value
    over the downloaded rows; after restore() the prefix's again; after a second step() the first step's.  After
    each step the sidecar path equals the rows path for every workflow, the failing ones included.

    as_generated (1511 workflows with new runs, 1500 split, 1460 of them with an OK prefix): the step changes the
    ID lists of 134 and 138 fail in it -- a generated history mostly ends in a closing decision, which touches no
    pending map (checksum_cases.passive_histories), so no seed reaches a third.  trimmed (1500 workflows, all
    split, 1463 with an OK prefix): 752 change, 81 fail.  A sidecar left by the step misstates the restored state
    only where the step overwrote a slot the prefix's list uses (checksum_cases.slots_overwritten): 15 workflows
    as generated, 76 trimmed -- the number of checksums the sidecar path gets wrong after restore() when the
    snapshot leaves the sidecar out."""
    import torch
    from cadence_amd.replication import PassiveReplication
    c = cc.passive_case(kind)
    pr = PassiveReplication(eng, c.batch)
    pr.setup()
    assert (pr.split == c.split).all() and (pr.prefix.exec["status"] == c.pre_r.exec["status"]).all()
    ok_pre = c.pre_r.exec["status"] == 0
    want_pre = cc.expected_checksums(c.pre_b, c.pre_r)
    assert (cc.expected_checksums(c.pre_b, pr.prefix)[ok_pre] == want_pre[ok_pre]).all()
    _both_equal(eng, pr.db, want_pre, ok_pre, "after setup")

    def step(what):
        pr.step()
        torch.cuda.synchronize(eng.dev)
        after = eng.download(pr.db)
        ok = (after.exec["status"] == 0) & ok_pre
        # the state after the step belongs to the step's descriptors (pr.db_new: the whole histories' tokens)
        want = cc.expected_checksums(pr.suffix, after)
        side, from_rows = _both_equal(eng, pr.db_new, want, ok, what)
        _equal(side, from_rows, np.ones(c.batch.n_wf, bool), what + ", sidecar path against rows path")
        return after, want, ok

    after, want_step, ok_step = step("after the step")
    sel = ok_pre & c.split
    lists_pre, lists_step = cc.id_lists(c.pre_b, pr.prefix), cc.id_lists(pr.suffix, after)
    changed = cc.lists_differ(lists_pre, lists_step) & sel
    overwritten = cc.slots_overwritten(lists_pre, lists_step) & sel      # where a stale sidecar shows after restore()
    failing = ~ok_step & sel
    assert failing.sum() >= 30
    if kind == "trimmed":
        assert 3 * changed.sum() >= c.split.sum() and overwritten.sum() >= 50
    else:
        assert changed.sum() >= 100 and overwritten.sum() >= 10
    pr.restore()
    torch.cuda.synchronize(eng.dev)
    _both_equal(eng, pr.db, want_pre, ok_pre, "after restore")
    again, want_again, ok_again = step("after the second step")
    assert (ok_again == ok_step).all() and (want_again[ok_step] == want_step[ok_step]).all()
    for f in ("status", "checksum", "payload_len"):
        assert (again.exec[f] == after.exec[f]).all(), f
