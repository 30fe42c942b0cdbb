"""The references test_gpu_checksum_states.py compares crr_checksum with, against each other on the CPU, and the
counts its cases rest on (so the GPU tests cannot pass on inputs that do not exercise what they are for).

The independent encoder (oracle/checksum_py) over the rows a host uploads for loaded states equals the oracle's
checksum of the prefix replay that produced them, for every loaded workflow and in every layout; the counts are
those the GPU tests' docstrings state.
"""
import numpy as np
import pytest

from cadence_amd import abi

import checksum_cases as cc


@pytest.mark.parametrize("layout", sorted(cc.LAYOUTS))
def test_encoder_over_uploaded_rows_equals_the_prefix_replay(layout):
    """600 histories: 582 loaded, 420 of them with a pending ID, in each layout."""
    b, rows, want, loaded, prefix = cc.loaded_reference("mixed", layout)
    assert loaded.sum() == 582
    assert (want[loaded] == prefix[loaded]).all()
    pending = cc.has_pending(cc.id_lists(b, rows))
    assert (pending & loaded).sum() == 420 and not (pending & ~loaded).any()
    # the rows a host uploads hold the loaded states and nothing else
    assert (rows.exec[~loaded] == np.zeros(1, abi.EXEC_ROW)).all()


def test_long_tail_case_reaches_the_wave_tail():
    """40 long-tail histories: 60 workflows, 50 loaded, 41 with a pending ID, 26 loaded ones in the wave tail."""
    b, rows, want, loaded, prefix = cc.loaded_reference("long", "interleaved")
    assert 0 < b.wave_begin < b.n_wf
    assert (want[loaded] == prefix[loaded]).all()
    pending = cc.has_pending(cc.id_lists(b, rows))
    in_tail = np.arange(b.n_wf) >= b.wave_begin
    assert (b.n_wf, int(loaded.sum()), int((pending & loaded).sum()), int((loaded & in_tail).sum())) == LONG_COUNTS


LONG_COUNTS = (60, 50, 41, 26)


def test_the_suffix_changes_id_lists_and_fails_some_workflows():
    """The step after the upload: the ID lists of 470 loaded workflows change, 426 of them in a step that ends OK;
    66 workflows of the batch end in an error, 57 of them loaded."""
    from oracle import oracle
    b, rows, _want, loaded, _prefix = cc.loaded_reference("mixed", "canonical")
    after = oracle.replay(b, 2)
    changed = cc.lists_differ(cc.id_lists(b, rows), cc.id_lists(b, after))
    ok = after.exec["status"] == 0
    assert ((changed & loaded).sum(), (changed & loaded & ok).sum()) == (470, 426)
    assert ((~ok).sum(), (~ok & loaded).sum()) == (66, 57)
    # the independent encoder agrees with the oracle's own checksum on every workflow that replayed OK
    assert (cc.expected_checksums(b, after)[ok] == after.exec["checksum"][ok]).all()


# (workflows, split, split with an OK prefix; of those: ID lists changed by the step, a slot of the prefix's
# lists overwritten by the step, failing in the step)
PASSIVE_COUNTS = {"as_generated": (1511, 1500, 1460, 134, 15, 138), "trimmed": (1500, 1500, 1463, 752, 76, 81)}


@pytest.mark.parametrize("kind", sorted(PASSIVE_COUNTS))
def test_passive_replication_case_counts(kind):
    """PassiveReplication's split replayed by the oracle: the counts test_gpu_checksum_states.test_passive_replication
    states, and the encoder against the oracle on the prefix state and on the state after the step."""
    c = cc.passive_case(kind)
    ok_pre = c.pre_r.exec["status"] == 0
    sel = ok_pre & c.split
    before, after = cc.id_lists(c.pre_b, c.pre_r), cc.id_lists(c.suf_b, c.suf_r)
    changed = cc.lists_differ(before, after) & sel
    overwritten = cc.slots_overwritten(before, after) & sel
    failing = (c.suf_r.exec["status"] != 0) & sel
    counts = (c.batch.n_wf, int(c.split.sum()), int(sel.sum()), int(changed.sum()), int(overwritten.sum()), int(failing.sum()))
    assert counts == PASSIVE_COUNTS[kind]
    assert failing.sum() >= 30
    if kind == "trimmed":
        assert 3 * changed.sum() >= c.split.sum() and overwritten.sum() >= 50
    assert (cc.expected_checksums(c.pre_b, c.pre_r)[ok_pre] == c.pre_r.exec["checksum"][ok_pre]).all()
    ok = sel & (c.suf_r.exec["status"] == 0)
    assert (cc.expected_checksums(c.suf_b, c.suf_r)[ok] == c.suf_r.exec["checksum"][ok]).all()
