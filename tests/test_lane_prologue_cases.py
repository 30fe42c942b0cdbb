"""CPU: the directed histories of tests/lane_prologue_cases.py do what they are named for.

The device tests compare with the oracle, so a perturbation that silently degenerated (an edit the flattener
drops, a step that is not a batch boundary) would pass there for the wrong reason.  Here the oracle alone must
give every kind its planned status at its planned step, leave the other workflows of the batch OK, and between
them the kinds must produce every status the prologue can return.
"""
import numpy as np
import pytest

from cadence_amd import abi
from cadence_amd.flatten import flatten, interleave
from cadence_amd.result import to_canonical_order

from lane_prologue_cases import (EVENTS, KINDS, KNOWN, RESUME_KINDS, SIZES, STATUSES, batch_of, perturbed_lanes,
                                 resume_histories, statuses)


def _oracle():
    from oracle import oracle
    return oracle


def test_one_perturbed_lane_in_every_wavefront():
    for n in SIZES:
        lanes = perturbed_lanes(n)
        assert len(lanes) == (n + 63) // 64 and sorted({w // 64 for w in lanes}) == list(range(len(lanes)))
        assert all(0 <= w < n for w in lanes)


@pytest.mark.parametrize("kind", list(KINDS))
def test_kind_gives_its_status_at_its_step(kind):
    c = KINDS[kind]
    canon, lanes = batch_of(kind, 65)
    for b in (canon, interleave(canon)):
        want = _oracle().replay(b, 0)
        st, fs = statuses(b, want)
        ex = to_canonical_order(b, want)
        assert (st[lanes] == int(c.status)).all(), (kind, st[lanes])
        if c.status != abi.Status.CAPACITY:   # the oracle reports an overflow after the replay, not at its step
            assert (fs[lanes] == c.fail_step).all(), (kind, fs[lanes])
        if c.vh_items is not None:
            assert (ex["n_vh_items"][lanes] == c.vh_items).all()
        others = np.setdiff1d(np.arange(65), lanes)
        assert (st[others] == 0).all() and (ex["n_vh_items"][others] == 1).all()


def test_every_prologue_status_occurs():
    seen = set()
    for kind in KINDS:
        canon, lanes = batch_of(kind, 1)
        st, _ = statuses(canon, _oracle().replay(canon, 0))
        seen.add(int(st[0]))
    assert STATUSES <= seen, STATUSES - seen
    assert 0 in seen   # growth with room, events after the close


def test_events_after_the_close_keep_the_previous_version():
    canon, lanes = batch_of("events after the close", 1)
    ex = _oracle().replay(canon, 0).exec
    last_version = int(canon.cols["version"][EVENTS - 1])
    assert ex["state"][0] == 2 and ex["n_vh_items"][0] == 2 and ex["signal_count"][0] == 6
    assert ex["current_version"][0] == last_version - 1


def test_resumed_kinds():
    pre, suf, plan, cut = resume_histories(129)
    assert len(plan) == 8 and {w // 64 for w in plan} == {0, 1}
    pre_b = flatten(pre, known_domains=KNOWN)
    pre_r = _oracle().replay(pre_b, 0)
    loaded = pre_r.to_loaded(pre_b)
    assert loaded.mask.all() and (loaded.exec["n_vh_items"] == 1).all()   # the suffix continues a history with an item
    suf_b = interleave(flatten(suf, known_domains=KNOWN, loaded=loaded))
    st, fs = statuses(suf_b, _oracle().replay(suf_b, 0))
    for w, kind in plan.items():
        want = int(RESUME_KINDS[kind][0])
        assert st[w] == want and fs[w] == (cut if want else -1), (w, kind, st[w], fs[w])
    others = np.setdiff1d(np.arange(129), list(plan))
    assert (st[others] == 0).all()
