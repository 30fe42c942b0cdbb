"""GPU: the lane loop's version-history prologue (replay_body) against the oracle, every exit of it.

The loop tests one predicate per event with a single ballot and runs the full checks only in a wavefront where
some lane misses it (tests/lane_prologue_cases.py).  Each batch is 1, 63, 64, 65 or 129 lockstep activity chains
on the 1-slot lane tier with one workflow of every wavefront perturbed, so the full checks run on a wavefront of
63 usual lanes and one unusual one.  Exec rows, version-history items, status and fail_step equal the oracle's
bit for bit.  A capacity error is the engine's own (the oracle reports an overflow after its replay, with no
failing step): there the failing workflow is compared with the oracle's replay of the events before the failing
one, and the other workflows with the oracle as usual.
"""
import numpy as np
import pytest

from cadence_amd import abi
from cadence_amd.flatten import flatten, interleave
from cadence_amd.result import ReplayResult, diff_results, to_canonical_order

from lane_prologue_cases import (EVENTS, KINDS, KNOWN, RESUME_KINDS, SIZES, batch_of, resume_histories, statuses)
from wave_walk_cases import _history, device_pos, truncated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


def _oracle():
    from oracle import oracle
    return oracle


def _replay(engine, batch):
    db = engine.upload(batch)
    engine.launch(db)
    return engine.download(db), db


def _in_small_tier(batch, db) -> bool:
    lanes = batch.n_wf if batch.wave_begin is None else batch.wave_begin
    seg = db.c_in.large_begin == lanes if batch.tiers is not None else True
    return bool(db.c_in.flags & abi.IN_LDS_SMALL) and lanes == batch.n_wf and seg


def _with_rows_of(got: ReplayResult, want: ReplayResult, batch, positions) -> ReplayResult:
    """``got`` with the exec row and table slots of the workflows at ``positions`` (device order) taken from ``want``."""
    out = ReplayResult(got.exec.copy(), {k: v.copy() for k, v in got.tables.items()})
    st = batch.wf_strides()
    for p in positions:
        out.exec[p] = want.exec[p]
        for name, _dt, base_f, cap_f, _n in abi.TABLES:
            if name == "tasks":   # no task emission: the table is not allocated
                continue
            idx = int(batch.wf[base_f][p]) + np.arange(int(batch.wf[cap_f][p])) * int(st[p])
            out.tables[name][idx] = want.tables[name][idx]
    return out


# what a failure at a step changes in the row of the events before it
FAILED_FIELDS = ("status", "fail_step", "flags", "checksum", "payload_len", "current_version", "src_next")


def _check_capacity_lanes(kind, ib, got, lanes):
    c = KINDS[kind]
    cut = [_history(truncated(c.build(w), c.fail_step), w) for w in lanes]
    cb = flatten(cut, known_domains=KNOWN)
    before = _oracle().replay(cb, 0)
    assert (before.exec["status"] == 0).all()
    ex = to_canonical_order(ib, got)
    for i, w in enumerate(lanes):
        for f in abi.EXEC_ROW.names:
            if f not in FAILED_FIELDS and f != "reserved":
                assert ex[f][w] == before.exec[f][i], (kind, w, f, ex[f][w], before.exec[f][i])
        assert ex["status"][w] == abi.Status.CAPACITY and ex["fail_step"][w] == c.fail_step
        assert ex["src_next"][w] == EVENTS and ex["checksum"][w] == 0 and ex["payload_len"][w] == 0
        assert not ex["flags"][w] & abi.EXEC_CHECKSUM_VALID
        # UpdateCurrentVersion precedes AddOrUpdateItem: the failing event's version
        assert ex["current_version"][w] == int(cb.cols["version"][0]) + 1
        assert ex["n_vh_items"][w] == c.vh_cap
    # the item the full history holds first, as the events before the failure left it
    p = device_pos(ib)[lanes]
    vh = got.tables["vh"][ib.wf["vh_base"][p].astype(np.int64)]
    assert (vh["event_id"] == before.tables["vh"][cb.wf["vh_base"]]["event_id"]).all()
    assert (vh["version"] == before.tables["vh"][cb.wf["vh_base"]]["version"]).all()


@pytest.mark.parametrize("kind", list(KINDS))
def test_prologue_exit(engine, kind):
    c = KINDS[kind]
    for n in SIZES:
        canon, lanes = batch_of(kind, n)
        ib = interleave(canon)
        pos = device_pos(ib)[lanes]
        assert sorted(int(p) // 64 for p in pos) == list(range((n + 63) // 64))   # one in every wavefront
        got, db = _replay(engine, ib)
        assert _in_small_tier(ib, db), (kind, n)
        want = _oracle().replay(ib, 0)
        st_w, fs_w = statuses(ib, want)
        assert (st_w[lanes] == int(c.status)).all(), (kind, n, st_w[lanes])   # the case did not degenerate
        st, fs = statuses(ib, got)
        print(kind, n, "status", st[lanes], "fail_step", fs[lanes], "oracle", st_w[lanes], fs_w[lanes])
        if c.status == abi.Status.CAPACITY:
            _check_capacity_lanes(kind, ib, got, lanes)
            got = _with_rows_of(got, want, ib, pos)
        d = diff_results(ib, got, ib, want)
        assert not d, f"{kind}, {n} workflows:\n" + "\n".join(d)
        others = np.setdiff1d(np.arange(n), lanes)
        assert (st[others] == 0).all() and (fs[others] == -1).all()
        if c.status != abi.Status.CAPACITY:
            assert (st[lanes] == int(c.status)).all() and (fs[lanes] == c.fail_step).all()
        # the canonical stride-1 layout of the same histories: the per-lane column addresses (general path)
        if n == 65 and c.vh_cap is None:
            got_c, _ = _replay(engine, canon)
            d = diff_results(ib, got, canon, got_c)
            assert not d, f"{kind}, canonical layout:\n" + "\n".join(d)


def test_lockstep_batch_without_perturbation(engine):
    """The batches' shape with every lane usual on every step but the first."""
    from wave_walk_cases import chain
    for n in SIZES:
        ib = interleave(flatten([_history(chain(w, 3), w) for w in range(n)], known_domains=KNOWN))
        got, db = _replay(engine, ib)
        assert _in_small_tier(ib, db)
        d = diff_results(ib, got, ib, _oracle().replay(ib, 0))
        assert not d, f"{n} workflows:\n" + "\n".join(d)
        assert (got.exec["status"] == 0).all() and (got.exec["n_vh_items"] == 1).all()


def test_resumed_from_a_loaded_state(engine):
    """The first event a call applies continues a loaded history (vh_n = 1 on entry): it is checked against the
    loaded last item, and a version change closes that item."""
    pre, suf, plan, cut = resume_histories(129)
    pre_b = interleave(flatten(pre, known_domains=KNOWN))
    pre_r = engine.replay(pre_b)
    d = diff_results(pre_b, pre_r, pre_b, _oracle().replay(pre_b, 0))
    assert not d, "\n".join(d)
    loaded = pre_r.to_loaded(pre_b)
    assert loaded.mask.all() and (loaded.exec["n_vh_items"] == 1).all()
    suf_b = interleave(flatten(suf, known_domains=KNOWN, loaded=loaded))
    got = engine.replay(suf_b)
    want = _oracle().replay(suf_b, 0)
    d = diff_results(suf_b, got, suf_b, want)
    assert not d, "\n".join(d)
    st, fs = statuses(suf_b, got)
    ex = to_canonical_order(suf_b, got)
    for w, kind in plan.items():
        status = int(RESUME_KINDS[kind][0])
        assert st[w] == status and fs[w] == (cut if status else -1), (w, kind, st[w], fs[w])
        assert ex["n_vh_items"][w] == (2 if kind == "growth" else 1)
    others = np.setdiff1d(np.arange(129), list(plan))
    assert (st[others] == 0).all() and (ex["n_vh_items"][others] == 1).all()
