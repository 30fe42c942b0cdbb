"""GPU: the lane loop's scalar column rows (WaveLaneSource, replay_lds) against the oracle.

The 1-slot and 2-slot LDS tiers address a step's columns as a scalar row pointer plus the thread's byte
offset: every lane still in the loop shares the step.  These cases put that under the shapes where it can
go wrong -- ragged event counts inside one wavefront (0..3-event histories beside a 41-event one, a
partial wavefront in a partial block), single lanes failing inside an otherwise lockstep wavefront, and
event types that are wave-uniform, then differ lane to lane (typed loads some lanes skip), then are uniform
again -- and compare every field with the oracle, bit for bit, in the interleaved layout and in the
canonical stride-1 layout (the per-lane address form of the general path).
"""
import random

import numpy as np
import pytest

from cadence_amd import abi
from cadence_amd.abi import EventType as ET
from cadence_amd.flatten import flatten, interleave
from cadence_amd.history import det_uuid
from cadence_amd.result import diff_results, to_canonical_order
from cadence_amd.synth_mixed import _Walk

from wave_walk_cases import KNOWN, _fail, _history, chain, truncated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


def _oracle():
    from oracle import oracle
    return oracle


def replay_with_flags(engine, batch):
    db = engine.upload(batch)
    engine.launch(db)
    return engine.download(db), db


def check(engine, batch):
    got, db = replay_with_flags(engine, batch)
    want = _oracle().replay(batch, 0)
    d = diff_results(batch, got, batch, want)
    assert not d, "\n".join(d)
    return got, db


def ran_in_small_tier(batch, db) -> bool:
    """Every workflow a lane of replay_lds_small_kernel: the flag bench.config2 reads, and (tiered batches) the
    1-slot segment covering all lanes."""
    lanes = batch.n_wf if batch.wave_begin is None else batch.wave_begin
    seg = db.c_in.large_begin == lanes if batch.tiers is not None else True
    return bool(db.c_in.flags & abi.IN_LDS_SMALL) and lanes == batch.n_wf and seg


def _ragged(engine, counts, seed):
    rng = random.Random(seed)
    counts = list(counts)
    rng.shuffle(counts)   # the canonical order is not the device order
    hs = [_history(truncated(chain(w, 6), n), w) for w, n in enumerate(counts)]
    canon = flatten(hs, known_domains=KNOWN)
    assert canon.n_wf == 209 and sorted(canon.wf["ev_count"]) == sorted(counts)
    ib = interleave(canon)
    got, db = check(engine, ib)
    assert ran_in_small_tier(ib, db)
    ex = to_canonical_order(ib, got)
    assert (ex["status"] == 0).sum() >= 209 - counts.count(0)   # a truncated chain is a valid open workflow
    # the same histories in the canonical stride-1 layout: the per-lane address form
    got_c, _ = check(engine, canon)
    d = diff_results(ib, got, canon, got_c)
    assert not d, "\n".join(d)
    return ib


def test_ragged_wave(engine):
    """209 workflows (three wavefronts plus 17 lanes, a partial wavefront in a partial block) whose event counts
    differ inside a wavefront (the s + 1 < n and s + 2 < n bounds of the loads).  The device order is longest
    first, so a wavefront holds the 41-event history beside 0-event ones only when fewer than 64 histories have
    events: the first batch is that one (41 .. 4, then four each of 3, 2, 1 and 0 events in the first wavefront,
    empty histories after it); the second fills every wavefront (41 .. 3 | 3, 2 | 2, 1, 0 | 0)."""
    long_part = [41] + [4 + (37 * i) // 46 for i in range(46, -1, -1)]
    assert len(long_part) == 48 and max(long_part) == 41 and min(long_part) == 4
    short = [3, 3, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1]
    ib = _ragged(engine, long_part + short + [0] * (209 - 60), 7)
    first = [int(c) for c in ib.wf["ev_count"][:64]]
    assert first[0] == 41 and first.count(3) == 4 and first.count(2) == 4 and first.count(1) == 4 and first.count(0) == 4
    ib = _ragged(engine, long_part + short + [0] * 4 + [3 - (i % 4) for i in range(209 - 64)], 8)
    per_wave = [set(int(c) for c in ib.wf["ev_count"][g:g + 64]) for g in range(0, 209, 64)]
    assert per_wave[1] == {3, 2} and per_wave[2] == {2, 1, 0} and per_wave[3] == {0}


def test_failures_inside_a_lockstep_wave(engine):
    """One wavefront of identical 23-event chains; single lanes fail at step 0, at a middle step and at the last
    step, each by another check.  The failing lanes' status, fail_step and partial state equal the oracle's
    (every field), and the other lanes' rows equal those of the wavefront with no failure at all."""
    n, last = 64, 22
    base = chain(0, 3)
    types = [e.event_type for b in base.batches for e in b]
    assert len(types) == last + 1
    started = types.index(int(ET.ActivityTaskStarted), 8)   # the second round's
    plan = {3: (0, "type"), 11: (started, "activity"), 17: (12, "id"), 18: (12, "version"),
            30: (13, "type"), 31: (last, "version"), 40: (last, "id"), 41: (last, "type"), 63: (7, "version")}
    clean = [chain(w, 3) for w in range(n)]
    dirty = [_fail(chain(w, 3), *plan[w]) if w in plan else chain(w, 3) for w in range(n)]
    cb = interleave(flatten([_history(k, w) for w, k in enumerate(clean)], known_domains=KNOWN))
    fb = interleave(flatten([_history(k, w) for w, k in enumerate(dirty)], known_domains=KNOWN))
    got_c, db_c = check(engine, cb)
    got_f, db_f = check(engine, fb)
    assert ran_in_small_tier(cb, db_c) and ran_in_small_tier(fb, db_f)
    ec, ef = to_canonical_order(cb, got_c), to_canonical_order(fb, got_f)
    assert (ec["status"] == 0).all()
    want_status = {"type": abi.Status.UNKNOWN_EVENT_TYPE, "version": abi.Status.VH_LOWER_VERSION,
                   "id": abi.Status.VH_EVENT_ID_NOT_INCREASING, "activity": abi.Status.MISSING_ACTIVITY_INFO}
    for w, (step, kind) in plan.items():
        assert ef["status"][w] == want_status[kind], (w, kind, ef["status"][w])
        assert ef["fail_step"][w] == step, (w, kind, ef["fail_step"][w])
    others = np.array([w for w in range(n) if w not in plan])
    for f in abi.EXEC_ROW.names:
        if f != "reserved":
            assert (ec[f][others] == ef[f][others]).all(), f


def _mixed_lane(w: int) -> _Walk:
    """Uniform types for four steps, a step where the lanes' types differ four ways (TimerStarted alone reads
    ref and key beside types that read neither), a lane-dependent external event, then uniform types again."""
    k = _Walk(random.Random(900001 + w), w, False, ["domain-a"])
    k.start()
    k.emit([k.start_decision()])
    done = k.ev(ET.DecisionTaskCompleted, scheduled_event_id=k.dec_sched, started_event_id=k.dec_started,
                binary_checksum="bin-0")
    sel = w % 4
    if sel == 0:
        out = k.ev(ET.TimerStarted, timer_id="t0", start_to_fire_timeout_seconds=100 + w)
    elif sel == 1:
        out = k.ev(ET.MarkerRecorded)
    elif sel == 2:
        out = k.ev(ET.UpsertWorkflowSearchAttributes)
    else:
        out = k.ev(ET.ActivityTaskScheduled, activity_id="0", domain="", schedule_to_start_timeout_seconds=60,
                   schedule_to_close_timeout_seconds=600, start_to_close_timeout_seconds=300,
                   heartbeat_timeout_seconds=0, retry_policy=None)
    k.emit([done, out])
    if sel == 0:
        ext = k.ev(ET.TimerFired, timer_id="t0")
    elif sel == 3:
        ext = k.ev(ET.ActivityTaskStarted, scheduled_event_id=out.id, request_id=det_uuid(w, "a", out.id))
    else:
        ext = k.ev(ET.WorkflowExecutionSignaled)
    k.emit([ext, k.sched_decision()])
    k.emit([k.start_decision()])
    k.emit([k.ev(ET.DecisionTaskCompleted, scheduled_event_id=k.dec_sched, started_event_id=k.dec_started,
                 binary_checksum="bin-0"), k.ev(ET.MarkerRecorded)])
    k.emit([k.ev(ET.WorkflowExecutionSignaled), k.sched_decision()])
    k.emit([k.start_decision()])
    return k


def test_uniform_then_divergent_types(engine):
    """One wavefront: steps 0-3 and 6-12 hold one type in every lane, steps 4-5 differ lane to lane.  At most one
    pending entry per map, so the 1-slot tier holds every lane."""
    ks = [_mixed_lane(w) for w in range(64)]
    types = np.array([[e.event_type for b in k.batches for e in b] for k in ks])
    assert types.shape == (64, 13)
    uniform = (types == types[0]).all(axis=0)
    assert uniform[:4].all() and not uniform[4] and not uniform[5] and uniform[6:].all()
    assert (types[0::4, 4] == ET.TimerStarted).all() and (types[1::4, 4] == ET.MarkerRecorded).all()
    canon = flatten([_history(k, w) for w, k in enumerate(ks)], known_domains=KNOWN)
    ib = interleave(canon)
    got, db = check(engine, ib)
    assert ran_in_small_tier(ib, db)
    ex = to_canonical_order(ib, got)
    assert (ex["status"] == 0).all()
    assert (ex["n_timer"][0::4] == 0).all() and (ex["n_activity"][3::4] == 1).all()
    got_c, _ = check(engine, canon)
    d = diff_results(ib, got, canon, got_c)
    assert not d, "\n".join(d)
