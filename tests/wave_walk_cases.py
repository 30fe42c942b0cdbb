"""Directed histories for the wave-per-workflow walk (replay_kernel.hip, the WaveSource branch of replay_body).

Builders only, no GPU.  A wavefront replays one history 64 events at a time (lane l of chunk c: step 64 c + l),
so every case here places its events at planned step indexes:

* ``failure_cases``: one failing event at a planned lane of chunk 1 or 2, or two of them in one chunk, followed
  by ``tail`` -- events that would change the state (a version-history item, the signal count, the cancel flag,
  the workflow state, the decision, two pending rows) if anything after the failure were applied;
* ``edge_cases``: state carried from one chunk into the next (decisions, failed decisions, batches, version
  bumps, dirty timer maps, reset points), valid histories left open;
* ``staircases``: one map filled to an arena limit in one batch, every second entry closed, two more inserted.

Chunk 0 holds WorkflowExecutionStarted and so always takes the per-event walk; everything here sits in chunk 1
or later, where a chunk of common types is resolved lane-parallel.  tests/test_wave_walk_cases.py pins every
planned step, status and bound against the CPU oracle; tests/test_gpu_wave_walk.py replays them on the device.
"""
from __future__ import annotations

import dataclasses
import random
from typing import Callable, Dict, List, Tuple

import numpy as np

from cadence_amd import abi
from cadence_amd.abi import EventType as ET
from cadence_amd.flatten import HistoryBatch, flatten, interleave
from cadence_amd.history import WorkflowHistory, det_uuid
from cadence_amd.synth_mixed import BASE_TS, _Walk

KNOWN = {"domain-a", "domain-b", "parent-domain"}

# the types that make a chunk take the per-event walk (replay_kernel.hip kLaneRare): the start, the closes,
# continue-as-new and anything unknown
RARE_TYPES = {int(ET.WorkflowExecutionStarted), int(ET.WorkflowExecutionCompleted), int(ET.WorkflowExecutionFailed),
              int(ET.WorkflowExecutionTimedOut), int(ET.WorkflowExecutionCanceled),
              int(ET.WorkflowExecutionTerminated), int(ET.WorkflowExecutionContinuedAsNew)}


def is_rare(t: int) -> bool:
    return t in RARE_TYPES or not 0 <= t < abi.EV_TYPE_COUNT


# ---- helpers shared with tests/test_gpu_lane_loop.py ---------------------------------------------------------
def _history(k: _Walk, w: int) -> WorkflowHistory:
    return WorkflowHistory(batches=k.batches, domain_failover_version=1, workflow_id=f"wf-{w}",
                           run_id=det_uuid("run", w), request_id=det_uuid("req", w),
                           branch_id=det_uuid("branch", w), now_ns=BASE_TS + 10 ** 15 + w)


def _activity(k: _Walk, aid: str):
    """[DecisionTaskCompleted, ActivityTaskScheduled] [ActivityTaskStarted] [ActivityTaskCompleted,
    DecisionTaskScheduled] [DecisionTaskStarted]: one round of the activity chain (6 events)."""
    done = k.ev(ET.DecisionTaskCompleted, scheduled_event_id=k.dec_sched, started_event_id=k.dec_started,
                binary_checksum="bin-0")
    sched = k.ev(ET.ActivityTaskScheduled, activity_id=aid, domain="", schedule_to_start_timeout_seconds=60,
                 schedule_to_close_timeout_seconds=600, start_to_close_timeout_seconds=300,
                 heartbeat_timeout_seconds=0, retry_policy=None)
    k.emit([done, sched])
    k.emit([k.ev(ET.ActivityTaskStarted, scheduled_event_id=sched.id, request_id=det_uuid(k.w, "a", sched.id))])
    k.emit([k.ev(ET.ActivityTaskCompleted, scheduled_event_id=sched.id), k.sched_decision()])
    k.emit([k.start_decision()])


def chain(w: int, activities: int, seed: int = 1) -> _Walk:
    """The activity-chain workflow (synth.activity_chain_template): 5 + 6 * activities events."""
    k = _Walk(random.Random(seed * 100003 + w), w, False, ["domain-a"])
    k.start()
    k.emit([k.start_decision()])
    for a in range(activities):
        _activity(k, str(a))
    k.emit([k.ev(ET.DecisionTaskCompleted, scheduled_event_id=k.dec_sched, started_event_id=k.dec_started,
                 binary_checksum="bin-0"), k.ev(ET.WorkflowExecutionCompleted)])
    return k


def truncated(k: _Walk, n: int):
    """The first n events of the walk, batch structure kept (the last batch may be cut short)."""
    out, left = [], n
    for b in k.batches:
        if left <= 0:
            break
        out.append(b[:left])
        left -= len(b)
    k.batches = out
    return k


def event_at(k: _Walk, step: int):
    return [e for b in k.batches for e in b][step]


def _fail(k: _Walk, step: int, kind: str):
    e = event_at(k, step)
    if kind == "id":
        e.id = max(1, e.id - 1)           # event ID not increasing
    elif kind == "version":
        e.version -= 1                    # lower version than the version history's last item
    elif kind == "type":
        e.event_type = 99                 # unknown event type
    elif kind == "activity":
        assert e.event_type == ET.ActivityTaskStarted
        e.attrs["scheduled_event_id"] = 424242   # no such pending activity
    return k


# ---- building blocks -----------------------------------------------------------------------------------------
def types_of(k: _Walk) -> List[int]:
    return [int(e.event_type) for b in k.batches for e in b]


def base(w: int) -> _Walk:
    """start(), [DecisionTaskStarted], [DecisionTaskCompleted, MarkerRecorded]: five events, no decision
    pending, state Running; the next event built is at step 5."""
    k = _Walk(random.Random(770001 + w), w, False, ["domain-a"])
    k.start()
    k.emit([k.start_decision()])
    k.emit([k.ev(ET.DecisionTaskCompleted, scheduled_event_id=k.dec_sched, started_event_id=k.dec_started,
                 binary_checksum="bin-0"), k.ev(ET.MarkerRecorded)])
    k.dec_sched = k.dec_started = None
    assert k.eid == 5
    return k


def pad_to(k: _Walk, step: int, bumps=()) -> _Walk:
    """Single-event [WorkflowExecutionSignaled] batches until the next event built is at step index ``step``
    (k.eid counts the events built so far).  ``bumps``: steps whose event raises the failover version by one."""
    assert k.eid <= step, (k.eid, step)
    while k.eid < step:
        if k.eid in bumps:
            k.version += 1
        k.emit([k.ev(ET.WorkflowExecutionSignaled)])
    return k


def _act(k: _Walk, aid: str, domain: str = ""):
    return k.ev(ET.ActivityTaskScheduled, activity_id=aid, domain=domain, schedule_to_start_timeout_seconds=60,
                schedule_to_close_timeout_seconds=600, start_to_close_timeout_seconds=300,
                heartbeat_timeout_seconds=0, retry_policy=None)


def _completed(k: _Walk, checksum: str = "bin-0"):
    e = k.ev(ET.DecisionTaskCompleted, scheduled_event_id=k.dec_sched, started_event_id=k.dec_started,
             binary_checksum=checksum)
    k.dec_sched = k.dec_started = None
    return e


def decide(k: _Walk, outputs: Callable[[_Walk], list] = lambda k: [], checksum: str = "bin-0"):
    """[DecisionTaskScheduled] [DecisionTaskStarted] [DecisionTaskCompleted, outputs...]: 3 + len(outputs) events."""
    k.emit([k.sched_decision()])
    k.emit([k.start_decision()])
    k.emit([_completed(k, checksum)] + outputs(k))


def tail(k: _Walk) -> _Walk:
    """Events that change the state if they are applied after a failure: a higher version (a version-history
    item), a signal and a cancel request, a scheduled decision (state Running, the decision fields), a
    completed decision with an activity and a timer (last_processed_event, two rows, timer tasks), signals."""
    k.version += 10
    k.emit([k.ev(ET.WorkflowExecutionSignaled), k.ev(ET.WorkflowExecutionCancelRequested)])
    k.emit([k.sched_decision()])
    k.emit([k.start_decision()])
    k.emit([_completed(k, "bin-tail"), _act(k, "tail-a"),
            k.ev(ET.TimerStarted, timer_id="tail-t", start_to_fire_timeout_seconds=77)])
    for _ in range(9):
        k.emit([k.ev(ET.WorkflowExecutionSignaled)])
    return k


# ---- 1. failures with events after them ----------------------------------------------------------------------
PROLOGUE_KINDS = ("id", "version", "invalid", "empty")
WALK_KINDS = ("activity", "child", "domain", "type", "decision")
STATUS = {"id": abi.Status.VH_EVENT_ID_NOT_INCREASING, "version": abi.Status.VH_LOWER_VERSION,
          "invalid": abi.Status.VH_INVALID_ITEM, "empty": abi.Status.EMPTY_HISTORY,
          "activity": abi.Status.MISSING_ACTIVITY_INFO, "child": abi.Status.MISSING_CHILD_INFO,
          "domain": abi.Status.DOMAIN_NOT_FOUND, "type": abi.Status.UNKNOWN_EVENT_TYPE,
          "decision": abi.Status.DECISION_NOT_FOUND}
# lanes 0, 1, 31, 62, 63 of chunk 1 and lanes 0, 63 of chunk 2
FAIL_STEPS = (64, 65, 95, 126, 127, 128, 191)


def bad_batch(k: _Walk, kind: str):
    """One batch whose only event fails in the given way (``empty``: a batch with no event: the step that
    fails is the next event's)."""
    if kind == "empty":
        k.emit([])
        return
    if kind in ("id", "version", "invalid"):
        e = k.ev(ET.WorkflowExecutionSignaled)
        if kind == "id":
            e.id -= 1                     # its predecessor's ID: not increasing
        elif kind == "version":
            e.version -= 1                # below the version history's last item
        else:
            e.version = -7                # no version at all
    elif kind == "activity":
        e = k.ev(ET.ActivityTaskStarted, scheduled_event_id=424242, request_id=det_uuid(k.w, "a", 424242))
    elif kind == "child":
        e = k.ev(ET.ChildWorkflowExecutionStarted, initiated_event_id=424242)
    elif kind == "domain":
        e = _act(k, "x", domain="unknown-domain")
    elif kind == "type":
        e = k.ev(99)
    elif kind == "decision":
        e = k.ev(ET.DecisionTaskStarted, scheduled_event_id=424242, request_id=det_uuid(k.w, k.eid))
    else:
        raise ValueError(kind)
    k.emit([e])


@dataclasses.dataclass
class FailCase:
    name: str
    build: Callable[[int], _Walk]     # workflow index -> the whole walk (failure(s) + tail)
    status: int
    fail_step: int
    fast: bool                        # no rare type in the failing event's chunk: it is resolved lane-parallel


def _one_failure(kind: str, step: int) -> Callable[[int], _Walk]:
    def build(w):
        k = pad_to(base(w), step)
        bad_batch(k, kind)
        return tail(k)
    return build


def _two_failures(first: str, a: int, second: str, b: int) -> Callable[[int], _Walk]:
    def build(w):
        k = pad_to(base(w), a)
        bad_batch(k, first)
        pad_to(k, b)
        bad_batch(k, second)
        return tail(k)
    return build


# (earlier kind, its step, later kind, its step): a prologue failure with a walk failure before / after it, a
# DecisionTaskStarted without its decision with a missing activity before / after it; the earlier step wins
TWO_FAILURES = (("activity", 74, "id", 84), ("id", 74, "activity", 84), ("child", 70, "version", 100),
                ("invalid", 70, "domain", 100), ("empty", 90, "activity", 100), ("activity", 90, "empty", 100),
                ("activity", 80, "decision", 90), ("decision", 80, "activity", 90), ("decision", 80, "id", 90),
                ("id", 80, "decision", 90), ("activity", 64, "version", 127), ("id", 64, "decision", 127),
                ("decision", 126, "id", 127), ("activity", 126, "decision", 127), ("decision", 128, "activity", 191),
                ("activity", 130, "decision", 131))


# the lane loop's kinds (_fail) on a 155-event activity chain: the event itself is made to fail, the chain's
# own events follow it (ActivityTaskStarted is at steps 5 + 6 r)
CHAIN_FAILURES = tuple((kind, step) for kind in ("id", "version", "type") for step in (64, 65, 70, 127)) + \
    (("activity", 65), ("activity", 71), ("activity", 125))


def failure_cases() -> List[FailCase]:
    out = []
    for kind, step in CHAIN_FAILURES:
        out.append(FailCase(f"chain:{kind}@{step}", lambda w, kind=kind, step=step: _fail(chain(w, 25), step, kind),
                            int(STATUS[kind]), step, kind != "type"))
    for kind in PROLOGUE_KINDS + WALK_KINDS:
        for step in FAIL_STEPS:
            out.append(FailCase(f"{kind}@{step}", _one_failure(kind, step), int(STATUS[kind]), step, kind != "type"))
    for first, a, second, b in TWO_FAILURES:
        assert a < b and a // 64 == b // 64
        out.append(FailCase(f"{first}@{a}+{second}@{b}", _two_failures(first, a, second, b), int(STATUS[first]), a,
                            "type" not in (first, second)))
    return out


def failure_histories(cases: List[FailCase]) -> List[WorkflowHistory]:
    """Workflow 2 i: case i whole; workflow 2 i + 1: the same walk (same workflow index, so the same times and
    IDs) cut after its failing event."""
    hs = []
    for i, c in enumerate(cases):
        hs.append(_history(c.build(i), i))
        hs.append(_history(truncated(c.build(i), c.fail_step + 1), i))
    return hs


# ---- 2. state carried across a chunk edge --------------------------------------------------------------------
EDGES = (64, 128)


@dataclasses.dataclass
class EdgeCase:
    name: str
    build: Callable[[int], _Walk]
    group: str                        # decision | failed | batch | version | timer | reset
    plan: Dict[int, int]              # step -> the event type planned there


def _fail_decision(k: _Walk, how: str):
    if how == "failed":
        k.emit([k.ev(ET.DecisionTaskFailed)])
    else:
        k.emit([k.ev(ET.DecisionTaskTimedOut, timeout_type=0 if k.dec_started is not None else 1)])
    k.dec_sched = k.dec_started = None


FAIL_TYPE = {"failed": int(ET.DecisionTaskFailed), "timed_out": int(ET.DecisionTaskTimedOut)}


def edge_cases(E: int) -> List[EdgeCase]:
    DS, DT, DC = int(ET.DecisionTaskScheduled), int(ET.DecisionTaskStarted), int(ET.DecisionTaskCompleted)
    AS, SG = int(ET.ActivityTaskScheduled), int(ET.WorkflowExecutionSignaled)
    out: List[EdgeCase] = []

    def add(name, group, plan):
        def deco(fn):
            out.append(EdgeCase(f"{name}@{E}", fn, group, plan))
            return fn
        return deco

    # -- a decision across the edge
    @add("scheduled|started", "decision", {E - 1: DS, E: DT})
    def _(w):
        k = pad_to(base(w), E - 1)
        k.emit([k.sched_decision()])
        k.emit([k.start_decision()])
        return pad_to(k, E + 4)

    @add("scheduled,started|completed,activity", "decision", {E - 2: DS, E - 1: DT, E: DC, E + 1: AS})
    def _(w):
        k = pad_to(base(w), E - 2)
        decide(k, lambda k: [_act(k, "a0")])
        return pad_to(k, E + 5)

    @add("scheduled|", "decision", {E - 1: DS})
    def _(w):   # the history ends at lane 63: exactly E events, a decision pending
        k = pad_to(base(w), E - 1)
        k.emit([k.sched_decision()])
        return k

    # -- failed and timed-out decisions
    for how in ("failed", "timed_out"):
        @add(f"{how}|transient pair", "failed", {E - 1: FAIL_TYPE[how], E: DS, E + 1: DT})
        def _(w, how=how):
            k = pad_to(base(w), E - 3)
            k.emit([k.sched_decision()])
            k.emit([k.start_decision()])
            _fail_decision(k, how)
            k.emit([k.sched_decision(attempt=1), k.start_decision()])
            return pad_to(k, E + 5)

    @add("scheduled, timed out|transient pair", "failed", {E - 2: DS, E - 1: FAIL_TYPE["timed_out"], E: DS, E + 1: DT})
    def _(w):   # schedule-to-start timeout: the decision never started
        k = pad_to(base(w), E - 2)
        k.emit([k.sched_decision()])
        _fail_decision(k, "timed_out")
        k.emit([k.sched_decision(attempt=1), k.start_decision()])
        return pad_to(k, E + 5)

    for n in (2, 3):
        for last in (E, E + 1, E + 2):   # the last failure at lane 0, 1, 2: pair | failure, scheduled | started, failure | pair
            plan = {last: FAIL_TYPE["failed" if n % 2 else "timed_out"], last - 1: DT, last - 2: DS}

            @add(f"{n} failures, last at {last - E}", "failed", plan)
            def _(w, n=n, last=last):
                k = pad_to(base(w), last - 3 * n + 1)
                k.emit([k.sched_decision()])
                k.emit([k.start_decision()])
                _fail_decision(k, "failed")
                for i in range(1, n):
                    k.emit([k.sched_decision(attempt=i), k.start_decision()])
                    _fail_decision(k, "timed_out" if i % 2 else "failed")
                assert k.eid == last + 1
                return k   # ends on the failure: the transient decision's fields are the exec row's

    @add("scheduled(attempt 2)|timed out", "failed", {E - 1: DS, E: FAIL_TYPE["timed_out"]})
    def _(w):   # the failure's attempt counts on from the carried decision's
        k = pad_to(base(w), E - 1)
        k.emit([k.sched_decision(attempt=2)])
        _fail_decision(k, "timed_out")
        return k

    @add("|scheduled(attempt 2), timed out", "failed", {E: DS, E + 1: FAIL_TYPE["timed_out"]})
    def _(w):   # ... and from a DecisionTaskScheduled of the same chunk
        k = pad_to(base(w), E)
        k.emit([k.sched_decision(attempt=2)])
        _fail_decision(k, "timed_out")
        return k

    # the transient decision started with no DecisionTaskScheduled event of its own: its ScheduleID is NextEventID
    # at the failure (the failed event's own ID here), which DecisionTaskStarted's check must find
    for name, at in (("failed, started inside a chunk", E + 12), ("|failed at 0, started", E), ("failed|started", E - 1)):
        @add(f"transient: {name}", "failed", {at: FAIL_TYPE["failed"], at + 1: DT})
        def _(w, at=at):
            k = pad_to(base(w), at - 2)
            k.emit([k.sched_decision()])
            k.emit([k.start_decision()])
            _fail_decision(k, "failed")
            k.dec_sched = k.eid            # the failed event's ID: the transient decision's ScheduleID
            k.emit([k.start_decision()])
            return pad_to(k, at + 5)

    @add("failed|timed out, nothing between", "failed", {E - 1: FAIL_TYPE["failed"], E: FAIL_TYPE["timed_out"]})
    def _(w):   # the transient decision itself times out: two failures counted from the carried attempt
        k = pad_to(base(w), E - 3)
        k.emit([k.sched_decision()])
        k.emit([k.start_decision()])
        _fail_decision(k, "failed")
        _fail_decision(k, "timed_out")
        return pad_to(k, E + 3)

    # -- batch boundaries
    @add("batch first at 63, activity insert at 0", "batch", {E - 3: DS, E - 2: DT, E - 1: DC, E: AS})
    def _(w):   # the insert's batch-first ID is the one carried in
        k = pad_to(base(w), E - 3)
        decide(k, lambda k: [_act(k, "a0")])
        return pad_to(k, E + 4)

    @add("two-signal batch over the edge", "batch", {E - 1: SG, E: SG})
    def _(w):
        k = pad_to(base(w), E - 1)
        k.emit([k.ev(ET.WorkflowExecutionSignaled), k.ev(ET.WorkflowExecutionSignaled)])
        return pad_to(k, E + 3)

    @add("batch last at 63, nothing after", "batch", {E - 2: SG, E - 1: DS})
    def _(w):   # exactly E events
        k = pad_to(base(w), E - 2)
        k.emit([k.ev(ET.WorkflowExecutionSignaled), k.sched_decision()])
        return k

    @add("batch cut at 63", "batch", {E - 1: SG})
    def _(w):   # exactly E events, the last batch open (no batch end in the chunk's last lanes)
        k = pad_to(base(w), E - 2)
        k.emit([k.ev(ET.WorkflowExecutionSignaled), k.ev(ET.WorkflowExecutionSignaled), k.ev(ET.MarkerRecorded)])
        return truncated(k, E)

    # -- version bumps
    for name, bumps in (("lane 0", {E}), ("lane 63", {E - 1}), ("lanes 63 and 0", {E - 1, E}),
                        ("lanes 0 and 63 of one chunk", {E, E + 63}), ("all 64 lanes", set(range(E, E + 64)))):
        @add(f"version bump at {name}", "version", {})
        def _(w, bumps=bumps):
            return pad_to(base(w), max(bumps) + 6, bumps=bumps)

    # -- timer state carried across the edge: the maps dirtied in one chunk, their batch's end at lane 0 of the next
    @add("dirty maps, batch end at 0", "timer", {E - 3: DC, E - 2: AS, E - 1: int(ET.TimerStarted), E: int(ET.MarkerRecorded)})
    def _(w):
        k = pad_to(base(w), E - 5)
        decide(k, lambda k: [_act(k, "a0"), k.ev(ET.TimerStarted, timer_id="t0", start_to_fire_timeout_seconds=50),
                             k.ev(ET.MarkerRecorded)])
        return pad_to(k, E + 4)

    # -- reset points: one checksum at lanes 5 and 40, a new one at lane 63, the first again in the next chunk
    @add("reset point dedup", "reset", {E + 5: DC, E + 40: DC, E + 63: DC, E + 69: DC})
    def _(w):
        k = base(w)
        for at, checksum in ((E + 5, "rp-x"), (E + 40, "rp-x"), (E + 63, "rp-new"), (E + 69, "rp-x")):
            pad_to(k, at - 2)
            decide(k, checksum=checksum)
        return pad_to(k, E + 74)

    return out


RAGGED_COUNTS = (63, 65, 127, 129, 192)


def ragged_histories(w0: int) -> List[WorkflowHistory]:
    """Activity chains (197 events) cut to 63, 65, 127, 129 and 192 events."""
    return [_history(truncated(chain(w0 + i, 32), n), w0 + i) for i, n in enumerate(RAGGED_COUNTS)]


RESUME_GROUPS = ("decision", "failed", "batch", "version")


def split_at(h: WorkflowHistory, step: int) -> Tuple[WorkflowHistory, WorkflowHistory, int]:
    """(prefix, suffix, events in the prefix): the history cut at the batch boundary nearest ``step`` that leaves
    at least one batch on each side."""
    ends = np.cumsum([len(b) for b in h.batches])[:-1]
    assert ends.size
    i = int(np.argmin(np.abs(ends - step)))
    pre = dataclasses.replace(h, batches=h.batches[:i + 1], final_token=None, refresh_tasks=False)
    return pre, dataclasses.replace(h, batches=h.batches[i + 1:]), int(ends[i])


# ---- 3. arena limits -----------------------------------------------------------------------------------------
STAIR_SIZES = {"act": (40, 41, 63, 64, 65, 128, 129, 320, 321), "timer": (32, 33, 48, 49, 128, 129, 160, 161),
               "child": (16, 17, 24, 25, 64, 65, 96, 97), "rc": (8, 9, 16, 17, 64, 65), "sig": (8, 9, 16, 17, 64, 65),
               "rp": (24, 25, 32, 33, 64, 65)}
# sizes whose slots cross a register of the row tables (slot j: lane j % 64 of register j / 64)
CROSS_SIZES = {"act": (64, 65, 128, 129), "timer": (128, 129), "child": (64, 65), "rc": (64, 65), "sig": (64, 65)}
COUNT_FIELD = {"act": "n_activity", "timer": "n_timer", "child": "n_child", "rc": "n_rc", "sig": "n_signal",
               "rp": "n_reset_points"}
WAVE_SMALL = {"act": 40, "timer": 32, "child": 16, "rc": 8, "sig": 8, "rp": 24}   # the small per-wave arena


def _insert(k: _Walk, m: str, i: int):
    if m == "act":
        return _act(k, f"a{i}")
    if m == "timer":
        return k.ev(ET.TimerStarted, timer_id=f"t{i}", start_to_fire_timeout_seconds=100 + i)
    t = {"child": ET.StartChildWorkflowExecutionInitiated, "rc": ET.RequestCancelExternalWorkflowExecutionInitiated,
         "sig": ET.SignalExternalWorkflowExecutionInitiated}[m]
    return k.ev(t, domain="")


def _close(k: _Walk, m: str, e):
    if m == "act":
        return k.ev(ET.ActivityTaskCompleted, scheduled_event_id=e.id)
    if m == "timer":
        return k.ev(ET.TimerFired, timer_id=e.attrs["timer_id"])      # looked up by TimerID
    t = {"child": ET.ChildWorkflowExecutionCompleted, "rc": ET.ExternalWorkflowExecutionCancelRequested,
         "sig": ET.ExternalWorkflowExecutionSignaled}[m]
    return k.ev(t, initiated_event_id=e.id)


@dataclasses.dataclass
class Stair:
    name: str
    map: str
    n: int                            # the live-set bound: the entries of the first batch
    final: int                        # live entries at the end
    cross: bool
    walk: _Walk


def staircase(w: int, m: str, n: int, cross: bool = False) -> Stair:
    """One DecisionTaskCompleted batch inserts n entries of map ``m`` (slots 0..n-1); every second entry is then
    closed, each in a batch of its own, and two more are inserted (into the lowest free slots, 0 and 2).
    ``cross``: instead only the entries in slots 63 and 64 (those that exist) are closed and as many inserted, so
    the re-used slots are the last lane of one register and the first of the next; an ActivityTaskCancelRequested
    then looks the last entry up by its ActivityID (timers are closed by TimerID anyway).
    Reset points are never removed: n - 1 completed decisions with checksums of their own beside the base's
    ``bin-0``, then two that repeat earlier ones."""
    k = base(w)
    if m == "rp":
        for i in range(n - 1):
            decide(k, checksum=f"rp-{i}")
        decide(k, checksum="rp-0")
        decide(k, checksum="bin-0")
        return Stair(f"rp-{n}", m, n, n, False, k)
    made = []

    def first(k):
        made.extend(_insert(k, m, i) for i in range(n))
        return list(made)

    decide(k, first)
    closing = [i for i in (63, 64) if i < n] if cross else list(range(0, n, 2))
    for i in closing:
        k.emit([_close(k, m, made[i])])
    more = len(closing) if cross else 2

    def second(k):
        outs = [_insert(k, m, n + j) for j in range(more)]
        if cross and m == "act":
            outs.append(k.ev(ET.ActivityTaskCancelRequested, activity_id=f"a{n - 1}"))
        return outs

    decide(k, second)
    pad_to(k, k.eid + 3)
    return Stair(f"{m}-{n}{'-cross' if cross else ''}", m, n, n - len(closing) + more, cross, k)


def staircases() -> List[Stair]:
    out, w = [], 0
    for m, sizes in STAIR_SIZES.items():
        for n in sizes:
            out.append(staircase(w, m, n))
            w += 1
    for m, sizes in CROSS_SIZES.items():
        for n in sizes:
            out.append(staircase(w, m, n, cross=True))
            w += 1
    return out


def in_small_arena(s: Stair) -> bool:
    return s.n <= WAVE_SMALL[s.map]


# ---- layouts: every history one wavefront --------------------------------------------------------------------
NO_BIG = {m: 2 ** 31 - 1 for m in ("act", "timer", "child", "rc", "sig", "rp")}
LAYOUTS = ("tiered", "tail_only", "untiered")


def wave_layout(canon: HistoryBatch, layout: str, emit: bool = False) -> HistoryBatch:
    """``tiered``: the default segments (a workflow past 64 entries in a map goes to replay_big_kernel);
    ``tail_only``: every workflow in replay_tail_kernel, whatever its live sets; ``untiered``: the tail inside
    replay_lds_kernel / replay_lds_small_kernel.  Every workflow is a wavefront's."""
    canon.emit_tasks = emit
    if layout == "tiered":
        b = interleave(canon, long_threshold=0)
    elif layout == "tail_only":
        b = interleave(canon, long_threshold=0, big_caps=NO_BIG)
    elif layout == "untiered":
        b = interleave(canon, long_threshold=0, tiered=False)
    else:
        raise ValueError(layout)
    b.emit_tasks = emit
    assert b.wave_begin == 0
    return b


def flat(hs: List[WorkflowHistory]) -> HistoryBatch:
    return flatten(hs, known_domains=KNOWN)


def device_pos(b: HistoryBatch) -> np.ndarray:
    """Canonical workflow -> its position in the device order."""
    inv = np.empty(b.n_wf, np.int64)
    inv[b.perm] = np.arange(b.n_wf)
    return inv
