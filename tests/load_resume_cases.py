"""Shared cases for the resumed replay of routed tasks planned from loaded states (include/cadence_load_resume.h), used
on the CPU (the host restatement) and on the GPU (the device against the host and against the existing host path).

Expected values come from the path the other tests already trust: ``persisted.load_states_host`` for the loaded image
and ``flatten(suffixes, loaded=image.resumable(mask))`` for the counts and capacities; the tasks' blobs are
``thrift_codec.serialize_history`` of the suffixes.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import List, Optional

import numpy as np

from cadence_amd import abi, blobs, decode, persisted
from cadence_amd.abi import EventType as ET
from cadence_amd.flatten import flatten
from cadence_amd.history import HistoryEvent, WorkflowHistory
from cadence_amd.thrift_codec import serialize_history

import store_cases as sc
from resume_cases import KNOWN

R = abi.ResumeOutcome
CAPS = [t[3] for t in abi.TABLES]           # act_cap .. task_cap
BASES = [t[2] for t in abi.TABLES]


def source_of(h: Optional[WorkflowHistory]) -> decode.WorkflowSource:
    """A task's event blobs and the host inputs its replay takes, as the replication task carries them."""
    if h is None:
        return decode.WorkflowSource(blobs=[])
    return decode.WorkflowSource(blobs=serialize_history(h), run_id=h.run_id, branch_id=h.branch_id,
                                 domain_failover_version=h.domain_failover_version, now_ns=h.now_ns,
                                 is_new_run=h.is_new_run, refresh_tasks=h.refresh_tasks, retention_days=h.retention_days)


def task_blob_set(histories: List[Optional[WorkflowHistory]]) -> blobs.BlobSet:
    """Workflow k of the result holds task k's blobs."""
    return blobs.blobset_from_sources([source_of(h) for h in histories])[0]


def counts_of(img: persisted.ResumeImage, strings: np.ndarray) -> np.ndarray:
    """The per-position counts of this call's events, from the host decoder over the gathered batch."""
    batch = decode.decode_histories(img.blob_set(strings).to_sources(), known_domains=KNOWN)
    return persisted.resume_counts_of(batch)


def host_resume(sbs, tasks, routes, tbs: blobs.BlobSet) -> persisted.ResumeImage:
    """The whole host restatement: plan and gather, the host decoder's counts of the gathered batch, the descriptors."""
    first = persisted.load_resume_host(sbs, tasks, routes, tbs)
    return persisted.load_resume_host(sbs, tasks, routes, tbs, counts_of(first, tbs.strings))


@dataclasses.dataclass
class Planned:
    rc: sc.ReplayedCase
    results: np.ndarray
    routes: np.ndarray
    mask: np.ndarray                  # persisted.apply_mask: the workflows a task is applied onto
    tbs: blobs.BlobSet                # the tasks' blobs, task order
    loaded: persisted.LoadedImage     # load_states_host(rc.sbs)
    want: object                      # flatten(rc.suf, loaded=loaded.resumable(mask))


def planned(rc: sc.ReplayedCase) -> Planned:
    results, routes = sc.decided(rc)
    mask = persisted.apply_mask(routes, rc.tasks, rc.sbs.n_wf)
    loaded = persisted.load_states_host(rc.sbs)
    want = flatten(rc.suf, known_domains=KNOWN, loaded=loaded.resumable(mask))
    tbs = task_blob_set([rc.suf[int(w)] for w in rc.tasks["wf"]])
    return Planned(rc, results, routes, mask, tbs, loaded, want)


@functools.lru_cache(maxsize=None)
def planned_small() -> Planned:
    return planned(sc.replayed_case())


@functools.lru_cache(maxsize=None)
def planned_large() -> Planned:
    return planned(sc.replayed_case_large())


def compare_with_flatten(p: Planned, img: persisted.ResumeImage) -> int:
    """Assert ``img`` (host or device) against the host path's values for every applied workflow, and what a position
    without a task holds; returns the number of applied workflows compared."""
    rc, want = p.rc, p.want
    n_wf = rc.sbs.n_wf
    applied = np.zeros(n_wf, bool)
    applied[img.rows["position"][img.rows["outcome"] == R.APPLIED]] = True
    assert (applied == (p.mask & p.loaded.mask)).all()
    assert (np.nonzero(img.task_of >= 0)[0] == np.nonzero(applied)[0]).all()
    compared = 0
    for w in range(n_wf):
        d = img.desc[w]
        if not applied[w]:
            assert int(d["ev_count"]) == 0 and not int(d["flags"]) & abi.WF_FLAG_RESUME and int(d["start_token_len"]) == 0, w
            assert all(int(d[c]) == 0 for c in CAPS) and int(img.wf[w]["blob_count"]) == 0 and int(img.key_count[w]) == 0, w
            continue
        k = int(img.task_of[w])
        assert int(rc.tasks[k]["wf"]) == w
        b0, nb = int(img.wf[w]["blob_begin"]), int(img.wf[w]["blob_count"])
        s0 = int(p.tbs.wf[k]["blob_begin"])
        assert nb == int(p.tbs.wf[k]["blob_count"]) and nb >= 1
        assert [img.blob(b0 + j) for j in range(nb)] == [p.tbs.blob(s0 + j) for j in range(nb)], w
        assert img.keys(w) == p.loaded.keys(w), w
        e = want.wf[w]
        for f in ["ev_count", "empty_batch_at", "flags", "init_version", "now_ns", "retention_days"] + CAPS:
            assert int(d[f]) == int(e[f]), (w, f, int(d[f]), int(e[f]))
        assert int(d["flags"]) & abi.WF_FLAG_RESUME and int(d["final_token_len"]) == abi.NO_TOKEN
        tok = want.arena[int(e["start_token_off"]):int(e["start_token_off"]) + int(e["start_token_len"])].tobytes()
        assert img.token(w) == tok == p.loaded.token(w), w
        assert int(d["start_token_off"]) % 8 == 0
        compared += 1
    for base_f, cap_f in zip(BASES, CAPS):
        c = img.desc[cap_f].astype(np.int64)
        assert (img.desc[base_f] == np.cumsum(c) - c).all(), base_f
    assert img.table_rows == [int(img.desc[c].astype(np.int64).sum()) for c in CAPS]
    return compared


# ---- hand cases -------------------------------------------------------------------------------------------------
def _ev(eid, t, **attrs):
    return HistoryEvent(id=eid, event_type=t, version=3, timestamp=1_600_000_000_000_000_000 + eid, task_id=1000 + eid, attrs=attrs)


def hand_history(k: int) -> WorkflowHistory:
    """A small task: a timer and an activity of its own, so every task inserts into two tables."""
    return WorkflowHistory(workflow_id="wf", run_id="run-%d" % k, branch_id="branch-%d" % k, now_ns=77 + k, retention_days=2 + k % 3,
                           domain_failover_version=5 + k,
                           batches=[[_ev(30 + k, ET.TimerStarted, timer_id="hand-timer-%d" % k, start_to_fire_timeout_seconds=9),
                                     _ev(31 + k, ET.ActivityTaskScheduled, activity_id="hand-act-%d" % k)]])


A, N = abi.ROUTE_APPLY_CURRENT, abi.ROUTE_NON_CURRENT
# store_cases.HAND_STATES: state 4 does not load; state 2's current branch has an empty token; states 2 and 3 hold
# pending entries (a dictionary), the others none.  (workflow, route, expected outcome, expected position)
HAND_TASKS = [
    (1, A, R.APPLIED, 1),
    (1, A, R.SHADOWED, 1),                  # two applied tasks for one workflow: the lowest index wins
    (4, A, R.NOT_LOADED, None),             # its load failed
    (len(sc.HAND_STATES), A, R.NOT_LOADED, None),   # out of range
    (0xFFFFFFFF, A, R.NOT_LOADED, None),
    (0, N, R.NOT_ROUTED, None),
    (2, A, R.APPLIED, 2),                   # no token
    (0, 77, R.NOT_ROUTED, None),            # a garbage route
    (3, A, R.APPLIED, 3),
    (5, A, R.APPLIED, 5),
    (3, A, R.SHADOWED, 3),
    (4, N, R.NOT_ROUTED, None),             # the route is looked at first
]


def hand_tasks(rows=None):
    rows = HAND_TASKS if rows is None else rows
    tasks, routes = np.zeros(len(rows), abi.REPL_TASK), np.zeros(len(rows), abi.NDC_ROUTE)
    for k, (w, route, _o, _p) in enumerate(rows):
        tasks[k]["wf"], routes[k]["route"] = w, route
    return tasks, routes, task_blob_set([hand_history(k) for k in range(len(rows))])


# ---- long and colliding keys ---------------------------------------------------------------------------------------
KEY_TIMERS = [3, 20, 70, 90, 5, 130, 12, 40]       # pending timers per state; half as many activities beside them


def _key_workflow(w: int, pairs, rng) -> WorkflowHistory:
    """A state that holds ``KEY_TIMERS[w]`` pending timers and half as many activities whose IDs are
    ``full_event_cases._long_key``'s (15 to 300 bytes; one pair per twelve collides under the ingest hash), and a last
    batch -- the task -- that fires, cancels and cancel-requests a third of them by ID and starts one of a new ID."""
    import full_event_cases as fe
    n_t, n_a = KEY_TIMERS[w], KEY_TIMERS[w] // 2
    names = [fe._long_key(w, i, pairs, rng) for i in range(n_t + n_a + 2)]
    eid = [0]

    def ev(t, **attrs):
        eid[0] += 1
        return HistoryEvent(id=eid[0], event_type=t, version=3, timestamp=1_600_000_000_000_000_000 + eid[0],
                            task_id=1000 + eid[0], attrs=attrs)
    b0 = [ev(ET.WorkflowExecutionStarted, task_start_to_close_timeout_seconds=10, execution_start_to_close_timeout_seconds=3600,
             first_decision_task_backoff_seconds=0, initiator=None),
          ev(ET.DecisionTaskScheduled, start_to_close_timeout_seconds=10, attempt=0)]
    b1 = [ev(ET.DecisionTaskStarted, scheduled_event_id=2, request_id="request-%d" % w)]
    b2 = [ev(ET.DecisionTaskCompleted, scheduled_event_id=2, started_event_id=3, binary_checksum="bin-%d" % w)]
    b2 += [ev(ET.TimerStarted, timer_id=names[i], start_to_fire_timeout_seconds=100 + i) for i in range(n_t)]
    b2 += [ev(ET.ActivityTaskScheduled, activity_id=names[n_t + i], domain="", schedule_to_start_timeout_seconds=10,
              schedule_to_close_timeout_seconds=20, start_to_close_timeout_seconds=10, heartbeat_timeout_seconds=0)
           for i in range(n_a)]
    task = []
    for i in range(0, n_t, 3):
        task.append(ev(ET.TimerFired if i % 2 else ET.TimerCanceled, timer_id=names[i]))
    for i in range(4, n_t, 12):          # both keys of every colliding pair
        task += [ev(ET.TimerFired, timer_id=names[j]) for j in (i, i + 1) if j < n_t and j % 3]
    task += [ev(ET.ActivityTaskCancelRequested, activity_id=names[n_t + i]) for i in range(0, n_a, 3)]
    task += [ev(ET.TimerStarted, timer_id=names[n_t + n_a], start_to_fire_timeout_seconds=7),
             ev(ET.TimerFired, timer_id=names[n_t + n_a]),
             ev(ET.ActivityTaskScheduled, activity_id=names[n_t + n_a + 1], domain="", schedule_to_start_timeout_seconds=10,
                schedule_to_close_timeout_seconds=20, start_to_close_timeout_seconds=10, heartbeat_timeout_seconds=0)]
    return WorkflowHistory(workflow_id="keys-%d" % w, run_id="keys-run-%d" % w, branch_id="keys-branch-%d" % w, now_ns=5000 + w,
                           batches=[b0, b1, b2, task])


@functools.lru_cache(maxsize=None)
def planned_keys() -> Planned:
    import random
    rng, pairs = random.Random(77), {}
    return planned(sc.replayed_case_of([_key_workflow(w, pairs, rng) for w in range(len(KEY_TIMERS))], 82, 2))


def key_tally(p: Planned):
    """Over the applied tasks' events that name a string: how many name a seeded one of at least 15 bytes, how many
    one of a pair of equal length and ingest hash in its state's dictionary, how many a new string; and the largest
    seeded dictionary."""
    import full_event_cases as fe
    n_long = n_coll = n_new = largest = 0
    for w in np.nonzero(p.mask & p.loaded.mask)[0]:
        d = p.loaded.keys(int(w))
        largest = max(largest, len(d))
        by = {}
        for s in d:
            by.setdefault((len(s.encode()), fe.str_hash(s.encode())), []).append(s)
        coll = {s for v in by.values() if len(v) > 1 for s in v}
        for e in p.rc.suf[int(w)].events:
            name = fe._KEY_ATTR.get(int(e.event_type))
            s = e.get(name, "") if name else ""
            if s and s in d:
                n_long += len(s.encode()) >= 15
                n_coll += s in coll
            elif s:
                n_new += 1
    return {"long": n_long, "colliding": n_coll, "new": n_new, "largest_dictionary": largest}
