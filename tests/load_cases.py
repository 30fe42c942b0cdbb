"""Shared cases for the persisted mutable-state loader (include/cadence_load.h): the round-trip workload,
the expected image restated in Python, and hand-built edge cases (used on the CPU and on the GPU)."""
from __future__ import annotations

import functools
import json
import os
from typing import Dict, List

import numpy as np

from cadence_amd import abi, persisted, synth_mixed
from cadence_amd.flatten import LoadedStates, flatten
from cadence_amd.thrift_codec import W

from resume_cases import KNOWN, split_histories

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sqlblobs_fields.json")
MAPS = [("act", "n_activity", abi.STATE_ACTIVITY, "schedule_id"), ("timer", "n_timer", abi.STATE_TIMER, "started_id"),
        ("child", "n_child", abi.STATE_CHILD, "initiated_id"), ("rc", "n_rc", abi.STATE_REQUEST_CANCEL, "initiated_id"),
        ("sig", "n_signal", abi.STATE_SIGNAL, "initiated_id")]


def fixture_fields() -> Dict[str, List]:
    with open(FIXTURE) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def prefix_case(n: int, seed: int, long_tail: bool = False):
    """(histories, prefixes, suffixes, split mask, canonical prefix batch, its oracle replay)."""
    from oracle import oracle
    if long_tail:
        hs = synth_mixed.long_tail_histories(n, seed, max_len=4000, run_cap=2000, multi_version=True, caps=None)
    else:
        hs = synth_mixed.mixed_histories(n, seed, multi_version=True, can_rate=0.3)
    pre, suf, mask = split_histories(hs, seed + 1)
    pre_b = flatten(pre, known_domains=KNOWN)
    return hs, pre, suf, mask, pre_b, oracle.replay(pre_b, 0)


def expected_image(loaded: LoadedStates, sbs: persisted.StateBlobSet) -> LoadedStates:
    """The image the loader must produce for ``sbs = encode_states(...)`` of the replayed states ``loaded``
    (``ReplayResult.to_loaded``): the replay's rows with what a persisted state cannot carry rewritten by the
    loader's rules -- provenance = blob indices, keys in first-seen blob order, MAPPED by greatest ScheduleID,
    and the per-call / in-memory fields at their Load values."""
    ex = loaded.exec.copy()
    rows = {k: v.copy() for k, v in loaded.rows.items()}
    offs = {k: np.cumsum(loaded.counts(k)) - loaded.counts(k) for k in rows}
    interners = []
    for w in range(ex.shape[0]):
        if not loaded.mask[w]:
            interners.append({"": 0})
            continue
        names = {v: k for k, v in loaded.interners[w].items()}
        ids: Dict[str, int] = {"": 0}

        def intern(s):
            return ids.setdefault(s, len(ids))

        def view(name, n_f):
            o = int(offs[name][w])
            return rows[name][o:o + int(ex[n_f][w])]

        b0, nb = int(sbs.wf["blob_begin"][w]), int(sbs.wf["blob_count"][w])
        tables = {kind: view(name, n_f) for name, n_f, kind, _ in MAPS}
        id_f = {kind: f for _n, _c, kind, f in MAPS}
        act_names = [names[int(k)] for k in tables[abi.STATE_ACTIVITY]["key"]]
        timer_names = [names[int(k)] for k in tables[abi.STATE_TIMER]["key"]]
        rp = view("rp", "n_reset_points")
        rp_names = [names[int(k)] for k in rp["key"]]
        for i in range(nb):
            B = sbs.blob[b0 + i]
            kind = int(B["kind"])
            if kind == abi.STATE_EXECUTION:
                ex["start_src"][w] = i
                if ex["decision_request_src"][w] >= 0:
                    ex["decision_request_src"][w] = i
                for j in range(rp.shape[0]):
                    rp["src"][j], rp["prev_index"][j], rp["key"][j] = i, j, intern(rp_names[j])
                continue
            t = tables[kind]
            if kind == abi.STATE_TIMER:
                s = sbs.strings[int(B["str_off"]):int(B["str_off"]) + int(B["str_len"])].tobytes().decode()
                j = timer_names.index(s)
                t["src"][j], t["key"][j] = i, intern(s)
                continue
            j = int(np.nonzero(t[id_f[kind]] == B["id"])[0][0])
            if kind == abi.STATE_ACTIVITY:
                t["sched_src"][j] = i
                t["started_src"][j] = -1 if t["started_id"][j] == abi.EMPTY_EVENT_ID else i
                t["key"][j] = intern(act_names[j])
            else:
                t["src"][j] = i
                if kind == abi.STATE_CHILD:
                    t["started_src"][j] = -1 if t["started_id"][j] == abi.EMPTY_EVENT_ID else i
        act = tables[abi.STATE_ACTIVITY]
        act["last_hb_timeout_vis_s"] = 0          # the SQL store does not persist it
        for j in range(act.shape[0]):              # Load: the greatest ScheduleID of an ActivityID is the mapped one
            same = [k for k in range(act.shape[0]) if act_names[k] == act_names[j]]
            top = max(same, key=lambda k: int(act["schedule_id"][k]))
            act["flags"][j] = (int(act["flags"][j]) & ~abi.ROW_MAPPED) | (abi.ROW_MAPPED if top == j else 0)
        ex["src_next"][w] = nb
        ex["token_src"][w] = 1 if ex["token_src"][w] != 0 else 0
        interners.append(ids)
    m = loaded.mask
    ex["checksum"] = 0
    ex["payload_len"] = 0
    ex["n_tasks"] = 0
    ex["current_version"][m] = abi.EMPTY_VERSION              # Load, mutable_state_builder.go:325
    ex["flags"][m] = (ex["flags"][m] & ~np.uint32(abi.EXEC_CHECKSUM_VALID)) | abi.EXEC_RESET_POINTS_SET
    # logDataInconsistency() calls are counted per ApplyEvents call, not persisted: a loaded state starts at 0
    ex["inconsistencies"] = 0
    return LoadedStates(ex, rows, m.copy(), interners)


def assert_image_equals(got: LoadedStates, want: LoadedStates):
    assert (got.mask == want.mask).all()
    for f in abi.EXEC_ROW.names:
        bad = np.nonzero(got.exec[f] != want.exec[f])[0]
        assert bad.size == 0, f"exec.{f}: wf {bad[:5]}: {got.exec[f][bad[:5]]} vs {want.exec[f][bad[:5]]}"
    for name in abi.LOAD_ROW_TABLES:
        a, b = got.rows[name], want.rows[name]
        assert a.shape == b.shape, name
        for f in a.dtype.names:
            bad = np.nonzero(a[f] != b[f])[0]
            assert bad.size == 0, f"{name}.{f}: rows {bad[:5]}: {a[f][bad[:5]]} vs {b[f][bad[:5]]}"
    assert got.interners == want.interners


# ---- hand-built states ---------------------------------------------------------------------------------------
def _row(dtype, **kw):
    r = np.zeros(1, dtype)
    for k, v in kw.items():
        r[k] = v
    return r[0]


TOKEN = b"\x59branch-token-bytes"


def exec_blob(nei=20, items=((19, 3),), points=(), **over) -> bytes:
    ex = _row(abi.EXEC_ROW, state=1, next_event_id=nei, last_first_event_id=nei - 2, last_event_task_id=777,
              last_processed_event=nei - 5, completion_event_batch_id=abi.EMPTY_EVENT_ID, decision_version=3,
              decision_schedule_id=nei - 2, decision_started_id=abi.EMPTY_EVENT_ID, decision_scheduled_ts=1_600_000_000_000_000_123,
              decision_orig_scheduled_ts=1_600_000_000_000_000_123, decision_started_ts=abi.ZERO_TIME,
              decision_timeout=10, decision_request_src=abi.SRC_EMPTY_UUID, decision_start_to_close=10, signal_count=2)
    v = persisted.execution_values(ex, TOKEN, list(items), list(points))
    v.update(over)
    return persisted.encode_struct("WorkflowExecutionInfo", v)


def activity_blob(schedule_id, activity_id, started_id=abi.EMPTY_EVENT_ID, **over):
    r = _row(abi.ACTIVITY_ROW, schedule_id=schedule_id, version=3, scheduled_batch_id=schedule_id - 1,
             scheduled_time=1_600_000_000_000_000_000 + schedule_id, started_id=started_id,
             started_time=abi.ZERO_TIME if started_id == abi.EMPTY_EVENT_ID else 1_600_000_001_000_000_000,
             cancel_request_id=abi.EMPTY_EVENT_ID, schedule_to_start=5, schedule_to_close=30, start_to_close=20, heartbeat=3,
             flags=abi.ROW_LIVE)
    v = persisted.activity_values(r, activity_id)
    v.update(over)
    return (abi.STATE_ACTIVITY, schedule_id, abi.GO_ZERO_TIME_NANOS, "", persisted.encode_struct("ActivityInfo", v))


def timer_blob(timer_id, started_id, **over):
    v = persisted.timer_values(_row(abi.TIMER_ROW, started_id=started_id, version=3, expiry_time=1_600_000_100_000_000_000, task_status=1))
    v.update(over)
    return (abi.STATE_TIMER, 0, 0, timer_id, persisted.encode_struct("TimerInfo", v))


def child_blob(initiated_id, started_id=abi.EMPTY_EVENT_ID):
    r = _row(abi.CHILD_ROW, initiated_id=initiated_id, version=3, initiated_batch_id=initiated_id - 1, started_id=started_id)
    return (abi.STATE_CHILD, initiated_id, 0, "", persisted.encode_struct("ChildExecutionInfo", persisted.child_values(r)))


def initiated_blob(initiated_id, signal):
    r = _row(abi.INITIATED_ROW, initiated_id=initiated_id, version=3, initiated_batch_id=initiated_id - 1)
    name = "SignalInfo" if signal else "RequestCancelInfo"
    return (abi.STATE_SIGNAL if signal else abi.STATE_REQUEST_CANCEL, initiated_id, 0, "",
            persisted.encode_struct(name, persisted.initiated_values(r, signal)))


def execution(raw: bytes):
    return (abi.STATE_EXECUTION, 0, 0, "", raw)


def good_workflow(i: int = 0):
    """A small healthy state: one of each pending entry."""
    return (20, [execution(exec_blob(points=[("bin-%d" % i, True)])), activity_blob(5, "a5"), timer_blob("t7", 7),
                 child_blob(9, 10), initiated_blob(11, False), initiated_blob(12, True)])


def big_workflow():
    """65 activities (repeated ActivityIDs) + 5 timers, out of ID order: past 64 blobs."""
    blobs = [activity_blob(100 + 2 * ((k * 37) % 65), "act-%d" % (k % 9)) for k in range(65)]
    blobs.insert(40, execution(exec_blob(nei=400, points=[("act-3", False), ("bin", True), ("bin", True)])))
    blobs += [timer_blob("act-%d" % k, 300 - k) for k in range(5)]
    return (400, blobs)


def unknown_fields_blob(kind_name: str, values: Dict[str, object]) -> bytes:
    """The struct with a field of an unknown id of every thrift type in front of, between and after its own."""
    known = persisted.encode_struct(kind_name, values)[:-1]
    w = W()
    w.i32(10, 12345)                    # a known id (i64 or binary in all six structs) with the wrong wire type: skipped
    w.boolean(1, True)
    w.field(3, 2)                       # byte
    w.b += b"\x07"
    w.double(3, 1.5)
    w.field(6, 4)                       # i16
    w.b += b"\x01\x02"
    w.i32(5, 7)
    w.i64(6, 8)
    w.string(7, "unknown")
    w.struct_(8, [lambda x: x.i64(1, 5), lambda x: x.struct_(2, [lambda y: y.list_strings(1, ["p", "q"]),
                                                                  lambda y: y.struct_(2, [lambda z: z.boolean(1, False)])])])
    w.map_string_binary(9, {"k": b"v", "k2": b""})
    tail = W()
    tail.field(14, 9000)                # set<i32>
    tail.b += bytes([8]) + (2).to_bytes(4, "big") + (1).to_bytes(4, "big") + (2).to_bytes(4, "big")
    tail.list_strings(9001, [])
    tail.field(13, 9002)                # empty map
    tail.b += bytes([11, 11]) + (0).to_bytes(4, "big")
    return bytes(w.b) + known + bytes(tail.b) + b"\x00"


FAILURES = {
    "no_execution": (abi.LoadStatus.EXECUTION_COUNT, lambda: (20, [activity_blob(5, "a5")])),
    "two_executions": (abi.LoadStatus.EXECUTION_COUNT, lambda: (20, [execution(exec_blob()), execution(exec_blob())])),
    "no_blobs": (abi.LoadStatus.EXECUTION_COUNT, lambda: (0, [])),
    "malformed_activity": (abi.LoadStatus.MALFORMED, lambda: (20, [execution(exec_blob()), activity_blob(5, "a5")[:4] + (b"\x0a\x00",)])),
    "malformed_nested_vh": (abi.LoadStatus.MALFORMED, lambda: (20, [execution(exec_blob(VersionHistories=b"\x59\x08\x00"))])),
    "bad_preamble_rp": (abi.LoadStatus.MALFORMED, lambda: (20, [execution(exec_blob(AutoResetPoints=b"\x58\x00"))])),
    "json_version_histories": (abi.LoadStatus.NESTED_ENCODING, lambda: (20, [execution(exec_blob(VersionHistoriesEncoding="json"))])),
    "json_reset_points": (abi.LoadStatus.NESTED_ENCODING, lambda: (20, [execution(exec_blob(AutoResetPointsEncoding="json"))])),
    "duplicate_activity": (abi.LoadStatus.DUPLICATE_ID, lambda: (20, [execution(exec_blob()), activity_blob(5, "a"), activity_blob(5, "b")])),
    "duplicate_timer_id": (abi.LoadStatus.DUPLICATE_ID, lambda: (20, [execution(exec_blob()), timer_blob("t", 5), timer_blob("t", 6)])),
    "duplicate_signal": (abi.LoadStatus.DUPLICATE_ID, lambda: (20, [initiated_blob(8, True), execution(exec_blob()), initiated_blob(8, True)])),
    "too_many_blobs": (abi.LoadStatus.TOO_LARGE,
                       lambda: (20, [execution(exec_blob())] + [initiated_blob(100 + k, False) for k in range(abi.LOAD_MAX_BLOBS)])),
    "too_many_reset_points": (abi.LoadStatus.TOO_LARGE,
                              lambda: (20, [execution(exec_blob(points=[("b%d" % k, True) for k in range(abi.LOAD_MAX_BLOBS + 1)]))])),
    "no_version_histories": (abi.LoadStatus.VERSION_HISTORIES, lambda: (20, [execution(exec_blob(VersionHistories=None))])),
    "empty_version_histories": (abi.LoadStatus.VERSION_HISTORIES,
                                lambda: (20, [execution(exec_blob(VersionHistories=persisted.encode_version_histories(0, [])))])),
    "current_index_out_of_range": (abi.LoadStatus.VERSION_HISTORIES,
                                   lambda: (20, [execution(exec_blob(VersionHistories=persisted.encode_version_histories(1, [(TOKEN, [(5, 1)])])))])),
}


def failure_batch():
    """Every failure status, each between two healthy workflows: (blob set, expected statuses)."""
    wfs, want = [], []
    for i, (name, (status, make)) in enumerate(FAILURES.items()):
        wfs += [good_workflow(i), make()]
        want += [0, int(status)]
    wfs.append(good_workflow(99))
    want.append(0)
    return persisted.build_blob_set(wfs), np.array(want, np.int32)


def truncation_batches():
    """Per blob kind: a batch holding every proper prefix of one full blob of that kind (each in its own
    workflow, with a healthy execution blob beside a truncated pending entry), all of which must report
    CRR_LOAD_MALFORMED; healthy workflows in front and behind."""
    full = {
        abi.STATE_EXECUTION: execution(exec_blob(points=[("bin-a", True), ("bin-b", False)], items=((5, 1), (19, 3)))),
        abi.STATE_ACTIVITY: activity_blob(5, "activity-five", 6),
        abi.STATE_TIMER: timer_blob("timer-seven", 7),
        abi.STATE_CHILD: child_blob(9, 10),
        abi.STATE_REQUEST_CANCEL: initiated_blob(11, False),
        abi.STATE_SIGNAL: initiated_blob(12, True),
    }
    out = {}
    for kind, blob in full.items():
        raw = blob[4]
        wfs = [good_workflow(0)]
        for n in range(len(raw)):
            cut = blob[:4] + (raw[:n],)
            wfs.append((20, [cut] if kind == abi.STATE_EXECUTION else [execution(exec_blob()), cut]))
        wfs.append(good_workflow(1))
        out[kind] = persisted.build_blob_set(wfs)
    return out


def edge_batches() -> Dict[str, persisted.StateBlobSet]:
    """Named hand-built batches the host and the device must agree on."""
    out = {"failures": failure_batch()[0], "big": persisted.build_blob_set([good_workflow(0), big_workflow(), good_workflow(1)]),
           "exec_only": persisted.build_blob_set([(20, [execution(exec_blob())])])}
    for n in (1, 63, 64, 65):
        out["n_wf_%d" % n] = persisted.build_blob_set([good_workflow(i) for i in range(n)])
    for kind, sbs in truncation_batches().items():
        out["truncated_%d" % kind] = sbs
    out.update(populated=populated_batch(False), populated_unknown=populated_batch(True), defaults=defaults_batch())
    return out

# ---- the wire-format cases (CPU assertions in test_load_states.py; the device decodes the same blobs) -------------
# what the loader reads: struct -> {field: (probe value, row table, row field, expected)}; built from the
# fixture's ids, not from the encoder's table
PROBES = {
    "ActivityInfo": {"Version": (901, "version"), "ScheduledEventBatchID": (902, "scheduled_batch_id"),
                     "ScheduledTimeNanos": (903, "scheduled_time"), "StartedID": (904, "started_id"),
                     "StartedTimeNanos": (905, "started_time"), "ScheduleToStartTimeoutSeconds": (906, "schedule_to_start"),
                     "ScheduleToCloseTimeoutSeconds": (907, "schedule_to_close"), "StartToCloseTimeoutSeconds": (908, "start_to_close"),
                     "HeartbeatTimeoutSeconds": (909, "heartbeat"), "CancelRequestID": (910, "cancel_request_id"),
                     "TimerTaskStatus": (911, "timer_task_status"), "Attempt": (912, "attempt")},
    "TimerInfo": {"Version": (921, "version"), "StartedID": (922, "started_id"), "ExpiryTimeNanos": (923, "expiry_time"),
                  "TaskID": (924, "task_status")},
    "ChildExecutionInfo": {"Version": (931, "version"), "InitiatedEventBatchID": (932, "initiated_batch_id"),
                           "StartedID": (933, "started_id")},
    "RequestCancelInfo": {"Version": (941, "version"), "InitiatedEventBatchID": (942, "initiated_batch_id")},
    "SignalInfo": {"Version": (951, "version"), "InitiatedEventBatchID": (952, "initiated_batch_id")},
    "WorkflowExecutionInfo": {
        "CompletionEventBatchID": (961, "completion_event_batch_id"), "DecisionTaskTimeoutSeconds": (962, "decision_start_to_close"),
        "State": (2, "state"), "CloseStatus": (5, "close_status"), "LastEventTaskID": (965, "last_event_task_id"),
        "LastFirstEventID": (966, "last_first_event_id"), "LastProcessedEvent": (967, "last_processed_event"),
        "DecisionVersion": (968, "decision_version"), "DecisionScheduleID": (969, "decision_schedule_id"),
        "DecisionStartedID": (970, "decision_started_id"), "DecisionTimeout": (971, "decision_timeout"),
        "DecisionAttempt": (972, "decision_attempt"), "DecisionStartedTimestampNanos": (973, "decision_started_ts"),
        "DecisionScheduledTimestampNanos": (974, "decision_scheduled_ts"),
        "DecisionOriginalScheduledTimestampNanos": (975, "decision_orig_scheduled_ts"),
        "RetryExpirationTimeNanos": (976, "expiration_ns"), "SignalCount": (977, "signal_count")},
}
TABLE_OF = {"ActivityInfo": ("act", abi.STATE_ACTIVITY), "TimerInfo": ("timer", abi.STATE_TIMER),
            "ChildExecutionInfo": ("child", abi.STATE_CHILD), "RequestCancelInfo": ("rc", abi.STATE_REQUEST_CANCEL),
            "SignalInfo": ("sig", abi.STATE_SIGNAL)}
FILLER = {"i64": 7, "i32": 7, "bool": True, "double": 1.5, "binary": b"filler", "list": ["x", "y"], "map": {"k": b"v"}}


def fully_populated(name, unknown=False):
    """Every field of the struct set, from the fixture table: probes where the loader reads, filler elsewhere;
    ``unknown``: with unknown_fields_blob's extra fields around them."""
    fields = [tuple(f) for f in fixture_fields()[name]]
    values = {f: FILLER[t] for f, _id, t in fields}
    values.update({f: v for f, (v, _row) in PROBES[name].items()})
    if name == "ActivityInfo":
        values["ActivityID"] = "probe-activity"
    if name == "WorkflowExecutionInfo":
        values.update(VersionHistories=persisted.encode_version_histories(0, [(TOKEN, [(4, 1), (19, 3)])]),
                      VersionHistoriesEncoding="thriftrw", AutoResetPointsEncoding="thriftrw",
                      AutoResetPoints=persisted.encode_reset_points([("bin-x", True), ("bin-y", False)]),
                      DecisionRequestID="a-real-request-id", StickyTaskList="sticky")
    if unknown:
        return unknown_fields_blob(name, values)
    return persisted.encode_struct(name, values, fields)


def populated_batch(unknown: bool) -> persisted.StateBlobSet:
    """A workflow whose every struct has every field set (encoded from the fixture's ids and types alone),
    between two healthy ones; ``unknown``: the structs also carry fields of unknown ids of
    every thrift type (nested three deep) and a known id with the wrong wire type."""
    blobs = []
    for name, (_tab, kind) in TABLE_OF.items():
        raw = fully_populated(name, unknown)
        assert (raw != fully_populated(name)) == unknown
        blobs.append((kind, 55, 991, "probe-timer", raw))
    blobs.insert(2, execution(fully_populated("WorkflowExecutionInfo", unknown)))
    return persisted.build_blob_set([good_workflow(0), (77, blobs), good_workflow(1)])


def defaults_batch() -> persisted.StateBlobSet:
    """Empty structs (every getter's zero value), and every time field at time.Time{}.UnixNano()."""
    vh = dict(VersionHistories=persisted.encode_version_histories(0, [(b"", [])]), VersionHistoriesEncoding="thriftrw")
    empty = [(abi.STATE_ACTIVITY, 5, 0, "", b"\x00"), (abi.STATE_TIMER, 0, 0, "t", b"\x00"), (abi.STATE_CHILD, 6, 0, "", b"\x00"),
             (abi.STATE_REQUEST_CANCEL, 7, 0, "", b"\x00"), (abi.STATE_SIGNAL, 8, 0, "", b"\x00"),
             execution(persisted.encode_struct("WorkflowExecutionInfo", vh))]
    z = abi.GO_ZERO_TIME_NANOS
    zero_times = [
        (abi.STATE_ACTIVITY, 5, z, "", persisted.encode_struct("ActivityInfo", {"ScheduledTimeNanos": z, "StartedTimeNanos": z})),
        (abi.STATE_TIMER, 0, 0, "t", persisted.encode_struct("TimerInfo", {"ExpiryTimeNanos": z})),
        execution(persisted.encode_struct("WorkflowExecutionInfo", dict(
            vh, DecisionStartedTimestampNanos=z, DecisionScheduledTimestampNanos=z,
            DecisionOriginalScheduledTimestampNanos=z, RetryExpirationTimeNanos=z, DecisionRequestID="emptyUuid")))]
    return persisted.build_blob_set([(9, empty), (9, zero_times)])
