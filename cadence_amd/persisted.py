"""Persisted mutable states: the SQL store's state blobs <-> the engine's resumable rows.

``encode_states`` is the writer side -- what ``GetWorkflowExecution`` returns for a replayed state: one
``sqlblobs.WorkflowExecutionInfo`` blob per execution and one ``ActivityInfo`` / ``TimerInfo`` /
``ChildExecutionInfo`` / ``RequestCancelInfo`` / ``SignalInfo`` blob per pending entry, in plain thrift
binary (``common/persistence/serialization/thrift_decoder.go:161-165``: no preamble), with the key columns
stored beside each blob (``common/persistence/sql/workflowStateMaps.go``).  Every field the Go writer sets
(``serialization/thrift_mapper.go:185-512``) is written, so the loader's skipping is exercised on realistic
blobs; it is the reference encoder for a cgo shim's tests.

``load_states_host`` decodes such a batch with the host restatement (``crr_load_states_host``) and
``StateLoader`` with the device implementation (``crr_load_states_plan`` / ``_read`` / ``_place``,
``include/cadence_load.h``).  Both return the dense loaded image as a ``LoadedImage`` (a
``flatten.LoadedStates`` plus tokens, dictionaries, statuses and flags).

``StateLoader.verify`` / ``load_states_verify_host`` make the check ``mutableStateBuilder.Load`` makes right
after materialising a state -- the stored ``checksum.Checksum`` against a freshly generated payload
(``include/cadence_load_verify.h``) -- for every state that loaded OK, sticky and multi-branch ones included.

``StateLoader.branches`` / ``load_branches_host`` give every branch of every loaded state, and
``StateLoader.ndc_prepare`` decides and routes replication tasks against those states on the device
(``include/cadence_load_ndc.h``): ``prepareVersionHistory`` through ``crr_ndc_prepare``, then
``prepareMutableState``'s route per task; ``apply_mask`` turns the routes into the workflows to resume.

``StateLoader.store_checksums`` / ``store_checksums_host`` give, per routed task, the checksum Go stores with the
state when it commits the task (``include/cadence_load_store.h``): from the rows the resumed replay left for a
task applied to the current branch, from the loaded image for one backfilled onto another branch.

``StateLoader.mutation`` / ``mutation_host`` give, per routed task, what else that commit writes
(``include/cadence_load_mutation.h``): the post-replay exec row, the pending entries to upsert and the keys to
delete; ``apply_mutation`` applies such a result to the persisted blobs as a host shim would.
"""
from __future__ import annotations

import ctypes
import dataclasses
import random
import struct
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from . import abi
from .flatten import HistoryBatch, LoadedStates
from .history import WorkflowHistory, det_uuid, thrift_history_branch_token
from .result import ReplayResult
from .thrift_codec import T_BOOL, T_DOUBLE, T_I32, T_I64, T_LIST, T_MAP, T_STRING, T_STRUCT, W


def _table(spec: str):
    return [(n, int(i), t) for n, i, t in (x.split(":") for x in spec.split())]


# .gen/go/sqlblobs/sqlblobs.go: (field, id, thrift type) of the six state structs
FIELDS = {
    "WorkflowExecutionInfo": _table(
        "ParentDomainID:10:binary ParentWorkflowID:12:binary ParentRunID:14:binary InitiatedID:16:i64 "
        "CompletionEventBatchID:18:i64 CompletionEvent:20:binary CompletionEventEncoding:22:binary TaskList:24:binary "
        "WorkflowTypeName:26:binary WorkflowTimeoutSeconds:28:i32 DecisionTaskTimeoutSeconds:30:i32 "
        "ExecutionContext:32:binary State:34:i32 CloseStatus:36:i32 StartVersion:38:i64 LastWriteEventID:44:i64 "
        "LastEventTaskID:48:i64 LastFirstEventID:50:i64 LastProcessedEvent:52:i64 StartTimeNanos:54:i64 "
        "LastUpdatedTimeNanos:56:i64 DecisionVersion:58:i64 DecisionScheduleID:60:i64 DecisionStartedID:62:i64 "
        "DecisionTimeout:64:i32 DecisionAttempt:66:i64 DecisionStartedTimestampNanos:68:i64 "
        "DecisionScheduledTimestampNanos:69:i64 CancelRequested:70:bool DecisionOriginalScheduledTimestampNanos:71:i64 "
        "CreateRequestID:72:binary DecisionRequestID:74:binary CancelRequestID:76:binary StickyTaskList:78:binary "
        "StickyScheduleToStartTimeout:80:i64 RetryAttempt:82:i64 RetryInitialIntervalSeconds:84:i32 "
        "RetryMaximumIntervalSeconds:86:i32 RetryMaximumAttempts:88:i32 RetryExpirationSeconds:90:i32 "
        "RetryBackoffCoefficient:92:double RetryExpirationTimeNanos:94:i64 RetryNonRetryableErrors:96:list "
        "HasRetryPolicy:98:bool CronSchedule:100:binary EventStoreVersion:102:i32 EventBranchToken:104:binary "
        "SignalCount:106:i64 HistorySize:108:i64 ClientLibraryVersion:110:binary ClientFeatureVersion:112:binary "
        "ClientImpl:114:binary AutoResetPoints:115:binary AutoResetPointsEncoding:116:binary SearchAttributes:118:map "
        "Memo:120:map VersionHistories:122:binary VersionHistoriesEncoding:124:binary"),
    "ActivityInfo": _table(
        "Version:10:i64 ScheduledEventBatchID:12:i64 ScheduledEvent:14:binary ScheduledEventEncoding:16:binary "
        "ScheduledTimeNanos:18:i64 StartedID:20:i64 StartedEvent:22:binary StartedEventEncoding:24:binary "
        "StartedTimeNanos:26:i64 ActivityID:28:binary RequestID:30:binary ScheduleToStartTimeoutSeconds:32:i32 "
        "ScheduleToCloseTimeoutSeconds:34:i32 StartToCloseTimeoutSeconds:36:i32 HeartbeatTimeoutSeconds:38:i32 "
        "CancelRequested:40:bool CancelRequestID:42:i64 TimerTaskStatus:44:i32 Attempt:46:i32 TaskList:48:binary "
        "StartedIdentity:50:binary HasRetryPolicy:52:bool RetryInitialIntervalSeconds:54:i32 "
        "RetryMaximumIntervalSeconds:56:i32 RetryMaximumAttempts:58:i32 RetryExpirationTimeNanos:60:i64 "
        "RetryBackoffCoefficient:62:double RetryNonRetryableErrors:64:list RetryLastFailureReason:66:binary "
        "RetryLastWorkerIdentity:68:binary RetryLastFailureDetails:70:binary"),
    "TimerInfo": _table("Version:10:i64 StartedID:12:i64 ExpiryTimeNanos:14:i64 TaskID:16:i64"),
    "ChildExecutionInfo": _table(
        "Version:10:i64 InitiatedEventBatchID:12:i64 StartedID:14:i64 InitiatedEvent:16:binary "
        "InitiatedEventEncoding:18:binary StartedWorkflowID:20:binary StartedRunID:22:binary StartedEvent:24:binary "
        "StartedEventEncoding:26:binary CreateRequestID:28:binary DomainID:29:binary DomainName:30:binary "
        "WorkflowTypeName:32:binary ParentClosePolicy:35:i32"),
    "RequestCancelInfo": _table("Version:10:i64 InitiatedEventBatchID:11:i64 CancelRequestID:12:binary"),
    "SignalInfo": _table("Version:10:i64 InitiatedEventBatchID:11:i64 RequestID:12:binary Name:14:binary Input:16:binary "
                         "Control:18:binary"),
}
KIND_STRUCT = ["WorkflowExecutionInfo", "ActivityInfo", "TimerInfo", "ChildExecutionInfo", "RequestCancelInfo",
               "SignalInfo"]
THRIFT_TYPE = {"bool": T_BOOL, "double": T_DOUBLE, "i32": T_I32, "i64": T_I64, "binary": T_STRING, "list": T_LIST,
               "map": T_MAP, "struct": T_STRUCT}


def write_value(w: W, fid: int, typ: str, v):
    """One field of thrift type ``typ`` (list: list<string>; map: map<string, binary>)."""
    if typ == "i64":
        w.i64(fid, v)
    elif typ == "i32":
        w.i32(fid, v)
    elif typ == "bool":
        w.boolean(fid, v)
    elif typ == "double":
        w.double(fid, v)
    elif typ == "binary":
        w.string(fid, v)
    elif typ == "list":
        w.list_strings(fid, list(v))
    elif typ == "map":
        w.map_string_binary(fid, dict(v))
    else:
        raise ValueError(typ)


def encode_struct(name: str, values: Dict[str, object], fields=None) -> bytes:
    """thriftrw's struct encoding: the set (non-None) fields in ascending id, then the stop byte."""
    w = W()
    for fname, fid, typ in sorted(fields or FIELDS[name], key=lambda f: f[1]):
        v = values.get(fname)
        if v is not None:
            write_value(w, fid, typ, v)
    unknown = set(values) - {f[0] for f in (fields or FIELDS[name])}
    if unknown:
        raise KeyError(f"{name}: no field {sorted(unknown)}")
    w.b += b"\x00"
    return bytes(w.b)


def to_unix_nano(t: int) -> int:
    """timeToUnixNanoPtr: the Go zero time (rows: ZERO_TIME) is written as time.Time{}.UnixNano()."""
    return abi.GO_ZERO_TIME_NANOS if int(t) == abi.ZERO_TIME else int(t)


def encode_version_histories(current: int, histories: Sequence) -> bytes:
    """shared.VersionHistories as a thriftrw DataBlob: ``histories`` = [(branch token, [(event id, version)])];
    a token or an items list that is None is left out of its VersionHistory struct."""
    w = W()
    w.b += b"\x59"
    w.i32(10, current)
    w.field(T_LIST, 20)
    w.b += bytes([T_STRUCT]) + struct.pack(">i", len(histories))
    for token, items in histories:
        if token is not None:
            w.string(10, token)
        if items is not None:
            w.field(T_LIST, 20)
            w.b += bytes([T_STRUCT]) + struct.pack(">i", len(items))
        for eid, ver in items or ():
            w.i64(10, eid)
            w.i64(20, ver)
            w.b += b"\x00"
        w.b += b"\x00"
    w.b += b"\x00"
    return bytes(w.b)


def encode_reset_points(points: Sequence) -> bytes:
    """shared.ResetPoints as a thriftrw DataBlob (the layout thrift_codec._reset_points writes inside a start
    event): ``points`` = [(binary checksum, resettable)]."""
    w = W()
    w.b += b"\x59"
    w.field(T_LIST, 10)
    w.b += bytes([T_STRUCT]) + struct.pack(">i", len(points))
    for i, (bc, resettable) in enumerate(points):
        w.string(10, bc)
        w.string(20, f"run-{i}")
        w.i64(30, 4 + i)
        w.i64(40, 1_500_000_000_000_000_000 + i)
        w.i64(50, 0)
        w.boolean(60, resettable)
        w.b += b"\x00"
    w.b += b"\x00"
    return bytes(w.b)


@dataclasses.dataclass
class StateBlobSet:
    """Host image of ``crr_state_batch``."""
    bytes: np.ndarray        # uint8: the blobs, then abi.INGEST_PAD zero bytes
    blob_off: np.ndarray     # uint64 [n_blobs + 1]
    blob: np.ndarray         # abi.STATE_BLOB [n_blobs]
    wf: np.ndarray           # abi.STATE_WF [n_wf]
    strings: np.ndarray      # uint8

    @property
    def n_blobs(self) -> int:
        return int(self.blob.shape[0])

    @property
    def n_wf(self) -> int:
        return int(self.wf.shape[0])

    @property
    def n_bytes(self) -> int:
        return int(self.blob_off[-1])

    def blob_bytes(self, b: int) -> bytes:
        return self.bytes[int(self.blob_off[b]):int(self.blob_off[b + 1])].tobytes()


def build_blob_set(workflows: Sequence) -> StateBlobSet:
    """``workflows``: per execution ``(next_event_id, [(kind, id, aux_time, timer_id, blob bytes), ...])``."""
    data = bytearray()
    strings = bytearray()
    offs = [0]
    blob_rows, wf_rows = [], []
    for nei, blobs in workflows:
        wf_rows.append((len(blob_rows), len(blobs), nei))
        for kind, bid, aux, timer_id, raw in blobs:
            s = timer_id.encode() if isinstance(timer_id, str) else bytes(timer_id or b"")
            blob_rows.append((kind, len(s), bid, aux, len(strings)))
            strings += s
            data += raw
            offs.append(len(data))
    return StateBlobSet(
        bytes=np.frombuffer(bytes(data) + bytes(abi.INGEST_PAD), np.uint8).copy(),
        blob_off=np.array(offs, np.uint64),
        blob=np.array(blob_rows, dtype=abi.STATE_BLOB) if blob_rows else np.zeros(0, abi.STATE_BLOB),
        wf=np.array(wf_rows, dtype=abi.STATE_WF) if wf_rows else np.zeros(0, abi.STATE_WF),
        strings=np.frombuffer(bytes(strings) + b"\0", np.uint8).copy())


def _inverse(interner: Optional[Dict[str, int]]) -> Dict[int, str]:
    return {v: k for k, v in (interner or {"": 0}).items()}


def execution_values(ex, token: bytes, vh_items, points, sticky: str = "", decoy_branch: bool = False,
                     branches=None) -> Dict[str, object]:
    """Field values of the execution blob for exec row ``ex`` (workflowExecutionInfoToThrift: every pointer
    field set; the nil-able ones the replay path leaves nil are omitted).  ``branches``: ``(histories, current
    index)`` written instead of the one branch ``(token, vh_items)`` -- ``histories`` a list of ``(token, items)``
    as ``encode_version_histories`` takes them, an entry that is None standing for ``(token, vh_items)``."""
    src = int(ex["decision_request_src"])
    request_id = "emptyUuid" if src == abi.SRC_EMPTY_UUID else ("" if src == abi.SRC_NONE else det_uuid("decision", src))
    histories = [(token, vh_items)]
    current = 0
    if decoy_branch:   # a second, non-current branch in front of the current one
        histories = [(b"decoy-branch-token", [(1, 0), (7, 3)])] + histories
        current = 1
    if branches is not None:
        histories = [(token, vh_items) if h is None else h for h in branches[0]]
        current = int(branches[1])
    v = {
        "ParentWorkflowID": "", "InitiatedID": abi.EMPTY_EVENT_ID, "CompletionEventEncoding": "",
        "TaskList": "task-list", "WorkflowTypeName": "workflow-type", "WorkflowTimeoutSeconds": 3600,
        "DecisionTaskTimeoutSeconds": int(ex["decision_start_to_close"]), "ExecutionContext": b"ctx",
        "State": int(ex["state"]), "CloseStatus": int(ex["close_status"]), "StartVersion": 0,
        "LastEventTaskID": int(ex["last_event_task_id"]), "LastFirstEventID": int(ex["last_first_event_id"]),
        "LastProcessedEvent": int(ex["last_processed_event"]), "StartTimeNanos": 1_600_000_000_000_000_000,
        "LastUpdatedTimeNanos": 1_600_000_000_500_000_000, "DecisionVersion": int(ex["decision_version"]),
        "DecisionScheduleID": int(ex["decision_schedule_id"]), "DecisionStartedID": int(ex["decision_started_id"]),
        "DecisionTimeout": int(ex["decision_timeout"]), "DecisionAttempt": int(ex["decision_attempt"]),
        "DecisionStartedTimestampNanos": to_unix_nano(ex["decision_started_ts"]),
        "DecisionScheduledTimestampNanos": to_unix_nano(ex["decision_scheduled_ts"]),
        "CancelRequested": bool(int(ex["flags"]) & abi.EXEC_CANCEL_REQUESTED),
        "DecisionOriginalScheduledTimestampNanos": to_unix_nano(ex["decision_orig_scheduled_ts"]),
        "CreateRequestID": det_uuid("create"), "DecisionRequestID": request_id, "CancelRequestID": "",
        "StickyTaskList": sticky, "StickyScheduleToStartTimeout": 0, "RetryAttempt": 0,
        "RetryInitialIntervalSeconds": 1, "RetryMaximumIntervalSeconds": 100, "RetryMaximumAttempts": 5,
        "RetryExpirationSeconds": 0, "RetryBackoffCoefficient": 2.0,
        # ExpirationTime: an unset one is the Go zero time
        "RetryExpirationTimeNanos": int(ex["expiration_ns"]) or abi.GO_ZERO_TIME_NANOS,
        "RetryNonRetryableErrors": ["bad-input"], "HasRetryPolicy": bool(int(ex["expiration_ns"])),
        "CronSchedule": "", "EventStoreVersion": 2, "EventBranchToken": token, "SignalCount": int(ex["signal_count"]),
        "HistorySize": 4096, "ClientLibraryVersion": "1.7.0", "ClientFeatureVersion": "1.7.0", "ClientImpl": "uber-go",
        "AutoResetPoints": encode_reset_points(points), "AutoResetPointsEncoding": "thriftrw",
        "SearchAttributes": {"CustomKeywordField": b'"v"'}, "Memo": {"note": b"memo"},
        "VersionHistories": encode_version_histories(current, histories), "VersionHistoriesEncoding": "thriftrw",
    }
    if int(ex["completion_event_batch_id"]) != abi.EMPTY_EVENT_ID:   # a *int64: nil until the workflow closes
        v["CompletionEventBatchID"] = int(ex["completion_event_batch_id"])
    return v


def activity_values(r, activity_id: str) -> Dict[str, object]:
    return {
        "Version": int(r["version"]), "ScheduledEventBatchID": int(r["scheduled_batch_id"]),
        "ScheduledEvent": b"scheduled-event", "ScheduledEventEncoding": "thriftrw",
        "ScheduledTimeNanos": to_unix_nano(r["scheduled_time"]), "StartedID": int(r["started_id"]),
        "StartedEventEncoding": "", "StartedTimeNanos": to_unix_nano(r["started_time"]), "ActivityID": activity_id,
        "RequestID": "" if int(r["started_id"]) == abi.EMPTY_EVENT_ID else det_uuid("activity", int(r["schedule_id"])),
        "ScheduleToStartTimeoutSeconds": int(r["schedule_to_start"]),
        "ScheduleToCloseTimeoutSeconds": int(r["schedule_to_close"]),
        "StartToCloseTimeoutSeconds": int(r["start_to_close"]), "HeartbeatTimeoutSeconds": int(r["heartbeat"]),
        "CancelRequested": bool(int(r["flags"]) & abi.ROW_CANCEL_REQUESTED), "CancelRequestID": int(r["cancel_request_id"]),
        "TimerTaskStatus": int(r["timer_task_status"]), "Attempt": int(r["attempt"]), "TaskList": "activity-tl",
        "StartedIdentity": "worker", "HasRetryPolicy": bool(int(r["flags"]) & abi.ROW_HAS_RETRY),
        "RetryInitialIntervalSeconds": 1, "RetryMaximumIntervalSeconds": 100, "RetryMaximumAttempts": 5,
        "RetryExpirationTimeNanos": abi.GO_ZERO_TIME_NANOS, "RetryBackoffCoefficient": 2.0,
        "RetryNonRetryableErrors": ["bad-input"], "RetryLastFailureReason": "", "RetryLastWorkerIdentity": "",
    }


def timer_values(r) -> Dict[str, object]:
    return {"Version": int(r["version"]), "StartedID": int(r["started_id"]),
            "ExpiryTimeNanos": to_unix_nano(r["expiry_time"]), "TaskID": int(r["task_status"])}


def child_values(r) -> Dict[str, object]:
    started = int(r["started_id"]) != abi.EMPTY_EVENT_ID
    return {"Version": int(r["version"]), "InitiatedEventBatchID": int(r["initiated_batch_id"]),
            "StartedID": int(r["started_id"]), "InitiatedEvent": b"initiated-event", "InitiatedEventEncoding": "thriftrw",
            "StartedWorkflowID": "child-wf" if started else "", "StartedRunID": b"0123456789abcdef" if started else None,
            "StartedEventEncoding": "", "CreateRequestID": det_uuid("child", int(r["initiated_id"])),
            "DomainID": "domain-id", "DomainName": "domain-a", "WorkflowTypeName": "child-type", "ParentClosePolicy": 0}


def initiated_values(r, signal: bool) -> Dict[str, object]:
    v = {"Version": int(r["version"]), "InitiatedEventBatchID": int(r["initiated_batch_id"])}
    if signal:
        v.update(RequestID=det_uuid("signal", int(r["initiated_id"])), Name="sig", Input=b"signal-input", Control=b"c")
    else:
        v["CancelRequestID"] = det_uuid("cancel", int(r["initiated_id"]))
    return v


def encode_states(batch: HistoryBatch, result: ReplayResult, histories: Sequence[WorkflowHistory],
                  shuffle_seed: Optional[int] = None, sticky: Iterable[int] = (), multi_branch: Iterable[int] = (),
                  branches=None) -> StateBlobSet:
    """The persisted form of the states ``result`` holds for ``batch`` (a replay of ``histories``), canonical
    workflow order: what the SQL store would return for each execution whose replay ended OK (any other
    workflow has no blobs).  The execution blob comes first, then activities, timers, children,
    request-cancels and signals in row order; ``shuffle_seed`` shuffles each execution's blobs.
    ``sticky`` / ``multi_branch``: workflow indices given a sticky task list / a second, non-current branch.
    ``branches``: ``{workflow index: (histories, current index)}`` (or a sequence indexed by workflow, None: as
    without it) -- the branch set written for that workflow, as ``execution_values`` takes it."""
    loaded = result.to_loaded(batch)
    sticky, multi_branch = set(sticky), set(multi_branch)
    if branches is None:
        branches = {}
    elif not isinstance(branches, dict):
        branches = {w: b for w, b in enumerate(branches) if b is not None}
    rng = random.Random(shuffle_seed) if shuffle_seed is not None else None
    offs = {name: np.cumsum(loaded.counts(name)) - loaded.counts(name) for name in loaded.rows}
    workflows = []
    for w, h in enumerate(histories):
        ex = loaded.exec[w]
        if not loaded.mask[w]:
            workflows.append((0, []))
            continue
        names = _inverse(loaded.interners[w] if loaded.interners is not None else None)

        def rows(name, n_f):
            o = int(offs[name][w])
            return loaded.rows[name][o:o + max(int(ex[n_f]), 0)]

        src = int(ex["token_src"])
        token = b"" if src == 0 else (thrift_history_branch_token(h.run_id, h.branch_id) if src == 1 else bytes(h.final_token))
        items = [(int(r["event_id"]), int(r["version"])) for r in rows("vh", "n_vh_items")]
        points = [(names[int(r["key"])], bool(int(r["flags"]) & abi.ROW_RESETTABLE)) for r in rows("rp", "n_reset_points")]
        blobs = [(abi.STATE_EXECUTION, 0, 0, "", encode_struct("WorkflowExecutionInfo", execution_values(
            ex, token, items, points, "sticky-tl" if w in sticky else "", w in multi_branch, branches.get(w))))]
        for r in rows("act", "n_activity"):
            blobs.append((abi.STATE_ACTIVITY, int(r["schedule_id"]), to_unix_nano(r["last_heartbeat_time"]), "",
                          encode_struct("ActivityInfo", activity_values(r, names[int(r["key"])]))))
        for r in rows("timer", "n_timer"):
            blobs.append((abi.STATE_TIMER, 0, 0, names[int(r["key"])], encode_struct("TimerInfo", timer_values(r))))
        for r in rows("child", "n_child"):
            blobs.append((abi.STATE_CHILD, int(r["initiated_id"]), 0, "", encode_struct("ChildExecutionInfo", child_values(r))))
        for r in rows("rc", "n_rc"):
            blobs.append((abi.STATE_REQUEST_CANCEL, int(r["initiated_id"]), 0, "",
                          encode_struct("RequestCancelInfo", initiated_values(r, False))))
        for r in rows("sig", "n_signal"):
            blobs.append((abi.STATE_SIGNAL, int(r["initiated_id"]), 0, "", encode_struct("SignalInfo", initiated_values(r, True))))
        if rng is not None:
            rng.shuffle(blobs)
        workflows.append((int(ex["next_event_id"]), blobs))
    return build_blob_set(workflows)


# ---- the loaded image -------------------------------------------------------------------------------------
@dataclasses.dataclass
class LoadedImage(LoadedStates):
    """The dense loaded image (``crr_load_image``): a ``LoadedStates`` (mask: status OK) plus the per-table
    offsets, current branch tokens, key dictionaries, statuses and flags."""
    offsets: Optional[np.ndarray] = None      # int64 [LOAD_TABLES, n_wf + 1]
    tokens: Optional[np.ndarray] = None       # uint8
    key_off: Optional[np.ndarray] = None      # uint64 into key_bytes
    key_len: Optional[np.ndarray] = None
    key_bytes: Optional[np.ndarray] = None
    status: Optional[np.ndarray] = None       # int32 abi.LoadStatus
    flags: Optional[np.ndarray] = None        # uint32 LOAD_FLAG_*
    err_blob: int = -1                        # lowest malformed blob index

    def token(self, w: int) -> bytes:
        o = self.offsets[abi.LOAD_T_TOKEN]
        return self.tokens[int(o[w]):int(o[w + 1])].tobytes()

    def keys(self, w: int) -> List[str]:
        """Key id k's string at index k - 1."""
        o = self.offsets[abi.LOAD_T_KEYS]
        kb = self.key_bytes
        return [kb[int(self.key_off[k]):int(self.key_off[k]) + int(self.key_len[k])].tobytes().decode()
                for k in range(int(o[w]), int(o[w + 1]))]

    def resumable(self, mask=None) -> LoadedStates:
        """The states to resume as ``flatten(..., loaded=)`` takes them: the workflows in ``mask`` that loaded OK;
        the others' exec rows zeroed and their rows dropped (what ``ReplayResult.to_loaded`` does)."""
        m = self.mask if mask is None else (self.mask & np.asarray(mask, bool))
        ex = self.exec.copy()
        ex[~m] = np.zeros(1, abi.EXEC_ROW)
        rows = {name: self.rows[name][np.repeat(m, self.counts(name))].copy() for name in abi.LOAD_ROW_TABLES}
        return LoadedStates(ex, rows, m, self.interners)

    def image_bytes(self) -> Dict[str, bytes]:
        """Every buffer of the image as bytes (host against device comparisons)."""
        out = {"exec": self.exec.tobytes(), "offsets": self.offsets.tobytes(), "tokens": self.tokens.tobytes(),
               "key_off": self.key_off.tobytes(), "key_len": self.key_len.tobytes(), "key_bytes": self.key_bytes.tobytes(),
               "status": self.status.tobytes(), "flags": self.flags.tobytes()}
        out.update({name: self.rows[name].tobytes() for name in abi.LOAD_ROW_TABLES})
        return out


_ROW_DTYPES = {t[0]: t[1] for t in abi.TABLES}


class _ImageBuffers:
    """Host buffers of a ``crr_load_image`` sized from a summary."""

    def __init__(self, S: abi.CLoadSummary):
        n = int(S.n_wf)
        tot = [int(x) for x in S.totals]
        self.exec = np.zeros(n, abi.EXEC_ROW)
        self.rows = {name: np.zeros(tot[t], _ROW_DTYPES[name]) for t, name in enumerate(abi.LOAD_ROW_TABLES)}
        self.offsets = np.zeros((abi.LOAD_TABLES, n + 1), np.int64)
        self.tokens = np.zeros(tot[abi.LOAD_T_TOKEN], np.uint8)
        self.key_off = np.zeros(tot[abi.LOAD_T_KEYS], np.uint64)
        self.key_len = np.zeros(tot[abi.LOAD_T_KEYS], np.uint32)
        self.key_bytes = np.zeros(tot[abi.LOAD_T_KEY_BYTES], np.uint8)
        self.status = np.zeros(n, np.int32)
        self.flags = np.zeros(n, np.uint32)
        self.c = abi.CLoadImage()
        self.c.exec = _ptr(self.exec)
        for t, name in enumerate(abi.LOAD_ROW_TABLES):
            self.c.rows[t] = _ptr(self.rows[name])
        for f in ("offsets", "tokens", "key_off", "key_len", "key_bytes", "status", "flags"):
            setattr(self.c, f, _ptr(getattr(self, f)))

    def image(self, S: abi.CLoadSummary) -> LoadedImage:
        img = LoadedImage(self.exec, self.rows, self.status == 0, None, self.offsets, self.tokens, self.key_off,
                          self.key_len, self.key_bytes, self.status, self.flags, int(S.err_blob))
        img.interners = [dict([("", 0)] + [(s, k + 1) for k, s in enumerate(img.keys(w))]) for w in range(int(S.n_wf))]
        return img


def _c_batch(sbs: StateBlobSet, ptr) -> abi.CStateBatch:
    c = abi.CStateBatch()
    c.bytes, c.blob_off, c.blob, c.wf, c.strings = (ptr(sbs.bytes), ptr(sbs.blob_off), ptr(sbs.blob), ptr(sbs.wf),
                                                    ptr(sbs.strings))
    c.n_blobs, c.n_wf = sbs.n_blobs, sbs.n_wf
    return c


def _host_lib():
    from . import decode
    L = decode.lib()
    if not getattr(L, "_load_bound", False):
        vp = ctypes.c_void_p
        L.crr_load_states_host.argtypes = [vp, vp, vp, ctypes.c_int]
        L.crr_load_states_host.restype = ctypes.c_int
        L.crr_load_states_verify_host.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int]
        L.crr_load_states_verify_host.restype = ctypes.c_int
        L.crr_load_branches_host.argtypes = [vp, vp, vp, ctypes.c_int]
        L.crr_load_branches_host.restype = ctypes.c_int
        L.crr_load_store_checksums_host.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_int]
        L.crr_load_store_checksums_host.restype = ctypes.c_int
        L.crr_load_store_vh_host.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp, ctypes.c_int]
        L.crr_load_store_vh_host.restype = ctypes.c_int
        L.crr_load_mutation_host.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, ctypes.c_int]
        L.crr_load_mutation_host.restype = ctypes.c_int
        L.crr_load_store_exec_host.argtypes = [vp, vp, vp, ctypes.c_uint32] + [vp] * 9 + [ctypes.c_size_t, vp, ctypes.c_int]
        L.crr_load_store_exec_host.restype = ctypes.c_int
        L.crr_load_resume_host.argtypes = [vp, vp, vp, ctypes.c_uint32] + [vp] * 6 + [ctypes.c_size_t, vp, vp, ctypes.c_int]
        L.crr_load_resume_host.restype = ctypes.c_int
        L._load_bound = True
    return L


def _ptr(a):
    """The address of an array; None for None or an empty one."""
    return a.ctypes.data if a is not None and a.size else None


def _ref(c):
    return ctypes.byref(c) if c is not None else None


def _host_batch(sbs: StateBlobSet) -> abi.CStateBatch:
    return _c_batch(sbs, lambda a: a.ctypes.data)


def _host_call(name: str, *args) -> None:
    rc = getattr(_host_lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {rc}")


def _two_calls(name: str, head, sizing, tail, outputs):
    """Sizes, allocate, write: ``name(*head, *sizing, *tail)`` fills the sizes struct ``tail`` points to; ``outputs()``
    then allocates exactly from it and returns (what the caller keeps, the arguments in place of ``sizing``)."""
    _host_call(name, *head, *sizing, *tail)
    kept, args = outputs()
    _host_call(name, *head, *args, *tail)
    return kept


def load_states_host(sbs: StateBlobSet, threads: int = 1) -> LoadedImage:
    """Decode with the host restatement (``crr_load_states_host``); ``interners`` come from the dictionaries."""
    c, S = _host_batch(sbs), abi.CLoadSummary()

    def outputs():
        buf = _ImageBuffers(S)
        return buf, (ctypes.byref(buf.c),)
    return _two_calls("crr_load_states_host", (ctypes.byref(c),), (None,), (ctypes.byref(S), threads), outputs).image(S)


def stored_checksums(entries: Sequence) -> np.ndarray:
    """``abi.STORED_CHECKSUM`` rows from ``(version, flavor, value bytes)`` tuples (``checksum.Checksum``); ``None``
    or an empty value: none stored (``value_len`` 0).  A value of four bytes is read big-endian (crc.go:47-53);
    one of another length keeps its length only, which is all a mismatch needs."""
    out = np.zeros(len(entries), abi.STORED_CHECKSUM)
    for i, e in enumerate(entries):
        if e is None:
            continue
        version, flavor, value = e
        value = bytes(value or b"")
        out[i] = (int(version), int(flavor), struct.unpack(">I", value)[0] if len(value) == 4 else 0, len(value))
    return out


def _stored_array(stored, n_wf: int) -> Optional[np.ndarray]:
    if stored is None:
        return None
    a = np.ascontiguousarray(stored, dtype=abi.STORED_CHECKSUM)
    if a.shape != (n_wf,):
        raise ValueError(f"stored: {a.shape} rows for {n_wf} workflows")
    return a


def load_states_verify_host(sbs: StateBlobSet, stored=None, invalidate_before_ns: int = 0, threads: int = 1) -> np.ndarray:
    """The check ``mutableStateBuilder.Load`` makes of every state of ``sbs`` (``crr_load_states_verify_host``):
    ``abi.VERIFY_ROW`` per workflow.  ``stored``: ``abi.STORED_CHECKSUM`` rows (``stored_checksums``); None: compute only."""
    c = _host_batch(sbs)
    st = _stored_array(stored, sbs.n_wf)
    out = np.zeros(sbs.n_wf, abi.VERIFY_ROW)
    _host_call("crr_load_states_verify_host", ctypes.byref(c), _ptr(st), int(invalidate_before_ns), _ptr(out), threads)
    return out


# ---- every branch of the loaded states; tasks decided and routed against them (include/cadence_load_ndc.h) -----
@dataclasses.dataclass
class Branches:
    """Host image of ``crr_load_branches``: workflow w's histories in stored order are
    ``branches[branch_begin[w]:branch_begin[w + 1]]`` (items ``items[item_begin:item_begin + item_count]``), their
    tokens at the same indices as ranges of the blob set's bytes; a workflow that did not load has none."""
    branches: np.ndarray      # abi.NDC_BRANCH
    items: np.ndarray         # abi.VH_ITEM (the local items only)
    tokens: np.ndarray        # abi.BRANCH_TOKEN
    branch_begin: np.ndarray  # int64 [n_wf + 1]
    current: np.ndarray       # int32 [n_wf]

    def of(self, w: int):
        """[(item list, token range)] of workflow w."""
        out = []
        for b in range(int(self.branch_begin[w]), int(self.branch_begin[w + 1])):
            o, n = int(self.branches[b]["item_begin"]), int(self.branches[b]["item_count"])
            out.append(([(int(x["event_id"]), int(x["version"])) for x in self.items[o:o + n]],
                        (int(self.tokens[b]["off"]), int(self.tokens[b]["len"]))))
        return out

    def image_bytes(self) -> Dict[str, bytes]:
        return {f: getattr(self, f).tobytes() for f in ("branches", "items", "tokens", "branch_begin", "current")}


def load_branches_host(sbs: StateBlobSet, threads: int = 1) -> Branches:
    """The branch table by the host restatement (``crr_load_branches_host``)."""
    c, P = _host_batch(sbs), abi.CLoadNdcSizes()

    def outputs():
        out = Branches(np.zeros(int(P.n_branches), abi.NDC_BRANCH), np.zeros(int(P.n_items), abi.VH_ITEM),
                       np.zeros(int(P.n_branches), abi.BRANCH_TOKEN), np.zeros(int(P.n_wf) + 1, np.int64),
                       np.zeros(int(P.n_wf), np.int32))
        d = abi.CLoadBranches()
        for f in ("branches", "items", "tokens", "branch_begin", "current"):
            setattr(d, f, _ptr(getattr(out, f)))
        return out, (ctypes.byref(d),)
    return _two_calls("crr_load_branches_host", (ctypes.byref(c),), (None,), (ctypes.byref(P), threads), outputs)


# ---- the checksum to store once a routed task is committed (include/cadence_load_store.h) ----------------------
def _after_image(after: Optional[LoadedStates], n_wf: int):
    """``crr_load_image`` over the post-replay states (``ReplayResult.to_loaded``, canonical workflow order; a
    workflow outside its mask counts as not resumed): (the struct or None, the arrays it points into)."""
    if after is None:
        return None, ()
    if after.exec.shape[0] != n_wf:
        raise ValueError(f"after: {after.exec.shape[0]} states for {n_wf} workflows")
    keep = [np.ascontiguousarray(after.exec, dtype=abi.EXEC_ROW), np.zeros((abi.LOAD_TABLES, n_wf + 1), np.int64),
            np.ascontiguousarray(~np.asarray(after.mask, bool), dtype=np.int32)]
    c = abi.CLoadImage()
    c.exec, c.offsets, c.status = (a.ctypes.data if a.size else None for a in keep)
    for t, name in enumerate(abi.LOAD_ROW_TABLES):
        keep[1][t, 1:] = np.cumsum(after.counts(name))
        rows = np.ascontiguousarray(after.rows[name], dtype=_ROW_DTYPES[name])
        if rows.shape[0] != int(keep[1][t, n_wf]):
            raise ValueError(f"after: {rows.shape[0]} {name} rows for counts of {int(keep[1][t, n_wf])}")
        keep.append(rows)
        c.rows[t] = rows.ctypes.data if rows.size else None
    return c, keep


def _task_arrays(tasks, last_events, results=None, routes=None):
    tasks = np.ascontiguousarray(tasks, dtype=abi.REPL_TASK)
    n = int(tasks.shape[0])
    out = [tasks, np.ascontiguousarray(last_events, dtype=abi.LAST_EVENT)]
    if results is not None:
        out += [np.ascontiguousarray(results, dtype=abi.NDC_RESULT), np.ascontiguousarray(routes, dtype=abi.NDC_ROUTE)]
    for a in out:
        if a.shape != (n,):
            raise ValueError(f"{a.shape} rows for {n} tasks")
    return out


def _store_args(sbs: StateBlobSet, tasks, last_events, results, routes, after):
    """What the store-family host calls begin with: (the arguments up to the after-image, the number of tasks, what
    those arguments point into -- to be kept until the last call returns)."""
    c = _host_batch(sbs)
    arrays = _task_arrays(tasks, last_events, results, routes)
    img, keep = _after_image(after, sbs.n_wf)
    tasks, last, results, routes = (_ptr(a) for a in arrays)
    n = int(arrays[0].shape[0])
    return (ctypes.byref(c), tasks, last, n, results, routes, _ref(img)), n, (arrays, keep)


def store_checksums_host(sbs: StateBlobSet, tasks, last_events, results, routes, after: Optional[LoadedStates] = None,
                         threads: int = 1) -> np.ndarray:
    """The checksum to store with each task's state once the task is committed, by the host restatement
    (``crr_load_store_checksums_host``): ``abi.STORE_ROW`` per task.  ``results`` / ``routes``: the decisions of
    ``ndc_prepare``; ``last_events``: ``abi.LAST_EVENT`` per task; ``after``: the states the resumed replay left
    (``ReplayResult.to_loaded``), None: no task can be ``APPLIED``."""
    head, n, _keep = _store_args(sbs, tasks, last_events, results, routes, after)
    out = np.zeros(n, abi.STORE_ROW)
    _host_call("crr_load_store_checksums_host", *head, _ptr(out), threads)
    return out


# ---- the VersionHistories blob to store with it (include/cadence_load_store_vh.h) -------------------------------
def store_version_histories_host(sbs: StateBlobSet, tasks, last_events, results, routes, after: Optional[LoadedStates] = None,
                                 threads: int = 1):
    """The thriftrw ``VersionHistories`` DataBlob to store with each task's state once the task is committed (field
    122 of the execution blob), by the host restatement (``crr_load_store_vh_host``), arguments as
    ``store_checksums_host``: ``(rows abi.VH_BLOB_ROW[n], blob_off uint64[n + 1], bytes uint8[blob_off[n]])`` -- task
    k's blob is ``bytes[blob_off[k]:blob_off[k + 1]]``, empty unless its outcome is ``APPLIED`` or ``BACKFILLED``."""
    head, n, _keep = _store_args(sbs, tasks, last_events, results, routes, after)
    P = abi.CVhBlobSizes()

    def outputs():
        rows, off = np.zeros(n, abi.VH_BLOB_ROW), np.zeros(n + 1, np.uint64)
        out = np.zeros((int(P.n_bytes) + 15) // 16 * 16, np.uint8)
        return (rows, off, out), (_ptr(rows), off.ctypes.data, _ptr(out), out.size)
    rows, off, out = _two_calls("crr_load_store_vh_host", head, (None, None, None, 0), (ctypes.byref(P), threads), outputs)
    return rows, off, out[:int(P.n_bytes)].copy()


# ---- the pending-entry mutation to store with them (include/cadence_load_mutation.h) ----------------------------
@dataclasses.dataclass
class Mutation:
    """What ``crr_load_mutation_run`` wrote: per task a row (``abi.MUTATION_ROW``), the exec rows of the APPLIED tasks
    dense in task order, and per pending map (``abi.MUTATION_MAPS``) the upserted rows and the deleted keys."""
    rows: np.ndarray                     # abi.MUTATION_ROW [n_tasks]
    exec: np.ndarray                     # abi.EXEC_ROW [n_exec]
    upsert: Dict[str, np.ndarray]        # map name -> its row dtype
    deleted: Dict[str, np.ndarray]       # map name -> int64 keys (a timer's interned TimerID widened)

    def exec_of(self, k: int):
        """Task k's post-replay exec row, None when it has none."""
        i = int(self.rows[k]["exec_index"])
        return None if i == abi.MUTATION_NO_EXEC else self.exec[i]

    def upserts(self, k: int, name: str) -> np.ndarray:
        m = self.rows[k]["map"][abi.MUTATION_MAPS.index(name)]
        return self.upsert[name][int(m["upsert_begin"]):int(m["upsert_begin"]) + int(m["n_upsert"])]

    def deletes(self, k: int, name: str) -> np.ndarray:
        m = self.rows[k]["map"][abi.MUTATION_MAPS.index(name)]
        return self.deleted[name][int(m["delete_begin"]):int(m["delete_begin"]) + int(m["n_delete"])]

    @property
    def n_bytes(self) -> int:
        """The bytes that cross to the host: the rows, the exec rows, the upserted rows and the keys."""
        return int(self.rows.nbytes + self.exec.nbytes + sum(a.nbytes for a in self.upsert.values()) +
                   sum(a.nbytes for a in self.deleted.values()))

    def image_bytes(self) -> Dict[str, bytes]:
        out = {"rows": self.rows.tobytes(), "exec": self.exec.tobytes()}
        out.update({"upsert." + n: self.upsert[n].tobytes() for n in abi.MUTATION_MAPS})
        out.update({"deleted." + n: self.deleted[n].tobytes() for n in abi.MUTATION_MAPS})
        return out


def _mutation_buffers(P: abi.CMutationSizes):
    """Host buffers of exactly the plan's totals and the ``crr_mutation_out`` over them."""
    ex = np.zeros(int(P.n_exec), abi.EXEC_ROW)
    up = {n: np.zeros(int(P.n_upsert[t]), _ROW_DTYPES[n]) for t, n in enumerate(abi.MUTATION_MAPS)}
    de = {n: np.zeros(int(P.n_delete[t]), np.int64) for t, n in enumerate(abi.MUTATION_MAPS)}
    o = abi.CMutationOut()
    o.exec, o.exec_capacity = _ptr(ex), ex.shape[0]
    for t, n in enumerate(abi.MUTATION_MAPS):
        o.upsert[t], o.upsert_capacity[t] = _ptr(up[n]), up[n].shape[0]
        o.deleted[t], o.delete_capacity[t] = _ptr(de[n]), de[n].shape[0]
    return ex, up, de, o


def mutation_host(sbs: StateBlobSet, tasks, last_events, results, routes, after: Optional[LoadedStates] = None,
                  threads: int = 1) -> Mutation:
    """The pending-entry mutation to store with each task's state once the task is committed, by the host restatement
    (``crr_load_mutation_host``), arguments as ``store_checksums_host``."""
    head, n, _keep = _store_args(sbs, tasks, last_events, results, routes, after)
    P = abi.CMutationSizes()

    def outputs():
        rows = np.zeros(n, abi.MUTATION_ROW)
        ex, up, de, o = _mutation_buffers(P)
        return Mutation(rows, ex, up, de), (_ptr(rows), ctypes.byref(o))
    return _two_calls("crr_load_mutation_host", head, (None, None), (ctypes.byref(P), threads), outputs)


# ---- the execution blob to store with them (include/cadence_load_store_exec.h) -----------------------------------
def exec_blob_tasks(now_ns, history_size_delta) -> np.ndarray:
    """``abi.EXEC_BLOB_TASK`` rows from the tasks' commit clocks and history-size deltas."""
    out = np.zeros(len(now_ns), abi.EXEC_BLOB_TASK)
    out["now_ns"], out["history_size_delta"] = now_ns, history_size_delta
    return out


def _c_task_blobs(bs, ptr):
    """``crr_blob_batch`` over a ``blobs.BlobSet`` of the tasks' event blobs (only the fields the encoder reads)."""
    from .ingest import CBlobBatch
    c = CBlobBatch()
    c.bytes, c.blob_off, c.wf = ptr(bs.bytes), ptr(bs.blob_off), ptr(bs.wf)
    c.n_blobs, c.n_wf = bs.n_blobs, bs.n_wf
    return c


def store_executions_host(sbs: StateBlobSet, tasks, last_events, results, routes, exec_tasks,
                          after: Optional[LoadedStates] = None, task_blobs=None, upserts=None, threads: int = 1):
    """The execution blob to store with each task's state once the task is committed, by the host restatement
    (``crr_load_store_exec_host``), arguments as ``store_checksums_host`` and: ``exec_tasks`` ``abi.EXEC_BLOB_TASK``
    per task; ``task_blobs`` a ``blobs.BlobSet`` of the tasks' event blobs, workflow w of it the task of workflow w
    (None: a request id of the task leaves the blob to the host); ``upserts`` per workflow whether the task's events
    hold an UpsertWorkflowSearchAttributes.  ``(rows abi.EXEC_BLOB_ROW[n], blob_off uint64[n + 1], bytes uint8[])``
    -- task k's blob is ``bytes[blob_off[k]:blob_off[k + 1]]``, empty unless the device encodes it."""
    head, n, _keep = _store_args(sbs, tasks, last_events, results, routes, after)
    xt = np.ascontiguousarray(exec_tasks, dtype=abi.EXEC_BLOB_TASK)
    if xt.shape != (n,):
        raise ValueError(f"{xt.shape} exec_tasks rows for {n} tasks")
    tb = _c_task_blobs(task_blobs, _ptr) if task_blobs is not None else None
    up = None if upserts is None else np.ascontiguousarray(upserts, dtype=np.uint8)
    if up is not None and up.shape != (sbs.n_wf,):
        raise ValueError(f"{up.shape} upsert flags for {sbs.n_wf} workflows")
    P = abi.CExecBlobSizes()

    def outputs():
        rows, off = np.zeros(n, abi.EXEC_BLOB_ROW), np.zeros(n + 1, np.uint64)
        out = np.zeros(max(int(P.n_bytes), 1), np.uint8)
        return (rows, off, out), (_ptr(rows), off.ctypes.data, out.ctypes.data, int(P.n_bytes))
    rows, off, out = _two_calls("crr_load_store_exec_host", (*head, _ptr(xt), _ref(tb), _ptr(up)), (None, None, None, 0),
                                (ctypes.byref(P), threads), outputs)
    return rows, off, out[:int(P.n_bytes)].copy()


# ---- the resumed replay of routed tasks planned from loaded states (include/cadence_load_resume.h) ---------------
@dataclasses.dataclass
class ResumeImage:
    """What ``crr_load_resume_plan`` / ``_gather`` / ``_finalize`` (or ``crr_load_resume_host``) produce, on the host:
    the per-task rows, the gathered blob batch with its seeds and ``task_of``, and -- once the inserts of this call
    are known -- the descriptors, the token arena and the slot-table totals."""
    sizes: abi.CLoadResumeSizes
    rows: np.ndarray                      # abi.LOAD_RESUME_ROW [n_tasks]
    bytes: np.ndarray                     # uint8 [n_bytes]
    blob_off: np.ndarray                  # uint64 [n_blobs + 1]
    wf: np.ndarray                        # blobs.BLOB_WF [n_wf]
    key_begin: np.ndarray
    key_count: np.ndarray
    key_off: np.ndarray                   # uint64 [n_keys] into ``bytes``
    key_len: np.ndarray
    task_of: np.ndarray                   # int32 [n_wf], -1: no task
    desc: Optional[np.ndarray] = None     # abi.WORKFLOW [n_wf]
    arena: Optional[np.ndarray] = None    # uint8 [token_bytes]
    table_rows: Optional[List[int]] = None

    def blob(self, j: int) -> bytes:
        return self.bytes[int(self.blob_off[j]):int(self.blob_off[j + 1])].tobytes()

    def keys(self, p: int) -> List[str]:
        """Position p's seeded strings, key id k at index k - 1."""
        b, n = int(self.key_begin[p]), int(self.key_count[p])
        return [self.bytes[int(self.key_off[e]):int(self.key_off[e]) + int(self.key_len[e])].tobytes().decode()
                for e in range(b, b + n)]

    def token(self, p: int) -> bytes:
        o = int(self.desc[p]["start_token_off"])
        return self.arena[o:o + int(self.desc[p]["start_token_len"])].tobytes()

    def blob_set(self, strings: np.ndarray):
        """The gathered batch as a ``blobs.BlobSet`` (``strings``: the task batch's)."""
        from .blobs import BlobSet
        data = np.concatenate([self.bytes, np.zeros(abi.INGEST_PAD, np.uint8)])
        return BlobSet(bytes=data, blob_off=self.blob_off.copy(), wf=self.wf.copy(), strings=strings)

    def image_bytes(self) -> Dict[str, bytes]:
        """Every buffer as bytes (host against device comparisons)."""
        out = {f: getattr(self, f).tobytes() for f in ("rows", "bytes", "blob_off", "wf", "key_begin", "key_count",
                                                         "key_off", "key_len", "task_of")}
        out["sizes"] = bytes(self.sizes)[4:]          # (err apart)
        if self.desc is not None:
            out.update(desc=self.desc.tobytes(), arena=self.arena.tobytes(), table_rows=repr(self.table_rows).encode())
        return out


class _ResumeBuffers:
    """Host buffers of a ``crr_load_resume_out`` sized exactly from a plan."""

    def __init__(self, P: abi.CLoadResumeSizes):
        from .blobs import BLOB_WF
        n = int(P.n_wf)
        self.bytes = np.zeros(int(P.n_bytes), np.uint8)
        self.blob_off = np.zeros(int(P.n_blobs) + 1, np.uint64)
        self.wf = np.zeros(n, BLOB_WF)
        self.key_begin, self.key_count = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.key_off, self.key_len = np.zeros(int(P.n_keys), np.uint64), np.zeros(int(P.n_keys), np.uint32)
        self.task_of = np.zeros(n, np.int32)
        self.c = abi.CLoadResumeOut()
        for f in ("bytes", "blob_off", "wf", "key_begin", "key_count", "key_off", "key_len", "task_of"):
            setattr(self.c, f, _ptr(getattr(self, f)))
        self.c.bytes_capacity, self.c.blob_capacity, self.c.key_capacity = int(P.n_bytes), int(P.n_blobs), int(P.n_keys)


def resume_counts_of(batch: HistoryBatch) -> np.ndarray:
    """The int32 ``[RESUME_COUNT_ROWS, n_wf]`` counts ``crr_load_resume_host`` takes, from a canonical batch of this
    call's events alone (``decode.decode_histories`` of the gathered blobs, or ``flatten`` without ``loaded``): its
    capacities are this call's inserts."""
    out = np.zeros((abi.RESUME_COUNT_ROWS, batch.n_wf), np.int32)
    out[0], out[1] = batch.wf["ev_count"], batch.wf["empty_batch_at"]
    for t, (_name, _dt, _base, cap_f, _n) in enumerate(abi.TABLES):
        out[2 + t] = batch.wf[cap_f]
    return out


def load_resume_host(sbs: StateBlobSet, tasks, routes, task_blobs, counts: Optional[np.ndarray] = None,
                     threads: int = 1) -> ResumeImage:
    """Plan the resumed replay of ``tasks`` onto the states of ``sbs`` with the host restatement
    (``crr_load_resume_host``): ``routes`` ``abi.NDC_ROUTE`` per task, ``task_blobs`` a ``blobs.BlobSet`` whose
    workflow k holds task k's event blobs; ``counts`` (``resume_counts_of``) adds the descriptors, the arena and the
    totals."""
    c = _host_batch(sbs)
    tasks = np.ascontiguousarray(tasks, dtype=abi.REPL_TASK)
    routes = np.ascontiguousarray(routes, dtype=abi.NDC_ROUTE)
    n = int(tasks.shape[0])
    if routes.shape != (n,):
        raise ValueError(f"{routes.shape} routes for {n} tasks")
    tb = _c_task_blobs(task_blobs, _ptr)
    P, Q = abi.CLoadResumeSizes(), abi.CLoadResumeTotals()
    cnt = None
    if counts is not None:
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        if cnt.shape != (abi.RESUME_COUNT_ROWS, sbs.n_wf):
            raise ValueError(f"{cnt.shape} counts for {sbs.n_wf} workflows")

    def outputs():
        rows = np.zeros(n, abi.LOAD_RESUME_ROW)
        buf = _ResumeBuffers(P)
        desc = np.zeros(sbs.n_wf, abi.WORKFLOW) if cnt is not None else None
        arena = np.zeros(int(P.token_bytes), np.uint8) if cnt is not None else None
        return (rows, buf, desc, arena), (_ptr(rows), ctypes.byref(buf.c), _ptr(desc), _ptr(arena), int(P.token_bytes))
    rows, buf, desc, arena = _two_calls("crr_load_resume_host",
                                        (ctypes.byref(c), _ptr(tasks), _ptr(routes), n, ctypes.byref(tb), _ptr(cnt)),
                                        (None, None, None, None, 0), (ctypes.byref(P), ctypes.byref(Q), threads), outputs)
    return ResumeImage(P, rows, buf.bytes, buf.blob_off, buf.wf, buf.key_begin, buf.key_count, buf.key_off, buf.key_len,
                       buf.task_of, desc, arena, [int(x) for x in Q.table_rows] if cnt is not None else None)


def _struct_fields(raw: bytes) -> Dict[int, bytes]:
    """The top-level fields of a thrift-binary struct whose fields are scalars, binaries, list<binary> or
    map<binary, binary> (the six state structs): field id -> the bytes of a binary field, b"" for any other."""
    size = {2: 1, 3: 1, 4: 8, 6: 2, 8: 4, 10: 8}
    out, p = {}, 0

    def binary(p):
        n = struct.unpack_from(">i", raw, p)[0]
        return raw[p + 4:p + 4 + n], p + 4 + n
    while raw[p] != 0:
        t, fid = raw[p], struct.unpack_from(">h", raw, p + 1)[0]
        p += 3
        out[fid] = b""
        if t in size:
            p += size[t]
        elif t == T_STRING:
            out[fid], p = binary(p)
        elif t == T_LIST and raw[p] == T_STRING:
            n = struct.unpack_from(">i", raw, p + 1)[0]
            p += 5
            for _ in range(n):
                p = binary(p)[1]
        elif t == T_MAP and raw[p] == T_STRING and raw[p + 1] == T_STRING:
            n = struct.unpack_from(">i", raw, p + 2)[0]
            p += 6
            for _ in range(2 * n):
                p = binary(p)[1]
        else:
            raise ValueError(f"field {fid}: type {t} is not one the state structs use")
    return out


_MAP_KIND = {"act": abi.STATE_ACTIVITY, "timer": abi.STATE_TIMER, "child": abi.STATE_CHILD, "rc": abi.STATE_REQUEST_CANCEL,
             "sig": abi.STATE_SIGNAL}


def apply_mutation(sbs: StateBlobSet, tasks, mutation: Mutation, vh_blobs, checksums, names, reset_points=None,
                   exec_blobs=None) -> StateBlobSet:
    """What a host shim does with the device's result: the store after every generated task's write.  For each task
    whose outcome is ``APPLIED`` or ``BACKFILLED`` its state's blobs (other states are kept as they are): the
    entries whose keys the mutation deletes dropped, the blobs of the upserted rows replaced or added (encoded with
    ``activity_values`` / ``timer_values`` / ``child_values`` / ``initiated_values``), and the execution blob written
    again -- from the gathered exec row for an APPLIED task -- with the task's ``VersionHistories`` blob as field 122.
    ``vh_blobs``: ``store_version_histories``' ``(rows, blob_off, bytes)``; ``checksums``: ``store_checksums``' rows
    (all three results must agree on every outcome); ``names``: per workflow its key dictionary after the task,
    ``{key id: string}`` or the interner ``{string: key id}``.  ``reset_points``: ``{workflow: [(binary checksum,
    resettable)]}`` for the tasks flagged ``MUTATION_RESET_POINTS_CHANGED`` (the reset-point rows are not part of
    the mutation); the others keep their stored ``AutoResetPoints``.  A state with more than one generated task takes
    the last one's write.  ``exec_blobs``: ``store_executions``' ``(rows, blob_off, bytes)``; a task with a blob there
    (``len`` > 0) takes it verbatim as its execution blob and ``next_event_id`` from its row, the others (left to the
    host by a ``EXEC_BLOB_HOST_*`` flag) are encoded here as without it."""
    tasks = np.ascontiguousarray(tasks, dtype=abi.REPL_TASK)
    vh_rows, vh_off, vh_bytes = vh_blobs
    rows = mutation.rows
    if not ((rows["outcome"] == vh_rows["outcome"]).all() and (rows["outcome"] == checksums["outcome"]).all()):
        raise ValueError("the mutation, the VersionHistories blobs and the checksums disagree on an outcome")
    states = []
    for w in range(sbs.n_wf):
        b0, nb = int(sbs.wf["blob_begin"][w]), int(sbs.wf["blob_count"][w])
        blobs = []
        for b in range(b0, b0 + nb):
            B = sbs.blob[b]
            s = sbs.strings[int(B["str_off"]):int(B["str_off"]) + int(B["str_len"])].tobytes().decode()
            blobs.append((int(B["kind"]), int(B["id"]), int(B["aux_time"]), s, sbs.blob_bytes(b)))
        states.append([int(sbs.wf["next_event_id"][w]), blobs])
    for k in range(tasks.shape[0]):
        outcome = int(rows[k]["outcome"])
        if outcome not in (abi.StoreOutcome.APPLIED, abi.StoreOutcome.BACKFILLED):
            continue
        w = int(tasks[k]["wf"])
        key_names = names[w]
        if any(isinstance(x, str) for x in key_names):
            key_names = _inverse(key_names)
        blobs = states[w][1]
        vh = bytes(vh_bytes[int(vh_off[k]):int(vh_off[k + 1])])
        ei = [i for i, b in enumerate(blobs) if b[0] == abi.STATE_EXECUTION][0]
        ready = None                                 # the execution blob as the device wrote it
        if exec_blobs is not None:
            x_rows, x_off, x_bytes = exec_blobs
            if int(x_rows[k]["outcome"]) != outcome:
                raise ValueError(f"task {k}: the execution blobs and the mutation disagree on the outcome")
            if int(x_rows[k]["len"]):
                ready = bytes(x_bytes[int(x_off[k]):int(x_off[k + 1])])
        if ready is not None:
            blobs[ei] = (abi.STATE_EXECUTION, 0, 0, "", ready)
            states[w][0] = int(x_rows[k]["next_event_id"])
            if outcome == abi.StoreOutcome.BACKFILLED:
                continue
        old = _struct_fields(blobs[ei][4]) if ready is None else None
        if outcome == abi.StoreOutcome.BACKFILLED:   # only field 122 changes: the blob's other bytes are kept
            raw = blobs[ei][4]
            at = raw.index(struct.pack(">bhi", T_STRING, 122, len(old[122])) + old[122])
            blobs[ei] = blobs[ei][:4] + (raw[:at] + struct.pack(">bhi", T_STRING, 122, len(vh)) + vh + raw[at + 7 + len(old[122]):],)
            continue
        if ready is None:
            ex = mutation.exec_of(k)
            v = execution_values(ex, old[104], [], [])
            v["VersionHistories"] = vh
            if int(rows[k]["flags"]) & abi.MUTATION_RESET_POINTS_CHANGED:
                if reset_points is None or w not in reset_points:
                    raise ValueError(f"task {k}: the reset points of workflow {w} changed and none were given")
                v["AutoResetPoints"] = encode_reset_points(reset_points[w])
            else:
                v["AutoResetPoints"] = old[115]
            blobs[ei] = (abi.STATE_EXECUTION, 0, 0, "", encode_struct("WorkflowExecutionInfo", v))
            states[w][0] = int(ex["next_event_id"])
        for name in abi.MUTATION_MAPS:
            kind = _MAP_KIND[name]

            def key_of(b, timer=name == "timer"):
                return b[3] if timer else b[1]
            gone = set(key_names[int(x)] if name == "timer" else int(x) for x in mutation.deletes(k, name))
            fresh = {}
            for r in mutation.upserts(k, name):
                if name == "act":
                    fresh[int(r["schedule_id"])] = (kind, int(r["schedule_id"]), to_unix_nano(r["last_heartbeat_time"]), "",
                                                    encode_struct("ActivityInfo", activity_values(r, key_names[int(r["key"])])))
                elif name == "timer":
                    fresh[key_names[int(r["key"])]] = (kind, 0, 0, key_names[int(r["key"])], encode_struct("TimerInfo", timer_values(r)))
                elif name == "child":
                    fresh[int(r["initiated_id"])] = (kind, int(r["initiated_id"]), 0, "", encode_struct("ChildExecutionInfo", child_values(r)))
                else:
                    fresh[int(r["initiated_id"])] = (kind, int(r["initiated_id"]), 0, "", encode_struct(
                        "SignalInfo" if name == "sig" else "RequestCancelInfo", initiated_values(r, name == "sig")))
            kept = []
            for b in blobs:   # REPLACE per upserted entry, then DELETE per deleted key (workflowStateMaps.go)
                if b[0] != kind:
                    kept.append(b)
                elif key_of(b) not in gone:
                    kept.append(fresh.pop(key_of(b), b))
            blobs[:] = kept + [b for key, b in fresh.items() if key not in gone]
    return build_blob_set([(nei, blobs) for nei, blobs in states])


def apply_mask(routes: np.ndarray, tasks: Optional[np.ndarray] = None, n_wf: Optional[int] = None) -> np.ndarray:
    """The workflows whose task is to be replayed onto the placed rows (``ROUTE_APPLY_CURRENT``), as
    ``LoadedImage.resumable(mask=...)`` takes them (canonical workflow order; ``replication.BlobReplication``'s
    ``split`` is the same mask at the device positions, ``mask[batch.perm]``).  ``tasks`` (``abi.REPL_TASK``) names
    each route's workflow; without it route k belongs to workflow k."""
    apply = np.asarray(routes["route"]) == abi.ROUTE_APPLY_CURRENT
    if tasks is None:
        return apply if n_wf is None else np.concatenate([apply, np.zeros(max(n_wf - apply.size, 0), bool)])[:n_wf]
    wf = np.asarray(tasks["wf"], np.int64)
    n = int(n_wf if n_wf is not None else (wf.max() + 1 if wf.size else 0))
    mask = np.zeros(n, bool)
    ok = apply & (wf < n)
    mask[wf[ok]] = True
    return mask


@dataclasses.dataclass
class DeviceBranches:
    """The branch table resident in HBM (``crr_load_branches``); ``items`` holds the local items, then the incoming
    items of the tasks it was built with."""
    plan: abi.CLoadNdcSizes
    tensors: Dict[str, object]
    c: abi.CLoadBranches

    def read(self) -> Branches:
        P = self.plan

        def host(f, dt, n):
            return self.tensors[f][:n * np.dtype(dt).itemsize].cpu().numpy().view(dt).copy()
        return Branches(host("branches", abi.NDC_BRANCH, int(P.n_branches)), host("items", abi.VH_ITEM, int(P.n_items)),
                        host("tokens", abi.BRANCH_TOKEN, int(P.n_branches)), host("branch_begin", np.int64, int(P.n_wf) + 1),
                        host("current", np.int32, int(P.n_wf)))


@dataclasses.dataclass
class DeviceStates:
    """A StateBlobSet resident in HBM."""
    blobs: StateBlobSet
    tensors: Dict[str, object]
    c: abi.CStateBatch


class StateLoader:
    """The device loader: ``upload`` the persisted bytes, ``plan`` (decode into the scratch), then ``read`` the
    dense image back, ``verify`` the stored checksums against it or ``place`` it into a resumed batch's outputs.
    No host fallback: a missing library or device raises."""

    def __init__(self, engine):
        self.engine = engine
        self.torch = engine.torch
        self.lib = engine.lib
        vp = ctypes.c_void_p
        L = self.lib
        L.crr_load_scratch_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.crr_load_scratch_bytes.restype = ctypes.c_size_t
        L.crr_load_states_plan.argtypes = [vp, vp, ctypes.c_size_t, vp, vp]
        L.crr_load_states_plan.restype = ctypes.c_int
        L.crr_load_states_read.argtypes = [vp, ctypes.c_size_t, vp, vp, vp]
        L.crr_load_states_read.restype = ctypes.c_int
        L.crr_load_states_place.argtypes = [vp, ctypes.c_size_t, vp, vp, vp, vp, vp]
        L.crr_load_states_place.restype = ctypes.c_int
        L.crr_load_states_verify.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_int64, vp, vp]
        L.crr_load_states_verify.restype = ctypes.c_int
        L.crr_load_ndc_scratch_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.crr_load_ndc_scratch_bytes.restype = ctypes.c_size_t
        L.crr_load_ndc_plan.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_size_t, vp, vp]
        L.crr_load_ndc_plan.restype = ctypes.c_int
        L.crr_load_ndc_run.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp, vp, ctypes.c_size_t, vp, vp, vp, vp, vp, vp, vp]
        L.crr_load_ndc_run.restype = ctypes.c_int
        L.crr_load_store_checksums.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_uint32] + [vp] * 9
        L.crr_load_store_checksums.restype = ctypes.c_int
        L.crr_load_store_vh_scratch_bytes.argtypes = [ctypes.c_uint32]
        L.crr_load_store_vh_scratch_bytes.restype = ctypes.c_size_t
        L.crr_load_store_vh_plan.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_uint32] + [vp] * 10 + [ctypes.c_size_t, vp, vp]
        L.crr_load_store_vh_plan.restype = ctypes.c_int
        L.crr_load_store_vh_run.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp] + [vp] * 11 + [ctypes.c_size_t, vp]
        L.crr_load_store_vh_run.restype = ctypes.c_int
        L.crr_load_mutation_scratch_bytes.argtypes = [ctypes.c_uint32]
        L.crr_load_mutation_scratch_bytes.restype = ctypes.c_size_t
        L.crr_load_mutation_plan.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_uint32] + [vp] * 9 + [ctypes.c_size_t, vp, vp]
        L.crr_load_mutation_plan.restype = ctypes.c_int
        L.crr_load_mutation_run.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp] + [vp] * 11 + [ctypes.c_size_t, vp]
        L.crr_load_mutation_run.restype = ctypes.c_int
        L.crr_load_store_exec_scratch_bytes.argtypes = [ctypes.c_uint32]
        L.crr_load_store_exec_scratch_bytes.restype = ctypes.c_size_t
        L.crr_load_store_exec_plan.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_uint32] + [vp] * 15 + [ctypes.c_size_t, vp, vp]
        L.crr_load_store_exec_plan.restype = ctypes.c_int
        L.crr_load_store_exec_run.argtypes = ([vp, vp, ctypes.c_size_t, vp, vp, vp] + [vp] * 15 +
                                              [ctypes.c_size_t, vp, vp, vp, ctypes.c_size_t, vp])
        L.crr_load_store_exec_run.restype = ctypes.c_int
        L.crr_load_resume_scratch_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.crr_load_resume_scratch_bytes.restype = ctypes.c_size_t
        L.crr_load_resume_plan.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_size_t, vp, vp]
        L.crr_load_resume_plan.restype = ctypes.c_int
        L.crr_load_resume_gather.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp, vp, vp, ctypes.c_size_t, vp, vp, vp]
        L.crr_load_resume_gather.restype = ctypes.c_int
        L.crr_load_resume_finalize.argtypes = [vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_uint64, vp, ctypes.c_size_t, vp, vp, vp,
                                               ctypes.c_size_t, vp, vp]
        L.crr_load_resume_finalize.restype = ctypes.c_int
        L.crr_load_resume_settle.argtypes = [vp, vp, ctypes.c_uint32, vp]
        L.crr_load_resume_settle.restype = ctypes.c_int
        L.crr_ingest_resume_counts.argtypes = [vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                                               ctypes.POINTER(ctypes.c_uint64)]
        L.crr_ingest_resume_counts.restype = ctypes.c_int
        self.last_ndc = None
        self.scratch = None
        self.scratch_bytes = 0
        self.summary = None
        self.grown = 0          # the size the last plan grew the scratch to (0: it fitted)

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.engine.dev).cuda_stream)

    def upload(self, sbs: StateBlobSet) -> DeviceStates:
        from .engine import _dev_bytes
        T = {f: _dev_bytes(self.torch, getattr(sbs, f), self.engine.dev, pad=abi.INGEST_PAD)
             for f in ("bytes", "blob_off", "blob", "wf", "strings")}
        return DeviceStates(sbs, T, self._c(sbs, T))

    @staticmethod
    def _c(sbs, T):
        c = abi.CStateBatch()
        for f in ("bytes", "blob_off", "blob", "wf", "strings"):
            setattr(c, f, T[f].data_ptr())
        c.n_blobs, c.n_wf = sbs.n_blobs, sbs.n_wf
        return c

    def _alloc(self, size: int):
        self.scratch = self.torch.empty(size + 16, dtype=self.torch.uint8, device=self.engine.dev)
        self.scratch_bytes = size

    def plan(self, ds: DeviceStates, scratch_bytes: Optional[int] = None) -> abi.CLoadSummary:
        """Decode; a scratch that proves too small is grown once to what the plan asked for."""
        want = int(scratch_bytes if scratch_bytes is not None else
                   self.lib.crr_load_scratch_bytes(ds.c.n_blobs, ds.c.n_wf))
        if self.scratch is None or self.scratch_bytes < want or scratch_bytes is not None:
            self._alloc(want)
        S = abi.CLoadSummary()
        self.grown = 0
        for _ in range(2):
            rc = self.lib.crr_load_states_plan(ctypes.byref(ds.c), ctypes.c_void_p(self.scratch.data_ptr()),
                                               ctypes.c_size_t(self.scratch_bytes), ctypes.byref(S), self._stream())
            if rc != 0:
                raise RuntimeError(f"crr_load_states_plan failed: {rc}")
            if S.err != abi.SCRATCH_TOO_SMALL:
                break
            self.grown = int(S.scratch_needed)
            self._alloc(self.grown)
        if S.err != 0:
            raise RuntimeError(f"crr_load_states_plan: err {S.err}")
        self.summary = S
        return S

    def read(self) -> LoadedImage:
        """The last plan's dense image, copied to the host."""
        S = self.summary
        buf = _ImageBuffers(S)
        rc = self.lib.crr_load_states_read(ctypes.c_void_p(self.scratch.data_ptr()), ctypes.c_size_t(self.scratch_bytes),
                                           ctypes.byref(S), ctypes.byref(buf.c), self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_states_read failed: {rc}")
        self.torch.cuda.synchronize(self.engine.dev)
        return buf.image(S)

    def verify(self, ds: DeviceStates, stored=None, invalidate_before_ns: int = 0) -> np.ndarray:
        """The check ``mutableStateBuilder.Load`` makes of every state of the last plan (``crr_load_states_verify``),
        ``ds`` being the batch that plan decoded: ``abi.VERIFY_ROW`` per workflow, copied to the host.  ``stored``:
        ``abi.STORED_CHECKSUM`` rows (``stored_checksums``); None: compute only.  Valid before or after ``read`` /
        ``place``."""
        from .engine import _dev_bytes
        n = int(ds.c.n_wf)
        st = _stored_array(stored, n)
        d_st = _dev_bytes(self.torch, st, self.engine.dev) if st is not None else None
        d_out = self.torch.empty(max(n, 1) * abi.VERIFY_ROW.itemsize, dtype=self.torch.uint8, device=self.engine.dev)
        rc = self.lib.crr_load_states_verify(ctypes.byref(ds.c), ctypes.c_void_p(self.scratch.data_ptr()),
                                             ctypes.c_size_t(self.scratch_bytes), ctypes.byref(self.summary),
                                             ctypes.c_void_p(d_st.data_ptr() if d_st is not None else None),
                                             int(invalidate_before_ns), ctypes.c_void_p(d_out.data_ptr()), self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_states_verify failed: {rc}")
        return d_out[:n * abi.VERIFY_ROW.itemsize].cpu().numpy().view(abi.VERIFY_ROW).copy()

    def place(self, db, perm: Optional[np.ndarray] = None):
        """Scatter the last plan's image into ``db``'s outputs (an ``engine.DeviceBatch``): device position p takes
        loaded workflow ``perm[p]`` (default: the batch's own ``perm``, identity for a canonical batch)."""
        if perm is None:
            perm = db.batch.perm
        p_ptr = None
        if perm is not None:
            db.tensors["load_perm"] = self.torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int64).astype(np.int32)).to(self.engine.dev)
            p_ptr = db.tensors["load_perm"].data_ptr()
        rc = self.lib.crr_load_states_place(ctypes.c_void_p(self.scratch.data_ptr()), ctypes.c_size_t(self.scratch_bytes),
                                            ctypes.byref(self.summary), ctypes.byref(db.c_in), ctypes.c_void_p(p_ptr),
                                            ctypes.byref(db.c_out), self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_states_place failed: {rc}")

    # ---- include/cadence_load_ndc.h ------------------------------------------------------------------------
    def _ndc(self, ds: DeviceStates, tasks, incoming_items):
        """Plan (one synchronisation) and enqueue the branch table of the last plan's states and, with tasks, their
        decisions and routes: (DeviceBranches, device tensors of results / routes / out_items / out_begin)."""
        from .engine import _dev_bytes
        torch, dev = self.torch, self.engine.dev
        tasks = np.zeros(0, abi.REPL_TASK) if tasks is None else np.ascontiguousarray(tasks, dtype=abi.REPL_TASK)
        inc = np.zeros(0, abi.VH_ITEM) if incoming_items is None else np.ascontiguousarray(incoming_items, dtype=abi.VH_ITEM)
        n_tasks, n_inc = int(tasks.shape[0]), int(inc.shape[0])
        d_tasks = _dev_bytes(torch, tasks, dev) if n_tasks else None
        d_inc = _dev_bytes(torch, inc, dev) if n_inc else None
        return self._ndc_device(ds, d_tasks, n_tasks, d_inc, n_inc)

    def _ndc_device(self, ds: DeviceStates, d_tasks, n_tasks: int, d_inc, n_inc: int):
        """``_ndc`` on tasks and incoming items already resident (device byte tensors; None: none)."""
        torch, dev, n_wf = self.torch, self.engine.dev, int(ds.c.n_wf)
        work_bytes = int(self.lib.crr_load_ndc_scratch_bytes(n_wf, n_tasks))
        work = torch.empty(work_bytes + 16, dtype=torch.uint8, device=dev)
        scratch = ctypes.c_void_p(self.scratch.data_ptr() if self.scratch is not None else None)
        P = abi.CLoadNdcSizes()

        def ptr(t):
            return ctypes.c_void_p(t.data_ptr() if t is not None else None)
        rc = self.lib.crr_load_ndc_plan(ctypes.byref(ds.c), scratch, ctypes.c_size_t(self.scratch_bytes),
                                        ctypes.byref(self.summary), ptr(d_tasks), n_tasks, n_inc, ptr(work),
                                        ctypes.c_size_t(work_bytes), ctypes.byref(P), self._stream())
        if rc != 0 or P.err != 0:
            raise RuntimeError(f"crr_load_ndc_plan failed: {rc} (err {P.err})")

        def buf(n, dt, fill=False):   # every buffer is written in full by the call, but for the new-branch items' room
            return (torch.zeros if fill else torch.empty)(max(n, 1) * np.dtype(dt).itemsize, dtype=torch.uint8, device=dev)
        T = {"branches": buf(int(P.n_branches), abi.NDC_BRANCH), "items": buf(int(P.n_items) + n_inc, abi.VH_ITEM),
             "tokens": buf(int(P.n_branches), abi.BRANCH_TOKEN), "branch_begin": buf(n_wf + 1, np.int64),
             "current": buf(n_wf, np.int32)}
        d = abi.CLoadBranches()
        for f, t in T.items():
            setattr(d, f, t.data_ptr())
        out = {"results": buf(n_tasks, abi.NDC_RESULT), "routes": buf(n_tasks, abi.NDC_ROUTE),
               "out_items": buf(int(P.n_out_items), abi.VH_ITEM, True), "out_begin": buf(n_tasks, np.uint32)}
        rc = self.lib.crr_load_ndc_run(ctypes.byref(ds.c), scratch, ctypes.c_size_t(self.scratch_bytes),
                                       ctypes.byref(self.summary), ptr(d_tasks), ptr(d_inc), ptr(work),
                                       ctypes.c_size_t(work_bytes), ctypes.byref(P), ctypes.byref(d), ptr(out["results"]),
                                       ptr(out["routes"]), ptr(out["out_items"]), ptr(out["out_begin"]), self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_ndc_run failed: {rc}")
        T["work"], T["tasks"], T["incoming"] = work, d_tasks, d_inc   # alive until the stream has run them
        return DeviceBranches(P, T, d), out

    def branches(self, ds: DeviceStates) -> DeviceBranches:
        """Every branch of every state of the last plan (``ds`` the batch it decoded), left on the device."""
        return self._ndc(ds, None, None)[0]

    def ndc_prepare(self, ds: DeviceStates, tasks, incoming_items, on_device: bool = False):
        """``prepareVersionHistory`` and ``prepareMutableState`` for replication ``tasks`` (``abi.REPL_TASK``, their
        incoming VersionHistoryItems in ``incoming_items``, ``abi.VH_ITEM``) against the states of the last plan:
        ``(results abi.NDC_RESULT[n], routes abi.NDC_ROUTE[n], out_items abi.VH_ITEM[])`` -- task k's new-branch
        items are ``out_items[out_begin[k]:][:results[k]["new_item_count"]]``, ``out_begin`` the exclusive prefix
        over the tasks of the longest local branch of each task's workflow (``self.last_ndc`` keeps it, the
        ``DeviceBranches`` and the device tensors).  ``on_device``: the three as device byte tensors, nothing
        copied back."""
        br, out = self._ndc(ds, tasks, incoming_items)
        self.last_ndc = (br, out)
        if on_device:
            return out["results"], out["routes"], out["out_items"]
        n = int(br.plan.n_tasks)

        def host(f, dt, k):
            return out[f][:k * np.dtype(dt).itemsize].cpu().numpy().view(dt).copy()
        self.last_out_begin = host("out_begin", np.uint32, n)
        return (host("results", abi.NDC_RESULT, n), host("routes", abi.NDC_ROUTE, n),
                host("out_items", abi.VH_ITEM, int(br.plan.n_out_items)))

    # ---- include/cadence_load_store.h ----------------------------------------------------------------------
    def _store_args(self, ds: DeviceStates, tasks, last_events, db, perm, what: str):
        """The read-only arguments ``crr_load_store_checksums`` and the calls of cadence_load_store_vh.h share, for
        the tasks the last ``ndc_prepare`` decided: (n, the tensors to keep alive, the arguments up to and including
        ``last_events``, the ones from ``results`` through ``position``)."""
        from .engine import _dev_bytes
        if self.last_ndc is None:
            raise RuntimeError(f"{what}: no ndc_prepare to take the decisions from")
        torch, dev = self.torch, self.engine.dev
        br, out = self.last_ndc
        tasks, last = _task_arrays(tasks, last_events)
        n, n_wf = int(tasks.shape[0]), int(ds.c.n_wf)
        if n > int(br.plan.n_tasks):
            raise ValueError(f"{n} tasks, {int(br.plan.n_tasks)} decided")
        T = {"tasks": _dev_bytes(torch, tasks, dev), "last": _dev_bytes(torch, last, dev)}
        if db is not None and perm is None:
            perm = db.batch.perm
        if db is not None and perm is not None:
            perm = np.asarray(perm, np.int64)
            pos = np.full(n_wf, abi.POSITION_NONE, np.uint32)
            here = np.nonzero((perm >= 0) & (perm < n_wf))[0]
            pos[perm[here]] = here
            T["position"] = _dev_bytes(torch, pos, dev)

        def ptr(t):
            return ctypes.c_void_p(t.data_ptr() if t is not None else None)
        head = (ctypes.byref(ds.c), ptr(self.scratch), ctypes.c_size_t(self.scratch_bytes), ctypes.byref(self.summary),
                ptr(T["tasks"]), ptr(T["last"]))
        tail = (ptr(out["results"]), ptr(out["routes"]), ctypes.byref(br.c), ctypes.byref(br.plan),
                ctypes.byref(db.c_in) if db is not None else None, ctypes.byref(db.c_out) if db is not None else None,
                ptr(T.get("position")))
        return n, T, head, tail

    def store_checksums(self, ds: DeviceStates, tasks, last_events, db=None, on_device: bool = False, perm=None):
        """The checksum to store with each task's state once the task is committed (``crr_load_store_checksums``),
        for the ``tasks`` the last ``ndc_prepare`` decided against the last plan's states (``self.last_ndc``: its
        decisions, routes and branch table stay on the device): ``abi.STORE_ROW`` per task.  ``last_events``:
        ``abi.LAST_EVENT`` per task.  ``db``: the resumed batch (an ``engine.DeviceBatch``) after its replay was
        enqueued, for the tasks routed to the current branch; the position map is the inverse of ``perm`` (default:
        the batch's own, as in ``place``).  Enqueued on the current stream; ``on_device``: the rows as a device byte
        tensor, nothing copied back."""
        n, T, head, tail = self._store_args(ds, tasks, last_events, db, perm, "store_checksums")
        T["rows"] = self.torch.empty(max(n, 1) * abi.STORE_ROW.itemsize, dtype=self.torch.uint8, device=self.engine.dev)
        rc = self.lib.crr_load_store_checksums(*head, n, *tail, ctypes.c_void_p(T["rows"].data_ptr()), self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_store_checksums failed: {rc}")
        self.last_store = T   # alive until the stream has run the kernel
        if on_device:
            return T["rows"]
        return T["rows"][:n * abi.STORE_ROW.itemsize].cpu().numpy().view(abi.STORE_ROW).copy()

    # ---- include/cadence_load_store_vh.h -------------------------------------------------------------------
    def store_version_histories_plan(self, ds: DeviceStates, tasks, last_events, db=None, perm=None) -> "VhBlobPlan":
        """Decide and size (``crr_load_store_vh_plan``, one synchronisation): the rows and offsets stay on the device,
        ``plan.sizes.n_bytes`` is what ``store_version_histories_run`` will write, rounded up to 16."""
        n, T, head, tail = self._store_args(ds, tasks, last_events, db, perm, "store_version_histories")
        torch, dev = self.torch, self.engine.dev
        work_bytes = int(self.lib.crr_load_store_vh_scratch_bytes(n))
        T["rows"] = torch.empty(max(n, 1) * abi.VH_BLOB_ROW.itemsize, dtype=torch.uint8, device=dev)
        T["blob_off"] = torch.empty((n + 1) * 8, dtype=torch.uint8, device=dev)
        T["work"] = torch.empty(work_bytes + 16, dtype=torch.uint8, device=dev)
        P = abi.CVhBlobSizes()
        rc = self.lib.crr_load_store_vh_plan(*head, n, *tail, ctypes.c_void_p(T["rows"].data_ptr()),
                                             ctypes.c_void_p(T["blob_off"].data_ptr()), ctypes.c_void_p(T["work"].data_ptr()),
                                             ctypes.c_size_t(work_bytes), ctypes.byref(P), self._stream())
        if rc != 0 or P.err != 0:
            raise RuntimeError(f"crr_load_store_vh_plan failed: {rc} (err {P.err})")
        return VhBlobPlan(n, P, T, head, tail)

    def store_version_histories_run(self, plan: "VhBlobPlan", out=None, capacity: Optional[int] = None):
        """Emit the planned blobs (``crr_load_store_vh_run``, enqueued on the current stream) into ``out``, a device
        uint8 tensor whose start is 16-byte aligned (default: one of exactly the padded size), of which ``capacity``
        bytes (default: all) may be written; returns ``out``.  Too small a capacity raises and launches nothing."""
        padded = (int(plan.sizes.n_bytes) + 15) // 16 * 16
        if out is None:
            out = self.torch.empty(max(padded, 16), dtype=self.torch.uint8, device=self.engine.dev)
        capacity = int(out.numel() if capacity is None else capacity)
        T = plan.tensors
        rc = self.lib.crr_load_store_vh_run(*plan.head, *plan.tail, ctypes.c_void_p(T["rows"].data_ptr()),
                                            ctypes.c_void_p(T["blob_off"].data_ptr()), ctypes.byref(plan.sizes),
                                            ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(capacity), self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_store_vh_run failed: {rc}")
        T["out"] = out
        self.last_store_vh = plan   # alive until the stream has run the kernel
        return out

    def store_version_histories(self, ds: DeviceStates, tasks, last_events, db=None, perm=None, on_device: bool = False):
        """The thriftrw ``VersionHistories`` DataBlob to store with each task's state once the task is committed
        (field 122 of the execution blob), generated on the device for the tasks the last ``ndc_prepare`` decided;
        arguments as ``store_checksums``, whose outcome and status every row repeats:
        ``(rows abi.VH_BLOB_ROW[n], blob_off uint64[n + 1], bytes uint8[blob_off[n]])`` -- task k's blob is
        ``bytes[blob_off[k]:blob_off[k + 1]]``, empty unless its outcome is ``APPLIED`` or ``BACKFILLED``.
        ``on_device``: the three as device byte tensors (``bytes`` padded to 16 with zeros), nothing more copied back."""
        plan = self.store_version_histories_plan(ds, tasks, last_events, db=db, perm=perm)
        out = self.store_version_histories_run(plan)
        T, n = plan.tensors, plan.n
        if on_device:
            return T["rows"], T["blob_off"], out
        return (T["rows"][:n * abi.VH_BLOB_ROW.itemsize].cpu().numpy().view(abi.VH_BLOB_ROW).copy(),
                T["blob_off"].cpu().numpy().view(np.uint64).copy(), out[:int(plan.sizes.n_bytes)].cpu().numpy().copy())

    # ---- include/cadence_load_mutation.h -------------------------------------------------------------------
    def mutation_plan(self, ds: DeviceStates, tasks, last_events, db=None, perm=None) -> "MutationPlan":
        """Decide, classify and count (``crr_load_mutation_plan``, one synchronisation): the rows stay on the device,
        ``plan.sizes`` holds the totals ``mutation_run`` will write.  Arguments as ``store_checksums``."""
        n, T, head, tail = self._store_args(ds, tasks, last_events, db, perm, "mutation")
        torch, dev = self.torch, self.engine.dev
        work_bytes = int(self.lib.crr_load_mutation_scratch_bytes(n))
        T["rows"] = torch.empty(max(n, 1) * abi.MUTATION_ROW.itemsize, dtype=torch.uint8, device=dev)
        T["work"] = torch.empty(work_bytes + 16, dtype=torch.uint8, device=dev)
        P = abi.CMutationSizes()
        rc = self.lib.crr_load_mutation_plan(*head, n, *tail, ctypes.c_void_p(T["rows"].data_ptr()),
                                             ctypes.c_void_p(T["work"].data_ptr()), ctypes.c_size_t(work_bytes),
                                             ctypes.byref(P), self._stream())
        if rc != 0 or P.err != 0:
            raise RuntimeError(f"crr_load_mutation_plan failed: {rc} (err {P.err})")
        return MutationPlan(n, P, T, head, tail)

    def mutation_run(self, plan: "MutationPlan", out=None, capacity=None):
        """Write the planned mutation (``crr_load_mutation_run``, enqueued on the current stream).  ``out``: device
        uint8 tensors (8-byte aligned) by ``"exec"``, ``"upsert.<map>"`` and ``"deleted.<map>"`` (default: each of
        exactly the plan's total); ``capacity``: rows / keys that may be written, by the same names (default: what the
        tensor holds).  Returns the tensors.  Too small a capacity raises and launches nothing."""
        torch, dev, P = self.torch, self.engine.dev, plan.sizes
        item = {"exec": abi.EXEC_ROW.itemsize}
        total = {"exec": int(P.n_exec)}
        for t, name in enumerate(abi.MUTATION_MAPS):
            item["upsert." + name], total["upsert." + name] = _ROW_DTYPES[name].itemsize, int(P.n_upsert[t])
            item["deleted." + name], total["deleted." + name] = 8, int(P.n_delete[t])
        out = dict(out or {})
        for f in item:
            if f not in out:
                out[f] = torch.empty(max(total[f], 1) * item[f], dtype=torch.uint8, device=dev)
        cap = {f: int(out[f].numel()) // item[f] for f in item}
        cap.update(capacity or {})
        o = abi.CMutationOut()
        o.exec, o.exec_capacity = out["exec"].data_ptr(), cap["exec"]
        for t, name in enumerate(abi.MUTATION_MAPS):
            o.upsert[t], o.upsert_capacity[t] = out["upsert." + name].data_ptr(), cap["upsert." + name]
            o.deleted[t], o.delete_capacity[t] = out["deleted." + name].data_ptr(), cap["deleted." + name]
        T = plan.tensors
        need = int(P.run_work_needed)
        if int(T["work"].numel()) < need + 16:
            T["work"] = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        rc = self.lib.crr_load_mutation_run(*plan.head, *plan.tail, ctypes.c_void_p(T["rows"].data_ptr()), ctypes.byref(P),
                                            ctypes.byref(o), ctypes.c_void_p(T["work"].data_ptr()), ctypes.c_size_t(need),
                                            self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_mutation_run failed: {rc}")
        T["out"] = out
        self.last_mutation = plan   # alive until the stream has run the kernels
        return out

    def mutation(self, ds: DeviceStates, tasks, last_events, db=None, perm=None, on_device: bool = False):
        """The pending-entry mutation to store with each task's state once the task is committed
        (include/cadence_load_mutation.h), for the tasks the last ``ndc_prepare`` decided; arguments as
        ``store_checksums``, whose outcome and status every row repeats.  Returns ``(rows abi.MUTATION_ROW[n], Mutation)``
        -- the Mutation's per-task, per-map views are ``exec_of`` / ``upserts`` / ``deletes``.  ``on_device``: ``(the
        rows as a device byte tensor, the output tensors by name, the plan)``, nothing more copied back."""
        plan = self.mutation_plan(ds, tasks, last_events, db=db, perm=perm)
        out = self.mutation_run(plan)
        if on_device:
            return plan.tensors["rows"], out, plan
        m = plan.download(out)
        return m.rows, m


    # ---- include/cadence_load_resume.h ---------------------------------------------------------------------
    def resume_plan(self, ds: DeviceStates, tasks, task_blobs) -> "ResumePlan":
        """Decide which task is applied onto which loaded state and size the gather (``crr_load_resume_plan``, one
        synchronisation) for the ``tasks`` (``abi.REPL_TASK``) the last ``ndc_prepare`` routed -- the routes stay on the
        device.  ``task_blobs``: the tasks' event blobs resident in HBM (an ``ingest.DeviceBlobs`` whose workflow k is
        task k).  The rows and the work buffer stay on the device; ``plan.sizes`` holds the totals."""
        from .engine import _dev_bytes
        if self.last_ndc is None:
            raise RuntimeError("resume_plan: no ndc_prepare to take the routes from")
        if getattr(task_blobs, "pending", None) is not None:
            # a transcoded task batch with a rejected blob: the gather would drop the rejection with the blob's index
            from .ingest import IngestError
            raise IngestError(*task_blobs.pending)
        torch, dev = self.torch, self.engine.dev
        br, out = self.last_ndc
        tasks = np.ascontiguousarray(tasks, dtype=abi.REPL_TASK)
        n, n_wf = int(tasks.shape[0]), int(ds.c.n_wf)
        if n > int(br.plan.n_tasks):
            raise ValueError(f"{n} tasks, {int(br.plan.n_tasks)} routed")
        work_bytes = int(self.lib.crr_load_resume_scratch_bytes(n_wf, n))
        T = {"tasks": _dev_bytes(torch, tasks, dev),
             "rows": torch.empty(max(n, 1) * abi.LOAD_RESUME_ROW.itemsize, dtype=torch.uint8, device=dev),
             "work": torch.empty(work_bytes + 16, dtype=torch.uint8, device=dev), "routes": out["routes"]}
        P = abi.CLoadResumeSizes()
        vp = ctypes.c_void_p
        rc = self.lib.crr_load_resume_plan(ctypes.byref(ds.c), vp(self.scratch.data_ptr() if self.scratch is not None else None),
                                           ctypes.c_size_t(self.scratch_bytes), ctypes.byref(self.summary),
                                           vp(T["tasks"].data_ptr()), vp(out["routes"].data_ptr()), n,
                                           ctypes.byref(task_blobs.c), vp(T["rows"].data_ptr()), vp(T["work"].data_ptr()),
                                           ctypes.c_size_t(work_bytes), ctypes.byref(P), self._stream())
        if rc != 0 or P.err != 0:
            raise RuntimeError(f"crr_load_resume_plan failed: {rc} (err {P.err})")
        T["work_bytes"] = work_bytes
        return ResumePlan(n, P, T, ds, task_blobs)

    @staticmethod
    def resume_out_sizes(P: abi.CLoadResumeSizes) -> Dict[str, int]:
        """Bytes of each output of ``resume_gather`` for a plan (``bytes`` without the readable pad)."""
        from .blobs import BLOB_WF
        n = int(P.n_wf)
        return {"bytes": int(P.n_bytes), "blob_off": (int(P.n_blobs) + 1) * 8, "wf": n * BLOB_WF.itemsize, "key_begin": n * 4,
                "key_count": n * 4, "key_off": int(P.n_keys) * 8, "key_len": int(P.n_keys) * 4, "task_of": n * 4}

    def resume_gather(self, plan: "ResumePlan", out=None, capacity=None):
        """Write the gathered blob batch, the seeds and ``task_of`` (``crr_load_resume_gather``, enqueued on the current
        stream).  ``out``: device uint8 tensors by ``resume_out_sizes``' names (default: each of exactly the plan's size,
        ``bytes`` with ``INGEST_PAD`` readable bytes behind it); ``capacity``: ``bytes`` / ``blobs`` / ``keys`` that may be
        written (default: the plan's totals).  Returns the tensors.  Too small a capacity raises and launches nothing."""
        torch, dev, P = self.torch, self.engine.dev, plan.sizes
        size = self.resume_out_sizes(P)
        out = dict(out or {})
        for f, nb in size.items():
            if f not in out:
                out[f] = torch.empty(max(nb, 1) + (abi.INGEST_PAD + 16 if f == "bytes" else 16), dtype=torch.uint8, device=dev)
        cap = {"bytes": int(P.n_bytes), "blobs": int(P.n_blobs), "keys": int(P.n_keys)}
        cap.update(capacity or {})
        o = abi.CLoadResumeOut()
        for f in size:
            setattr(o, f, out[f].data_ptr())
        o.bytes_capacity, o.blob_capacity, o.key_capacity = cap["bytes"], cap["blobs"], cap["keys"]
        T, ds = plan.tensors, plan.ds
        vp = ctypes.c_void_p
        rc = self.lib.crr_load_resume_gather(ctypes.byref(ds.c), vp(self.scratch.data_ptr() if self.scratch is not None else None),
                                             ctypes.c_size_t(self.scratch_bytes), ctypes.byref(self.summary),
                                             vp(T["tasks"].data_ptr()), ctypes.byref(plan.task_blobs.c), vp(T["rows"].data_ptr()),
                                             vp(T["work"].data_ptr()), ctypes.c_size_t(T["work_bytes"]), ctypes.byref(P),
                                             ctypes.byref(o), self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_resume_gather failed: {rc}")
        T["out"] = out
        self.last_resume = plan   # alive until the stream has run the kernels
        return out

    def resume_blobs(self, plan: "ResumePlan"):
        """The gathered batch of the last ``resume_gather`` of ``plan`` as an ``ingest.DeviceBlobs`` (the strings and
        the known domains are the task batch's) and the ``ingest.CIngestResume`` naming its seeds; the descriptors
        ``crr_load_resume_finalize`` writes and ``crr_ingest_layout_resume`` continues in place are ``tensors["desc"]``."""
        from .ingest import CBlobBatch, CIngestResume, DeviceBlobs, _TranscodedShape
        P, T = plan.sizes, plan.tensors
        out = T["out"]
        c = CBlobBatch.from_buffer_copy(plan.task_blobs.c)
        c.bytes, c.blob_off, c.wf = out["bytes"].data_ptr(), out["blob_off"].data_ptr(), out["wf"].data_ptr()
        c.n_blobs, c.n_wf = int(P.n_blobs), int(P.n_wf)
        if "desc" not in T:
            T["desc"] = self.torch.zeros(max(int(P.n_wf), 1) * abi.WORKFLOW.itemsize + 16, dtype=self.torch.uint8, device=self.engine.dev)
        R = CIngestResume()
        R.loaded_wf, R.wave_begin = T["desc"].data_ptr(), 0
        for f in ("key_begin", "key_count", "key_off", "key_len"):
            setattr(R, f, out[f].data_ptr())
        tensors = dict(plan.task_blobs.tensors)
        tensors.update(bytes=out["bytes"], blob_off=out["blob_off"], wf=out["wf"])
        return DeviceBlobs(_TranscodedShape(int(P.n_bytes), int(P.n_blobs), int(P.n_wf)), tensors, c), R

    def resume_finalize(self, plan: "ResumePlan", gdb, ingest, arena=None) -> abi.CLoadResumeTotals:
        """The descriptors and the token arena (``crr_load_resume_finalize``, one synchronisation) once ``ingest`` has
        planned the gathered batch ``gdb`` (``crr_ingest_plan_resume``): ``plan.tensors["desc"]`` / ``["arena"]``
        (``arena``: a device uint8 tensor of at least ``token_bytes`` to write instead of a fresh one)."""
        torch, dev, P, T = self.torch, self.engine.dev, plan.sizes, plan.tensors
        counts, stride = ctypes.c_void_p(), ctypes.c_uint64()
        vp = ctypes.c_void_p
        rc = self.lib.crr_ingest_resume_counts(ctypes.byref(gdb.c), vp(ingest.scratch.data_ptr()), ctypes.c_size_t(ingest.scratch_bytes),
                                               ctypes.byref(counts), ctypes.byref(stride))
        if rc != 0:
            raise RuntimeError(f"crr_ingest_resume_counts failed: {rc}")
        T["arena"] = arena if arena is not None else torch.zeros(int(P.token_bytes) + 16, dtype=torch.uint8, device=dev)
        Q = abi.CLoadResumeTotals()
        rc = self.lib.crr_load_resume_finalize(vp(self.scratch.data_ptr() if self.scratch is not None else None),
                                               ctypes.c_size_t(self.scratch_bytes), ctypes.byref(self.summary),
                                               vp(T["out"]["wf"].data_ptr()), counts, stride, vp(T["work"].data_ptr()),
                                               ctypes.c_size_t(T["work_bytes"]), ctypes.byref(P), vp(T["desc"].data_ptr()),
                                               vp(T["arena"].data_ptr()), ctypes.c_size_t(int(P.token_bytes)), ctypes.byref(Q),
                                               self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_resume_finalize failed: {rc}")
        plan.totals = Q
        return Q

    def resume(self, ds: DeviceStates, tasks, task_blobs, ingest, emit_tasks: bool = False, max_events: Optional[int] = None):
        """The resumed replay of the routed ``tasks`` onto the last plan's states, laid out on the device: plan, gather,
        ``crr_ingest_plan_resume`` over the gathered batch, finalize, the outputs allocated, the loaded rows placed,
        ``crr_ingest_layout_resume``, ``crr_load_resume_settle``.  Returns an ``engine.DeviceBatch`` ready for ``engine.launch`` (canonical layout:
        device position p is loaded workflow p), which the store methods take as ``db=``; ``self.last_resume`` keeps
        the plan.  ``max_events``: the event capacity the ingest scratch is first sized for (``DeviceIngest.plan``).  A
        task blob the decoder rejects raises ``ingest.IngestError`` with the task's index as ``.task``; nothing is
        enqueued after it."""
        from .engine import DeviceBatch
        from .ingest import IngestError, _ShellBatch
        torch, dev = self.torch, self.engine.dev
        plan = self.resume_plan(ds, tasks, task_blobs)
        self.resume_gather(plan)
        gdb, R = self.resume_blobs(plan)
        try:
            S = ingest.plan(gdb, resume=R, max_events=max_events)
        except IngestError as e:
            from .blobs import BLOB_WF
            n = int(plan.sizes.n_wf)
            out = plan.tensors["out"]
            begin = out["wf"][:n * BLOB_WF.itemsize].cpu().numpy().view(BLOB_WF)["blob_begin"].astype(np.int64)
            task_of = out["task_of"][:n * 4].cpu().numpy().view(np.int32)
            p = int(np.searchsorted(begin, e.blob, side="right")) - 1     # the last position whose range starts at or before it
            task = int(task_of[p]) if 0 <= p < n else -1
            err = IngestError(e.code, e.blob)
            err.task = task
            err.args = (f"{e.args[0]}: task {task}",)
            raise err from None
        Q = self.resume_finalize(plan, gdb, ingest)
        n = int(plan.sizes.n_wf)
        T = plan.tensors
        ci = abi.CInputs()
        T["wf"] = T["desc"]                                # the layout continues the descriptors in place
        ingest.allocate_inputs(S, T, ci, wf_in_place=T["desc"])
        ci.arena = T["arena"].data_ptr()
        ci.n_wf, ci.stride, ci.wave_begin, ci.big_begin = n, 1, 0, n
        ci.flags = (abi.IN_HAS_NEW_RUN if S.has_new_run else 0) | (abi.IN_EMIT_TASKS if emit_tasks else 0)
        co = abi.COutputs()
        T["exec"] = torch.zeros(max(n, 1) * abi.EXEC_ROW.itemsize, dtype=torch.uint8, device=dev)
        co.exec = T["exec"].data_ptr()
        table_rows = {}
        for j, (name, dt, *_r) in enumerate(abi.TABLES):
            table_rows[name] = int(Q.table_rows[j])
            rows = 1 if name == "tasks" and not emit_tasks else max(table_rows[name], 1)
            T["out_" + name] = torch.zeros(rows * dt.itemsize, dtype=torch.uint8, device=dev)
            setattr(co, name, T["out_" + name].data_ptr())
        T["scratch"] = torch.zeros(2 * n + abi.SCRATCH_EXTRA_WORDS, dtype=torch.int32, device=dev)
        co.scratch = T["scratch"].data_ptr()
        for t, name in enumerate(abi.ID_TABLES):
            T["ids_" + name] = torch.zeros(max(table_rows[name], 1), dtype=torch.int64, device=dev)
            co.live_ids[t] = T["ids_" + name].data_ptr()
        T["perm"] = torch.arange(max(n, 1), dtype=torch.int32, device=dev)
        shapes = ingest.input_shapes(S)
        shapes["arena"] = int(plan.sizes.token_bytes)
        shell = _ShellBatch(n, emit_tasks, table_rows, 0, (0, 0, 0, 0, 0, n), shapes)
        db = DeviceBatch(shell, T, ci, co, self.engine.device)
        self.place(db)
        ingest.layout_resume(gdb, R, S, ci)
        # the layout sets the RESUME flag on every descriptor it continues; a position without a task stays a workflow
        # without events that resumes nothing
        rc = self.lib.crr_load_resume_settle(ctypes.c_void_p(T["out"]["task_of"].data_ptr()), ctypes.c_void_p(T["desc"].data_ptr()),
                                             n, self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_resume_settle failed: {rc}")
        T["gathered"], T["resume"], T["summary"] = gdb, R, S
        return db

    # ---- include/cadence_load_store_exec.h -----------------------------------------------------------------
    def store_executions_plan(self, vh_plan: "VhBlobPlan", exec_tasks, task_blobs=None) -> "ExecBlobPlan":
        """Decide, size and script (``crr_load_store_exec_plan``, one synchronisation) the execution blobs of the tasks
        ``vh_plan`` (``store_version_histories_plan``) was made for.  ``exec_tasks``: ``abi.EXEC_BLOB_TASK`` per task;
        ``task_blobs``: the tasks' event blobs resident in HBM (an ``ingest.DeviceBlobs``, workflow p of it device
        position p: the batch ``crr_ingest_plan_resume`` took), None: a request id of the task leaves its blob to the
        host.  The rows, offsets and scripts stay on the device; ``plan.sizes.n_bytes`` is what the run writes."""
        from .engine import _dev_bytes
        torch, dev, n = self.torch, self.engine.dev, vh_plan.n
        xt = np.ascontiguousarray(exec_tasks, dtype=abi.EXEC_BLOB_TASK)
        if xt.shape != (n,):
            raise ValueError(f"{xt.shape} exec_tasks rows for {n} tasks")
        work_bytes = int(self.lib.crr_load_store_exec_scratch_bytes(n))
        T = {"exec_tasks": _dev_bytes(torch, xt, dev), "task_blobs": task_blobs,
             "rows": torch.empty(max(n, 1) * abi.EXEC_BLOB_ROW.itemsize, dtype=torch.uint8, device=dev),
             "blob_off": torch.empty((n + 1) * 8, dtype=torch.uint8, device=dev),
             "work": torch.empty(work_bytes + 16, dtype=torch.uint8, device=dev)}
        V = vh_plan.tensors

        def ptr(t):
            return ctypes.c_void_p(t.data_ptr() if t is not None else None)
        mid = (ptr(T["exec_tasks"]), ptr(V["rows"]), ptr(V["blob_off"]), ctypes.byref(vh_plan.sizes),
               ctypes.byref(task_blobs.c) if task_blobs is not None else None)
        P = abi.CExecBlobSizes()
        rc = self.lib.crr_load_store_exec_plan(*vh_plan.head, n, *vh_plan.tail, *mid, ptr(T["rows"]), ptr(T["blob_off"]),
                                               ptr(T["work"]), ctypes.c_size_t(work_bytes), ctypes.byref(P), self._stream())
        if rc != 0 or P.err != 0:
            raise RuntimeError(f"crr_load_store_exec_plan failed: {rc} (err {P.err})")
        return ExecBlobPlan(n, P, T, vh_plan, mid, work_bytes)

    def store_executions_run(self, plan: "ExecBlobPlan", vh_bytes, out=None, capacity: Optional[int] = None):
        """Emit the planned blobs (``crr_load_store_exec_run``, enqueued on the current stream behind the
        ``store_version_histories_run`` that wrote ``vh_bytes``) into ``out``, a device uint8 tensor whose start is
        16-byte aligned (default: one of exactly ``n_bytes``), of which ``capacity`` bytes (default: all) may be
        written; returns ``out``.  Too small a capacity raises and launches nothing."""
        n_bytes = int(plan.sizes.n_bytes)
        if out is None:
            out = self.torch.empty(max(n_bytes, 16), dtype=self.torch.uint8, device=self.engine.dev)
        capacity = int(out.numel() if capacity is None else capacity)
        T, v = plan.tensors, plan.vh_plan

        def ptr(t):
            return ctypes.c_void_p(t.data_ptr() if t is not None else None)
        rc = self.lib.crr_load_store_exec_run(*v.head, *v.tail, *plan.mid, ptr(T["rows"]), ptr(T["blob_off"]), ptr(T["work"]),
                                              ctypes.c_size_t(plan.work_bytes), ctypes.byref(plan.sizes), ptr(vh_bytes),
                                              ptr(out), ctypes.c_size_t(capacity), self._stream())
        if rc != 0:
            raise RuntimeError(f"crr_load_store_exec_run failed: {rc}")
        T["out"], T["vh_bytes"] = out, vh_bytes
        self.last_store_exec = plan   # alive until the stream has run the kernel
        return out

    def store_executions(self, ds: DeviceStates, tasks, last_events, exec_tasks, db=None, perm=None, task_blobs=None,
                         on_device: bool = False):
        """The execution blob to store with each task's state once the task is committed
        (include/cadence_load_store_exec.h), generated on the device behind the ``VersionHistories`` blobs of the same
        tasks; arguments as ``store_version_histories`` and ``store_executions_plan``.  Returns ``((rows
        abi.EXEC_BLOB_ROW[n], blob_off uint64[n + 1], bytes uint8[blob_off[n]]), store_version_histories' three)`` --
        task k's blob is ``bytes[blob_off[k]:blob_off[k + 1]]``, empty unless the device encodes it (``rows["flags"]``
        says why not).  ``on_device``: all six as device byte tensors, nothing more copied back."""
        vh_plan = self.store_version_histories_plan(ds, tasks, last_events, db=db, perm=perm)
        vh_out = self.store_version_histories_run(vh_plan)
        plan = self.store_executions_plan(vh_plan, exec_tasks, task_blobs=task_blobs)
        out = self.store_executions_run(plan, vh_out)
        T, V, n = plan.tensors, vh_plan.tensors, plan.n
        if on_device:
            return (T["rows"], T["blob_off"], out), (V["rows"], V["blob_off"], vh_out)
        return ((plan.rows(), T["blob_off"].cpu().numpy().view(np.uint64).copy(), out[:int(plan.sizes.n_bytes)].cpu().numpy().copy()),
                (V["rows"][:n * abi.VH_BLOB_ROW.itemsize].cpu().numpy().view(abi.VH_BLOB_ROW).copy(),
                 V["blob_off"].cpu().numpy().view(np.uint64).copy(), vh_out[:int(vh_plan.sizes.n_bytes)].cpu().numpy().copy()))


@dataclasses.dataclass
class ResumePlan:
    """A finished ``crr_load_resume_plan``: the host sizes, the device rows and work buffer, the states and the task
    blobs it was made for; ``resume_gather`` adds its output tensors, ``resume`` the descriptors and the arena."""
    n: int
    sizes: abi.CLoadResumeSizes
    tensors: Dict[str, object]
    ds: DeviceStates
    task_blobs: object                    # ingest.DeviceBlobs
    totals: Optional[abi.CLoadResumeTotals] = None

    def rows(self) -> np.ndarray:
        return self.tensors["rows"][:self.n * abi.LOAD_RESUME_ROW.itemsize].cpu().numpy().view(abi.LOAD_RESUME_ROW).copy()

    def download(self, out=None) -> ResumeImage:
        """The gather's output tensors (default: the last gather's) copied to the host, exactly the plan's totals of
        each; with a finished ``resume`` the descriptors, the arena and the totals too."""
        from .blobs import BLOB_WF
        P, T = self.sizes, self.tensors
        out = out if out is not None else T["out"]
        n = int(P.n_wf)

        def host(f, dt, k):
            return out[f][:k * np.dtype(dt).itemsize].cpu().numpy().view(dt).copy()
        img = ResumeImage(P, self.rows(), host("bytes", np.uint8, int(P.n_bytes)), host("blob_off", np.uint64, int(P.n_blobs) + 1),
                          host("wf", BLOB_WF, n), host("key_begin", np.uint32, n), host("key_count", np.uint32, n),
                          host("key_off", np.uint64, int(P.n_keys)), host("key_len", np.uint32, int(P.n_keys)),
                          host("task_of", np.int32, n))
        if self.totals is not None:
            img.desc = T["desc"][:n * abi.WORKFLOW.itemsize].cpu().numpy().view(abi.WORKFLOW).copy()
            img.arena = T["arena"][:int(P.token_bytes)].cpu().numpy().copy()
            img.table_rows = [int(x) for x in self.totals.table_rows]
        return img


@dataclasses.dataclass
class ExecBlobPlan:
    """A finished ``crr_load_store_exec_plan``: the host sizes, the device rows / offsets / work buffer (the edit
    scripts), the ``VersionHistories`` plan it was made from and the arguments ``crr_load_store_exec_run`` takes again."""
    n: int
    sizes: abi.CExecBlobSizes
    tensors: Dict[str, object]
    vh_plan: "VhBlobPlan"
    mid: tuple
    work_bytes: int

    def rows(self) -> np.ndarray:
        return self.tensors["rows"][:self.n * abi.EXEC_BLOB_ROW.itemsize].cpu().numpy().view(abi.EXEC_BLOB_ROW).copy()


@dataclasses.dataclass
class MutationPlan:
    """A finished ``crr_load_mutation_plan``: the host sizes, the device rows and work buffer and the arguments of the
    call, which ``crr_load_mutation_run`` takes again."""
    n: int
    sizes: abi.CMutationSizes
    tensors: Dict[str, object]
    head: tuple
    tail: tuple

    def rows(self) -> np.ndarray:
        return self.tensors["rows"][:self.n * abi.MUTATION_ROW.itemsize].cpu().numpy().view(abi.MUTATION_ROW).copy()

    def download(self, out) -> Mutation:
        """The run's output tensors copied to the host: exactly the plan's totals of each."""
        P = self.sizes

        def host(f, dt, k):
            return out[f][:k * np.dtype(dt).itemsize].cpu().numpy().view(dt).copy()
        return Mutation(self.rows(), host("exec", abi.EXEC_ROW, int(P.n_exec)),
                        {n: host("upsert." + n, _ROW_DTYPES[n], int(P.n_upsert[t])) for t, n in enumerate(abi.MUTATION_MAPS)},
                        {n: host("deleted." + n, np.int64, int(P.n_delete[t])) for t, n in enumerate(abi.MUTATION_MAPS)})


@dataclasses.dataclass
class VhBlobPlan:
    """A finished ``crr_load_store_vh_plan``: the host sizes, the device rows / offsets / work buffer and the
    arguments of the call, which ``crr_load_store_vh_run`` takes again."""
    n: int
    sizes: abi.CVhBlobSizes
    tensors: Dict[str, object]
    head: tuple
    tail: tuple
