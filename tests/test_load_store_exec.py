"""The execution blob of a committed replication task, by the host restatement (crr_load_store_exec_host,
include/cadence_load_store_exec.h): the CPU side of tests/test_gpu_load_store_exec.py.  Expected bytes are
exec_blob_cases' full re-encoding of the decoded stored blob with the header's overrides applied in Python (hand blobs
that no Go writer makes: written out by hand); the round trip applies the blobs to the persisted states and loads them
again."""
import ctypes
import os
import re

import numpy as np

from cadence_amd import abi, persisted
from cadence_amd.persisted import (apply_mutation, load_states_host, load_states_verify_host, mutation_host,
                                   store_checksums_host, store_executions_host, store_version_histories_host)

import asan_tool
import exec_blob_cases as xc
import mutation_cases as mc
import store_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O = abi.StoreOutcome
F = xc.HOST_FLAGS


def test_header_pins():
    """The test to run against the parent commit: it needs nothing but the header, the two libraries and abi.py."""
    from cadence_amd import decode, engine
    text = open(os.path.join(ROOT, "include", "cadence_load_store_exec.h")).read()
    assert set(re.findall(r"\b(crr_load_\w+)\s*\(", text)) >= {
        "crr_load_store_exec_scratch_bytes", "crr_load_store_exec_plan", "crr_load_store_exec_run", "crr_load_store_exec_host"}
    dev = ctypes.CDLL(engine.LIB_PATH)
    for f in ("crr_load_store_exec_scratch_bytes", "crr_load_store_exec_plan", "crr_load_store_exec_run"):
        assert hasattr(dev, f), f
    assert hasattr(decode.lib(), "crr_load_store_exec_host")
    dev.crr_abi_version.restype = ctypes.c_int
    assert dev.crr_abi_version() == abi.ABI_VERSION == 8
    abi.check_layout(dev)
    assert dev.crr_sizeof(36) == abi.EXEC_BLOB_TASK.itemsize == 16
    assert dev.crr_sizeof(37) == abi.EXEC_BLOB_ROW.itemsize == 24
    assert dev.crr_sizeof(38) == ctypes.sizeof(abi.CExecBlobSizes) == 48
    assert dev.crr_sizeof(29) == 0 and dev.crr_sizeof(32) == 0      # the two indices earlier pins keep unassigned
    assert dev.crr_sizeof(39) == 0
    assert "crr_sizeof(36..38)" in open(os.path.join(ROOT, "include", "cadence_replay.h")).read()
    assert [abi.EXEC_BLOB_ROW.fields[f][1] for f in ("outcome", "status", "flags", "len", "next_event_id")] == [0, 4, 8, 12, 16]
    assert [abi.EXEC_BLOB_TASK.fields[f][1] for f in ("now_ns", "history_size_delta")] == [0, 8]
    S = abi.CExecBlobSizes
    assert [getattr(S, f).offset for f in ("err", "n_tasks", "n_bytes", "n_blobs", "n_host", "work_needed", "run_work_needed")] == \
        [0, 4, 8, 16, 24, 32, 40]
    for name, value in (("RESET_POINTS", 1), ("SEARCH_ATTRIBUTES", 2), ("REQUEST_ID", 4), ("STORED_SHAPE", 8)):
        assert re.search(r"#define CRR_EXEC_BLOB_HOST_%s\s+%du" % (name, value), text)
        assert getattr(abi, "EXEC_BLOB_HOST_" + name) == value
    dev.crr_load_store_exec_scratch_bytes.restype = ctypes.c_size_t
    dev.crr_load_store_exec_scratch_bytes.argtypes = [ctypes.c_uint32]
    assert dev.crr_load_store_exec_scratch_bytes(0) % 16 == 0
    assert dev.crr_load_store_exec_scratch_bytes(1000) > dev.crr_load_store_exec_scratch_bytes(10) > 0


def test_the_decoder_reads_back_what_the_encoder_writes():
    """exec_blob_cases.decode_struct is the inverse of persisted.encode_struct on all six structs."""
    import load_cases as lc
    raw = lc.exec_blob(points=[("bin", True)], CompletionEventBatchID=9)
    v = xc.decode_struct("WorkflowExecutionInfo", raw)
    assert persisted.encode_struct("WorkflowExecutionInfo", v) == raw
    assert v["RetryNonRetryableErrors"] == ["bad-input"] and v["Memo"] == {"note": b"memo"} and v["RetryBackoffCoefficient"] == 2.0
    for kind, _id, _aux, _s, blob in (lc.activity_blob(5, "a5"), lc.timer_blob("t", 7), lc.child_blob(9, 10),
                                      lc.initiated_blob(11, False), lc.initiated_blob(12, True)):
        name = persisted.KIND_STRUCT[kind]
        assert persisted.encode_struct(name, xc.decode_struct(name, blob)) == blob


def _host(c, task_blobs=True, threads=1, sel=None):
    sel = slice(None) if sel is None else sel
    return store_executions_host(c.sbs, c.tasks[sel], c.last_events[sel], c.results[sel], c.routes[sel], c.exec_tasks[sel],
                                 c.after, xc.task_blob_set(c.task_histories) if task_blobs else None, c.upserts, threads)


def test_hand_states():
    c = xc.hand_case()
    got = _host(c)
    xc.assert_result(got, c.want, "hand states")
    rows, off, data = got
    k, want = c.names, c.want
    blob = lambda name: data[int(off[k[name]]):int(off[k[name] + 1])].tobytes()   # noqa: E731
    stored = lambda name: xc.exec_blob_of(c.sbs, int(c.tasks[k[name]]["wf"]))     # noqa: E731
    # outcome and status are crr_store_row's, every outcome but NOT_RESUMED is here (test below)
    store = store_checksums_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.after)
    assert (rows["outcome"] == store["outcome"]).all() and (rows["status"] == store["status"]).all()
    assert set(int(x) for x in rows["outcome"]) == set(int(x) for x in O) - {int(O.NOT_RESUMED)}
    for name in ("no_route", "new_branch", "not_loaded", "vh_error", "duplicate", "failed"):
        assert rows[k[name]]["len"] == 0 and rows[k[name]]["flags"] == 0 and rows[k[name]]["next_event_id"] == 0, name
    # the sticky state with client fields: the blob shrinks, by exactly those strings
    assert len(blob("sticky")) == len(stored("sticky")) - len("sticky-task-list-of-a-worker") - len("1.7.0") * 2 - len("uber-go")
    v = xc.decode_struct("WorkflowExecutionInfo", blob("sticky"))
    assert v["StickyTaskList"] == v["ClientLibraryVersion"] == v["ClientFeatureVersion"] == v["ClientImpl"] == b""
    assert v["StickyScheduleToStartTimeout"] == 0 and v["CancelRequested"] is True
    assert v["DecisionOriginalScheduledTimestampNanos"] == abi.GO_ZERO_TIME_NANOS      # CRR_ZERO_TIME as Go writes it
    # field 18: inserted (11 bytes more than the same blob without it), patched, dropped
    assert b"\x0a\x00\x12" + (24).to_bytes(8, "big") in blob("insert18") and b"\x0a\x00\x12" not in stored("insert18")
    assert len(blob("insert18")) == len(blob("rq_none")) + 11 + len("emptyUuid")
    assert xc.decode_struct("WorkflowExecutionInfo", blob("patch18"))["CompletionEventBatchID"] == 25
    assert "CompletionEventBatchID" not in xc.decode_struct("WorkflowExecutionInfo", blob("drop18"))
    assert len(blob("drop18")) == len(blob("patch18")) - 11
    # field 74 in its four sources
    rq = lambda name: xc.decode_struct("WorkflowExecutionInfo", blob(name))["DecisionRequestID"]   # noqa: E731
    assert rq("sticky") == b"emptyUuid" and rq("rq_none") == b"" and rq("rq_stored") == b"a-stored-decision-request-id"
    assert rq("rq_task") == b"the-task's-decision-request-id" and want.from_task[k["rq_task"]]
    assert rows[k["rq_not_started"]]["flags"] == F["rq"] and rows[k["rq_not_started"]]["len"] == 0
    assert rows[k["rq_not_started"]]["outcome"] == O.APPLIED and rows[k["rq_not_started"]]["next_event_id"] == 26
    # unknown ids in front, between and behind; fields out of ascending order: verbatim but for the values
    assert blob("unknown").startswith(stored("unknown")[:20]) and blob("unknown")[-40:] == stored("unknown")[-40:]
    assert blob("unordered") == xc._unordered_blob(dict(now=xc.NOW, hist=57, vh=persisted.encode_version_histories(0, [(xc.lc.TOKEN, [(25, 3)])])))
    assert blob("sparse")[:22] == b"\x0a\x00\x38" + xc.NOW.to_bytes(8, "big") + b"\x0a\x00\x6c" + (7).to_bytes(8, "big")
    # an overridden field of another type, one held twice
    for name in ("wrong_type", "twice"):
        assert rows[k[name]]["flags"] == F["shape"] and rows[k[name]]["len"] == 0 and rows[k[name]]["outcome"] == O.APPLIED
    assert rows[k["upsert"]]["flags"] == F["sa"] and rows[k["reset_points"]]["flags"] == F["rp"]
    # backfills: three fields, everything else as stored; the Go zero time as a clock; a negative delta
    v0, v1 = xc.decode_struct("WorkflowExecutionInfo", stored("backfill")), xc.decode_struct("WorkflowExecutionInfo", blob("backfill"))
    assert {f for f in v1 if v0.get(f) != v1[f]} == {"LastUpdatedTimeNanos", "HistorySize", "VersionHistories"} and set(v0) == set(v1)
    assert v1["HistorySize"] == 4096 + 512 and rows[k["backfill"]]["next_event_id"] == 20
    z = xc.decode_struct("WorkflowExecutionInfo", blob("zero_time"))
    assert z["LastUpdatedTimeNanos"] == abi.GO_ZERO_TIME_NANOS and z["HistorySize"] == 96
    assert xc.decode_struct("WorkflowExecutionInfo", blob("backfill_again"))["HistorySize"] == 4000
    # a zero-length blob between two generated ones
    a, b, d = k["backfill"], k["no_route"], k["zero_time"]
    assert (a + 1, b + 1) == (b, d) and off[b] == off[d] and rows[a]["len"] > 0 and rows[d]["len"] > 0
    # threads, and any subset in any order
    assert all(x.tobytes() == y.tobytes() for x, y in zip(_host(c, threads=4), got))
    order = np.random.default_rng(2).permutation(c.tasks.shape[0])[:12]
    sub = _host(c, sel=order)
    for i, j in enumerate(order):
        assert sub[2][int(sub[1][i]):int(sub[1][i + 1])].tobytes() == want.blobs[j] and sub[0][i]["flags"] == want.rows[j]["flags"]


def test_hand_states_without_task_blobs_or_a_replay():
    c = xc.hand_case()
    got = _host(c, task_blobs=False)
    xc.assert_result(got, c.want_without_blobs, "no task blobs")
    k = c.names
    assert got[0][k["rq_task"]]["flags"] == F["rq"] and got[0][k["rq_task"]]["len"] == 0
    changed = np.nonzero(c.want.rows["len"] != c.want_without_blobs.rows["len"])[0]
    assert list(changed) == [k["rq_task"]]
    # no post-replay state: every task on the current route is NOT_RESUMED, the backfills are as before
    rows, off, data = store_executions_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.exec_tasks, None)
    cur = c.routes["route"] == abi.ROUTE_APPLY_CURRENT
    assert (rows["outcome"][cur] == O.NOT_RESUMED).all() and (rows["len"][cur] == 0).all()
    for name in ("backfill", "zero_time", "unordered", "sparse", "backfill_again"):
        assert data[int(off[k[name]]):int(off[k[name] + 1])].tobytes() == c.want.blobs[k[name]], name


def test_hand_states_with_populated_task_blobs():
    """The request id taken from task blobs shaped as a history service persists them (full_event_cases: every field
    of the schema present, the task's first event padded so that the DecisionTaskStarted event lies beyond 13 KB):
    exec_request_id skips whole populated events; rows, offsets and blobs are the hand case's expectation."""
    import full_event_cases as fe
    from thrift_tree import parse_blob
    c = xc.hand_case()
    plain = xc.task_blob_set(c.task_histories)
    tb = fe.populated_task_blobs(plain)
    w = c.names["rq_task"]
    b0 = int(tb.wf["blob_begin"][w])
    assert int(tb.wf["blob_count"][w]) == 3 and int(tb.blob_off[b0 + 2] - tb.blob_off[b0]) > 13 * 1024
    started = fe._events_of(parse_blob(tb.blob(b0 + 2)))[2][1][1]                 # event number 3 of the task
    assert len(next(f for f in started if f[1] == 90)[2]) == len(fe.SCHEMA["DecisionTaskStartedEventAttributes"][1])
    assert tb.n_bytes > 4 * plain.n_bytes
    got = store_executions_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.exec_tasks, c.after, tb, c.upserts, 1)
    xc.assert_result(got, c.want, "hand states, populated task blobs")
    assert got[0][c.names["rq_task"]]["len"] > 0 and got[0][c.names["rq_not_started"]]["flags"] == F["rq"]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, _host(c)))


def test_capacity_one_byte_short_and_exact():
    c = xc.hand_case()
    host = persisted._host_lib()
    cb = persisted._c_batch(c.sbs, lambda a: a.ctypes.data)
    img, _keep = persisted._after_image(c.after, c.sbs.n_wf)
    n = c.tasks.shape[0]
    total = len(c.want_without_blobs.data)

    def call(out, cap):
        P = abi.CExecBlobSizes()
        rc = host.crr_load_store_exec_host(ctypes.byref(cb), c.tasks.ctypes.data, c.last_events.ctypes.data, n,
                                           c.results.ctypes.data, c.routes.ctypes.data, ctypes.byref(img),
                                           c.exec_tasks.ctypes.data, None, c.upserts.ctypes.data, None, None,
                                           out.ctypes.data + 64 if out is not None else None, cap, ctypes.byref(P), 1)
        return rc, P
    rc, P = call(None, 0)
    assert rc == 0 and int(P.n_bytes) == total and int(P.n_tasks) == n
    assert int(P.n_blobs) == int((c.want_without_blobs.rows["len"] > 0).sum())
    assert int(P.n_host) == int((c.want_without_blobs.rows["flags"] != 0).sum()) == 6
    buf = np.full(total + 128, 0x5A, np.uint8)
    assert call(buf, total - 1)[0] == -1 and (buf == 0x5A).all()
    assert call(buf, total)[0] == 0
    assert (buf[:64] == 0x5A).all() and (buf[64 + total:] == 0x5A).all() and buf[64:64 + total].tobytes() == c.want_without_blobs.data


def _check_replayed(x: xc.ReplayedExec, what: str):
    rc, r = x.r.rc, x.r
    args = (rc.sbs, rc.tasks, rc.last_events, r.results, r.routes, x.exec_tasks, r.after)
    got = store_executions_host(*args, x.task_blobs, x.upserts, threads=4)
    xc.assert_result(got, x.want, what)
    without = store_executions_host(*args, None, x.upserts)
    xc.assert_result(without, x.want_without_blobs, what + ", no task blobs")
    t = xc.tally(x)
    print(what, t, "without task blobs:", xc.tally(x, x.want_without_blobs))
    # only the tasks whose request id is theirs differ between the two
    differ = np.nonzero(x.want.rows["len"] != x.want_without_blobs.rows["len"])[0]
    assert differ.size == t["from_task"] and x.want.from_task[differ].all()
    assert t["closes"] == 0     # (no encoded replayed task closes its workflow: field 18's insertion is the hand states')
    return got, t


def test_replayed_case_a_one_task_per_state():
    got, t = _check_replayed(xc.case_a(), "case A")
    assert t["device"] >= 200 and t["from_task"] >= 8 and t["device_backfills"] == t["backfilled"] == 42
    assert t["rp"] >= 1 and t["sa"] >= 1


def test_replayed_case_b_split_anywhere():
    got, t = _check_replayed(xc.case_b(), "case B")
    assert t["rp"] >= 100 and t["sa"] >= 3 and t["device"] >= 80


def _round_trip(x: xc.ReplayedExec):
    r, rc = x.r, x.r.rc
    args = (rc.sbs, rc.tasks, rc.last_events, r.results, r.routes, r.after)
    m = mutation_host(*args)
    vh, store = store_version_histories_host(*args), store_checksums_host(*args)
    ex = store_executions_host(rc.sbs, rc.tasks, rc.last_events, r.results, r.routes, x.exec_tasks, r.after, x.task_blobs, x.upserts)
    applied, stored, points = np.zeros(rc.sbs.n_wf, bool), [None] * rc.sbs.n_wf, {}
    for k in np.nonzero(m.rows["outcome"] == O.APPLIED)[0]:
        w = int(rc.tasks[k]["wf"])
        applied[w] = True
        stored[w] = (abi.CHECKSUM_PAYLOAD_V1, abi.CHECKSUM_FLAVOR_CRC32, int(store["value"][k]).to_bytes(4, "big"))
        points[w] = mc.reset_points_of(r.after, w)
    names = [r.after.interners[w] for w in range(rc.sbs.n_wf)]
    new = apply_mutation(rc.sbs, rc.tasks, m, vh, store, names, reset_points=points, exec_blobs=ex)
    # the default keeps today's behaviour byte for byte, and differs from the device blobs' (the host stub keeps strings)
    old = apply_mutation(rc.sbs, rc.tasks, m, vh, store, names, reset_points=points)
    assert old.bytes.tobytes() == apply_mutation(rc.sbs, rc.tasks, m, vh, store, names, points, None).bytes.tobytes()
    assert old.bytes.tobytes() != new.bytes.tobytes()
    got, want = load_states_host(new), load_states_host(sc.reencoded_applied(rc, applied))
    for w in np.nonzero(applied)[0]:
        assert mc.persisted_view(got, int(w)) == mc.persisted_view(want, int(w)), w
    v = load_states_verify_host(new, persisted.stored_checksums(stored))
    assert (v["outcome"][applied] == abi.VerifyOutcome.MATCH).all()
    rows = ex[0]
    n_dev = 0
    for k in np.nonzero(rows["len"] > 0)[0]:
        w = int(rc.tasks[k]["wf"])
        d = xc.decode_struct("WorkflowExecutionInfo", xc.exec_blob_of(new, w))
        assert d["LastUpdatedTimeNanos"] == int(x.exec_tasks[k]["now_ns"])
        assert d["HistorySize"] == 4096 + int(x.exec_tasks[k]["history_size_delta"])
        assert int(new.wf["next_event_id"][w]) == int(rows[k]["next_event_id"])
        if int(rows[k]["outcome"]) == O.APPLIED:
            assert d["ClientLibraryVersion"] == d["ClientFeatureVersion"] == d["ClientImpl"] == d["StickyTaskList"] == b""
            n_dev += 1
    return n_dev


def test_round_trip_device_blobs_load_as_the_snapshot():
    assert _round_trip(xc.case_a()) >= 200
    assert _round_trip(xc.case_b()) >= 80


def test_host_restatement_under_asan_and_ubsan(tmp_path):
    asan_tool.build_and_run(tmp_path, "load_store_exec_asan")
