"""CPU: the persisted mutable-state loader's host restatement (crr_load_states_host, include/cadence_load.h).

Replayed states are written as the SQL store persists them (cadence_amd/persisted.encode_states), decoded
back and compared field for field with the replay's own rows, rewritten by a Python restatement of the
loader's rules (load_cases.expected_image).  tests/golden/sqlblobs_fields.json -- field names, ids and thrift
types transcribed from the reference's generated sqlblobs code -- pins the wire format on both sides, so an
encoder and a decoder that agree with each other cannot both be wrong.
"""
import numpy as np
import pytest

from cadence_amd import abi, persisted
from cadence_amd.persisted import build_blob_set, encode_states, load_states_host

import asan_tool
import load_cases as lc


def _status(sbs):
    return load_states_host(sbs).status


# ---- the wire format -----------------------------------------------------------------------------------------
def test_encoder_uses_the_fixture_ids_and_types():
    fx = lc.fixture_fields()
    assert set(fx) == set(persisted.FIELDS) == set(persisted.KIND_STRUCT)
    for name, fields in fx.items():
        assert [tuple(f) for f in fields] == persisted.FIELDS[name], name


PROBES, TABLE_OF = lc.PROBES, lc.TABLE_OF


@pytest.mark.parametrize("unknown", [False, True])
def test_decoder_reads_the_fixture_ids_with_every_field_populated(unknown):
    """Every field of every struct populated (those the loader skips too), encoded from the fixture's ids and
    types alone; with ``unknown``: fields of unknown ids of each thrift type around them."""
    img = load_states_host(lc.populated_batch(unknown))
    assert img.status.tolist() == [0, 0, 0]
    assert img.flags.tolist() == [0, abi.LOAD_FLAG_STICKY, 0]
    for name, (tab, _kind) in TABLE_OF.items():
        o = img.offsets[abi.LOAD_ROW_TABLES.index(tab)]
        assert o[2] - o[1] == 1, name
        row = img.rows[tab][int(o[1])]
        for f, (v, rf) in PROBES[name].items():
            assert row[rf] == v, (name, f)
    act = img.rows["act"][int(img.offsets[0][1])]
    assert act["schedule_id"] == 55 and act["last_heartbeat_time"] == 991 and act["last_hb_timeout_vis_s"] == 0
    assert act["flags"] == abi.ROW_LIVE | abi.ROW_MAPPED | abi.ROW_CANCEL_REQUESTED | abi.ROW_HAS_RETRY
    assert (act["sched_src"], act["started_src"]) == (0, 0)
    ex = img.exec[1]
    for f, (v, rf) in PROBES["WorkflowExecutionInfo"].items():
        assert ex[rf] == v, f
    assert ex["flags"] == abi.EXEC_CANCEL_REQUESTED | abi.EXEC_RESET_POINTS_SET
    assert (ex["status"], ex["fail_step"], ex["current_version"], ex["next_event_id"]) == (0, -1, abi.EMPTY_VERSION, 77)
    assert (ex["start_src"], ex["decision_request_src"], ex["src_next"], ex["token_src"]) == (2, 2, 6, 1)
    assert (ex["checksum"], ex["payload_len"], ex["n_tasks"], ex["inconsistencies"]) == (0, 0, 0, 0)
    assert img.token(1) == lc.TOKEN
    # keys in first-seen blob order: the activity (blob 0), the timer (1), the execution blob's reset points (2)
    assert img.keys(1) == ["probe-activity", "probe-timer", "bin-x", "bin-y"]
    o = img.offsets[6]
    rp = img.rows["rp"][int(o[1]):int(o[2])]
    assert rp.tolist() == [(2, 0, 3, abi.ROW_LIVE | abi.ROW_RESETTABLE), (2, 1, 4, abi.ROW_LIVE)]
    o = img.offsets[5]
    assert img.rows["vh"][int(o[1]):int(o[2])].tolist() == [(4, 1), (19, 3)]


def test_absent_fields_take_the_getter_defaults_and_times_stay_distinct():
    """Empty structs: every getter's zero value (an absent time is Unix 0, not the Go zero time); a time equal
    to time.Time{}.UnixNano() becomes CRR_ZERO_TIME."""
    img = load_states_host(lc.defaults_batch())
    assert img.status.tolist() == [0, 0]
    want = np.zeros(1, abi.ACTIVITY_ROW)[0]
    want["schedule_id"], want["flags"] = 5, abi.ROW_LIVE | abi.ROW_MAPPED      # (ActivityID "": key 0, still mapped)
    assert img.rows["act"][0] == want                 # started_id 0 (GetStartedID), times Unix 0, started_src 0
    assert img.rows["timer"][0].tolist() == (0, 0, 0, 0, 1, 1, abi.ROW_LIVE)
    assert img.rows["child"][0].tolist() == (6, 0, 0, 0, 2, 2, abi.ROW_LIVE, 0)
    assert img.rows["rc"][0].tolist() == (7, 0, 0, 3, abi.ROW_LIVE)
    assert img.rows["sig"][0].tolist() == (8, 0, 0, 4, abi.ROW_LIVE)
    e = img.exec[0]
    want = np.zeros(1, abi.EXEC_ROW)[0]
    for f, v in dict(fail_step=-1, flags=abi.EXEC_RESET_POINTS_SET, next_event_id=9, completion_event_batch_id=abi.EMPTY_EVENT_ID,
                     current_version=abi.EMPTY_VERSION, decision_request_src=abi.SRC_NONE, start_src=5, n_activity=1, n_timer=1,
                     n_child=1, n_rc=1, n_signal=1, src_next=6).items():
        want[f] = v
    assert e == want                                  # token_src 0: the empty token; no items, no reset points
    a, t, e = img.rows["act"][1], img.rows["timer"][1], img.exec[1]
    assert a["scheduled_time"] == a["started_time"] == a["last_heartbeat_time"] == abi.ZERO_TIME
    assert t["expiry_time"] == abi.ZERO_TIME
    assert e["decision_started_ts"] == e["decision_scheduled_ts"] == e["decision_orig_scheduled_ts"] == abi.ZERO_TIME
    assert e["expiration_ns"] == 0 and e["decision_request_src"] == abi.SRC_EMPTY_UUID


# ---- the round trip ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", [None, 11])
def test_round_trip_of_replayed_prefix_states(shuffle):
    hs, pre, _suf, _mask, pre_b, pre_r = lc.prefix_case(600, 71)
    sbs = encode_states(pre_b, pre_r, pre, shuffle_seed=shuffle)
    loaded = pre_r.to_loaded(pre_b)
    assert loaded.mask.sum() > 400 and (~loaded.mask).sum() >= 0
    got = load_states_host(sbs)
    assert (got.status[loaded.mask] == 0).all() and (got.status[~loaded.mask] == abi.LoadStatus.EXECUTION_COUNT).all()
    assert (got.flags == 0).all() and got.err_blob == -1
    lc.assert_image_equals(got, lc.expected_image(loaded, sbs))
    # row mix worth testing, rows sorted by ID within each workflow
    assert all(got.rows[t].shape[0] > 20 for t in ("act", "timer", "child", "vh", "rp")) and got.rows["rc"].shape[0] > 0
    for t, name in enumerate(abi.LOAD_ROW_TABLES[:5]):
        ids = got.rows[name][got.rows[name].dtype.names[0]]
        first = np.zeros(ids.shape[0], bool)
        first[got.offsets[t][:-1][np.diff(got.offsets[t]) > 0]] = True
        assert (np.diff(ids)[~first[1:]] > 0).all(), name
    # the current branch token: the start token flatten puts in the arena
    for w in np.nonzero(loaded.mask)[0]:
        d = pre_b.wf[w]
        want = pre_b.arena[int(d["start_token_off"]):int(d["start_token_off"]) + int(d["start_token_len"])].tobytes()
        if loaded.exec["token_src"][w] == 1:
            assert got.token(w) == want
    assert (loaded.exec["token_src"][loaded.mask] == 1).sum() > 400
    # threads: the same bytes
    assert load_states_host(sbs, threads=4).image_bytes() == got.image_bytes()


def test_flags_sticky_and_current_index_one_of_two_histories():
    hs, pre, _suf, _mask, pre_b, pre_r = lc.prefix_case(600, 71)
    loaded = pre_r.to_loaded(pre_b)
    ok = np.nonzero(loaded.mask)[0]
    sticky, multi = set(ok[::3].tolist()), set(ok[::5].tolist())
    sbs = encode_states(pre_b, pre_r, pre, sticky=sticky, multi_branch=multi)
    got = load_states_host(sbs)
    want = np.zeros(len(pre), np.uint32)
    want[list(sticky)] |= abi.LOAD_FLAG_STICKY
    want[list(multi)] |= abi.LOAD_FLAG_MULTI_BRANCH
    assert (got.flags == want).all()
    lc.assert_image_equals(got, lc.expected_image(loaded, sbs))    # the right branch's items and token
    plain = load_states_host(encode_states(pre_b, pre_r, pre))
    assert got.tokens.tobytes() == plain.tokens.tobytes() and got.rows["vh"].tobytes() == plain.rows["vh"].tobytes()


# ---- edge cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_a_wavefront(n):
    img = load_states_host(build_blob_set([lc.good_workflow(i) for i in range(n)]))
    assert (img.status == 0).all() and img.exec.shape[0] == n
    assert all(np.array_equal(img.offsets[t], np.arange(n + 1)) for t in range(7))
    assert [img.keys(w) for w in range(n)] == [["bin-%d" % w, "a5", "t7"] for w in range(n)]


def test_execution_blob_alone():
    img = load_states_host(build_blob_set([(20, [lc.execution(lc.exec_blob())])]))
    e = img.exec[0]
    assert img.status[0] == 0 and (e["n_activity"], e["n_timer"], e["n_vh_items"], e["src_next"], e["start_src"]) == (0, 0, 1, 1, 0)
    assert img.keys(0) == [] and img.token(0) == lc.TOKEN


def test_sixty_five_activities_with_repeated_ids():
    img = load_states_host(build_blob_set([lc.good_workflow(0), lc.big_workflow(), lc.good_workflow(1)]))
    assert img.status.tolist() == [0, 0, 0]
    o = img.offsets[0]
    act = img.rows["act"][int(o[1]):int(o[2])]
    assert act.shape[0] == 65 and (np.diff(act["schedule_id"]) > 0).all()
    names = img.keys(1)
    assert names[:3] == ["act-0", "act-1", "act-2"] and sorted(names) == sorted(["act-%d" % k for k in range(9)] + ["bin"])
    by_name = {}
    for r in act:                                   # the greatest ScheduleID of each ActivityID is the mapped one
        by_name.setdefault(int(r["key"]), []).append(r)
    assert len(by_name) == 9
    for rows in by_name.values():
        assert [bool(r["flags"] & abi.ROW_MAPPED) for r in rows] == [False] * (len(rows) - 1) + [True]
    # provenance: each row's blob index holds its schedule_id
    sbs = build_blob_set([lc.good_workflow(0), lc.big_workflow(), lc.good_workflow(1)])
    b0 = int(sbs.wf["blob_begin"][1])
    assert (sbs.blob["id"][b0 + act["sched_src"]] == act["schedule_id"]).all()
    t = img.rows["timer"][int(img.offsets[1][1]):int(img.offsets[1][2])]
    assert (np.diff(t["started_id"]) > 0).all() and [names[k - 1] for k in t["key"]] == ["act-%d" % k for k in (4, 3, 2, 1, 0)]
    rp = img.rows["rp"][int(img.offsets[6][1]):int(img.offsets[6][2])]
    assert [names[k - 1] for k in rp["key"]] == ["act-3", "bin", "bin"] and rp["src"].tolist() == [40] * 3


def test_each_failure_status_leaves_the_rest_of_the_batch_alone():
    sbs, want = lc.failure_batch()
    img = load_states_host(sbs)
    assert img.status.tolist() == want.tolist()
    good = load_states_host(build_blob_set([lc.good_workflow(0)]))
    for w in range(want.shape[0]):
        if want[w]:
            assert img.exec[w] == np.zeros(1, abi.EXEC_ROW)[0] and img.flags[w] == 0
            assert all(img.offsets[t][w] == img.offsets[t][w + 1] for t in range(abi.LOAD_TABLES))
        else:
            assert img.exec[w] == good.exec[0]
            assert all(img.offsets[t][w + 1] - img.offsets[t][w] == good.offsets[t][1] for t in range(abi.LOAD_T_KEY_BYTES))
    # the summary names the lowest malformed blob
    names = list(lc.FAILURES)
    w = 2 * names.index("malformed_activity") + 1
    assert img.err_blob == int(sbs.wf["blob_begin"][w]) + 1


@pytest.mark.parametrize("kind", range(6))
def test_every_truncation_length_reports_malformed(kind):
    sbs = lc.truncation_batches()[kind]
    st = _status(sbs)
    assert st.shape[0] > 10 and st[0] == 0 and st[-1] == 0
    assert (st[1:-1] == abi.LoadStatus.MALFORMED).all(), np.nonzero(st[1:-1] != abi.LoadStatus.MALFORMED)[0]


def test_libraries_export_the_loader_and_reject_bad_arguments():
    """cadence_load.h: the device entry points are in the replay library, the restatement in the host library;
    invalid arguments are refused before anything touches a device."""
    import ctypes
    import os
    import re
    from cadence_amd import decode, engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r"\b(crr_load_\w+)\s*\(", open(os.path.join(root, "include", "cadence_load.h")).read()))
    assert declared == {"crr_load_scratch_bytes", "crr_load_states_plan", "crr_load_states_read", "crr_load_states_place",
                        "crr_load_states_host"}
    dev = ctypes.CDLL(engine.LIB_PATH)
    for s in declared - {"crr_load_states_host"}:
        assert hasattr(dev, s), s
    assert hasattr(decode.lib(), "crr_load_states_host")
    dev.crr_abi_version.restype = ctypes.c_int
    assert dev.crr_abi_version() == abi.ABI_VERSION == 8
    dev.crr_load_scratch_bytes.restype = ctypes.c_size_t
    dev.crr_load_scratch_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    assert dev.crr_load_scratch_bytes(1000, 100) > dev.crr_load_scratch_bytes(10, 1) > 0
    S = abi.CLoadSummary()
    assert dev.crr_load_states_plan(None, None, 0, ctypes.byref(S), None) == -1
    assert dev.crr_load_states_read(None, 0, ctypes.byref(S), None, None) == -1
    assert dev.crr_load_states_place(None, 0, ctypes.byref(S), None, None, None, None) == -1
    host = persisted._host_lib()
    assert host.crr_load_states_host(None, None, ctypes.byref(S), 1) == -1
    sbs = build_blob_set([lc.good_workflow(0), lc.good_workflow(1)])
    sbs.wf["blob_begin"][1] += 1            # ranges that are not consecutive
    c = persisted._c_batch(sbs, lambda a: a.ctypes.data)
    assert host.crr_load_states_host(ctypes.byref(c), None, ctypes.byref(S), 1) == -1


def test_host_restatement_under_asan_and_ubsan(tmp_path):
    assert "6 full blobs OK, 1033 truncations malformed" in asan_tool.build_and_run(tmp_path, "load_states_asan")
