"""The pending-entry mutation of a committed replication task, by the host restatement (crr_load_mutation_host,
include/cadence_load_mutation.h): the CPU side of tests/test_gpu_load_mutation.py.  Expected values are
mutation_cases' Python restatement of the header's semantics over the expected loaded image and the oracle's resumed
replay; the round trip applies the result to the persisted blobs and loads them again."""
import ctypes
import functools
import os
import re

import numpy as np

from cadence_amd import abi, persisted
from cadence_amd.persisted import (apply_mutation, load_states_host, load_states_verify_host, mutation_host,
                                   store_checksums_host, store_version_histories_host)

import asan_tool
import mutation_cases as mc
import store_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O = abi.StoreOutcome


def test_header_pins():
    """The test to run against the parent commit: it needs nothing but the header, the two libraries and abi.py."""
    from cadence_amd import decode, engine
    text = open(os.path.join(ROOT, "include", "cadence_load_mutation.h")).read()
    assert set(re.findall(r"\b(crr_load_\w+)\s*\(", text)) == {
        "crr_load_mutation_scratch_bytes", "crr_load_mutation_plan", "crr_load_mutation_run", "crr_load_mutation_host"}
    dev = ctypes.CDLL(engine.LIB_PATH)
    for f in ("crr_load_mutation_scratch_bytes", "crr_load_mutation_plan", "crr_load_mutation_run"):
        assert hasattr(dev, f), f
    assert hasattr(decode.lib(), "crr_load_mutation_host")
    dev.crr_abi_version.restype = ctypes.c_int
    assert dev.crr_abi_version() == abi.ABI_VERSION == 8
    abi.check_layout(dev)
    assert dev.crr_sizeof(33) == abi.MUTATION_ROW.itemsize == 96
    assert dev.crr_sizeof(34) == ctypes.sizeof(abi.CMutationSizes) == 112
    assert dev.crr_sizeof(35) == ctypes.sizeof(abi.CMutationOut) == 176
    assert dev.crr_sizeof(29) == 0 and dev.crr_sizeof(32) == 0      # the two indices earlier pins keep unassigned
    assert "crr_sizeof(33..35)" in open(os.path.join(ROOT, "include", "cadence_replay.h")).read()
    # struct offsets as the header lays them out
    assert [abi.MUTATION_ROW.fields[f][1] for f in ("outcome", "status", "flags", "exec_index", "map")] == [0, 4, 8, 12, 16]
    assert abi.MUTATION_MAP.itemsize == 16 and abi.MUTATION_ROW["map"].shape == (5,)
    assert [abi.MUTATION_MAP.fields[f][1] for f in ("upsert_begin", "n_upsert", "delete_begin", "n_delete")] == [0, 4, 8, 12]
    S, Q = abi.CMutationSizes, abi.CMutationOut
    assert [getattr(S, f).offset for f in ("err", "n_tasks", "n_exec", "n_upsert", "n_delete", "work_needed", "run_work_needed")] == \
        [0, 4, 8, 16, 56, 96, 104]
    assert [getattr(Q, f).offset for f in ("exec", "exec_capacity", "upsert", "upsert_capacity", "deleted", "delete_capacity")] == \
        [0, 8, 16, 56, 96, 136]
    assert re.search(r"#define CRR_MUTATION_MAPS 5\b", text) and re.search(r"#define CRR_MUTATION_RESET_POINTS_CHANGED 1u", text)
    assert abi.MUTATION_MAPS == abi.LOAD_ROW_TABLES[:5] and abi.MUTATION_NO_EXEC == 0xFFFFFFFF
    for words, name in zip((14, 5, 6, 4, 4), abi.MUTATION_MAPS):   # every row image is whole 8-byte words
        assert mc.DTYPES[name].itemsize == 8 * words
    assert abi.EXEC_ROW.itemsize == 208


def test_hand_states_reach_every_outcome():
    c = sc.hand_case()
    before = load_states_host(c.sbs)
    want, tally = mc.expected_mutation(c.tasks, c.want, before, c.after)
    assert set(int(x) for x in want.rows["outcome"]) == set(int(x) for x in O)
    got = mutation_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.after)
    mc.assert_mutation(got, want, "with the replayed states")
    # outcome and status are crr_store_row's
    store = store_checksums_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.after)
    assert (got.rows["outcome"] == store["outcome"]).all() and (got.rows["status"] == store["status"]).all()
    applied = got.rows["outcome"] == O.APPLIED
    assert applied.sum() == 3 and got.exec.shape[0] == 3 and (got.rows["exec_index"][applied] == [0, 1, 2]).all()
    assert (got.rows["exec_index"][~applied] == abi.MUTATION_NO_EXEC).all()
    for f in ("n_upsert", "n_delete"):
        assert (got.rows["map"][f][~applied] == 0).all()
    assert (got.rows["flags"][~applied] == 0).all()
    # the three replayed states had nothing pending before: every row the replay left is new
    assert [tally.new[m] for m in mc.MAPS] == [3, 1, 1, 2, 1] and sum(tally.deleted.values()) == 0
    # BACKFILLED: reported, nothing pending changes, no exec row
    back = got.rows["outcome"] == O.BACKFILLED
    assert back.sum() >= 5
    # no post-replay state: no task can be APPLIED, nothing is gathered
    none = mutation_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, None)
    assert (none.rows["outcome"] == c.want_without["outcome"]).all() and (none.rows["status"] == c.want_without["status"]).all()
    assert none.exec.shape[0] == 0 and none.n_bytes == none.rows.nbytes
    # tasks are independent: any order, any subset
    order = np.random.default_rng(1).permutation(c.tasks.shape[0])[:20]
    sub = mutation_host(c.sbs, c.tasks[order], c.last_events[order], c.results[order], c.routes[order], c.after, threads=3)
    want_sub, _ = mc.expected_mutation(c.tasks[order], c.want[order], before, c.after)
    mc.assert_mutation(sub, want_sub, "a shuffled subset")


def test_hand_states_every_classification_per_map():
    c = mc.hand_classification_case()
    want, tally = mc.expected_mutation(c.tasks, c.store_rows, c.before, c.after)
    # the Python restatement against the lists written out by hand
    for k, w in enumerate(c.tasks["wf"]):
        for m in mc.MAPS:
            ups, dels = c.want[int(w)][m]
            assert [int(x) for x in want.upserts(k, m)[mc.KEY_F[m]]] == ups, (k, m)
            assert [int(x) for x in want.deletes(k, m)] == dels, (k, m)
        assert bool(want.rows[k]["flags"] & abi.MUTATION_RESET_POINTS_CHANGED) == c.want[int(w)]["flag"]
    assert tally.restarted == 3 and tally.status_only == 2      # workflow 0 is named by two tasks, workflow 3 by one
    got = mutation_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.after)
    mc.assert_mutation(got, want)
    # the restarted TimerID is one upsert and no delete; the row carries the new started_id
    k3 = int(np.nonzero(c.tasks["wf"] == 3)[0][0])
    assert got.deletes(k3, "timer").shape[0] == 0 and [int(x) for x in got.upserts(k3, "timer")["started_id"]] == [12]
    # a change in a derived field only is not an upsert: activity 5 (MAPPED, last_hb_timeout_vis_s), child 17 (padding)
    k0 = int(np.nonzero(c.tasks["wf"] == 0)[0][0])
    assert 5 not in got.upserts(k0, "act")["schedule_id"] and 17 not in got.upserts(k0, "child")["initiated_id"]
    # an untouched state: the exec row alone
    k1 = int(np.nonzero(c.tasks["wf"] == 1)[0][0])
    assert got.rows[k1]["flags"] == 0 and (got.rows[k1]["map"]["n_upsert"] == 0).all() and (got.rows[k1]["map"]["n_delete"] == 0).all()
    assert got.exec_of(k1).tobytes() == c.after.exec[1].tobytes()
    # the two tasks that name workflow 0 get the same mutation
    a, b = np.nonzero(c.tasks["wf"] == 0)[0]
    for m in mc.MAPS:
        assert got.upserts(a, m).tobytes() == got.upserts(b, m).tobytes() and got.deletes(a, m).tobytes() == got.deletes(b, m).tobytes()
    assert mutation_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.after, threads=4).image_bytes() == got.image_bytes()


@functools.lru_cache(maxsize=None)
def _small_host():
    r = mc.replayed_small()
    return r, mutation_host(r.rc.sbs, r.rc.tasks, r.rc.last_events, r.results, r.routes, r.after)


def _print_tally(what, t: mc.Tally):
    print(what, "applied tasks", len(t.applied_tasks), "new", t.new, "deleted", t.deleted, "changed", t.changed,
          "untouched", t.untouched, "restarted", t.restarted, "status only", t.status_only)


def test_replayed_case():
    r, got = _small_host()
    _print_tally("replayed case:", r.tally)
    mc.assert_mutation(got, r.want)
    t = r.tally
    assert len(t.applied_tasks) >= 30 and (got.rows["outcome"] == O.BACKFILLED).sum() >= 5
    assert t.new["act"] >= 40 and t.deleted["act"] >= 4 and t.changed["act"] >= 3 and t.untouched["act"] >= 15
    assert t.new["timer"] >= 15 and t.deleted["timer"] >= 2
    # no untouched row is reported: what is reported is exactly the new and the changed rows
    for m in mc.MAPS:
        assert got.upsert[m].shape[0] == t.new[m] + t.changed[m] and got.deleted[m].shape[0] == t.deleted[m]
    assert got.exec.shape[0] == len(t.applied_tasks)


def test_replayed_case_through_the_long_tail():
    r = mc.replayed_tail()
    _print_tally("long tail:", r.tally)
    got = mutation_host(r.rc.sbs, r.rc.tasks, r.rc.last_events, r.results, r.routes, r.after, threads=4)
    mc.assert_mutation(got, r.want)
    t = r.tally
    assert t.restarted >= 15 and t.status_only >= 5 and t.changed["child"] >= 30
    assert t.deleted["rc"] >= 50 and t.deleted["sig"] >= 50
    # each restart is an upsert with no delete
    for k in t.applied_tasks:
        w = int(r.rc.tasks[k]["wf"])
        before, after = sc.rows_of(r.before, w)["timer"], sc.rows_of(r.after, w)["timer"]
        old = {int(x["key"]): int(x["started_id"]) for x in before}
        for x in after:
            if int(x["key"]) in old and old[int(x["key"])] != int(x["started_id"]):
                assert int(x["key"]) in got.upserts(k, "timer")["key"] and int(x["key"]) not in got.deletes(k, "timer")


def _round_trip(r: mc.Replayed, m: persisted.Mutation, vh, store, load, verify):
    """apply_mutation of a result, loaded again: the states equal the snapshot's in every persisted field and verify
    MATCH against the generated checksums."""
    rc = r.rc
    applied, stored = np.zeros(rc.sbs.n_wf, bool), [None] * rc.sbs.n_wf
    points = {}
    for k in np.nonzero(m.rows["outcome"] == O.APPLIED)[0]:
        w = int(rc.tasks[k]["wf"])
        applied[w] = True
        stored[w] = (abi.CHECKSUM_PAYLOAD_V1, abi.CHECKSUM_FLAVOR_CRC32, int(store["value"][k]).to_bytes(4, "big"))
        points[w] = mc.reset_points_of(r.after, w)
    assert applied.sum() >= 30
    names = [r.after.interners[w] for w in range(rc.sbs.n_wf)]
    new = apply_mutation(rc.sbs, rc.tasks, m, vh, store, names, reset_points=points)
    got, want = load(new), load(sc.reencoded_applied(rc, applied))
    for w in np.nonzero(applied)[0]:
        assert mc.persisted_view(got, int(w)) == mc.persisted_view(want, int(w)), w
    v = verify(new, persisted.stored_checksums(stored))
    assert (v["outcome"][applied] == abi.VerifyOutcome.MATCH).all()
    # a backfilled state: the stored pending entries, the new VersionHistories
    back = np.nonzero(m.rows["outcome"] == O.BACKFILLED)[0]
    assert back.size >= 5
    stored_before = load(rc.sbs)
    for k in back:
        w = int(rc.tasks[k]["wf"])
        a, b = mc.persisted_view(got, w), mc.persisted_view(stored_before, w)
        assert {x: a[x] for x in mc.MAPS} == {x: b[x] for x in mc.MAPS} and a["exec"]["n_vh_items"] >= b["exec"]["n_vh_items"]
    return new


def test_round_trip_applied_mutation_loads_as_the_snapshot():
    r, got = _small_host()
    args = (r.rc.sbs, r.rc.tasks, r.rc.last_events, r.results, r.routes, r.after)
    _round_trip(r, got, store_version_histories_host(*args), store_checksums_host(*args), load_states_host, load_states_verify_host)


def _host_call(c, rows, out, n=None, after="case"):
    host = persisted._host_lib()
    cb = persisted._c_batch(c.sbs, lambda a: a.ctypes.data)
    img, keep = persisted._after_image(c.after if after == "case" else after, c.sbs.n_wf)
    P = abi.CMutationSizes()
    n = c.tasks.shape[0] if n is None else n
    rc = host.crr_load_mutation_host(ctypes.byref(cb), c.tasks.ctypes.data, c.last_events.ctypes.data, n, c.results.ctypes.data,
                                     c.routes.ctypes.data, ctypes.byref(img) if img is not None else None,
                                     rows.ctypes.data if rows is not None else None,
                                     ctypes.byref(out) if out is not None else None, ctypes.byref(P), 1)
    return rc, P, keep


GUARD = 0x5A


def _guarded(P: abi.CMutationSizes, short=None):
    """Output buffers of exactly the plan's totals (``short``: that one a row short) between guard bytes."""
    bufs, o = {}, abi.CMutationOut()

    def make(name, count, item):
        count = max(count - (1 if name == short else 0), 0)
        a = np.full(count * item + 32, GUARD, np.uint8)
        bufs[name] = (a, count * item)
        return a.ctypes.data + 16, count
    o.exec, o.exec_capacity = make("exec", int(P.n_exec), abi.EXEC_ROW.itemsize)
    for t, m in enumerate(abi.MUTATION_MAPS):
        o.upsert[t], o.upsert_capacity[t] = make("upsert." + m, int(P.n_upsert[t]), mc.DTYPES[m].itemsize)
        o.deleted[t], o.delete_capacity[t] = make("deleted." + m, int(P.n_delete[t]), 8)
    return bufs, o


def _guards_intact(bufs, written=True):
    for name, (a, n) in bufs.items():
        assert (a[:16] == GUARD).all() and (a[16 + n:] == GUARD).all(), name
        if not written:
            assert (a == GUARD).all(), name


def test_capacity_exactly_the_totals_and_one_row_short():
    c = mc.hand_classification_case()
    want, _ = mc.expected_mutation(c.tasks, c.store_rows, c.before, c.after)
    rc, P, _k = _host_call(c, None, None)
    assert rc == 0 and int(P.n_exec) == 5 and int(P.n_tasks) == 5 and int(P.run_work_needed) > 0
    assert [int(x) for x in P.n_upsert] == [want.upsert[m].shape[0] for m in mc.MAPS]
    assert [int(x) for x in P.n_delete] == [want.deleted[m].shape[0] for m in mc.MAPS]
    rows = np.zeros(c.tasks.shape[0], abi.MUTATION_ROW)
    bufs, o = _guarded(P)
    assert _host_call(c, rows, o)[0] == 0
    _guards_intact(bufs)
    assert rows.tobytes() == want.rows.tobytes()
    assert bufs["exec"][0][16:-16].tobytes() == want.exec.tobytes()
    for m in mc.MAPS:
        assert bufs["upsert." + m][0][16:-16].tobytes() == want.upsert[m].tobytes(), m
        assert bufs["deleted." + m][0][16:-16].tobytes() == want.deleted[m].tobytes(), m
    for short in ["exec"] + ["upsert." + m for m in mc.MAPS] + ["deleted." + m for m in mc.MAPS]:
        bufs, o = _guarded(P, short)
        rows[:] = 0
        assert _host_call(c, rows, o)[0] == -1, short
        _guards_intact(bufs, written=False)
        assert not rows.tobytes().strip(b"\0"), short


def test_bad_arguments():
    from cadence_amd import engine
    dev = ctypes.CDLL(engine.LIB_PATH)
    vp = ctypes.c_void_p
    dev.crr_load_mutation_plan.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_uint32] + [vp] * 9 + [ctypes.c_size_t, vp, vp]
    dev.crr_load_mutation_run.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp] + [vp] * 11 + [ctypes.c_size_t, vp]
    S, N, P = abi.CLoadSummary(), abi.CLoadNdcSizes(), abi.CMutationSizes()
    assert dev.crr_load_mutation_plan(None, None, 0, ctypes.byref(S), None, None, 0, None, None, None, ctypes.byref(N),
                                      None, None, None, None, None, 0, ctypes.byref(P), None) == -1
    assert dev.crr_load_mutation_run(None, None, 0, ctypes.byref(S), None, None, None, None, None, ctypes.byref(N), None, None,
                                     None, None, ctypes.byref(P), None, None, 0, None) == -1
    c = mc.hand_classification_case()
    host = persisted._host_lib()
    cb = persisted._c_batch(c.sbs, lambda a: a.ctypes.data)
    rows = np.zeros(c.tasks.shape[0], abi.MUTATION_ROW)
    args = [c.tasks.ctypes.data, c.last_events.ctypes.data, c.tasks.shape[0], c.results.ctypes.data, c.routes.ctypes.data, None,
            rows.ctypes.data, None, ctypes.byref(P), 1]
    assert host.crr_load_mutation_host(None, *args) == -1
    for drop in (0, 1, 3, 4, 8):
        bad = list(args)
        bad[drop] = None
        assert host.crr_load_mutation_host(ctypes.byref(cb), *bad) == -1, drop
    img = abi.CLoadImage()                                                    # an after-image without exec rows
    bad = list(args)
    bad[5] = ctypes.byref(img)
    assert host.crr_load_mutation_host(ctypes.byref(cb), *bad) == -1
    assert host.crr_load_mutation_host(ctypes.byref(cb), *args) == 0
    assert (rows["outcome"] == O.NOT_RESUMED).all() and int(P.n_exec) == 0 and int(P.run_work_needed) == 0


def test_empty_batch_and_no_tasks():
    empty = persisted.build_blob_set([])
    tasks = np.zeros(3, abi.REPL_TASK)
    tasks["wf"] = [0, 5, 0xFFFFFFFF]
    routes = np.zeros(3, abi.NDC_ROUTE)
    routes["route"] = abi.ROUTE_APPLY_CURRENT
    got = mutation_host(empty, tasks, np.zeros(3, abi.LAST_EVENT), np.zeros(3, abi.NDC_RESULT), routes)
    assert (got.rows["outcome"] == O.NOT_LOADED).all() and (got.rows["exec_index"] == abi.MUTATION_NO_EXEC).all()
    assert got.exec.shape[0] == 0 and all(got.upsert[m].shape[0] == 0 and got.deleted[m].shape[0] == 0 for m in mc.MAPS)
    c = mc.hand_classification_case()
    none = mutation_host(c.sbs, c.tasks[:0], c.last_events[:0], c.results[:0], c.routes[:0], c.after)
    assert none.rows.shape == (0,) and none.exec.shape == (0,) and none.n_bytes == 0


def garbage_case():
    """The hand classification case with an exec row that failed its replay (workflow 1, status 9, counts no table
    holds) and one whose counts no table holds (workflow 2: its rows are those the image has for it, none)."""
    c = mc.hand_classification_case()
    ex = c.after.exec.copy()
    ex["status"][1] = 9
    for f in ("n_activity", "n_timer", "n_child", "n_rc", "n_signal", "n_reset_points"):
        ex[f][1] = 1 << 30
        ex[f][2] = 0x7FFFFFFF
    ex["n_vh_items"][2] = -5
    return c, ex


def test_failed_replays_and_garbage_counts_stay_within_the_image():
    c, ex = garbage_case()
    # the dense image holds what the counts said when it was built: the garbage counts are clamped to that
    img, keep = persisted._after_image(c.after, c.sbs.n_wf)
    img.exec = ex.ctypes.data                # (the case's own exec rows stay as they are)
    host = persisted._host_lib()
    cb = persisted._c_batch(c.sbs, lambda a: a.ctypes.data)
    P = abi.CMutationSizes()
    args = (ctypes.byref(cb), c.tasks.ctypes.data, c.last_events.ctypes.data, c.tasks.shape[0], c.results.ctypes.data,
            c.routes.ctypes.data, ctypes.byref(img))
    assert host.crr_load_mutation_host(*args, None, None, ctypes.byref(P), 1) == 0
    rows = np.zeros(c.tasks.shape[0], abi.MUTATION_ROW)
    bufs, o = _guarded(P)
    assert host.crr_load_mutation_host(*args, rows.ctypes.data, ctypes.byref(o), ctypes.byref(P), 1) == 0
    _guards_intact(bufs)
    want, _ = mc.expected_mutation(c.tasks, c.store_rows, c.before, c.after)
    k1, k2 = int(np.nonzero(c.tasks["wf"] == 1)[0][0]), int(np.nonzero(c.tasks["wf"] == 2)[0][0])
    assert (int(rows[k1]["outcome"]), int(rows[k1]["status"])) == (int(O.REPLAY_FAILED), 9)
    assert (rows[k1]["map"]["n_upsert"] == 0).all() and (rows[k1]["map"]["n_delete"] == 0).all() and rows[k1]["exec_index"] == abi.MUTATION_NO_EXEC
    # workflow 2's image holds no pending row: clamped, its mutation is what it was, every entry deleted
    assert (rows[k2]["map"]["n_upsert"] == 0).all() and (rows[k2]["map"]["n_delete"] == want.rows[k2]["map"]["n_delete"]).all()
    # no other task's result changes
    for k in range(c.tasks.shape[0]):
        if k not in (k1, k2):
            for f in ("outcome", "status", "flags"):
                assert rows[k][f] == want.rows[k][f]
            assert (rows[k]["map"]["n_upsert"] == want.rows[k]["map"]["n_upsert"]).all()
            assert (rows[k]["map"]["n_delete"] == want.rows[k]["map"]["n_delete"]).all()


def test_host_restatement_under_asan_and_ubsan(tmp_path):
    asan_tool.build_and_run(tmp_path, "load_mutation_asan")
