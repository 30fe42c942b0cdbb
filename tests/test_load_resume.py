"""CPU: the resumed replay of routed tasks planned from loaded states (include/cadence_load_resume.h): the header's
pins, the host restatement (crr_load_resume_host) against the host path the other tests trust --
``flatten(suffixes, loaded=load_states_host(...).resumable(mask))`` -- on the replayed case, hand cases for every
outcome, and the stand-alone sanitizer program.
"""
import ctypes
import os

import numpy as np

from cadence_amd import abi, blobs, persisted

import asan_tool
import load_resume_cases as rc_
import store_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = abi.ResumeOutcome


def test_header_pins():
    dev = ctypes.CDLL(os.path.join(ROOT, "cadence_amd", "libcadence_replay.so"))
    dev.crr_sizeof.restype = ctypes.c_size_t
    assert dev.crr_sizeof(40) == abi.LOAD_RESUME_ROW.itemsize == 8
    assert dev.crr_sizeof(41) == ctypes.sizeof(abi.CLoadResumeSizes) == 80
    assert dev.crr_sizeof(42) == ctypes.sizeof(abi.CLoadResumeOut) == 88
    assert dev.crr_sizeof(43) == ctypes.sizeof(abi.CLoadResumeTotals) == 72
    assert dev.crr_sizeof(39) == 0 and dev.crr_sizeof(29) == 0 and dev.crr_sizeof(32) == 0   # the indices earlier pins keep unassigned
    assert dev.crr_abi_version() == 8
    for name in ("crr_load_resume_scratch_bytes", "crr_load_resume_plan", "crr_load_resume_gather", "crr_load_resume_finalize",
                 "crr_load_resume_settle", "crr_ingest_resume_counts"):
        assert hasattr(dev, name), name
    assert hasattr(persisted._host_lib(), "crr_load_resume_host")
    header = open(os.path.join(ROOT, "include", "cadence_load_resume.h")).read()
    assert "#define CRR_RESUME_COUNT_ROWS 10" in header and abi.RESUME_COUNT_ROWS == 10
    for name, v in (("APPLIED", 0), ("SHADOWED", 1), ("NOT_ROUTED", 2), ("NOT_LOADED", 3)):
        assert "CRR_RESUME_%s = %d" % (name, v) in header and int(R[name]) == v
    assert "crr_sizeof(40..43)" in open(os.path.join(ROOT, "include", "cadence_replay.h")).read()


def test_restatement_equals_the_host_path_on_the_replayed_case():
    p = rc_.planned_small()
    rc = p.rc
    assert rc.sbs.n_wf == 64 and rc.tasks.shape[0] == 62
    assert int((p.routes["route"] == abi.ROUTE_APPLY_CURRENT).sum()) == 51
    img = rc_.host_resume(rc.sbs, rc.tasks, p.routes, p.tbs)
    assert rc_.compare_with_flatten(p, img) == 51
    P = img.sizes
    assert int(P.n_applied) == 51 and int(P.n_tasks) == 62 and int(P.n_wf) == 64
    out = img.rows["outcome"]
    assert int((out == R.APPLIED).sum()) == 51 and int((out == R.NOT_ROUTED).sum()) == 11
    # the sizes are the sums of what was compared
    applied = np.nonzero(img.task_of >= 0)[0]
    assert int(P.n_keys) == sum(len(p.loaded.keys(int(w))) for w in applied) > 0
    assert int(P.key_bytes) == sum(len(s.encode()) for w in applied for s in p.loaded.keys(int(w)))
    assert int(P.blob_bytes) == sum(len(p.tbs.blob(int(p.tbs.wf[k]["blob_begin"]) + j))
                                    for k in img.task_of[applied] for j in range(int(p.tbs.wf[k]["blob_count"])))
    assert int(P.n_bytes) == (int(P.blob_bytes) + 15) // 16 * 16 + int(P.key_bytes) == img.bytes.shape[0]
    assert int(P.token_bytes) == sum((len(p.loaded.token(int(w))) + 7) // 8 * 8 for w in applied) == img.arena.shape[0]
    # blob ranges are consecutive and cover the gathered blobs
    bb, bc = img.wf["blob_begin"].astype(np.int64), img.wf["blob_count"].astype(np.int64)
    assert (bb == np.cumsum(bc) - bc).all() and int(bc.sum()) == int(P.n_blobs) == img.blob_off.shape[0] - 1
    kc = img.key_count.astype(np.int64)
    assert (img.key_begin == np.cumsum(kc) - kc).all()
    # the tasks are in shuffled order: the gather reorders
    assert (np.diff(img.task_of[applied]) < 0).any()


def test_hand_cases_every_outcome():
    c = sc.hand_case()
    tasks, routes, tbs = rc_.hand_tasks()
    img = rc_.host_resume(c.sbs, tasks, routes, tbs)
    loaded = persisted.load_states_host(c.sbs)
    assert not loaded.mask[4] and loaded.mask[[0, 1, 2, 3, 5]].all()
    for k, (_w, _route, outcome, pos) in enumerate(rc_.HAND_TASKS):
        assert int(img.rows[k]["outcome"]) == int(outcome), k
        assert int(img.rows[k]["position"]) == (0xFFFFFFFF if pos is None else pos), k
    assert img.task_of.tolist() == [-1, 0, 6, 8, -1, 9]
    # a state with no token; states with an empty dictionary and with one
    assert loaded.token(2) == b"" and int(img.desc[2]["start_token_len"]) == 0 and int(img.desc[2]["flags"]) & abi.WF_FLAG_RESUME
    assert loaded.token(1) != b"" and img.token(1) == loaded.token(1)
    dicts = [len(loaded.keys(w)) for w in range(6)]
    assert dicts[1] == 0 and int(img.key_count[1]) == 0 and max(dicts[2], dicts[3]) > 0
    for w in (1, 2, 3, 5):
        assert img.keys(w) == loaded.keys(w)
        k = int(img.task_of[w])
        b0 = int(img.wf[w]["blob_begin"])
        assert int(img.wf[w]["blob_count"]) == 1 and img.blob(b0) == tbs.blob(int(tbs.wf[k]["blob_begin"]))
        h = rc_.hand_history(k)
        d = img.desc[w]
        assert (int(d["init_version"]), int(d["now_ns"]), int(d["retention_days"])) == (h.domain_failover_version, h.now_ns, h.retention_days)
        # each task starts one timer and schedules one activity on top of the loaded rows
        assert int(d["timer_cap"]) == int(loaded.exec[w]["n_timer"]) + 1 and int(d["act_cap"]) == int(loaded.exec[w]["n_activity"]) + 1
        assert int(d["vh_cap"]) == int(loaded.exec[w]["n_vh_items"]) + 1 and int(d["ev_count"]) == 2 and int(d["empty_batch_at"]) == -1
    for w in (0, 4):
        d = img.desc[w]
        assert int(d["ev_count"]) == 0 and int(d["flags"]) == 0 and all(int(d[f]) == 0 for f in rc_.CAPS)
    for base_f, cap_f in zip(rc_.BASES, rc_.CAPS):
        cap = img.desc[cap_f].astype(np.int64)
        assert (img.desc[base_f] == np.cumsum(cap) - cap).all()


def test_no_applied_task_at_all():
    c = sc.hand_case()
    rows = [(1, abi.ROUTE_NON_CURRENT, R.NOT_ROUTED, None), (4, abi.ROUTE_APPLY_CURRENT, R.NOT_LOADED, None),
            (99, abi.ROUTE_APPLY_CURRENT, R.NOT_LOADED, None), (2, abi.ROUTE_REBUILD, R.NOT_ROUTED, None)]
    tasks, routes, tbs = rc_.hand_tasks(rows)
    img = rc_.host_resume(c.sbs, tasks, routes, tbs)
    P = img.sizes
    assert [int(x) for x in (P.n_applied, P.n_blobs, P.blob_bytes, P.n_keys, P.key_bytes, P.token_bytes, P.n_bytes)] == [0] * 7
    assert img.table_rows == [0] * 8 and img.blob_off.tolist() == [0] and (img.task_of == -1).all()
    assert [int(x) for x in img.rows["outcome"]] == [int(r[2]) for r in rows]
    assert not img.desc["flags"].any() and not img.desc["ev_count"].any()
    # no task, and no state
    img = rc_.host_resume(c.sbs, tasks[:0], routes[:0], rc_.task_blob_set([]))
    assert int(img.sizes.n_applied) == 0 and img.rows.shape == (0,)
    empty = persisted.build_blob_set([])
    img = persisted.load_resume_host(empty, tasks, routes, tbs, np.zeros((abi.RESUME_COUNT_ROWS, 0), np.int32))
    assert [int(x) for x in img.rows["outcome"]] == [int(R.NOT_ROUTED), int(R.NOT_LOADED), int(R.NOT_LOADED), int(R.NOT_ROUTED)]


def test_blob_ranges_outside_the_task_batch_read_as_no_blobs():
    c = sc.hand_case()
    tasks, routes, tbs = rc_.hand_tasks()
    wf = tbs.wf.copy()
    wf[0]["blob_begin"], wf[0]["blob_count"] = tbs.n_blobs + 3, 1
    wf[6]["blob_begin"], wf[6]["blob_count"] = 2, 0xFFFFFFFF
    bad = blobs.BlobSet(bytes=tbs.bytes, blob_off=tbs.blob_off, wf=wf, strings=tbs.strings)
    img = persisted.load_resume_host(c.sbs, tasks, routes, bad)
    assert img.task_of.tolist() == [-1, 0, 6, 8, -1, 9]
    assert img.wf["blob_count"].tolist() == [0, 0, 0, 1, 0, 1] and int(img.sizes.n_blobs) == 2


def test_host_restatement_under_asan_and_ubsan(tmp_path):
    assert "24 batches" in asan_tool.build_and_run(tmp_path, "load_resume_asan")
