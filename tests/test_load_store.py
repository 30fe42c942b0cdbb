"""The checksum to store for routed replication tasks, by the host restatement (crr_load_store_checksums_host,
include/cadence_load_store.h): the value Go's generateChecksum gives when CloseTransactionAsMutation commits a task
applied to the current branch or backfilled onto another one.

Expected values are oracle/checksum_py.encode_payload + zlib.crc32 over the values the cases wrote into the blobs, the
oracle's rows for the replayed part and a few-line AddOrUpdateItem (store_cases.py).  A stand-alone program runs the
same call under AddressSanitizer / UndefinedBehaviorSanitizer.
"""
import ctypes
import functools
import os
import re

import numpy as np

from cadence_amd import abi, persisted
from cadence_amd.persisted import load_states_verify_host, store_checksums_host

import asan_tool
import store_cases as sc
import verify_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O = abi.StoreOutcome


def assert_rows(got: np.ndarray, want: np.ndarray, what=""):
    assert got.dtype == abi.STORE_ROW and got.shape == want.shape
    for f in abi.STORE_ROW.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what} {f}: {bad.size} tasks differ, first {bad[:5]}: {got[f][bad[:5]]} vs {want[f][bad[:5]]}"


def test_hand_states_reach_every_outcome():
    c = sc.hand_case()
    assert set(int(x) for x in c.want["outcome"]) == set(int(x) for x in O)
    assert {int(abi.Status.VH_LOWER_VERSION), int(abi.Status.VH_EVENT_ID_NOT_INCREASING), int(abi.Status.VH_INVALID_ITEM),
            int(abi.Status.NDC_BAD_INDEX)} <= set(int(x) for x in c.want["status"][c.want["outcome"] == O.VH_ERROR])
    got = store_checksums_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.after)
    assert_rows(got, c.want, "with the replayed states")
    gen = np.isin(got["outcome"], [O.APPLIED, O.BACKFILLED])
    assert (got["value"][~gen] == 0).all() and (got["payload_len"][~gen] == 0).all() and (got["payload_len"][gen] > 60).all()
    # no post-replay state: no task can be APPLIED
    none = store_checksums_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, None)
    assert_rows(none, c.want_without, "without them")
    assert not (none["outcome"] == O.APPLIED).any() and (none["outcome"] == O.NOT_RESUMED).sum() >= 6
    # tasks are independent: any order, any subset
    order = np.random.default_rng(1).permutation(c.tasks.shape[0])[:20]
    sub = store_checksums_host(c.sbs, c.tasks[order], c.last_events[order], c.results[order], c.routes[order], c.after, threads=3)
    assert sub.tobytes() == got[order].tobytes()


def test_backfilled_value_is_what_the_next_load_verifies():
    """The value generated for a backfill is the one the next Load verifies: a state written with the updated
    branch (the equal-version case, the last item's event ID moved from 19 to 20) has it as its verify value."""
    st = dict(sc.HAND_STATES[1])
    hs = list(st["histories"])
    hs[0] = (hs[0][0], [(5, 1), (20, 3)])
    after_state = persisted.build_blob_set([vc.state(**dict(st, histories=hs))[0]])
    want = load_states_verify_host(after_state)[0]
    c = sc.hand_case()
    k = [i for i in range(c.tasks.shape[0]) if c.tasks[i]["wf"] == 1 and c.routes[i]["route"] == abi.ROUTE_NON_CURRENT][0]
    last = c.last_events[k:k + 1].copy()
    last[0] = (20, 3)
    got = store_checksums_host(c.sbs, c.tasks[k:k + 1], last, c.results[k:k + 1], c.routes[k:k + 1])[0]
    assert (int(got["value"]), int(got["payload_len"]), int(got["outcome"])) == (int(want["computed"]), int(want["payload_len"]), int(O.BACKFILLED))


def test_task_case_with_the_expected_routes():
    c = sc.routed_case()
    got = store_checksums_host(c.sbs, c.tasks, c.last_events, c.results, c.routes)
    assert_rows(got, c.want)
    non_current = (c.routes["route"] == abi.ROUTE_NON_CURRENT) & (c.results["action"] == abi.NDC_APPEND)
    assert non_current.sum() >= 20 and (got["outcome"][non_current] == O.BACKFILLED).all()
    assert (got["outcome"] == O.BACKFILLED).sum() == non_current.sum()
    apply = c.routes["route"] == abi.ROUTE_APPLY_CURRENT
    assert apply.sum() >= 60 and (got["outcome"][apply] == O.NOT_RESUMED).all()
    # the three states that do not load and the two tasks past the batch
    past = c.tasks["wf"] >= c.sbs.n_wf
    assert past.sum() == 2 and (got["outcome"] == O.NOT_LOADED).sum() >= 5 and (got["outcome"][past] == O.NOT_LOADED).all()
    assert {int(O.NO_ROUTE), int(O.NEW_BRANCH)} <= set(int(x) for x in got["outcome"])
    assert store_checksums_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, threads=4).tobytes() == got.tobytes()


@functools.lru_cache(maxsize=None)
def _replayed_host():
    """The replayed case decided by the oracle's decisions and the restated routing of the values written, the
    after-image the oracle's replay of the whole histories: (case, results, routes, resumed mask, after, rows)."""
    rc = sc.replayed_case()
    res, routes = sc.decided(rc)
    resumed = persisted.apply_mask(routes, rc.tasks, rc.sbs.n_wf)
    after = rc.one_r.to_loaded(rc.one_b, mask=resumed)
    got = store_checksums_host(rc.sbs, rc.tasks, rc.last_events, res, routes, after)
    return rc, res, routes, resumed, after, got


def test_replayed_states_applied_and_backfilled():
    rc, res, routes, resumed, after, got = _replayed_host()
    want = sc.expected_replayed(rc, routes, res, resumed, after)
    assert_rows(got, want)
    wf = rc.tasks["wf"]
    applied, two = got["outcome"] == O.APPLIED, rc.two_branch[wf]
    assert (applied & two).sum() >= 15 and (applied & ~two).sum() >= 15 and (got["outcome"] == O.BACKFILLED).sum() >= 5
    # a single-branch state that is not sticky: the replay's own checksum
    single = applied & ~two
    assert (got["value"][single] == rc.one_r.exec["checksum"][wf[single]]).all()
    assert (got["payload_len"][single] == rc.one_r.exec["payload_len"][wf[single]]).all()
    # ... which is not the value to store for a two-branch state: the gap this interface closes
    assert (got["value"][applied & two] != rc.one_r.exec["checksum"][wf[applied & two]]).all()


def test_round_trip_generated_values_verify_as_stored():
    rc, _res, _routes, _resumed, _after, got = _replayed_host()
    applied = np.zeros(rc.sbs.n_wf, bool)
    stored = [None] * rc.sbs.n_wf
    for k in np.nonzero(got["outcome"] == O.APPLIED)[0]:
        w = int(rc.tasks[k]["wf"])
        applied[w] = True
        stored[w] = (abi.CHECKSUM_PAYLOAD_V1, abi.CHECKSUM_FLAVOR_CRC32, int(got["value"][k]).to_bytes(4, "big"))
    assert applied.sum() >= 30
    sbs = sc.reencoded_applied(rc, applied)
    v = load_states_verify_host(sbs, persisted.stored_checksums(stored))
    assert (v["outcome"][applied] == abi.VerifyOutcome.MATCH).all()


def test_header_pins_and_bad_arguments():
    from cadence_amd import decode, engine
    text = open(os.path.join(ROOT, "include", "cadence_load_store.h")).read()
    assert set(re.findall(r"\b(crr_load_\w+)\s*\(", text)) == {"crr_load_store_checksums", "crr_load_store_checksums_host"}
    dev = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(dev, "crr_load_store_checksums") and hasattr(decode.lib(), "crr_load_store_checksums_host")
    dev.crr_abi_version.restype = ctypes.c_int
    assert dev.crr_abi_version() == abi.ABI_VERSION == 8
    abi.check_layout(dev)
    assert dev.crr_sizeof(27) == abi.STORE_ROW.itemsize == 16 and dev.crr_sizeof(28) == abi.LAST_EVENT.itemsize == 16
    assert dev.crr_sizeof(29) == 0
    assert [int(x) for x in O] == list(range(8))
    for name in O.__members__:
        assert re.search(r"CRR_STORE_%s = %d\b" % (name, int(O[name])), text), name
    # invalid shapes: -1, as the sibling calls
    vp = ctypes.c_void_p
    dev.crr_load_store_checksums.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_uint32] + [vp] * 9
    S, P = abi.CLoadSummary(), abi.CLoadNdcSizes()
    assert dev.crr_load_store_checksums(None, None, 0, ctypes.byref(S), None, None, 0, None, None, None, ctypes.byref(P),
                                        None, None, None, None, None) == -1
    host = persisted._host_lib()
    c = sc.hand_case()
    cb = persisted._c_batch(c.sbs, lambda a: a.ctypes.data)
    out = np.zeros(c.tasks.shape[0], abi.STORE_ROW)
    args = [c.tasks.ctypes.data, c.last_events.ctypes.data, c.tasks.shape[0], c.results.ctypes.data, c.routes.ctypes.data, None,
            out.ctypes.data, 1]
    assert host.crr_load_store_checksums_host(None, *args) == -1
    for drop in (0, 1, 3, 4, 6):
        bad = list(args)
        bad[drop] = None
        assert host.crr_load_store_checksums_host(ctypes.byref(cb), *bad) == -1, drop
    assert host.crr_load_store_checksums_host(ctypes.byref(cb), None, None, 0, None, None, None, None, 1) == 0   # no tasks
    img = abi.CLoadImage()                                                    # an after-image without exec rows
    bad = list(args)
    bad[5] = ctypes.byref(img)
    assert host.crr_load_store_checksums_host(ctypes.byref(cb), *bad) == -1
    assert host.crr_load_store_checksums_host(ctypes.byref(cb), *args) == 0 and out.tobytes() == c.want_without.tobytes()


def test_empty_batch_and_no_tasks():
    empty = persisted.build_blob_set([])
    tasks = np.zeros(3, abi.REPL_TASK)
    tasks["wf"] = [0, 5, 0xFFFFFFFF]
    routes = np.zeros(3, abi.NDC_ROUTE)
    routes["route"] = abi.ROUTE_APPLY_CURRENT
    got = store_checksums_host(empty, tasks, np.zeros(3, abi.LAST_EVENT), np.zeros(3, abi.NDC_RESULT), routes)
    assert got.tolist() == [(0, int(O.NOT_LOADED), 0, 0)] * 3
    c = sc.hand_case()
    none = store_checksums_host(c.sbs, c.tasks[:0], c.last_events[:0], c.results[:0], c.routes[:0], c.after)
    assert none.shape == (0,)


def test_host_restatement_under_asan_and_ubsan(tmp_path):
    asan_tool.build_and_run(tmp_path, "load_store_asan")
