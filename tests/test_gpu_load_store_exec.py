"""GPU: the execution blob of committed replication tasks (include/cadence_load_store_exec.h): the size, offsets and
emit kernels of load_kernel.hip.

The device's rows, offsets and bytes equal the host restatement's and the Python expectation's (exec_blob_cases.py):
on the hand states, whose post-task exec rows are written into the replay's outputs by hand, and end to end -- upload,
plan, decide and route on the device, place, replay, VersionHistories blobs, execution blobs -- with the interleaved
layout, with and without the tasks' event blobs, and on 1366 tasks (more than one block of each kernel, more than 1024
scanned elements, 16-byte lanes that straddle two blobs, runs of zero-length tasks).  The task blobs are the suffix
batches' thriftrw bytes in device-position order, the batch a resume ingest of the same tasks takes; the replay's own
inputs are the host-flattened ones the other store tests use.
"""
import dataclasses
import functools

import numpy as np
import pytest

from cadence_amd import abi, persisted
from cadence_amd.flatten import flatten, interleave
from cadence_amd.history import WorkflowHistory
from cadence_amd.persisted import StateLoader, apply_mask, store_executions_host

import exec_blob_cases as xc
import mutation_cases as mc
import store_cases as sc
from resume_cases import KNOWN

pytestmark = pytest.mark.gpu
O = abi.StoreOutcome
F = xc.HOST_FLAGS
CANARY = 0xC3


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


@pytest.fixture(scope="module")
def loader(engine):
    return StateLoader(engine)


@pytest.fixture(scope="module")
def ingest(engine):
    from cadence_amd.ingest import DeviceIngest
    return DeviceIngest(engine)


def _position_blobs(ingest, histories, lay):
    """The tasks' event blobs resident in HBM, workflow p of the batch device position p."""
    perm = lay.perm if lay.perm is not None else np.arange(lay.n_wf)
    return ingest.upload(xc.task_blob_set([histories[int(w)] for w in perm]))


def _set_decisions(loader, results, routes):
    torch = loader.torch
    for name, rows in (("results", results), ("routes", routes)):
        raw = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy())
        loader.last_ndc[1][name][:raw.numel()].copy_(raw)


@pytest.fixture(scope="module")
def hand(engine, loader, ingest):
    """The hand case on the device: the loaded rows placed into a resumed batch's outputs, the post-task exec rows (and
    the one changed reset point) written over them instead of a replay."""
    c = xc.hand_case()
    torch, n_wf = loader.torch, c.sbs.n_wf
    marker = WorkflowHistory(batches=[[xc._ev(20, xc.ET.MarkerRecorded)]])
    hs = [h if h is not None else marker for h in c.task_histories]
    ds = loader.upload(c.sbs)
    loader.plan(ds)
    lay = flatten(hs, known_domains=KNOWN, loaded=loader.read().resumable(np.ones(n_wf, bool)))
    assert lay.perm is None and lay.stride == 1
    db = engine.upload(dataclasses.replace(lay, init=None), live_ids=True)
    loader.place(db, perm=lay.perm)
    raw = db.tensors["exec"]
    ex = raw.cpu().numpy().view(abi.EXEC_ROW).copy()
    placed = ex[:n_wf].copy()
    ex[:n_wf] = c.after.exec
    for f in ("start_src", "src_next"):                       # (the device loader's own, equal to the host loader's)
        assert (placed[f] == c.after.exec[f]).all()
    raw.copy_(torch.from_numpy(ex.view(np.uint8).reshape(-1)))
    w = int(c.tasks[c.names["reset_points"]]["wf"])
    rp = db.tensors["out_rp"].cpu().numpy().view(abi.RESET_POINT_ROW).copy()
    rp[int(lay.wf["rp_base"][w])]["flags"] ^= abi.ROW_RESETTABLE
    db.tensors["out_rp"].copy_(torch.from_numpy(rp.view(np.uint8).reshape(-1)))
    loader.ndc_prepare(ds, c.tasks, np.zeros(0, abi.VH_ITEM), on_device=True)   # the branch table; the decisions are replaced
    _set_decisions(loader, c.results, c.routes)
    return c, ds, db, lay, _position_blobs(ingest, c.task_histories, lay)


def test_hand_states_equal_the_host_and_the_expectation(loader, hand):
    c, ds, db, lay, tb = hand
    got, vh = loader.store_executions(ds, c.tasks, c.last_events, c.exec_tasks, db=db, perm=lay.perm, task_blobs=tb)
    xc.assert_result(got, c.want, "hand states on the device")
    host = store_executions_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.exec_tasks, c.after,
                                 xc.task_blob_set(c.task_histories), c.upserts)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, host))
    store = loader.store_checksums(ds, c.tasks, c.last_events, db=db, perm=lay.perm)
    assert (got[0]["outcome"] == store["outcome"]).all() and (got[0]["status"] == store["status"]).all()
    assert (got[0]["outcome"] == vh[0]["outcome"]).all()
    # without the task blobs: the one task whose request id is its own goes to the host
    got2, _ = loader.store_executions(ds, c.tasks, c.last_events, c.exec_tasks, db=db, perm=lay.perm)
    xc.assert_result(got2, c.want_without_blobs, "hand states, no task blobs")
    # without a replay: the backfills alone
    got3, _ = loader.store_executions(ds, c.tasks, c.last_events, c.exec_tasks)
    cur = c.routes["route"] == abi.ROUTE_APPLY_CURRENT
    assert (got3[0]["outcome"][cur] == O.NOT_RESUMED).all() and (got3[0]["len"][cur] == 0).all()
    k = c.names["backfill"]
    assert got3[2][int(got3[1][k]):int(got3[1][k + 1])].tobytes() == c.want.blobs[k]


def test_hand_states_with_populated_task_blobs(loader, ingest, hand):
    """The task blobs with every schema field present and the DecisionTaskStarted event more than 13 KB into the
    task's bytes (full_event_cases.populated_task_blobs): the device reads the same request id, so rows, offsets and
    bytes equal the hand expectation and the host restatement on the same blobs."""
    import full_event_cases as fe
    c, ds, db, lay, _tb = hand
    perm = lay.perm if lay.perm is not None else np.arange(lay.n_wf)
    pop = fe.populated_task_blobs(xc.task_blob_set([c.task_histories[int(w)] for w in perm]))
    assert pop.n_bytes > 3 * 13 * 1024
    got, _vh = loader.store_executions(ds, c.tasks, c.last_events, c.exec_tasks, db=db, perm=lay.perm,
                                       task_blobs=ingest.upload(pop))
    xc.assert_result(got, c.want, "hand states on the device, populated task blobs")
    host = store_executions_host(c.sbs, c.tasks, c.last_events, c.results, c.routes, c.exec_tasks, c.after,
                                 fe.populated_task_blobs(xc.task_blob_set(c.task_histories)), c.upserts)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, host))


def test_capacity_one_byte_short_and_canaries(loader, hand):
    c, ds, db, lay, tb = hand
    torch, dev = loader.torch, loader.engine.dev
    vh_plan = loader.store_version_histories_plan(ds, c.tasks, c.last_events, db=db, perm=lay.perm)
    vh_out = loader.store_version_histories_run(vh_plan)
    plan = loader.store_executions_plan(vh_plan, c.exec_tasks, task_blobs=tb)
    n = int(plan.sizes.n_bytes)
    assert n == len(c.want.data) and n % 16 != 0
    assert int(plan.sizes.n_blobs) == int((c.want.rows["len"] > 0).sum()) and int(plan.sizes.n_host) == 5
    assert int(plan.sizes.run_work_needed) <= int(plan.sizes.work_needed) == plan.work_bytes
    whole = torch.full((n + 128,), CANARY, dtype=torch.uint8, device=dev)
    out = whole[64:64 + n]
    with pytest.raises(RuntimeError):
        loader.store_executions_run(plan, vh_out, out=out, capacity=n - 1)
    torch.cuda.synchronize()
    assert bool((whole == CANARY).all())                      # refused: nothing launched
    loader.store_executions_run(plan, vh_out, out=out, capacity=n)
    a = whole.cpu().numpy()
    assert (a[:64] == CANARY).all() and (a[64 + n:] == CANARY).all() and a[64:64 + n].tobytes() == c.want.data
    # too small a work buffer: reported, nothing launched
    from cadence_amd.abi import CExecBlobSizes
    import ctypes
    P = CExecBlobSizes()
    T = plan.tensors
    rows0 = T["rows"].clone()
    rc = loader.lib.crr_load_store_exec_plan(*vh_plan.head, plan.n, *vh_plan.tail, *plan.mid, ctypes.c_void_p(T["rows"].data_ptr()),
                                             ctypes.c_void_p(T["blob_off"].data_ptr()), ctypes.c_void_p(T["work"].data_ptr()),
                                             ctypes.c_size_t(plan.work_bytes - 16), ctypes.byref(P), loader._stream())
    torch.cuda.synchronize()
    assert rc == 0 and P.err == abi.SCRATCH_TOO_SMALL and int(P.work_needed) == plan.work_bytes and bool((T["rows"] == rows0).all())
    # a VersionHistories row that disagrees with its task (another length than its offsets give): the plan returns -1
    vh_rows = vh_plan.tensors["rows"]
    keep = vh_rows.clone()
    v = keep.cpu().numpy().view(abi.VH_BLOB_ROW).copy()
    v[c.names["backfill"]]["len"] += 1
    vh_rows.copy_(torch.from_numpy(v.view(np.uint8).reshape(-1)))
    with pytest.raises(RuntimeError, match="-1"):
        loader.store_executions_plan(vh_plan, c.exec_tasks, task_blobs=tb)
    vh_rows.copy_(keep)
    again = loader.store_executions_plan(vh_plan, c.exec_tasks, task_blobs=tb)
    assert int(again.sizes.n_bytes) == n


@dataclasses.dataclass
class Run:
    x: xc.ReplayedExec
    lay: object
    want: xc.Expected
    want_without: xc.Expected
    host: tuple
    got: tuple
    got_without: tuple
    vh: tuple


def _end_to_end(engine, loader, ingest, x: xc.ReplayedExec, layout) -> Run:
    """upload -> plan -> decide and route on the device -> place -> replay -> the VersionHistories blobs and the
    execution blobs of the same tasks, with and without the tasks' event blobs."""
    from oracle import oracle
    r, rc = x.r, x.r.rc
    ds = loader.upload(rc.sbs)
    loader.plan(ds)
    loader.ndc_prepare(ds, rc.tasks, rc.incoming, on_device=True)
    n = rc.tasks.shape[0]
    routes = loader.last_ndc[1]["routes"][:n * abi.NDC_ROUTE.itemsize].cpu().numpy().view(abi.NDC_ROUTE).copy()
    results = loader.last_ndc[1]["results"][:n * abi.NDC_RESULT.itemsize].cpu().numpy().view(abi.NDC_RESULT).copy()
    mask = apply_mask(routes, rc.tasks, rc.sbs.n_wf)
    assert (mask == r.mask).all()
    lay = layout(flatten(rc.suf, known_domains=KNOWN, loaded=loader.read().resumable(mask)))
    db = engine.upload(dataclasses.replace(lay, init=None), live_ids=True)
    loader.place(db, perm=lay.perm)
    engine.launch(db)
    tb = _position_blobs(ingest, x.task_histories, lay)
    got, vh = loader.store_executions(ds, rc.tasks, rc.last_events, x.exec_tasks, db=db, perm=lay.perm, task_blobs=tb)
    got_without, _ = loader.store_executions(ds, rc.tasks, rc.last_events, x.exec_tasks, db=db, perm=lay.perm)
    after = oracle.replay(lay, 0).to_loaded(lay, mask=mask)
    store_rows = sc.expected_replayed(rc, routes, results, mask, after)
    host = store_executions_host(rc.sbs, rc.tasks, rc.last_events, results, routes, x.exec_tasks, after, x.task_blobs, x.upserts)
    return Run(x, lay, xc.replayed_expected(r, after, store_rows, x.exec_tasks, True),
               xc.replayed_expected(r, after, store_rows, x.exec_tasks, False), host, got, got_without, vh)


def _check(run: Run, what: str):
    xc.assert_result(run.host, run.want, what + ": the host restatement against the expectation")
    xc.assert_result(run.got, run.want, what + ": the device against the expectation")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(run.got, run.host))
    xc.assert_result(run.got_without, run.want_without, what + ": the device without the task blobs")
    assert (run.got[0]["outcome"] == run.vh[0]["outcome"]).all()


def test_case_a_end_to_end(engine, loader, ingest):
    run = _end_to_end(engine, loader, ingest, xc.case_a(), interleave)
    assert run.lay.stride == 64 and run.lay.perm is not None and (run.lay.perm != np.arange(run.lay.n_wf)).any()
    _check(run, "case A")
    t, t0 = xc.tally(run.x, run.want), xc.tally(run.x, run.want_without)
    assert t["device"] >= 200 and t["from_task"] >= 8 and t["device_backfills"] == 42
    # the second run: those tasks become HOST_REQUEST_ID and every other blob is unchanged
    assert t0["rq"] == t["from_task"] and t0["device"] == t["device"] - t["from_task"]
    rows, off, data = run.got
    rows0, off0, data0 = run.got_without
    for k in range(rows.shape[0]):
        if run.want.from_task[k] and rows[k]["len"]:
            assert rows0[k]["flags"] == F["rq"] and rows0[k]["len"] == 0
        else:
            assert data[int(off[k]):int(off[k + 1])].tobytes() == data0[int(off0[k]):int(off0[k + 1])].tobytes()


def test_case_b_flags_and_bytes(engine, loader, ingest):
    run = _end_to_end(engine, loader, ingest, xc.case_b(), interleave)
    _check(run, "case B")
    t = xc.tally(run.x, run.want)
    assert t["rp"] >= 100 and t["sa"] >= 3 and t["device"] >= 80


@functools.lru_cache(maxsize=None)
def _large():
    return xc.replayed_exec(mc.replayed(sc.replayed_case_large()))


def test_end_to_end_on_1366_tasks(engine, loader, ingest):
    run = _end_to_end(engine, loader, ingest, _large(), interleave)
    rows, off, data = run.got
    assert rows.shape[0] == 1366
    _check(run, "large case")
    late = np.arange(rows.shape[0]) >= 1024
    assert ((rows["len"] > 0) & late).sum() >= 50 and ((rows["len"] == 0) & late).sum() >= 5
    lens = rows["len"][rows["len"] > 0]
    assert (lens % 16 != 0).any() and len(set(int(o) % 16 for o in off[:-1][rows["len"] > 0])) >= 8   # lanes straddle blobs
    zero = rows["len"] == 0
    assert (zero[1:] & zero[:-1]).any()                        # runs of zero-length tasks
    assert int(off[-1]) > 1024 * 16                            # more than one block of the emit kernel


def test_empty_state_batch_and_no_tasks(loader):
    empty = persisted.build_blob_set([])
    ds = loader.upload(empty)
    loader.plan(ds)
    tasks = np.zeros(3, abi.REPL_TASK)
    tasks["wf"] = [0, 5, 0xFFFFFFFF]
    loader.ndc_prepare(ds, tasks, np.zeros(0, abi.VH_ITEM), on_device=True)
    (rows, off, data), _ = loader.store_executions(ds, tasks, np.zeros(3, abi.LAST_EVENT), np.zeros(3, abi.EXEC_BLOB_TASK))
    assert (rows["outcome"] == O.NOT_LOADED).all() and not rows["len"].any() and not off.any() and data.shape[0] == 0
    (rows, off, data), _ = loader.store_executions(ds, tasks[:0], np.zeros(0, abi.LAST_EVENT), np.zeros(0, abi.EXEC_BLOB_TASK))
    assert rows.shape == (0,) and off.tolist() == [0] and data.shape[0] == 0
