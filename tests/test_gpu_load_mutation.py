"""GPU: the pending-entry mutation of committed replication tasks (include/cadence_load_mutation.h): the count,
offsets, emit and gather kernels of load_kernel.hip.

The device's rows, offsets, gathered rows and keys equal the host restatement's byte for byte and equal the Python
expectation (mutation_cases.py): on hand-made decisions without a replay, and end to end -- upload, plan, decide and
route on the device, place, replay, plan and run the mutation -- with the interleaved layout (stride 64, a position map
that is not the identity), through the wave tail (stride 1), and on 1366 tasks (block sums of more than ten blocks,
generated tasks past task 1024).  The device's result applied to the persisted blobs loads and verifies as the
snapshot does; a failed replay's row or counts no table holds leave every lane within its descriptor and every buffer's
guard words as they were.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from cadence_amd import abi, persisted
from cadence_amd.flatten import LoadedStates, flatten, interleave
from cadence_amd.persisted import StateLoader, apply_mask, apply_mutation, mutation_host

import mutation_cases as mc
import store_cases as sc
from resume_cases import KNOWN

pytestmark = pytest.mark.gpu
O = abi.StoreOutcome
GUARD = 0x5A


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


@pytest.fixture(scope="module")
def loader(engine):
    return StateLoader(engine)


def _set_decisions(loader, results, routes):
    torch = loader.torch
    for name, rows in (("results", results), ("routes", routes)):
        raw = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy())
        loader.last_ndc[1][name][:raw.numel()].copy_(raw)


def test_hand_made_decisions_equal_the_host_restatement(loader):
    """No replay: every outcome a task can have without one (APPLIED and REPLAY_FAILED are reached end to end below)."""
    c = sc.hand_case()
    ds = loader.upload(c.sbs)
    loader.plan(ds)
    loader.ndc_prepare(ds, c.tasks, np.zeros(0, abi.VH_ITEM), on_device=True)   # the branch table; the decisions are replaced
    _set_decisions(loader, c.results, c.routes)
    rows, got = loader.mutation(ds, c.tasks, c.last_events)
    host = mutation_host(c.sbs, c.tasks, c.last_events, c.results, c.routes)
    assert got.image_bytes() == host.image_bytes() and rows.tobytes() == host.rows.tobytes()
    want, _ = mc.expected_mutation(c.tasks, c.want_without, persisted.load_states_host(c.sbs), None)
    mc.assert_mutation(got, want, "hand case")
    assert {int(O.BACKFILLED), int(O.NOT_LOADED), int(O.NO_ROUTE), int(O.NEW_BRANCH), int(O.VH_ERROR), int(O.NOT_RESUMED)} == \
        set(int(x) for x in rows["outcome"])
    assert got.exec.shape[0] == 0 and (rows["exec_index"] == abi.MUTATION_NO_EXEC).all()
    # outcome and status are the checksum rows'
    store = loader.store_checksums(ds, c.tasks, c.last_events)
    assert (rows["outcome"] == store["outcome"]).all() and (rows["status"] == store["status"]).all()
    # a prefix of the tasks
    assert loader.mutation(ds, c.tasks[:5], c.last_events[:5])[0].tobytes() == host.rows[:5].tobytes()
    with pytest.raises(ValueError):
        loader.mutation(ds, np.concatenate([c.tasks, c.tasks]), np.concatenate([c.last_events, c.last_events]))


@dataclasses.dataclass
class Run:
    r: mc.Replayed
    lay: object
    mask: np.ndarray
    after: LoadedStates           # the oracle's replay of the device's layout, canonical order
    want: persisted.Mutation
    host: persisted.Mutation
    got: persisted.Mutation
    store: np.ndarray
    vh: tuple
    pos: np.ndarray               # the device position of each task's workflow
    ds: object
    db: object
    plan: object


def _end_to_end(engine, loader, r: mc.Replayed, layout) -> Run:
    """upload -> plan -> decide and route on the device -> place -> replay -> the mutation, the checksums and the
    VersionHistories blobs of the same tasks."""
    from oracle import oracle
    rc = r.rc
    ds = loader.upload(rc.sbs)
    loader.plan(ds)
    verify0 = loader.verify(ds)
    loader.ndc_prepare(ds, rc.tasks, rc.incoming, on_device=True)
    n = rc.tasks.shape[0]
    routes = loader.last_ndc[1]["routes"][:n * abi.NDC_ROUTE.itemsize].cpu().numpy().view(abi.NDC_ROUTE).copy()
    results = loader.last_ndc[1]["results"][:n * abi.NDC_RESULT.itemsize].cpu().numpy().view(abi.NDC_RESULT).copy()
    assert results.tobytes() == r.results.tobytes() and (routes["route"] == r.routes["route"]).all()
    mask = apply_mask(routes, rc.tasks, rc.sbs.n_wf)
    assert (mask == r.mask).all()
    lay = layout(flatten(rc.suf, known_domains=KNOWN, loaded=loader.read().resumable(mask)))
    db = engine.upload(dataclasses.replace(lay, init=None), live_ids=True)
    loader.place(db, perm=lay.perm)
    engine.launch(db)
    plan = loader.mutation_plan(ds, rc.tasks, rc.last_events, db=db, perm=lay.perm)
    got = plan.download(loader.mutation_run(plan))
    store = loader.store_checksums(ds, rc.tasks, rc.last_events, db=db, perm=lay.perm)
    vh = loader.store_version_histories(ds, rc.tasks, rc.last_events, db=db, perm=lay.perm)
    after = oracle.replay(lay, 0).to_loaded(lay, mask=mask)
    want = mc.after_on(r, after)
    host = mutation_host(rc.sbs, rc.tasks, rc.last_events, results, routes, after)
    # the loader's scratch is as it was
    assert loader.verify(ds).tobytes() == verify0.tobytes()
    pos = np.zeros(rc.sbs.n_wf, np.int64)
    pos[lay.perm if lay.perm is not None else np.arange(lay.n_wf)] = np.arange(lay.n_wf)
    return Run(r, lay, mask, after, want, host, got, store, vh, pos[rc.tasks["wf"]], ds, db, plan)


def _check(run: Run, what: str):
    mc.assert_mutation(run.host, run.want, what + ": the host restatement against the expectation")
    mc.assert_mutation(run.got, run.want, what + ": the device against the expectation")
    assert run.got.image_bytes() == run.host.image_bytes()
    assert (run.got.rows["outcome"] == run.store["outcome"]).all() and (run.got.rows["status"] == run.store["status"]).all()
    P = run.plan.sizes
    assert int(P.n_exec) == run.want.exec.shape[0]
    assert [int(x) for x in P.n_upsert] == [run.want.upsert[m].shape[0] for m in mc.MAPS]
    assert [int(x) for x in P.n_delete] == [run.want.deleted[m].shape[0] for m in mc.MAPS]


@pytest.fixture(scope="module")
def interleaved(engine, loader):
    return _end_to_end(engine, loader, mc.replayed_small(), interleave)


def test_end_to_end_on_the_replayed_case(interleaved):
    run = interleaved
    lay, t = run.lay, run.r.tally
    assert lay.stride == 64 and lay.perm is not None and (lay.perm != np.arange(lay.n_wf)).any()
    assert (np.diff(run.r.rc.tasks["wf"].astype(np.int64)) < 0).any()       # the tasks are in shuffled order
    _check(run, "replayed case")
    # (the classification does not depend on the layout: the tally is the canonical replay's)
    assert len(t.applied_tasks) >= 30 and (run.got.rows["outcome"] == O.BACKFILLED).sum() >= 5
    assert t.new["act"] >= 40 and t.deleted["act"] >= 4 and t.changed["act"] >= 3 and t.untouched["act"] >= 15
    assert t.new["timer"] >= 15 and t.deleted["timer"] >= 2
    # no untouched row is reported
    for m in mc.MAPS:
        assert run.got.upsert[m].shape[0] == t.new[m] + t.changed[m] and run.got.deleted[m].shape[0] == t.deleted[m]


def test_capacity_exactly_the_totals_and_one_row_short(loader, interleaved):
    run = interleaved
    P, torch, dev = run.plan.sizes, loader.torch, loader.engine.dev
    item = {"exec": abi.EXEC_ROW.itemsize}
    total = {"exec": int(P.n_exec)}
    for t, m in enumerate(mc.MAPS):
        item["upsert." + m], total["upsert." + m] = mc.DTYPES[m].itemsize, int(P.n_upsert[t])
        item["deleted." + m], total["deleted." + m] = 8, int(P.n_delete[t])
    whole = {f: torch.full((total[f] * item[f] + 32,), GUARD, dtype=torch.uint8, device=dev) for f in item}
    out = {f: whole[f][16:16 + total[f] * item[f]] for f in item}
    for short in ("exec", "upsert.act", "deleted.timer"):
        assert total[short] > 0
        with pytest.raises(RuntimeError):
            loader.mutation_run(run.plan, out=out, capacity=dict(total, **{short: total[short] - 1}))
    torch.cuda.synchronize()
    assert all(bool((whole[f] == GUARD).all()) for f in whole)               # refused: nothing launched
    got = run.plan.download(loader.mutation_run(run.plan, out=out, capacity=total))
    assert got.image_bytes() == run.host.image_bytes()
    for f in whole:
        a = whole[f].cpu().numpy()
        assert (a[:16] == GUARD).all() and (a[-16:] == GUARD).all(), f


def test_end_to_end_through_the_wave_tail(engine, loader):
    run = _end_to_end(engine, loader, mc.replayed_tail(), interleave)
    lay, t = run.lay, run.r.tally
    assert lay.stride == 64 and 0 < lay.wave_begin < lay.n_wf
    _check(run, "long tail")
    assert t.restarted >= 15 and t.status_only >= 5 and t.changed["child"] >= 30
    assert t.deleted["rc"] >= 50 and t.deleted["sig"] >= 50
    applied = run.got.rows["outcome"] == O.APPLIED
    in_tail = run.pos >= lay.wave_begin
    assert (applied & in_tail).sum() >= 5 and (applied & ~in_tail).sum() >= 5
    # each restarted TimerID is an upsert with no delete
    restarts = 0
    for k in t.applied_tasks:
        w = int(run.r.rc.tasks[k]["wf"])
        old = {int(x["key"]): int(x["started_id"]) for x in sc.rows_of(run.r.before, w)["timer"]}
        for x in sc.rows_of(run.after, w)["timer"]:
            if int(x["key"]) in old and old[int(x["key"])] != int(x["started_id"]):
                restarts += 1
                assert int(x["key"]) in run.got.upserts(k, "timer")["key"] and int(x["key"]) not in run.got.deletes(k, "timer")
    assert restarts >= 15


@functools.lru_cache(maxsize=None)
def _large():
    return mc.replayed(sc.replayed_case_large())


def test_end_to_end_on_1366_tasks(engine, loader):
    """1400 states, 1366 tasks: eleven blocks of block sums, offsets that cross blocks, generated tasks past task 1024."""
    run = _end_to_end(engine, loader, _large(), interleave)
    assert run.r.rc.sbs.n_wf == 1400 and run.r.rc.tasks.shape[0] == 1366
    _check(run, "large case")
    rows = run.got.rows
    late = np.arange(rows.shape[0]) >= 1024
    assert ((rows["outcome"] == O.APPLIED) & late).sum() >= 50 and ((rows["outcome"] == O.BACKFILLED) & late).sum() >= 5
    assert (rows["map"]["n_upsert"][late].sum(axis=0)[:2] > 0).all() and rows["exec_index"][late & (rows["outcome"] == O.APPLIED)].min() > 500


def test_round_trip_device_mutation_loads_as_the_snapshot(loader, interleaved):
    run = interleaved
    rc, m = run.r.rc, run.got
    applied, stored, points = np.zeros(rc.sbs.n_wf, bool), [None] * rc.sbs.n_wf, {}
    for k in np.nonzero(m.rows["outcome"] == O.APPLIED)[0]:
        w = int(rc.tasks[k]["wf"])
        applied[w] = True
        stored[w] = (abi.CHECKSUM_PAYLOAD_V1, abi.CHECKSUM_FLAVOR_CRC32, int(run.store["value"][k]).to_bytes(4, "big"))
        points[w] = mc.reset_points_of(run.after, w)
    assert applied.sum() >= 30
    new = apply_mutation(rc.sbs, rc.tasks, m, run.vh, run.store, [run.after.interners[w] for w in range(rc.sbs.n_wf)],
                         reset_points=points)

    def load(sbs, st=None):
        ds = loader.upload(sbs)
        loader.plan(ds)
        return loader.read(), (loader.verify(ds, persisted.stored_checksums(st)) if st is not None else None)
    got, v = load(new, stored)
    assert (v["outcome"][applied] == abi.VerifyOutcome.MATCH).all()
    want, _ = load(sc.reencoded_applied(rc, applied))
    for w in np.nonzero(applied)[0]:
        assert mc.persisted_view(got, int(w)) == mc.persisted_view(want, int(w)), w


def test_failed_replays_and_garbage_counts_stay_within_the_descriptor(engine, loader):
    """An exec row with a status is REPLAY_FAILED with zero counts; counts no table holds are clamped to the
    descriptor's capacity -- the mutation is then the one of a state with exactly the capacity's slots live, which the
    host restatement gives for an image that holds those slots (the same inputs pass the stand-alone sanitizer program
    of tools/load_mutation_asan.cpp in test_load_mutation.py); the guard words around every output are intact and no
    other task's result changes."""
    run = _end_to_end(engine, loader, mc.replayed_small(), interleave)
    rc, lay, db, torch, dev = run.r.rc, run.lay, run.db, loader.torch, loader.engine.dev
    applied = np.nonzero(run.got.rows["outcome"] == O.APPLIED)[0]
    k_fail, k_wild = int(applied[0]), int(applied[-1])
    p_fail, p_wild = int(run.pos[k_fail]), int(run.pos[k_wild])
    w_wild = int(rc.tasks[k_wild]["wf"])
    assert (rc.tasks["wf"] == w_wild).sum() == 1
    raw = db.tensors["exec"]
    ex = raw.cpu().numpy().view(abi.EXEC_ROW).copy()
    ex[p_fail]["status"] = 7
    ex[p_wild]["n_activity"], ex[p_wild]["n_timer"], ex[p_wild]["n_child"] = 2**31 - 1, -5, 2**31 - 1
    ex[p_wild]["n_reset_points"] = 2**31 - 1
    raw.copy_(torch.from_numpy(ex.view(np.uint8).reshape(-1)))
    plan = loader.mutation_plan(run.ds, rc.tasks, rc.last_events, db=db, perm=lay.perm)
    P = plan.sizes
    item = {"exec": abi.EXEC_ROW.itemsize}
    total = {"exec": int(P.n_exec)}
    for t, m in enumerate(mc.MAPS):
        item["upsert." + m], total["upsert." + m] = mc.DTYPES[m].itemsize, int(P.n_upsert[t])
        item["deleted." + m], total["deleted." + m] = 8, int(P.n_delete[t])
    whole = {f: torch.full((total[f] * item[f] + 32,), GUARD, dtype=torch.uint8, device=dev) for f in item}
    got = plan.download(loader.mutation_run(plan, out={f: whole[f][16:16 + total[f] * item[f]] for f in item}, capacity=total))
    for f in whole:
        a = whole[f].cpu().numpy()
        assert (a[:16] == GUARD).all() and (a[-16:] == GUARD).all(), f
    assert (int(got.rows[k_fail]["outcome"]), int(got.rows[k_fail]["status"])) == (int(O.REPLAY_FAILED), 7)
    assert got.rows[k_fail]["exec_index"] == abi.MUTATION_NO_EXEC and not got.rows[k_fail]["map"]["n_upsert"].any() \
        and not got.rows[k_fail]["map"]["n_delete"].any()
    # the image the clamped counts stand for: the capacity's slots of the device tables for the wild workflow
    D = lay.wf[p_wild]
    st = 1 if p_wild >= lay.wave_begin else int(lay.stride)
    after = run.after
    ex2 = after.exec.copy()
    rows2 = {}
    for name, dt, base_f, cap_f, n_f in abi.TABLES[:7]:
        c = after.counts(name)
        o = int((np.cumsum(c) - c)[w_wild])
        mine = after.rows[name][o:o + int(c[w_wild])]
        if name in ("act", "child", "rp"):
            table = db.tensors["out_" + name].cpu().numpy().view(dt)
            mine = table[int(D[base_f]) + st * np.arange(int(D[cap_f]))].copy()
        elif name == "timer":
            mine = mine[:0]
        rows2[name] = np.concatenate([after.rows[name][:o], mine, after.rows[name][o + int(c[w_wild]):]])
        ex2[n_f][w_wild] = mine.shape[0]
    ex2["status"][int(rc.tasks[k_fail]["wf"])] = 7
    img, keep = persisted._after_image(LoadedStates(ex2, rows2, after.mask, None), rc.sbs.n_wf)
    wild = ex2.copy()                                                           # the exec rows with the counts as given
    for f in ("n_activity", "n_timer", "n_child", "n_reset_points"):
        wild[f][w_wild] = ex[p_wild][f]
    img.exec = wild.ctypes.data
    host = persisted._host_lib()
    cb = persisted._c_batch(rc.sbs, lambda a: a.ctypes.data)
    Q = abi.CMutationSizes()
    args = (ctypes.byref(cb), rc.tasks.ctypes.data, rc.last_events.ctypes.data, rc.tasks.shape[0], run.r.results.ctypes.data,
            run.r.routes.ctypes.data, ctypes.byref(img))
    assert host.crr_load_mutation_host(*args, None, None, ctypes.byref(Q), 1) == 0
    assert bytes(Q)[8:96] == bytes(P)[8:96]                                     # the same totals
    hrows = np.zeros(rc.tasks.shape[0], abi.MUTATION_ROW)
    hex_, hup, hde, o = persisted._mutation_buffers(Q)
    assert host.crr_load_mutation_host(*args, hrows.ctypes.data, ctypes.byref(o), ctypes.byref(Q), 1) == 0
    assert got.image_bytes() == persisted.Mutation(hrows, hex_, hup, hde).image_bytes()
    # values: no timer is live after, so every timer before is deleted and none upserted; the counts of the clamped
    # maps are bounded by the capacity
    W = got.rows[k_wild]
    n_timer_before = int(sc.rows_of(run.r.before, w_wild)["timer"].shape[0])
    assert int(W["outcome"]) == O.APPLIED and int(W["map"][1]["n_upsert"]) == 0 and int(W["map"][1]["n_delete"]) == n_timer_before
    assert int(W["map"][0]["n_upsert"]) <= int(D["act_cap"]) and int(W["map"][2]["n_upsert"]) <= int(D["child_cap"])
    assert got.exec_of(k_wild)["n_activity"] == 2**31 - 1
    # no other task's result changes
    for k in range(rc.tasks.shape[0]):
        if k in (k_fail, k_wild):
            continue
        assert got.rows[k]["outcome"] == run.got.rows[k]["outcome"] and got.rows[k]["flags"] == run.got.rows[k]["flags"]
        for m in mc.MAPS:
            assert got.upserts(k, m).tobytes() == run.got.upserts(k, m).tobytes() and got.deletes(k, m).tobytes() == run.got.deletes(k, m).tobytes()
        a, b = got.exec_of(k), run.got.exec_of(k)
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())


def test_empty_state_batch_and_no_tasks(loader):
    empty = persisted.build_blob_set([])
    ds = loader.upload(empty)
    loader.plan(ds)
    tasks = np.zeros(3, abi.REPL_TASK)
    tasks["wf"] = [0, 5, 0xFFFFFFFF]
    loader.ndc_prepare(ds, tasks, np.zeros(0, abi.VH_ITEM), on_device=True)
    rows, got = loader.mutation(ds, tasks, np.zeros(3, abi.LAST_EVENT))
    assert (rows["outcome"] == O.NOT_LOADED).all() and (rows["exec_index"] == abi.MUTATION_NO_EXEC).all()
    assert not rows["map"]["n_upsert"].any() and not rows["map"]["n_delete"].any() and got.exec.shape[0] == 0
    rows, got = loader.mutation(ds, tasks[:0], np.zeros(0, abi.LAST_EVENT))
    assert rows.shape == (0,) and got.n_bytes == 0
