"""GPU: the resumed replay of routed tasks planned on the device from loaded states (include/cadence_load_resume.h):
the bid, rows, count, offsets, index, gather, caps and descriptor kernels of load_kernel.hip.

The device's rows, gathered batch, seeds, descriptors, arena and totals equal the host restatement's byte for byte
(load_resume_cases.host_resume: crr_load_resume_host around the host decoder's counts) on 62 and on 1366 tasks --
block sums of eleven blocks, applied tasks and workflows past index 1024 -- into buffers of exactly the planned sizes
between guard bytes.  End to end -- upload, plan, route on the device, ``StateLoader.resume``, launch -- the rows of every
applied workflow equal the existing path's (host ``flatten`` of the same suffixes, upload, place, launch) and the
oracle's, and the store calls on that batch equal their host restatements.  Long and colliding seeded keys, a blob the
decoder rejects, and a seeded dictionary that outgrows the ingest scratch's table region.
"""
import dataclasses

import numpy as np
import pytest

from cadence_amd import abi, blobs, persisted
from cadence_amd.flatten import flatten
from cadence_amd.persisted import StateLoader
from cadence_amd.replication import _compare_rows
from cadence_amd.result import ReplayResult

import exec_blob_cases as xc
import load_resume_cases as lrc
import mutation_cases as mc
import store_cases as sc
from resume_cases import KNOWN

pytestmark = pytest.mark.gpu
O = abi.StoreOutcome
R = abi.ResumeOutcome
GUARD = 0x5A


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


@dataclasses.dataclass
class Run:
    p: lrc.Planned
    ds: object
    db: object
    plan: object
    img: persisted.ResumeImage
    routes: np.ndarray
    results: np.ndarray


def _routed(loader, p: lrc.Planned):
    rc = p.rc
    ds = loader.upload(rc.sbs)
    loader.plan(ds)
    loader.ndc_prepare(ds, rc.tasks, rc.incoming, on_device=True)
    n = rc.tasks.shape[0]
    routes = loader.last_ndc[1]["routes"][:n * abi.NDC_ROUTE.itemsize].cpu().numpy().view(abi.NDC_ROUTE).copy()
    results = loader.last_ndc[1]["results"][:n * abi.NDC_RESULT.itemsize].cpu().numpy().view(abi.NDC_RESULT).copy()
    assert (routes["route"] == p.routes["route"]).all()
    return ds, routes, results


def _resume(loader, ingest, p: lrc.Planned, **kw) -> Run:
    """upload -> plan -> decide and route on the device -> ``StateLoader.resume`` (nothing launched yet)."""
    ds, routes, results = _routed(loader, p)
    db = loader.resume(ds, p.rc.tasks, ingest.upload(p.tbs), ingest, **kw)
    plan = loader.last_resume
    return Run(p, ds, db, plan, plan.download(), routes, results)


def _assert_equal_images(got: persisted.ResumeImage, want: persisted.ResumeImage, what: str, laid_out: bool = True):
    """Byte for byte; ``laid_out``: ``got`` was read after ``StateLoader.resume``, whose layout wrote each descriptor's
    ``ev_begin`` (the restatement leaves it 0) -- every other field, the flags settled after the layout included, is
    compared as it is."""
    if laid_out:
        got = dataclasses.replace(got, desc=got.desc.copy())
        assert (got.desc["ev_begin"][got.desc["ev_count"] == 0] >= 0).all()
        got.desc["ev_begin"] = 0
    a, b = got.image_bytes(), want.image_bytes()
    assert a.keys() == b.keys()
    for f in a:
        assert a[f] == b[f], f"{what}: {f} differs"


@pytest.fixture(scope="module")
def small(loader, ingest):
    return _resume(loader, ingest, lrc.planned_small())


def test_device_equals_the_restatement_on_the_replayed_case(small):
    run, p = small, small.p
    host = lrc.host_resume(p.rc.sbs, p.rc.tasks, run.routes, p.tbs)
    _assert_equal_images(run.img, host, "replayed case")
    assert lrc.compare_with_flatten(p, run.img) == 51
    assert int(run.img.sizes.n_bytes) % 16 != 0          # the tail lane's byte-wise stores


def test_device_equals_the_restatement_on_1366_tasks(loader, ingest):
    """1400 states, 1366 tasks: eleven blocks of block sums, offsets that cross blocks, applied tasks and workflows past
    index 1024."""
    p = lrc.planned_large()
    run = _resume(loader, ingest, p)
    assert p.rc.sbs.n_wf == 1400 and p.rc.tasks.shape[0] == 1366 and int(run.img.sizes.n_applied) == 1138
    host = lrc.host_resume(p.rc.sbs, p.rc.tasks, run.routes, p.tbs)
    _assert_equal_images(run.img, host, "large case")
    assert lrc.compare_with_flatten(p, run.img) == 1138
    late = np.arange(1366) >= 1024
    assert ((run.img.rows["outcome"] == R.APPLIED) & late).sum() >= 50 and (run.img.task_of[1024:] >= 1024).sum() >= 10
    assert int(run.img.desc["act_base"][1399]) > 2000 and int(run.img.key_begin[1399]) > 5000


def test_duplicate_tasks_failed_loads_and_indices_out_of_range(loader, ingest):
    """The bids on the device: 1366 tasks and 300 copies of them in front and behind (the lowest index wins a workflow
    across blocks, the others are shadowed), tasks routed to the current branch that name a state whose load failed or
    an index past the batch; rows, gathered batch and descriptors equal the restatement's."""
    p = lrc.planned_large()
    rc = p.rc
    n0 = rc.tasks.shape[0]
    front, back = np.arange(0, n0, 9)[:150], np.arange(4, n0, 7)[:150]
    src = np.concatenate([front, np.arange(n0), back])
    tasks = rc.tasks[src].copy()
    q = dataclasses.replace(p, rc=dataclasses.replace(rc, tasks=tasks), routes=p.routes[src], results=p.results[src])
    ds, routes, _results = _routed(loader, q)                 # the copies are routed as their originals
    failed = np.nonzero(~p.loaded.mask)[0]
    apply = np.nonzero(routes["route"] == abi.ROUTE_APPLY_CURRENT)[0]
    moved = apply[-6:]
    tasks["wf"][moved] = [failed[0], failed[-1], rc.sbs.n_wf, rc.sbs.n_wf + 77, 0xFFFFFFFF, failed[1]]
    tbs = lrc.task_blob_set([rc.suf[int(rc.tasks[k]["wf"])] for k in src])
    db = loader.resume(ds, tasks, ingest.upload(tbs), ingest)
    img = loader.last_resume.download()
    host = lrc.host_resume(rc.sbs, tasks, routes, tbs)
    _assert_equal_images(img, host, "duplicates")
    out = img.rows["outcome"]
    assert (out == R.SHADOWED).sum() >= 200 and (out[moved] == R.NOT_LOADED).all() and (out == R.NOT_ROUTED).sum() >= 100
    for k in np.nonzero(out == R.SHADOWED)[0]:
        assert 0 <= img.task_of[img.rows["position"][k]] < k
    won = img.task_of[img.task_of >= 0]
    assert (won < 150).sum() >= 100 and (won >= 150).sum() >= 900 and (out[won] == R.APPLIED).all()
    # only the positions with a task resume, after the layout too
    flags = db.tensors["desc"][:rc.sbs.n_wf * abi.WORKFLOW.itemsize].cpu().numpy().view(abi.WORKFLOW)["flags"]
    assert (((flags & abi.WF_FLAG_RESUME) != 0) == (img.task_of >= 0)).all() and (img.task_of < 0).sum() >= 200


def test_work_buffer_too_small(loader, ingest):
    import ctypes
    p = lrc.planned_small()
    ds, _routes, _results = _routed(loader, p)
    dtb = ingest.upload(p.tbs)
    plan = loader.resume_plan(ds, p.rc.tasks, dtb)
    T, vp, P = plan.tensors, ctypes.c_void_p, abi.CLoadResumeSizes()
    rows0 = T["rows"].clone()
    rc = loader.lib.crr_load_resume_plan(ctypes.byref(ds.c), vp(loader.scratch.data_ptr()), ctypes.c_size_t(loader.scratch_bytes),
                                         ctypes.byref(loader.summary), vp(T["tasks"].data_ptr()), vp(T["routes"].data_ptr()), plan.n,
                                         ctypes.byref(dtb.c), vp(T["rows"].data_ptr()), vp(T["work"].data_ptr()),
                                         ctypes.c_size_t(T["work_bytes"] - 16), ctypes.byref(P), loader._stream())
    assert rc == 0 and P.err == abi.SCRATCH_TOO_SMALL and int(P.work_needed) == T["work_bytes"] == int(plan.sizes.work_needed)
    assert int(P.n_applied) == 0 and bool((T["rows"] == rows0).all())       # nothing launched


def test_exact_size_buffers_between_guards(loader, ingest):
    """Every output of the gather and the arena of the finalize sized exactly (the byte total is no multiple of 16),
    guard bytes on both sides intact; a capacity one short is refused and nothing is launched."""
    p = lrc.planned_small()
    torch, dev = loader.torch, loader.engine.dev
    ds, routes, _results = _routed(loader, p)
    plan = loader.resume_plan(ds, p.rc.tasks, ingest.upload(p.tbs))
    P = plan.sizes
    size = loader.resume_out_sizes(P)
    assert size["bytes"] % 16 != 0 and min(size.values()) > 0
    # (the gathered bytes are followed by CRR_INGEST_PAD readable bytes, which the gather does not write: guards too)
    whole = {f: torch.full((nb + 32 + (abi.INGEST_PAD if f == "bytes" else 0),), GUARD, dtype=torch.uint8, device=dev)
             for f, nb in size.items()}
    out = {f: whole[f][16:] for f in size}
    for short in ("bytes", "blobs", "keys"):
        total = {"bytes": int(P.n_bytes), "blobs": int(P.n_blobs), "keys": int(P.n_keys)}
        with pytest.raises(RuntimeError):
            loader.resume_gather(plan, out=out, capacity={short: total[short] - 1})
    torch.cuda.synchronize()
    assert all(bool((whole[f] == GUARD).all()) for f in whole)               # refused: nothing launched
    loader.resume_gather(plan, out=out)
    gdb, resume = loader.resume_blobs(plan)
    ingest.plan(gdb, resume=resume)
    arena = torch.full((int(P.token_bytes) + 32,), GUARD, dtype=torch.uint8, device=dev)
    loader.resume_finalize(plan, gdb, ingest, arena=arena[16:])
    torch.cuda.synchronize()
    for f, nb in size.items():
        a = whole[f].cpu().numpy()
        assert (a[:16] == GUARD).all() and (a[16 + nb:] == GUARD).all(), f
    a = arena.cpu().numpy()
    assert (a[:16] == GUARD).all() and (a[16 + int(P.token_bytes):] == GUARD).all()
    host = lrc.host_resume(p.rc.sbs, p.rc.tasks, routes, p.tbs)
    _assert_equal_images(plan.download(out), host, "exact-size buffers", laid_out=False)


def _relaid(run: Run, lay, res: ReplayResult, applied: np.ndarray) -> ReplayResult:
    """The device batch's result in ``lay``'s slot tables: an applied workflow's capacities are equal in both layouts
    (test_load_resume.py), its bases differ where a workflow without a task has capacities of its own in ``lay``."""
    from cadence_amd.result import allocate_host
    out = allocate_host(lay)
    out.exec[:] = res.exec
    d = run.img.desc
    for name, _dt, base_f, cap_f, _n in abi.TABLES[:7]:
        for w in np.nonzero(applied)[0]:
            cap = int(d[cap_f][w])
            assert cap == int(lay.wf[cap_f][w])
            out.tables[name][int(lay.wf[base_f][w]):int(lay.wf[base_f][w]) + cap] = res.tables[name][int(d[base_f][w]):int(d[base_f][w]) + cap]
    return out


@pytest.fixture(scope="module")
def replayed(engine, ingest):
    """The small case resumed and launched through a loader of its own (the tests below read its scratch again), and
    the two references: the existing path on the device and the oracle."""
    from oracle import oracle
    own = StateLoader(engine)
    p = lrc.planned_small()
    run = _resume(own, ingest, p)
    engine.launch(run.db)
    res = engine.download(run.db)
    applied = p.mask & p.loaded.mask
    lay = flatten(p.rc.suf, known_domains=KNOWN, loaded=own.read().resumable(p.mask))
    db2 = engine.upload(dataclasses.replace(lay, init=None), live_ids=True)
    own.place(db2)
    engine.launch(db2)
    existing = engine.download(db2)
    ref = oracle.replay(lay, 0)
    return own, run, lay, _relaid(run, lay, res, applied), existing, ref, applied


def test_end_to_end_rows_equal_the_existing_path_and_the_oracle(replayed):
    _own, run, lay, got, existing, ref, applied = replayed
    assert int(applied.sum()) == 51
    assert _compare_rows(lay, got, existing, applied) == 0
    assert _compare_rows(lay, got, ref, applied) == 0
    assert (got.exec["status"][applied] == 0).sum() >= 30 and int(got.exec["n_activity"][applied].sum()) > 50


def test_store_calls_on_the_resumed_batch_equal_their_restatements(loader, replayed):
    own, run, lay, _got, _existing, ref, applied = replayed
    p, rc, db, ds = run.p, run.p.rc, run.db, run.ds
    after = ref.to_loaded(lay, mask=p.mask)
    args = (rc.sbs, rc.tasks, rc.last_events, run.results, run.routes)
    store = own.store_checksums(ds, rc.tasks, rc.last_events, db=db)
    assert store.tobytes() == persisted.store_checksums_host(*args, after).tobytes()
    assert int((store["outcome"] == O.APPLIED).sum()) >= 30
    vh = own.store_version_histories(ds, rc.tasks, rc.last_events, db=db)
    hvh = persisted.store_version_histories_host(*args, after)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(vh, hvh))
    rows, m = own.mutation(ds, rc.tasks, rc.last_events, db=db)
    hm = persisted.mutation_host(*args, after)
    assert m.image_bytes() == hm.image_bytes() and rows.tobytes() == hm.rows.tobytes()
    xt = xc.exec_tasks_of(rc.tasks.shape[0])
    got, _vh = own.store_executions(ds, rc.tasks, rc.last_events, xt, db=db, task_blobs=db.tensors["gathered"])
    hs = list(rc.suf)
    upserts = np.array([any(e.event_type == abi.EventType.UpsertWorkflowSearchAttributes for e in xc.events_of(h)) for h in hs], np.uint8)
    host = persisted.store_executions_host(*args, xt, after, xc.task_blob_set(hs), upserts)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, host))
    assert int((got[0]["len"] > 0).sum()) >= 20
    # the mutation applied to the persisted blobs loads and verifies as the snapshot does
    done, stored, points = np.zeros(rc.sbs.n_wf, bool), [None] * rc.sbs.n_wf, {}
    for k in np.nonzero(m.rows["outcome"] == O.APPLIED)[0]:
        w = int(rc.tasks[k]["wf"])
        done[w] = True
        stored[w] = (abi.CHECKSUM_PAYLOAD_V1, abi.CHECKSUM_FLAVOR_CRC32, int(store["value"][k]).to_bytes(4, "big"))
        points[w] = mc.reset_points_of(after, w)
    assert done.sum() >= 30
    new = persisted.apply_mutation(rc.sbs, rc.tasks, m, vh, store, [after.interners[w] for w in range(rc.sbs.n_wf)], reset_points=points)
    ds2 = loader.upload(new)
    loader.plan(ds2)
    got_img, v = loader.read(), loader.verify(ds2, persisted.stored_checksums(stored))
    assert (v["outcome"][done] == abi.VerifyOutcome.MATCH).all()
    ds3 = loader.upload(sc.reencoded_applied(rc, done))
    loader.plan(ds3)
    want_img = loader.read()
    for w in np.nonzero(done)[0]:
        assert mc.persisted_view(got_img, int(w)) == mc.persisted_view(want_img, int(w)), w


def test_long_and_colliding_seeded_keys(engine, loader, ingest):
    """States holding up to 196 keyed entries of 15 to 300 bytes, pairs of them colliding under the ingest hash; the
    tasks fire, cancel and cancel-request them by ID: each such event's key is the loader's id, a new string gets the
    next one, and the replayed rows equal the oracle's."""
    from oracle import oracle
    p = lrc.planned_keys()
    tally = lrc.key_tally(p)                              # counted on the CPU
    assert tally["long"] >= 200 and tally["colliding"] >= 50 and tally["new"] >= 10 and tally["largest_dictionary"] > 64
    run = _resume(loader, ingest, p)
    host = lrc.host_resume(p.rc.sbs, p.rc.tasks, run.routes, p.tbs)
    _assert_equal_images(run.img, host, "key case")
    applied = p.mask & p.loaded.mask
    assert lrc.compare_with_flatten(p, run.img) == int(applied.sum()) == 6
    engine.launch(run.db)
    res = engine.download(run.db)
    b = ingest.to_host_batch(run.db)                       # the event columns the layout wrote
    import full_event_cases as fe
    n_long = n_new = 0
    for w in np.nonzero(applied)[0]:
        d = p.loaded.keys(int(w))
        begin, n = int(b.wf["ev_begin"][w]), int(b.wf["ev_count"][w])
        events = p.rc.suf[int(w)].events
        assert n == len(events)
        new = {}
        for j, e in enumerate(events):
            name = fe._KEY_ATTR.get(int(e.event_type))
            s = e.get(name, "") if name else ""
            if not s:
                continue
            want = d.index(s) + 1 if s in d else new.setdefault(s, len(d) + 1 + len(new))
            assert int(b.cols["key"][begin + j]) == want, (w, j, s)
            n_long += s in d and len(s.encode()) >= 15
            n_new += s not in d
        assert (b.cols["key"][begin:begin + n] == p.want.cols["key"][int(p.want.wf["ev_begin"][w]):][:n]).all()
    assert n_long == tally["long"] and n_new == tally["new"]
    got = _relaid(run, p.want, res, applied)
    assert _compare_rows(p.want, got, oracle.replay(p.want, 0), applied) == 0
    assert (got.exec["status"][applied] == 0).all()


def test_a_blob_that_is_not_thriftrw_names_its_task(loader, ingest):
    from cadence_amd.ingest import IngestError
    p = lrc.planned_small()
    ds, _routes, _results = _routed(loader, p)
    applied_tasks = np.nonzero(p.routes["route"] == abi.ROUTE_APPLY_CURRENT)[0]
    k = int(applied_tasks[len(applied_tasks) // 2])
    bad = p.tbs.bytes.copy()
    bad[int(p.tbs.blob_off[int(p.tbs.wf[k]["blob_begin"])])] ^= 0xFF          # the preamble byte
    tb = ingest.upload(blobs.BlobSet(bytes=bad, blob_off=p.tbs.blob_off, wf=p.tbs.wf, strings=p.tbs.strings))
    with pytest.raises(IngestError) as e:
        loader.resume(ds, p.rc.tasks, tb, ingest)
    assert e.value.task == k and "task %d" % k in str(e.value)
    plan = loader.last_resume
    assert plan.totals is None and "exec" not in plan.tensors               # neither finalized nor placed nor laid out
    # a rejection a transcode of the task batch recorded is raised, not dropped with the blob's index
    pend = ingest.upload(p.tbs)
    pend.pending = (e.value.code, 3)
    with pytest.raises(IngestError) as e2:
        loader.resume(ds, p.rc.tasks, pend, ingest)
    assert (e2.value.code, e2.value.blob) == (e.value.code, 3)
    # a blob of a task that is not applied is never decoded
    k2 = int(np.nonzero(p.routes["route"] != abi.ROUTE_APPLY_CURRENT)[0][0])
    bad = p.tbs.bytes.copy()
    bad[int(p.tbs.blob_off[int(p.tbs.wf[k2]["blob_begin"])])] ^= 0xFF
    loader.resume(ds, p.rc.tasks, ingest.upload(blobs.BlobSet(bytes=bad, blob_off=p.tbs.blob_off, wf=p.tbs.wf, strings=p.tbs.strings)), ingest)


def test_seeded_dictionary_larger_than_the_table_region_grows_the_scratch_once(engine, loader):
    """The ingest scratch first sized for the task's events alone: the seeds do not fit its table region
    (CRR_INGEST_SCRATCH_TOO_SMALL), the plan grows it once, and the rows still equal the oracle's."""
    from cadence_amd.ingest import DeviceIngest
    from oracle import oracle
    p = lrc.planned_keys()
    host = lrc.host_resume(p.rc.sbs, p.rc.tasks, p.routes, p.tbs)
    n_ev, n_keys = int(host.desc["ev_count"].astype(np.int64).sum()), int(host.sizes.n_keys)
    assert n_ev + 2 < n_keys < 3 * n_ev                                      # too small once, large enough doubled
    fresh = DeviceIngest(engine)
    run = _resume(loader, fresh, p, max_events=n_ev + 1)
    assert fresh.replans == 1
    _assert_equal_images(run.img, host, "grown scratch")
    engine.launch(run.db)
    applied = p.mask & p.loaded.mask
    got = _relaid(run, p.want, engine.download(run.db), applied)
    assert _compare_rows(p.want, got, oracle.replay(p.want, 0), applied) == 0


def test_no_states_and_no_tasks(loader, ingest):
    empty = persisted.build_blob_set([])
    ds = loader.upload(empty)
    loader.plan(ds)
    tasks = np.zeros(3, abi.REPL_TASK)
    tasks["wf"] = [0, 5, 0xFFFFFFFF]
    loader.ndc_prepare(ds, tasks, np.zeros(0, abi.VH_ITEM), on_device=True)
    plan = loader.resume_plan(ds, tasks, ingest.upload(lrc.task_blob_set([lrc.hand_history(k) for k in range(3)])))
    assert int(plan.sizes.n_applied) == 0 and int(plan.sizes.n_bytes) == 0
    assert (plan.rows()["outcome"] != R.APPLIED).all() and (plan.rows()["position"] == 0xFFFFFFFF).all()
    c = sc.hand_case()
    ds = loader.upload(c.sbs)
    loader.plan(ds)
    loader.ndc_prepare(ds, c.tasks, np.zeros(0, abi.VH_ITEM), on_device=True)
    plan = loader.resume_plan(ds, c.tasks[:0], ingest.upload(lrc.task_blob_set([])))
    out = loader.resume_gather(plan)
    img = plan.download(out)
    assert int(plan.sizes.n_applied) == 0 and (img.task_of == -1).all() and img.blob_off.tolist() == [0]
