"""GPU: the VersionHistories blob to store for routed replication tasks (include/cadence_load_store_vh.h):
load_store_vh_size_kernel, the scan, and the output-stationary load_store_vh_emit_kernel.

The device's rows, offsets and bytes equal the host restatement's byte for byte on hand-built states with hand-made
decisions, on ndc_load_cases.task_case (about 400 shuffled tasks over three wavefronts, the not-generated ones in the
middle), on short blobs of many lengths (every start residue mod 16, chunks that hold one blob's tail and the next
one's head, runs of zero-length tasks) and on one state of 230 items behind a 300-byte token (a blob that spans
several wavefronts' chunks).  End to end -- upload, plan, decide and route on the device, place, replay, generate --
the blobs equal the bytes expected from the values written and the oracle's rows (vh_blob_cases.py), with the
interleaved layout and through the wave tail, and every row repeats the outcome and status of the checksum row of
the same call sequence; stored back as field 122 with the device's checksum, the states load to the expected branch
table and verify; the inputs are only read; guard bytes on both sides of the output stay intact, also when an exec
row holds a count no table holds.
"""
import dataclasses

import numpy as np
import pytest

from cadence_amd import abi, persisted
from cadence_amd.flatten import flatten, interleave
from cadence_amd.persisted import StateLoader, apply_mask, store_version_histories_host

import load_cases as lc
import ndc_load_cases as nc
import store_cases as sc
import vh_blob_cases as vb
from resume_cases import KNOWN

pytestmark = pytest.mark.gpu
O = abi.StoreOutcome
GUARD = 64


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


@pytest.fixture(scope="module")
def loader(engine):
    return StateLoader(engine)


def _same(got, want, what=""):
    for name, g, w in zip(("rows", "blob_off", "bytes"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.shape} vs {w.shape}"
        bad = np.nonzero(g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))[0]
        assert bad.size == 0, f"{what} {name}: {bad.size} bytes differ, first at {bad[:5]}"


def _hand_decided(loader, sbs, tasks, results, routes):
    """The states planned, the branch table built, and the decisions replaced by the hand-made ones."""
    ds = loader.upload(sbs)
    loader.plan(ds)
    loader.ndc_prepare(ds, tasks, np.zeros(0, abi.VH_ITEM), on_device=True)
    torch = loader.torch
    for name, rows in (("results", results), ("routes", routes)):
        raw = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy())
        loader.last_ndc[1][name][:raw.numel()].copy_(raw)
    return ds


def _guarded_run(loader, plan):
    """The run into exactly the padded size between two guard patterns: (bytes [n_bytes], the padded tail, guards intact)."""
    torch = loader.torch
    n_bytes = int(plan.sizes.n_bytes)
    padded = (n_bytes + 15) // 16 * 16
    buf = torch.full((GUARD + padded + GUARD,), 0xA5, dtype=torch.uint8, device=loader.engine.dev)
    loader.store_version_histories_run(plan, out=buf[GUARD:GUARD + max(padded, 1)], capacity=padded)
    host = buf.cpu().numpy()
    intact = bool((host[:GUARD] == 0xA5).all() and (host[GUARD + padded:] == 0xA5).all())
    return host[GUARD:GUARD + n_bytes].copy(), host[GUARD + n_bytes:GUARD + padded].copy(), intact, buf


def _read(plan):
    n = plan.n
    return (plan.tensors["rows"][:n * abi.VH_BLOB_ROW.itemsize].cpu().numpy().view(abi.VH_BLOB_ROW).copy(),
            plan.tensors["blob_off"].cpu().numpy().view(np.uint64).copy())


def test_hand_made_decisions_equal_the_host_restatement(loader):
    c = sc.hand_case()
    ds = _hand_decided(loader, c.sbs, c.tasks, c.results, c.routes)
    got = loader.store_version_histories(ds, c.tasks, c.last_events)
    host = store_version_histories_host(c.sbs, c.tasks, c.last_events, c.results, c.routes)
    _same(got, host, "hand case")
    vb.assert_blobs(*got, vb.hand_expected(c, c.want_without), "hand case")
    assert (got[0]["outcome"] == c.want_without["outcome"]).all() and (got[0]["status"] == c.want_without["status"]).all()
    sums = loader.store_checksums(ds, c.tasks, c.last_events)
    assert (got[0]["outcome"] == sums["outcome"]).all() and (got[0]["status"] == sums["status"]).all()
    # a prefix of the tasks gives the prefix of the result; none launches nothing; more than were decided is refused
    r5, o5, d5 = loader.store_version_histories(ds, c.tasks[:5], c.last_events[:5])
    assert r5.tobytes() == host[0][:5].tobytes() and o5.tobytes() == host[1][:6].tobytes()
    assert d5.tobytes() == host[2][:int(host[1][5])].tobytes()
    r0, o0, d0 = loader.store_version_histories(ds, c.tasks[:0], c.last_events[:0])
    assert r0.shape == (0,) and o0.tolist() == [0] and d0.shape == (0,)
    with pytest.raises(ValueError):
        loader.store_version_histories(ds, np.concatenate([c.tasks, c.tasks]), np.concatenate([c.last_events, c.last_events]))
    with pytest.raises(RuntimeError):
        StateLoader(loader.engine).store_version_histories(ds, c.tasks, c.last_events)


def test_task_case_equals_the_host_restatement_and_reads_only(loader):
    c = sc.routed_case()
    ds = loader.upload(c.sbs)
    loader.plan(ds)
    verify0 = loader.verify(ds)
    results, routes, _out = loader.ndc_prepare(ds, c.tasks, nc.task_case().incoming)
    table0 = loader.last_ndc[0].read().image_bytes()
    image0 = loader.read().image_bytes()
    plan = loader.store_version_histories_plan(ds, c.tasks, c.last_events)
    data, tail, intact, _buf = _guarded_run(loader, plan)
    rows, off = _read(plan)
    host = store_version_histories_host(c.sbs, c.tasks, c.last_events, results, routes)
    _same((rows, off, data), host, "task_case")
    assert intact and (tail == 0).all()
    vb.assert_blobs(rows, off, data, vb.routed_expected(c), "task_case")
    assert int(plan.sizes.n_generated) == int((rows["len"] > 0).sum()) >= 20 and (rows["outcome"] == O.NOT_RESUMED).sum() >= 60
    gen = np.nonzero(rows["len"] > 0)[0]
    assert (np.diff(gen) >= 4).any()        # not-generated tasks in the middle: runs of three and more
    # a capacity one byte short launches nothing
    padded = (int(plan.sizes.n_bytes) + 15) // 16 * 16
    buf = loader.torch.full((padded,), 0xA5, dtype=loader.torch.uint8, device=loader.engine.dev)
    with pytest.raises(RuntimeError):
        loader.store_version_histories_run(plan, out=buf, capacity=padded - 1)
    assert bool((buf == 0xA5).all())
    # the loader's scratch and the branch table are only read
    assert loader.verify(ds).tobytes() == verify0.tobytes()
    assert loader.last_ndc[0].read().image_bytes() == table0 and loader.read().image_bytes() == image0


@pytest.mark.parametrize("n_states,n_tasks", nc.LARGE_CASES)
def test_task_case_past_one_element_per_scan_thread(loader, n_states, n_tasks):
    """More than 1024 tasks (ndc_load_cases.LARGE_CASES): the scans that turn the tasks' lengths into blob offsets and
    their marks into the generated count give each thread several elements, a clipped last chunk and idle threads
    behind it.  Rows, offsets and bytes equal the host restatement's and the expected blobs; blob_off is the
    exclusive prefix of len; n_generated counts the generated tasks; the guard bytes stay intact.

    (1300, 2500): 160 blobs, 57,869 bytes, 91 of them behind task 1024.  (1025, 1025): 71 blobs, 26,166 bytes."""
    c = sc.routed_case(n_states, n_tasks)
    assert c.sbs.n_wf == n_states > 1024 and c.tasks.shape[0] == n_tasks > 1024
    ds = loader.upload(c.sbs)
    loader.plan(ds)
    results, routes, _out = loader.ndc_prepare(ds, c.tasks, nc.task_case(n_states, n_tasks).incoming)
    plan = loader.store_version_histories_plan(ds, c.tasks, c.last_events)
    data, tail, intact, _buf = _guarded_run(loader, plan)
    rows, off = _read(plan)
    host = store_version_histories_host(c.sbs, c.tasks, c.last_events, results, routes)
    _same((rows, off, data), host, "task_case")
    assert intact and (tail == 0).all()
    vb.assert_blobs(rows, off, data, vb.routed_expected(c, n_states, n_tasks), "task_case")
    assert (off == np.concatenate([[0], np.cumsum(rows["len"].astype(np.uint64))]).astype(np.uint64)).all()
    generated = rows["len"] > 0
    assert int(plan.sizes.n_generated) == int(generated.sum()) >= 50 and int(plan.sizes.n_bytes) == int(off[-1]) > 20_000
    assert (generated == np.isin(c.want["outcome"], vb.GENERATED)).all() and generated[n_tasks // 2:].sum() >= 10


@pytest.mark.parametrize("name", ["seams", "large"])
def test_seams_and_one_large_state(loader, name):
    (sbs, tasks, last, results, routes), want = vb.seam_case() if name == "seams" else vb.large_case()
    host = store_version_histories_host(sbs, tasks, last, results, routes)
    vb.assert_blobs(*host, want, name)
    if name == "seams":
        vb.assert_seams(host[0], host[1])
    else:       # ~5.7 KB: more than five wavefronts' chunks, an item seam at every offset of a chunk
        k = int(np.argmax(host[0]["len"]))
        assert int(host[0][k]["len"]) > 5 * 64 * 16
        items_at = int(host[1][k]) + 16 + 15 + 300
        assert set((items_at + 23 * j) % 16 for j in range(230)) == set(range(16))
    ds = _hand_decided(loader, sbs, tasks, results, routes)
    plan = loader.store_version_histories_plan(ds, tasks, last)
    data, tail, intact, _buf = _guarded_run(loader, plan)
    _same(_read(plan) + (data,), host, name)
    assert intact and (tail == 0).all()


def _end_to_end(engine, loader, rc: sc.ReplayedCase, layout):
    """upload -> plan -> decide and route on the device -> place -> replay -> generate (test_gpu_load_store's
    sequence): (plan, checksum rows, expected rows, expected blobs, layout, device position per task, states, batch)."""
    from oracle import oracle
    ds = loader.upload(rc.sbs)
    loader.plan(ds)
    loader.ndc_prepare(ds, rc.tasks, rc.incoming, on_device=True)
    n = rc.tasks.shape[0]
    out = loader.last_ndc[1]
    results = out["results"][:n * abi.NDC_RESULT.itemsize].cpu().numpy().view(abi.NDC_RESULT).copy()
    routes = out["routes"][:n * abi.NDC_ROUTE.itemsize].cpu().numpy().view(abi.NDC_ROUTE).copy()
    mask = apply_mask(routes, rc.tasks, rc.sbs.n_wf)
    lay = layout(flatten(rc.suf, known_domains=KNOWN, loaded=loader.read().resumable(mask)))
    db = engine.upload(dataclasses.replace(lay, init=None), live_ids=True)
    loader.place(db, perm=lay.perm)
    engine.launch(db)
    sums = loader.store_checksums(ds, rc.tasks, rc.last_events, db=db)
    plan = loader.store_version_histories_plan(ds, rc.tasks, rc.last_events, db=db)
    after = oracle.replay(lay, 0).to_loaded(lay, mask=mask)
    want = sc.expected_replayed(rc, routes, results, mask, after)
    pos = np.zeros(rc.sbs.n_wf, np.int64)
    pos[lay.perm if lay.perm is not None else np.arange(lay.n_wf)] = np.arange(lay.n_wf)
    return plan, sums, want, vb.replayed_expected(rc, want, after), lay, pos[rc.tasks["wf"]], ds, db, after


def _check_end_to_end(loader, rc, plan, sums, want, blobs, what):
    data, tail, intact, _buf = _guarded_run(loader, plan)
    rows, off = _read(plan)
    assert intact and (tail == 0).all()
    for f in ("outcome", "status"):
        assert (rows[f] == sums[f]).all() and (rows[f] == want[f]).all(), f
    vb.assert_blobs(rows, off, data, blobs, what)
    return rows, off, data


@pytest.fixture(scope="module")
def interleaved(engine, loader):
    rc = sc.replayed_case()
    return (rc,) + _end_to_end(engine, loader, rc, interleave)


def test_end_to_end_on_the_replayed_case(loader, interleaved):
    rc, plan, sums, want, blobs, lay, *_ = interleaved
    assert lay.stride == 64 and lay.perm is not None and (lay.perm != np.arange(lay.n_wf)).any()
    rows, _off, _data = _check_end_to_end(loader, rc, plan, sums, want, blobs, "replayed case")
    applied, two = rows["outcome"] == O.APPLIED, rc.two_branch[rc.tasks["wf"]]
    assert (applied & two).sum() >= 15 and (applied & ~two).sum() >= 15 and (rows["outcome"] == O.BACKFILLED).sum() >= 5


def test_round_trip_device_blobs_load_and_verify(loader, interleaved):
    """The states after their task as the store would hold them, field 122 replaced by the device's blob and the
    device's checksum stored: uploaded and planned again they verify, and their branch table is the expected one."""
    rc, plan, sums, _want, _blobs, _lay, _pos, _ds, _db, after = interleaved
    rows, off = _read(plan)
    data = _guarded_run(loader, plan)[0]
    blobs = vb.blobs_of(rows, off, data)
    applied, by_wf = np.zeros(rc.sbs.n_wf, bool), {}
    for k in np.nonzero(rows["outcome"] == O.APPLIED)[0]:
        applied[int(rc.tasks[k]["wf"])] = True
        by_wf[int(rc.tasks[k]["wf"])] = int(k)
    assert applied.sum() >= 30
    stored_states = nc.workflows_of(sc.reencoded_applied(rc, applied))
    wfs, stored, table = [], [], []
    for w in np.nonzero(applied)[0]:
        k = by_wf[int(w)]
        wfs.append(vb.with_vh_blob(stored_states[int(w)], blobs[k]))
        stored.append(vb.stored_of(sums[k]["value"]))
        table.append(nc.expected_of(*sc.histories_of(rc, int(w), vb._vh_rows(after, int(w)))))
    new = persisted.build_blob_set(wfs)
    ds = loader.upload(new)
    loader.plan(ds)
    v = loader.verify(ds, persisted.stored_checksums(stored))
    assert (v["outcome"] == abi.VerifyOutcome.MATCH).all()
    assert nc.table_of(new, loader.branches(ds).read()) == table


def test_end_to_end_through_the_wave_tail(engine, loader):
    hs = lc.prefix_case(150, 62, long_tail=True)[0]
    rc = sc.replayed_case_of(hs, 63, 3, shuffle_seed=6, last_only=False)
    plan, sums, want, blobs, lay, pos, *_ = _end_to_end(engine, loader, rc, interleave)
    assert lay.stride == 64 and 0 < lay.wave_begin < lay.n_wf
    rows, _off, _data = _check_end_to_end(loader, rc, plan, sums, want, blobs, "long tail")
    applied, two = rows["outcome"] == O.APPLIED, rc.two_branch[rc.tasks["wf"]]
    in_tail = pos >= lay.wave_begin
    assert (applied & in_tail).sum() >= 5 and (applied & ~in_tail).sum() >= 5 and (applied & two & in_tail).any()
    assert (applied & two).sum() >= 5 and (applied & ~two).sum() >= 5 and (rows["outcome"] == O.BACKFILLED).sum() >= 3


def test_end_to_end_past_1024_states_and_tasks(engine, loader):
    """store_cases.replayed_case_large through upload, plan, decide and route, place, replay and generate: 1400 states
    and 1366 tasks (683 two-branch states), 1138 APPLIED and 228 BACKFILLED, 293 and 49 of them at task index 1024
    or above -- behind the first element of every scan thread.  The checksum rows and the blobs equal the values
    expected from the values written and the oracle's rows."""
    rc = sc.replayed_case_large()
    assert rc.sbs.n_wf > 1024 and rc.tasks.shape[0] > 1024
    plan, sums, want, blobs, lay, _pos, *_ = _end_to_end(engine, loader, rc, interleave)
    assert lay.stride == 64 and lay.n_wf > 1024
    rows, _off, _data = _check_end_to_end(loader, rc, plan, sums, want, blobs, "1400 states")
    for f in abi.STORE_ROW.names:
        bad = np.nonzero(sums[f] != want[f])[0]
        assert bad.size == 0, f"checksum rows, {f}: {bad.size} tasks differ, first {bad[:5]}"
    assert int(plan.sizes.n_generated) == int((rows["len"] > 0).sum()) == rows.shape[0]
    past = rows["outcome"][1024:]
    assert (past == O.APPLIED).sum() >= 100 and (past == O.BACKFILLED).sum() >= 20
    applied, two = rows["outcome"] == O.APPLIED, rc.two_branch[rc.tasks["wf"]]
    assert (applied & two)[1024:].sum() >= 20 and (applied & ~two)[1024:].sum() >= 20


def test_garbage_counts_stay_within_the_descriptor_and_the_lanes_own_bytes(engine, loader):
    """An exec row whose n_vh_items no table holds (2^31 - 1) is clamped to the descriptor's capacity: the task's
    blob grows by 23 bytes per item of the capacity's room, every other task's row and bytes are as before, and the
    guard bytes around the output stay intact."""
    rc = sc.replayed_case()
    plan, _sums, _want, _blobs, lay, pos, ds, db, _after = _end_to_end(engine, loader, rc, interleave)
    rows, off = _read(plan)
    data = _guarded_run(loader, plan)[0]
    before_blobs = vb.blobs_of(rows, off, data)
    raw = db.tensors["exec"]
    ex = raw.cpu().numpy().view(abi.EXEC_ROW).copy()
    # the last applied task whose descriptor has room beyond the items the replay left
    roomy = [int(k) for k in np.nonzero(rows["outcome"] == O.APPLIED)[0]
             if int(lay.wf[int(pos[k])]["vh_cap"]) > int(ex[int(pos[k])]["n_vh_items"])]
    assert roomy
    k_wild = roomy[-1]
    p_wild = int(pos[k_wild])
    n_before = int(ex[p_wild]["n_vh_items"])
    ex[p_wild]["n_vh_items"] = 2**31 - 1
    raw.copy_(loader.torch.from_numpy(ex.view(np.uint8).reshape(-1)))
    again = loader.store_version_histories_plan(ds, rc.tasks, rc.last_events, db=db)
    data2, tail2, intact, _buf = _guarded_run(loader, again)
    rows2, off2 = _read(again)
    vb.assert_layout(rows2, off2, data2)
    grown = 23 * (int(lay.wf[p_wild]["vh_cap"]) - n_before)
    assert grown > 0 and int(rows2[k_wild]["len"]) == int(rows[k_wild]["len"]) + grown and int(rows2[k_wild]["outcome"]) == O.APPLIED
    rest = np.ones(rows.shape[0], bool)
    rest[k_wild] = False
    assert rows2[rest].tobytes() == rows[rest].tobytes()
    after_blobs = vb.blobs_of(rows2, off2, data2)
    assert all(after_blobs[k] == before_blobs[k] for k in np.nonzero(rest)[0])
    # the grown blob: the same bytes up to the items' count, which is now the capacity
    assert after_blobs[k_wild][:16] == before_blobs[k_wild][:16] and len(after_blobs[k_wild]) == int(rows2[k_wild]["len"])
    assert intact and (tail2 == 0).all()


def test_empty_state_batch(loader):
    empty = persisted.build_blob_set([])
    ds = loader.upload(empty)
    loader.plan(ds)
    tasks = np.zeros(3, abi.REPL_TASK)
    tasks["wf"] = [0, 5, 0xFFFFFFFF]
    loader.ndc_prepare(ds, tasks, np.zeros(0, abi.VH_ITEM), on_device=True)
    rows, off, data = loader.store_version_histories(ds, tasks, np.zeros(3, abi.LAST_EVENT))
    assert rows.tolist() == [(0, int(O.NOT_LOADED), 0, 0)] * 3 and off.tolist() == [0, 0, 0, 0] and data.shape == (0,)
    rows, off, data = loader.store_version_histories(ds, tasks[:0], np.zeros(0, abi.LAST_EVENT))
    assert rows.shape == (0,) and off.tolist() == [0] and data.shape == (0,)
