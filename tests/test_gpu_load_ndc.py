"""GPU: branch decisions and routing for replication tasks against persisted states, from the persisted bytes
(include/cadence_load_ndc.h).

The device branch table equals the host restatement's byte for byte; every crr_ndc_result field and every
new-branch item run equals oracle.ndc_prepare on ndc.pack of NdcTasks built from the values written into the blobs
(ndc_load_cases.task_case: 130 states over three wavefronts, the not-loaded ones in the middle of one, a 600-item
branch and a 70-branch state past ndc_prepare_kernel's LDS stage, about 400 shuffled tasks); routes equal the
Python restatement of prepareMutableState; the tasks routed APPLY_CURRENT resume to the oracle's rows; and the
loader's scratch is left as it was.

The reference's rebuild case (conflict_resolver_test.go:189-260) calls prepareMutableState with branch index 1
directly.  Through prepareVersionHistory the same state cannot give index 1 (test_load_ndc_cases.
test_known_answer_rebuild says why): the task forks a new branch holding branch 1's items, so the device answer
checked here is a rebuild from (event 1, version 12) on the new branch, index 2.
"""
import dataclasses

import numpy as np
import pytest

from cadence_amd import abi, persisted, synth_mixed
from cadence_amd.flatten import flatten, interleave
from cadence_amd.persisted import StateLoader, apply_mask, encode_states, load_branches_host, load_states_host
from cadence_amd.result import diff_results

import ndc_load_cases as nc
from resume_cases import KNOWN, split_histories

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


@pytest.fixture(scope="module")
def loader(engine):
    return StateLoader(engine)


@pytest.fixture(scope="module")
def decided(loader):
    """task_case planned, decided and routed on the device once: (case, device states, branch table read back,
    results, routes, out_items, out_begin)."""
    case = nc.task_case()
    ds = loader.upload(case.sbs)
    loader.plan(ds)
    results, routes, out_items = loader.ndc_prepare(ds, case.tasks, case.incoming)
    return case, ds, loader.last_ndc[0].read(), results, routes, out_items, loader.last_out_begin.copy()


def _same_table(dev: persisted.Branches, host: persisted.Branches, what=""):
    d, h = dev.image_bytes(), host.image_bytes()
    for k in h:
        assert d[k] == h[k], f"{what}: {k} differs"


def test_device_branch_table_equals_host(loader, decided):
    case, ds, table, *_ = decided
    host = load_branches_host(case.sbs)
    _same_table(table, host, "with tasks")
    assert host.branches.shape[0] > 300 and int(host.branches["item_count"].max()) == 600
    # the table alone (no tasks), and the replayed states with random branch sets
    _same_table(loader.branches(ds).read(), host, "alone")
    sbs, want = nc.replayed_branch_states()
    ds2 = loader.upload(sbs)
    loader.plan(ds2)
    dev = loader.branches(ds2).read()
    _same_table(dev, load_branches_host(sbs), "replayed")
    assert nc.table_of(sbs, dev) == want


def _check_results(case, results, out_items, out_begin):
    want, _want_routes, want_items = nc.expected_routes(case)
    assert results.dtype == abi.NDC_RESULT and results.shape == want.shape
    for f in abi.NDC_RESULT.names:
        bad = np.nonzero(results[f] != want[f])[0]
        assert bad.size == 0, f"{f}: {bad.size} tasks differ, first {bad[:3]}: {results[f][bad[:3]]} vs {want[f][bad[:3]]}"
    # out_begin: the exclusive prefix over the tasks of the longest local branch of each task's workflow
    room = np.array([max(len(b) for b in t.local) if t is not None else 0 for t in case.ndc_tasks], np.int64)
    assert (out_begin == np.cumsum(room) - room).all() and out_items.shape[0] == int(room.sum())
    for k in range(len(case.tasks)):
        n = int(results[k]["new_item_count"])
        got = [(int(x["event_id"]), int(x["version"])) for x in out_items[int(out_begin[k]):int(out_begin[k]) + n]]
        assert got == want_items[k], k
    # not-loaded and out-of-range tasks: the new status, !doContinue, zeros
    nd = np.array([t is None for t in case.ndc_tasks])
    assert nd.sum() >= 5 and (case.tasks["wf"][nd] >= case.sbs.n_wf).sum() == 2
    zero = np.zeros(1, abi.NDC_RESULT)
    zero["status"], zero["action"] = abi.Status.NDC_STATE_NOT_LOADED, abi.NDC_DUPLICATE
    assert all(results[k].tobytes() == zero.tobytes() for k in np.nonzero(nd)[0])


def test_results_equal_the_oracle_on_the_values_written(decided):
    case, _ds, _table, results, _routes, out_items, out_begin = decided
    _check_results(case, results, out_items, out_begin)


def _check_routes(case, routes):
    _want, want, _items = nc.expected_routes(case)
    assert routes.dtype == abi.NDC_ROUTE
    for f in abi.NDC_ROUTE.names:
        bad = np.nonzero(routes[f] != want[f])[0]
        assert bad.size == 0, f"{f}: {bad.size} tasks differ, first {bad[:3]}: {routes[f][bad[:3]]} vs {want[f][bad[:3]]}"
    assert set(int(r) for r in routes["route"]) == set(range(5))
    assert tuple(routes[case.known["no_rebuild"]]) == (abi.ROUTE_APPLY_CURRENT, 0, 0, 0, 0, 0)
    assert tuple(routes[case.known["rebuild"]]) == (abi.ROUTE_REBUILD, 0, 2, 0, 1, 12)


def test_routes_equal_the_restatement_and_the_known_answers(decided):
    case, _ds, _table, _results, routes, _out, _ob = decided
    _check_routes(case, routes)


@pytest.mark.parametrize("n_states,n_tasks", nc.LARGE_CASES)
def test_more_than_one_element_per_scan_thread(loader, n_states, n_tasks):
    """The branch table, the decisions, the routes and the new-branch room with more than 1024 states and tasks:
    the loader's one-block scans then give each thread a chunk of several elements, a clipped last chunk and idle
    threads behind it, and the second row of the states' scan starts at n_wf + 1 (ndc_load_cases.LARGE_CASES).

    (1300, 2500): 3392 branches (the longest 600 items), 11 tasks not decided, routes NONE / APPLY_CURRENT /
    NON_CURRENT / REBUILD / BAD_REQUEST 1346 / 521 / 233 / 388 / 12, 12323 items of new-branch room.
    (1025, 1025): 2699 branches, 7 tasks not decided, routes 570 / 199 / 89 / 165 / 2, 4779 items of room."""
    case = nc.task_case(n_states, n_tasks)
    assert case.sbs.n_wf == n_states > 1024 and case.tasks.shape[0] == n_tasks > 1024
    ds = loader.upload(case.sbs)
    loader.plan(ds)
    results, routes, out_items = loader.ndc_prepare(ds, case.tasks, case.incoming)
    table, out_begin = loader.last_ndc[0].read(), loader.last_out_begin.copy()
    host = load_branches_host(case.sbs)
    _same_table(table, host, "with tasks")
    assert host.branches.shape[0] > 2 * 1024 and int(host.branches["item_count"].max()) == 600
    assert nc.table_of(case.sbs, table) == nc.written_table(case)
    _same_table(loader.branches(ds).read(), host, "alone")
    _check_results(case, results, out_items, out_begin)
    _check_routes(case, routes)
    assert np.bincount(routes["route"], minlength=5).min() >= 2


def test_no_tasks_and_no_states(loader, decided):
    case, ds, table, *_ = decided
    loader.plan(ds)
    res, routes, out = loader.ndc_prepare(ds, np.zeros(0, abi.REPL_TASK), np.zeros(0, abi.VH_ITEM))
    assert res.shape == routes.shape == (0,) and out.shape == (0,)
    _same_table(loader.last_ndc[0].read(), table, "n_tasks == 0")
    empty = persisted.build_blob_set([])
    ds0 = loader.upload(empty)
    loader.plan(ds0)
    tasks = np.zeros(3, abi.REPL_TASK)
    tasks["wf"] = [0, 5, 0xFFFFFFFF]
    tasks["incoming_count"] = 1
    res, routes, out = loader.ndc_prepare(ds0, tasks, np.array([(3, 1)], abi.VH_ITEM))
    assert (res["status"] == abi.Status.NDC_STATE_NOT_LOADED).all() and (res["action"] == abi.NDC_DUPLICATE).all()
    assert (routes["route"] == abi.ROUTE_NONE).all() and (routes["status"] == abi.Status.NDC_STATE_NOT_LOADED).all()
    assert out.shape == (0,)
    t0 = loader.last_ndc[0].read()
    _same_table(t0, load_branches_host(empty), "n_wf == 0")
    assert t0.branch_begin.tolist() == [0]
    # an incoming range outside the incoming items is refused, not read
    loader.plan(ds)
    tasks = case.tasks[:4].copy()
    tasks["wf"] = 1
    tasks["incoming_begin"] = [0, case.incoming.shape[0], 0xFFFFFFFF, 5]
    tasks["incoming_count"] = [case.incoming.shape[0] + 1, 1, 2, 0xFFFFFFFF]
    res, routes, _ = loader.ndc_prepare(ds, tasks, case.incoming)
    assert (res["status"] == abi.Status.NDC_BAD_INDEX).all() and (routes["route"] == abi.ROUTE_NONE).all()


# ---- end to end: load -> verify -> branch decision -> route -> resume ------------------------------------------
def _vh_items(batch, res):
    loaded = res.to_loaded(batch)
    c = loaded.counts("vh")
    o = np.cumsum(c) - c
    rows = loaded.rows["vh"]
    return [[(int(r["event_id"]), int(r["version"])) for r in rows[int(o[w]):int(o[w]) + int(c[w])]] if loaded.mask[w] else None
            for w in range(c.shape[0])]


def test_apply_current_tasks_resume_to_the_oracle(engine, loader):
    from oracle import oracle
    hs = synth_mixed.mixed_histories(64, 81, multi_version=True)
    pre, suf, split = split_histories(hs, 82, last_only=True)       # each last batch is a replication task
    pre_b, one_b = flatten(pre, known_domains=KNOWN), flatten(hs, known_domains=KNOWN)
    pre_r, one_r = oracle.replay(pre_b, 0), oracle.replay(one_b, 0)
    local, after = _vh_items(pre_b, pre_r), _vh_items(one_b, one_r)
    sel = np.array([bool(split[w]) and local[w] is not None and after[w] is not None for w in range(len(hs))])
    assert sel.sum() > 40
    # half the states get a second, lower-version branch that shares the first version; on half of those it is the
    # current one, so the task extends a branch that is not current
    branches, own_is_current = {}, np.ones(len(hs), bool)
    for w in np.nonzero(sel)[0][::2]:
        if local[w][0][0] < 2:
            continue
        cur = int((w // 2) % 2)
        branches[int(w)] = ([None, (b"stale-branch-token", [(1, local[w][0][1])])], cur)
        own_is_current[w] = cur == 0
    assert sum(1 for _b, c in branches.values() if c == 1) >= 5 and sum(1 for _b, c in branches.values() if c == 0) >= 5
    sbs = encode_states(pre_b, pre_r, pre, shuffle_seed=8, branches=branches)
    tasks, incoming = np.zeros(int(sel.sum()), abi.REPL_TASK), []
    for k, w in enumerate(np.nonzero(sel)[0]):
        first = suf[w].batches[0][0]
        tasks[k] = (w, len(incoming), len(after[w]), 0, first.id, first.version)
        incoming.extend(after[w])
    order = np.random.default_rng(5).permutation(tasks.shape[0])
    tasks = tasks[order]
    ds = loader.upload(sbs)
    loader.plan(ds)
    # what verify, read and place give before the new calls
    verify0, img0 = loader.verify(ds), loader.read()
    lay = interleave(flatten(suf, known_domains=KNOWN, loaded=img0.resumable(split)))
    db0 = engine.upload(dataclasses.replace(lay, init=None), live_ids=True)
    loader.place(db0, perm=lay.perm)
    placed0 = engine.download(db0)

    results, routes, _out = loader.ndc_prepare(ds, tasks, np.array(incoming, abi.VH_ITEM))
    assert (results["status"] == 0).all()
    mask = apply_mask(routes, tasks, sbs.n_wf)
    assert (mask == (sel & own_is_current)).all()
    not_current = routes["route"][~own_is_current[tasks["wf"]]]
    assert not_current.size >= 5 and np.isin(not_current, [abi.ROUTE_REBUILD, abi.ROUTE_BAD_REQUEST]).all()

    # the loader's scratch is as it was: verify, read and place give the same bytes
    assert loader.verify(ds).tobytes() == verify0.tobytes()
    img = loader.read()
    h, d0, d1 = load_states_host(sbs).image_bytes(), img0.image_bytes(), img.image_bytes()
    for k in h:
        assert d1[k] == d0[k] == h[k], k
    db1 = engine.upload(dataclasses.replace(lay, init=None), live_ids=True)
    loader.place(db1, perm=lay.perm)
    placed1 = engine.download(db1)
    assert placed1.exec.tobytes() == placed0.exec.tobytes()
    for name, *_ in abi.TABLES[:7]:
        assert placed1.tables[name].tobytes() == placed0.tables[name].tobytes(), name

    # replaying only the routed tasks through the resume path gives the oracle's rows
    loaded = img.resumable(mask=mask)
    assert (loaded.mask == mask).all()
    suf_b = interleave(flatten(suf, known_domains=KNOWN, loaded=loaded))
    suf_r = engine.replay(suf_b)
    d = diff_results(suf_b, suf_r, suf_b, oracle.replay(suf_b, 0))
    assert not d, "\n".join(d)
    # and the resumed current branch is the incoming history the task carried
    resumed = _vh_items(suf_b, suf_r)
    for w in np.nonzero(mask)[0]:
        assert resumed[w] == after[w], w
