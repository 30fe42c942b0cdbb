"""GPU: the checksum to store for routed replication tasks (include/cadence_load_store.h), load_store_kernel.

The device rows equal the host restatement's byte for byte on hand-built states with hand-made decisions and on
ndc_load_cases.task_case (130 states over three wavefronts, about 400 shuffled tasks, the not-generated ones in the
middle of a wavefront).  End to end -- upload, plan, decide and route on the device, place, replay, generate -- the
values equal the ones expected from the values written and the oracle's rows (store_cases.py), with the interleaved
layout (a position map that is not the identity) and through the wave tail (stride 1); they equal the replay's own
checksum on single-branch states and differ from it on every two-branch one, which is the gap this call closes;
the loader's scratch and the branch table are only read; the generated values verify as stored on the
re-encoded states; and a failed replay's row or counts no table holds do not take a lane out of its tables.
"""
import dataclasses

import numpy as np
import pytest

from cadence_amd import abi, persisted
from cadence_amd.flatten import flatten, interleave
from cadence_amd.persisted import StateLoader, apply_mask, store_checksums_host

import load_cases as lc
import store_cases as sc
from resume_cases import KNOWN

pytestmark = pytest.mark.gpu
O = abi.StoreOutcome


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


@pytest.fixture(scope="module")
def loader(engine):
    return StateLoader(engine)


def _same(got: np.ndarray, want: np.ndarray, what=""):
    assert got.dtype == abi.STORE_ROW and got.shape == want.shape
    for f in abi.STORE_ROW.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what} {f}: {bad.size} tasks differ, first {bad[:5]}: {got[f][bad[:5]]} vs {want[f][bad[:5]]}"


def _device_rows(loader, ds, n: int, dt, name: str) -> np.ndarray:
    return loader.last_ndc[1][name][:n * dt.itemsize].cpu().numpy().view(dt).copy()


def test_hand_made_decisions_equal_the_host_restatement(loader):
    c = sc.hand_case()
    ds = loader.upload(c.sbs)
    loader.plan(ds)
    loader.ndc_prepare(ds, c.tasks, np.zeros(0, abi.VH_ITEM), on_device=True)   # the branch table; the decisions are replaced
    torch = loader.torch
    for name, rows in (("results", c.results), ("routes", c.routes)):
        raw = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy())
        loader.last_ndc[1][name][:raw.numel()].copy_(raw)
    got = loader.store_checksums(ds, c.tasks, c.last_events)
    host = store_checksums_host(c.sbs, c.tasks, c.last_events, c.results, c.routes)
    assert got.tobytes() == host.tobytes()
    _same(got, c.want_without, "hand case")
    assert {int(O.BACKFILLED), int(O.NOT_LOADED), int(O.NO_ROUTE), int(O.NEW_BRANCH), int(O.VH_ERROR), int(O.NOT_RESUMED)} == \
        set(int(x) for x in got["outcome"])
    # a prefix of the tasks, and none: nothing launched, nothing written
    assert loader.store_checksums(ds, c.tasks[:5], c.last_events[:5]).tobytes() == host[:5].tobytes()
    assert loader.store_checksums(ds, c.tasks[:0], c.last_events[:0]).shape == (0,)
    with pytest.raises(ValueError):
        loader.store_checksums(ds, np.concatenate([c.tasks, c.tasks]), np.concatenate([c.last_events, c.last_events]))


def test_task_case_equals_the_host_restatement(loader):
    c = sc.routed_case()
    ds = loader.upload(c.sbs)
    loader.plan(ds)
    verify0 = loader.verify(ds)
    results, routes, _out = loader.ndc_prepare(ds, c.tasks, sc.nc.task_case().incoming)
    table0 = loader.last_ndc[0].read().image_bytes()
    got = loader.store_checksums(ds, c.tasks, c.last_events)
    assert got.tobytes() == store_checksums_host(c.sbs, c.tasks, c.last_events, results, routes).tobytes()
    _same(got, c.want, "task_case")
    assert (got["outcome"] == O.BACKFILLED).sum() >= 20 and (got["outcome"] == O.NOT_RESUMED).sum() >= 60
    # the loader's scratch and the branch table are only read
    assert loader.verify(ds).tobytes() == verify0.tobytes()
    assert loader.last_ndc[0].read().image_bytes() == table0


@pytest.mark.parametrize("n_states,n_tasks", sc.nc.LARGE_CASES)
def test_task_case_past_one_element_per_scan_thread(loader, n_states, n_tasks):
    """The checksum rows with more than 1024 states and tasks (ndc_load_cases.LARGE_CASES: the branch table and the
    tasks' rows they read come out of scans whose threads hold several elements each): the rows equal the Python
    expectation (oracle/checksum_py + zlib over the values written) and the host restatement's.

    (1300, 2500): BACKFILLED / NOT_LOADED / NO_ROUTE / NEW_BRANCH / NOT_RESUMED 160 / 11 / 1735 / 73 / 521.
    (1025, 1025): 71 / 7 / 730 / 18 / 199."""
    c = sc.routed_case(n_states, n_tasks)
    assert c.sbs.n_wf == n_states > 1024 and c.tasks.shape[0] == n_tasks > 1024
    ds = loader.upload(c.sbs)
    loader.plan(ds)
    results, routes, _out = loader.ndc_prepare(ds, c.tasks, sc.nc.task_case(n_states, n_tasks).incoming)
    got = loader.store_checksums(ds, c.tasks, c.last_events)
    _same(got, c.want, "task_case")
    assert got.tobytes() == store_checksums_host(c.sbs, c.tasks, c.last_events, results, routes).tobytes()
    outcomes = np.bincount(got["outcome"], minlength=len(O))
    assert set(np.nonzero(outcomes)[0]) == {int(O.BACKFILLED), int(O.NOT_LOADED), int(O.NO_ROUTE), int(O.NEW_BRANCH), int(O.NOT_RESUMED)}
    assert outcomes[O.BACKFILLED] >= 50 and outcomes[O.NOT_RESUMED] >= 150 and outcomes[O.NEW_BRANCH] >= 10
    assert (got["outcome"][n_tasks // 2:] == O.BACKFILLED).sum() >= 10     # behind the scan's first threads too


def test_empty_state_batch(loader):
    empty = persisted.build_blob_set([])
    ds = loader.upload(empty)
    loader.plan(ds)
    tasks = np.zeros(3, abi.REPL_TASK)
    tasks["wf"] = [0, 5, 0xFFFFFFFF]
    loader.ndc_prepare(ds, tasks, np.zeros(0, abi.VH_ITEM), on_device=True)
    got = loader.store_checksums(ds, tasks, np.zeros(3, abi.LAST_EVENT))
    assert got.tolist() == [(0, int(O.NOT_LOADED), 0, 0)] * 3
    assert loader.store_checksums(ds, tasks[:0], np.zeros(0, abi.LAST_EVENT)).shape == (0,)


def _end_to_end(engine, loader, rc: sc.ReplayedCase, layout):
    """upload -> plan -> decide and route on the device -> place -> replay -> generate: (rows, expected rows, the
    replay's own checksum per task, the device position per task, the layout, the resumed mask, the device states,
    the device batch)."""
    from oracle import oracle
    ds = loader.upload(rc.sbs)
    loader.plan(ds)
    verify0 = loader.verify(ds)
    loader.ndc_prepare(ds, rc.tasks, rc.incoming, on_device=True)
    n = rc.tasks.shape[0]
    results, routes = _device_rows(loader, ds, n, abi.NDC_RESULT, "results"), _device_rows(loader, ds, n, abi.NDC_ROUTE, "routes")
    table0 = loader.last_ndc[0].read().image_bytes()
    want_res, want_routes = sc.decided(rc)
    assert results.tobytes() == want_res.tobytes() and (routes["route"] == want_routes["route"]).all()
    mask = apply_mask(routes, rc.tasks, rc.sbs.n_wf)
    lay = layout(flatten(rc.suf, known_domains=KNOWN, loaded=loader.read().resumable(mask)))
    db = engine.upload(dataclasses.replace(lay, init=None), live_ids=True)
    loader.place(db, perm=lay.perm)
    engine.launch(db)
    got = loader.store_checksums(ds, rc.tasks, rc.last_events, db=db)
    res = engine.download(db)
    after = oracle.replay(lay, 0).to_loaded(lay, mask=mask)
    want = sc.expected_replayed(rc, routes, results, mask, after)
    # the loader's scratch and the branch table are as they were
    assert loader.verify(ds).tobytes() == verify0.tobytes()
    assert loader.last_ndc[0].read().image_bytes() == table0
    own = res.to_loaded(lay, mask=mask).exec
    wf = rc.tasks["wf"]
    pos = np.zeros(rc.sbs.n_wf, np.int64)
    pos[lay.perm if lay.perm is not None else np.arange(lay.n_wf)] = np.arange(lay.n_wf)
    return got, want, own[wf], pos[wf], lay, mask, ds, db


def _check_against_the_replay(rc, got, own):
    applied, two = got["outcome"] == O.APPLIED, rc.two_branch[rc.tasks["wf"]]
    single = applied & ~two
    assert (got["value"][single] == own["checksum"][single]).all() and (got["payload_len"][single] == own["payload_len"][single]).all()
    assert (got["value"][applied & two] != own["checksum"][applied & two]).all()   # the gap being closed
    return applied, two


@pytest.fixture(scope="module")
def interleaved(engine, loader):
    rc = sc.replayed_case()
    return (rc,) + _end_to_end(engine, loader, rc, interleave)


def test_end_to_end_on_the_replayed_case(interleaved):
    rc, got, want, own, _pos, lay, _mask, *_ = interleaved
    assert lay.stride == 64 and lay.perm is not None and (lay.perm != np.arange(lay.n_wf)).any()
    _same(got, want, "replayed case")
    applied, two = _check_against_the_replay(rc, got, own)
    assert (applied & two).sum() >= 15 and (applied & ~two).sum() >= 15 and (got["outcome"] == O.BACKFILLED).sum() >= 5


def test_round_trip_device_values_verify_as_stored(loader, interleaved):
    rc, got, *_ = interleaved
    applied, stored = np.zeros(rc.sbs.n_wf, bool), [None] * rc.sbs.n_wf
    for k in np.nonzero(got["outcome"] == O.APPLIED)[0]:
        w = int(rc.tasks[k]["wf"])
        applied[w] = True
        stored[w] = (abi.CHECKSUM_PAYLOAD_V1, abi.CHECKSUM_FLAVOR_CRC32, int(got["value"][k]).to_bytes(4, "big"))
    assert applied.sum() >= 30
    ds = loader.upload(sc.reencoded_applied(rc, applied))
    loader.plan(ds)
    v = loader.verify(ds, persisted.stored_checksums(stored))
    assert (v["outcome"][applied] == abi.VerifyOutcome.MATCH).all()


def test_end_to_end_through_the_wave_tail(engine, loader):
    hs = lc.prefix_case(150, 62, long_tail=True)[0]
    rc = sc.replayed_case_of(hs, 63, 3, shuffle_seed=6, last_only=False)      # prefix_case's own split
    got, want, own, pos, lay, mask, *_ = _end_to_end(engine, loader, rc, interleave)
    assert lay.stride == 64 and 0 < lay.wave_begin < lay.n_wf
    _same(got, want, "long tail")
    applied, two = _check_against_the_replay(rc, got, own)
    in_tail = pos >= lay.wave_begin
    assert (applied & in_tail).sum() >= 5 and (applied & ~in_tail).sum() >= 5 and (applied & two & in_tail).any()
    assert (applied & two).sum() >= 5 and (got["outcome"] == O.BACKFILLED).sum() >= 3


def test_failed_replays_and_garbage_counts_stay_within_the_descriptor(engine, loader):
    """An exec row whose replay failed is reported with its status; counts that no table holds (negative, 2^31 - 1)
    are clamped to the descriptor's capacities before a row is addressed: the payload then has exactly the
    capacity's rows (8 bytes per ID, 23 per version-history item), and no other task's row changes."""
    rc = sc.replayed_case()
    got, _want, _own, pos, lay, _mask, ds, db = _end_to_end(engine, loader, rc, interleave)
    applied = np.nonzero(got["outcome"] == O.APPLIED)[0]
    k_fail, k_wild = int(applied[0]), int(applied[-1])
    raw = db.tensors["exec"]
    ex = raw.cpu().numpy().view(abi.EXEC_ROW).copy()
    p_fail, p_wild = int(pos[k_fail]), int(pos[k_wild])
    ex[p_fail]["status"] = 7
    before = ex[p_wild].copy()
    ex[p_wild]["n_activity"], ex[p_wild]["n_timer"], ex[p_wild]["n_vh_items"] = 2**31 - 1, -5, 2**31 - 1
    raw.copy_(loader.torch.from_numpy(ex.view(np.uint8).reshape(-1)))
    again = loader.store_checksums(ds, rc.tasks, rc.last_events, db=db)
    assert tuple(again[k_fail]) == (0, int(O.REPLAY_FAILED), 0, 7)
    D = lay.wf[p_wild]
    grown = (8 * (int(D["act_cap"]) - int(before["n_activity"])) - 8 * int(before["n_timer"])
             + 23 * (int(D["vh_cap"]) - int(before["n_vh_items"])))
    assert int(again[k_wild]["outcome"]) == O.APPLIED and int(again[k_wild]["payload_len"]) == int(got[k_wild]["payload_len"]) + grown
    rest = np.ones(got.shape[0], bool)
    rest[[k_fail, k_wild]] = False
    assert again[rest].tobytes() == got[rest].tobytes()
