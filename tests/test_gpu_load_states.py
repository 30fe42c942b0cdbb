"""GPU: persisted mutable-state blobs decoded on the device into resumable rows (include/cadence_load.h).

The device image equals the host restatement's byte for byte (truncated blobs included: they end in a
status); the loaded states resume to the oracle's rows; crr_load_states_place writes what engine.upload
writes for the same loaded states; and crr_checksum is valid on placed rows before any replay.
"""
import dataclasses

import numpy as np
import pytest

from cadence_amd import abi
from cadence_amd.flatten import flatten, interleave
from cadence_amd.persisted import StateLoader, encode_states, load_states_host
from cadence_amd.result import _live_canonical, diff_results, to_canonical_order

import load_cases as lc
from resume_cases import KNOWN, load_stable

pytestmark = pytest.mark.gpu

# row fields that carry provenance (blob / step indices) or per-workflow key ids: they differ between a state
# loaded from persistence and the same state replayed from its first event
# (+ what resume_cases.compare_split_with_one_shot leaves out: the per-call inconsistencies / n_tasks, padding)
PROVENANCE = {"exec": {"decision_request_src", "start_src", "src_next", "reserved", "inconsistencies", "n_tasks"},
              # + LastHeartbeatTimeoutVisibilityInSeconds: the SQL store has no column or blob field for it
              # (workflowStateMaps.go:144-187), so a loaded activity has 0 where the in-memory one may not
              "act": {"sched_src", "started_src", "key", "last_hb_timeout_vis_s"}, "timer": {"src", "key"}, "child": {"src", "started_src", "reserved"},
              "rc": {"src"}, "sig": {"src"}, "vh": set(), "rp": {"src", "prev_index", "key"}}


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


@pytest.fixture(scope="module")
def loader(engine):
    return StateLoader(engine)


def _oracle():
    from oracle import oracle
    return oracle


def _device_image(loader, sbs, scratch_bytes=None):
    loader.plan(loader.upload(sbs), scratch_bytes)
    return loader.read()


def _same(dev, host, what):
    d, h = dev.image_bytes(), host.image_bytes()
    for k in h:
        assert d[k] == h[k], f"{what}: {k} differs"
    assert dev.err_blob == host.err_blob, what


def test_device_image_equals_host_on_edge_cases(loader):
    for name, sbs in lc.edge_batches().items():
        host = load_states_host(sbs)
        _same(_device_image(loader, sbs), host, name)
        if name.startswith("truncated"):
            assert (host.status[1:-1] == abi.LoadStatus.MALFORMED).all()


def test_device_plan_refuses_blob_ranges_the_host_refuses(loader):
    """Ranges that are not consecutive, or do not cover the blobs: -1 from both entry points."""
    import ctypes
    from cadence_amd import persisted
    for how in ("gap", "short"):
        sbs = persisted.build_blob_set([lc.good_workflow(i) for i in range(70)])
        if how == "gap":
            sbs.wf["blob_begin"][40] += 1
        else:
            sbs.wf["blob_count"][69] -= 1
        S = abi.CLoadSummary()
        c = persisted._c_batch(sbs, lambda a: a.ctypes.data)
        assert persisted._host_lib().crr_load_states_host(ctypes.byref(c), None, ctypes.byref(S), 1) == -1
        with pytest.raises(RuntimeError, match="crr_load_states_plan failed: -1"):
            loader.plan(loader.upload(sbs))
    _same(_device_image(loader, lc.edge_batches()["n_wf_65"]), load_states_host(lc.edge_batches()["n_wf_65"]), "after a refusal")


def test_device_image_equals_host_on_replayed_states_and_grows_its_scratch(loader):
    _hs, pre, _suf, _mask, pre_b, pre_r = lc.prefix_case(3000, 61)
    ok = np.nonzero(pre_r.to_loaded(pre_b).mask)[0]
    sbs = encode_states(pre_b, pre_r, pre, shuffle_seed=3, sticky=ok[::7], multi_branch=ok[::11])
    host = load_states_host(sbs, threads=4)
    lc.assert_image_equals(host, lc.expected_image(pre_r.to_loaded(pre_b), sbs))
    _same(_device_image(loader, sbs), host, "mixed")
    assert loader.grown == 0
    # a scratch just short of the dense image: the plan reports the size it needs and is run again
    short = int(loader.summary.scratch_needed) - 64
    _same(_device_image(loader, sbs, scratch_bytes=short), host, "grown")
    assert loader.grown == short + 64


def _resume(engine, loader, case, layout, seed):
    hs, pre, suf, mask, pre_b, pre_r = case
    sbs = encode_states(pre_b, pre_r, pre, shuffle_seed=seed)
    img = _device_image(loader, sbs)
    loaded = img.resumable(mask)                     # the split workflows whose state loaded OK
    assert (loaded.mask == (pre_r.to_loaded(pre_b).mask & mask)).all()
    suf_b = layout(flatten(suf, known_domains=KNOWN, loaded=loaded))
    suf_r = engine.replay(suf_b)
    d = diff_results(suf_b, suf_r, suf_b, _oracle().replay(suf_b, 0))
    assert not d, "\n".join(d)
    # against the one-shot replay of the whole histories, wherever Load reproduces the in-memory state
    one_b = layout(flatten(hs, known_domains=KNOWN))
    one = engine.replay(one_b)
    e1, e2 = to_canonical_order(one_b, one), to_canonical_order(suf_b, suf_r)
    # Load-stable is a property of the in-memory state that was persisted (resume_cases.load_stable): every live
    # activity still mapped by its ActivityID; the loaded image itself always maps the latest one, as Load does
    sel = load_stable(pre_r.to_loaded(pre_b)) & loaded.mask & (e1["status"] == 0) & (e2["status"] == 0)
    # AutoResetPoints nil in memory comes back non-nil from persistence (DeserializeResetPoints never returns nil,
    # serializer.go:144-148): the one bit of the state Load itself changes, set on both sides here
    e1, e2 = e1.copy(), e2.copy()
    e1["flags"] |= abi.EXEC_RESET_POINTS_SET
    e2["flags"] |= abi.EXEC_RESET_POINTS_SET
    for f in abi.EXEC_ROW.names:
        if f not in PROVENANCE["exec"]:
            bad = np.nonzero((e1[f] != e2[f]) & sel)[0]
            assert bad.size == 0, f"exec.{f}: wf {bad[:5]}: {e1[f][bad[:5]]} vs {e2[f][bad[:5]]}"
    l1, l2 = _live_canonical(one_b, one), _live_canonical(suf_b, suf_r)
    for name, _dt, _b, _c, n_f in abi.TABLES[:7]:
        a = l1[name][np.repeat(sel, np.maximum(e1[n_f], 0))]
        b = l2[name][np.repeat(sel, np.maximum(e2[n_f], 0))]
        assert a.shape == b.shape, name
        for f in a.dtype.names:
            if f not in PROVENANCE[name]:
                bad = np.nonzero(a[f] != b[f])[0]
                assert bad.size == 0, f"{name}.{f}: rows {bad[:5]}: {a[f][bad[:5]]} vs {b[f][bad[:5]]}"
    return int(sel.sum()), loaded, suf_b


def test_resume_from_the_device_loaded_image_mixed(engine, loader):
    n, loaded, _ = _resume(engine, loader, lc.prefix_case(3000, 61), interleave, 5)
    assert loaded.mask.sum() > 1500 and n > 1200


def test_resume_from_the_device_loaded_image_long_tail(engine, loader):
    n, _loaded, _ = _resume(engine, loader, lc.prefix_case(150, 62, long_tail=True), interleave, 6)
    assert n > 50


def _tables(res):
    return {name: res.tables[name] for name, *_ in abi.TABLES[:7]}


@pytest.mark.parametrize("layout", ["stride64_wave_tail", "stride1"])
def test_place_equals_upload_and_reports_capacity(engine, loader, layout):
    hs, pre, suf, mask, pre_b, pre_r = lc.prefix_case(3000, 61)
    sbs = encode_states(pre_b, pre_r, pre)
    img = _device_image(loader, sbs)
    loaded = img.resumable(mask)
    lay = (lambda b: interleave(b, long_threshold=30)) if layout == "stride64_wave_tail" else (lambda b: b)
    suf_b = lay(flatten(suf, known_domains=KNOWN, loaded=loaded))
    if layout == "stride64_wave_tail":
        assert suf_b.stride == 64 and 0 < suf_b.wave_begin < suf_b.n_wf
        assert (suf_b.wf["flags"][suf_b.wave_begin:] & abi.WF_FLAG_RESUME).any()
    want = engine.download(engine.upload(suf_b))                 # the host wrote batch.init into the buffers
    fresh = dataclasses.replace(suf_b, init=None)
    db = engine.upload(fresh)
    loader.place(db, perm=suf_b.perm)
    got = engine.download(db)
    assert got.exec.tobytes() == want.exec.tobytes()
    for name, rows in _tables(want).items():
        assert got.tables[name].tobytes() == rows.tobytes(), name
    # the live-ID sidecar: the ID column of every placed row
    for t, name in enumerate(abi.ID_TABLES):
        ids = db.tensors["ids_" + name].cpu().numpy()
        rows = want.tables[name]
        n = min(ids.shape[0], rows.shape[0])
        assert (ids[:n] == rows[rows.dtype.names[0]][:n]).all(), name
    # a workflow sized too small: CRR_ERR_CAPACITY, zero counts, nothing outside its own slots changes
    resumed = np.nonzero(((fresh.wf["flags"] & abi.WF_FLAG_RESUME) != 0) & (want.exec["n_activity"] > 0))[0]
    bad = resumed[:: max(1, resumed.size // 30)][:30]
    small = dataclasses.replace(fresh, wf=fresh.wf.copy())
    small.wf["act_cap"][bad] = want.exec["n_activity"][bad] - 1
    db2 = engine.upload(small)
    loader.place(db2, perm=suf_b.perm)
    r2 = engine.download(db2)
    assert (r2.exec["status"][bad] == abi.Status.CAPACITY).all() and (r2.exec["fail_step"][bad] == want.exec["src_next"][bad]).all()
    for f in ("n_activity", "n_timer", "n_child", "n_rc", "n_signal", "n_vh_items", "n_reset_points"):
        assert (r2.exec[f][bad] == 0).all(), f
    keep = np.ones(fresh.n_wf, bool)
    keep[bad] = False
    assert r2.exec[keep].tobytes() == want.exec[keep].tobytes()
    st = fresh.wf_strides()
    for name, _dt, base_f, cap_f, _n in abi.TABLES[:7]:
        own = np.zeros(want.tables[name].shape[0], bool)
        for w in bad:
            idx = int(fresh.wf[base_f][w]) + np.arange(int(fresh.wf[cap_f][w])) * int(st[w])
            own[idx[idx < own.size]] = True
        assert (r2.tables[name][~own] == want.tables[name][~own]).all(), name
        assert (r2.tables[name][own] == np.zeros(1, r2.tables[name].dtype)).all(), name


def test_checksum_is_valid_on_placed_rows_before_any_replay(engine, loader):
    hs, pre, suf, mask, pre_b, pre_r = lc.prefix_case(3000, 61)
    ok = np.nonzero(pre_r.to_loaded(pre_b).mask)[0]
    sbs = encode_states(pre_b, pre_r, pre, shuffle_seed=9, sticky=ok[::7], multi_branch=ok[::11])
    img = _device_image(loader, sbs)
    loaded = img.resumable(mask)
    suf_b = interleave(flatten(suf, known_domains=KNOWN, loaded=loaded))
    db = engine.upload(dataclasses.replace(suf_b, init=None), live_ids=True)
    loader.place(db, perm=suf_b.perm)
    got = engine.checksum(db)
    canon = suf_b.perm                                         # device position -> canonical workflow
    sel = loaded.mask[canon] & (img.flags[canon] == 0)
    assert sel.sum() > 1000 and (loaded.mask[canon] & (img.flags[canon] != 0)).sum() > 100
    want = pre_r.exec["checksum"][canon]                      # the prefix replay's checksum of the same state
    bad = np.nonzero((got != want) & sel)[0]
    assert bad.size == 0, f"{bad.size} checksums differ, first position {bad[:5]}"
