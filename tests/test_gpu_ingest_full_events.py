"""The device ingest (ingest_kernel.hip, json_ingest_kernel.hip) on real-shaped blobs (tests/full_event_cases.py):
every field of the reference's event schema on the fast and the general pass, blobs walked from HBM and every
edge of the LDS staging loop, keys longer than a KeyRef's 16 inline bytes and keys whose str_hash collides, the
resume ingest and the JSON transcode of such blobs.  Each layout is checked byte-identical to the host path
(decode_histories + interleave; tests/test_decode_full_events.py pins that path on the same fixtures), and where
stated the replay of the device-laid-out inputs against the oracle."""
import json
import random

import numpy as np
import pytest

from cadence_amd import abi, synth_mixed
from cadence_amd.abi import EventType as ET
from cadence_amd.blobs import KNOWN_DOMAINS
from cadence_amd.decode import WorkflowSource, decode_histories
from cadence_amd.flatten import interleave
from cadence_amd.history import HistoryEvent, WorkflowHistory
from cadence_amd.json_codec import event_json
from cadence_amd.result import diff_results

import full_event_cases as F
from test_decode import sources_of
from test_gpu_ingest import _assert_same_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


def _host_path(bs):
    canon = decode_histories(bs.to_sources(), known_domains=KNOWN_DOMAINS)
    return canon, interleave(canon)


def _replay_equals_oracle(eng, out, want, canon):
    from oracle import oracle
    eng.launch(out)
    res = eng.download(out)
    d = diff_results(want, res, canon, oracle.replay(canon, 8))
    assert not d, d[:3]


def _upload_exact(eng, ing, bs):
    """The blob bytes in a buffer of exactly n_bytes + CRR_INGEST_PAD (test_device_ingest_blobs_flush_against_the_pad)."""
    from cadence_amd.ingest import INGEST_PAD
    db = ing.upload(bs)
    end = bs.n_bytes
    t = eng.torch.zeros(end + INGEST_PAD, dtype=eng.torch.uint8, device=eng.dev)
    t[:end].copy_(eng.torch.from_numpy(np.ascontiguousarray(bs.bytes[:end])))
    db.tensors["bytes"] = t
    db.c.bytes = t.data_ptr()
    return db


@pytest.fixture(scope="module")
def populated():
    """300 mixed workflows, their blobs populated in each mode; the host path of each, once."""
    hs = synth_mixed.mixed_histories(300, 61, multi_version=True, invalid_rate=0.2, can_rate=0.4)
    src = sources_of(hs)
    out = {}
    for mode in F.MODES:
        bs = F.blobset_of(F.populate_sources(src, mode, seed=5))
        out[mode] = (bs, *_host_path(bs))
    return out


@pytest.mark.parametrize("mode", F.MODES)
def test_populated_events_on_the_fast_and_general_pass(eng, populated, mode):
    """Every schema field present: skipped inline by the fast pass (`full`, `empty`, `wrong_type`), or the blob
    deferred to blob_decode_general_kernel by a list<struct> on its first event (`general`).  `general` also
    through a DeviceIngest that has just planned the `full` blobs and the other way round: the scratch (and the
    deferral marks in it) is reused."""
    from cadence_amd.ingest import DeviceIngest
    bs, canon, want = populated[mode]
    ing = DeviceIngest(eng)
    out = ing.ingest(ing.upload(bs))
    _assert_same_inputs(ing.to_host_batch(out), want)
    if mode == "full":
        _replay_equals_oracle(eng, out, want, canon)
    if mode == "general":
        for order in (("full", "general"), ("general", "full")):
            ing2 = DeviceIngest(eng)
            for m in order:
                b, _c, w = populated[m]
                _assert_same_inputs(ing2.to_host_batch(ing2.ingest(ing2.upload(b))), w)


def test_staging_window_edges(eng):
    """window_batch(): blobs walked from HBM at b0 % 16 in {0, 1, 8, 15} (one of many small events, one of 1 MB,
    the batch's last one against the pad), a blob that fits its window with zero slack and the same one 16 bytes
    longer, an over-size blob in mid-wavefront, a window refilled nine times, an empty blob at a window edge."""
    from cadence_amd.ingest import DeviceIngest
    wb = F.window_batch()
    assert sum(p.kind == "hbm" for p in wb.path) >= 6 and wb.path[wb.roles["fit0"]].slack == 0
    canon, want = _host_path(wb.bs)
    ing = DeviceIngest(eng)
    out = ing.ingest(_upload_exact(eng, ing, wb.bs))
    _assert_same_inputs(ing.to_host_batch(out), want)
    _replay_equals_oracle(eng, out, want, canon)


def _paddable_workflow(w: int, n_batches: int) -> WorkflowHistory:
    """Started + DecisionTaskScheduled, then batches of one ActivityTaskScheduled event: every blob paddable."""
    h = F._edge_workflow(w)
    h.batches = [b for b in h.batches if b][:3]
    eid = 6
    while len(h.batches) < n_batches:
        h.batches.append([F._act(eid, 1, synth_mixed.BASE_TS + 900 + eid, f"over-{eid}")])
        eid += 1
    return h


def test_blob_walked_from_hbm_alone(eng):
    """A batch of one workflow with one 40 KB blob; and a batch whose every blob is over-size (two wavefronts: in
    the first, 64 lanes take the HBM path one after another)."""
    from cadence_amd.ingest import DeviceIngest
    rng = random.Random(3)
    one = WorkflowHistory(batches=[F._edge_workflow(0).batches[0]])
    src = sources_of([one])
    src[0].blobs = [F.pad_blob(F.populate(src[0].blobs[0], "full", rng), 40_000)]
    h = _paddable_workflow(1, 70)
    src2 = sources_of([h])
    blobs = [F.populate(b, "full", rng) for b in src2[0].blobs]
    blobs = [b if i == 1 else F.pad_blob(b, F.K_STAGE_BYTES + 100 + 7 * i) for i, b in enumerate(blobs)]
    blobs[1] = F.pad_event(blobs[1], 0, F.K_STAGE_BYTES + 100)      # (DecisionTaskStarted: its identity)
    src2[0].blobs = blobs
    ing = DeviceIngest(eng)
    for s in (src, src2):
        bs = F.blobset_of(s)
        path, _its = F.window_path(bs.blob_off)
        assert all(p.kind == "hbm" for p in path) and len(path) in (1, 70)
        canon, want = _host_path(bs)
        out = ing.ingest(ing.upload(bs))
        _assert_same_inputs(ing.to_host_batch(out), want)
        _replay_equals_oracle(eng, out, want, canon)


def test_long_and_colliding_keys(eng):
    """long_key_histories(): keys of 15..300 bytes, equal in their first 16 bytes, differing at the last byte, and
    pairs with the same length and str_hash (only those make same_bytes return false) through both interning
    passes.  The key ids are the host's (first-seen order over the key table keys_of() holds)."""
    from cadence_amd.ingest import DeviceIngest
    from test_decode import keys_of
    hs = F.long_key_histories()
    st = F.key_statistics(hs)
    assert st["colliding_pairs"] >= 100 and st["longer_than_16"] > 1000
    bs = F.blobset_of(sources_of(hs))
    canon, want = _host_path(bs)
    assert sum(1 for k in set(keys_of(canon)) if len(k) > 16) > 1000
    ing = DeviceIngest(eng)
    out = ing.ingest(ing.upload(bs))
    got = ing.to_host_batch(out)
    np.testing.assert_array_equal(got.cols["key"], want.cols["key"])
    assert got.reset_keys.tolist() == want.reset_keys.tolist()
    _assert_same_inputs(got, want)
    _replay_equals_oracle(eng, out, want, canon)


def test_resume_ingest_of_populated_blobs(eng):
    """The passive-replication layout (crr_ingest_plan_resume / crr_ingest_layout_resume) over populated suffix
    blobs of the long-key histories, a few of them over 13 KB: the long keys the loaded state already holds are
    matched to the loaded key ids (same_bytes against the seeds), new ones continue after them; columns,
    descriptors and the replayed rows equal the host path's."""
    from cadence_amd.replication import BlobReplication, PassiveReplication, _prefix_key_count
    hs = F.long_key_histories()
    # a last batch that names one key the workflow already holds and one new key, for every third workflow and
    # the ones with more than 64 keys (their loaded dictionaries seed the resume pass's hash table)
    n_added = n_many = 0
    for w, h in enumerate(hs):
        keys = F.workflow_keys(h)
        if h.is_new_run or not h.batches or not h.batches[-1] or not keys or (w % 3 and len(set(keys)) <= 64):
            continue
        e = h.batches[-1][-1]
        long_old = next((k for k in keys if len(k) > 16), None)
        if long_old is None:
            continue
        h.batches.append([HistoryEvent(int(ET.ActivityTaskCancelRequested), e.id + 1 + k, e.version, e.timestamp + 1 + k,
                                       e.task_id + 1 + k, {"activity_id": name})
                          for k, name in enumerate((long_old, "a-new-key-of-the-last-batch-%04d" % w))])
        n_added += 1
        n_many += len(set(keys)) > 64
    assert n_added >= 50 and n_many >= 3
    src = F.populate_sources(sources_of(hs), "full", seed=7)
    n_big = 0
    for s in src:          # the last batch is the replication task's payload
        last = max((i for i, b in enumerate(s.blobs) if b), default=None)
        if last is not None and last > 0 and n_big < 4 and F.can_pad(s.blobs[last]):
            s.blobs[last] = F.pad_blob(s.blobs[last], 14_000 + 5 * n_big)
            n_big += 1
    assert n_big == 4
    canon_bs = F.blobset_of(src)
    canon = decode_histories(canon_bs.to_sources(), known_domains=KNOWN_DOMAINS)
    b = interleave(canon, long_threshold=150)
    pr = PassiveReplication(eng, b)
    pr.setup()
    pr.restore()
    pr.step()
    host = eng.download(pr.db)
    br = BlobReplication(pr, canon_bs)
    br.setup()
    rb = br.blobs.blobs
    assert int(np.diff(rb.blob_off.astype(np.int64)).max()) > F.K_STAGE_BYTES
    assert sum(p.kind == "hbm" for p in F.window_path(rb.blob_off)[0]) >= 1
    pr.restore()
    S = br.step()
    dev = eng.download(pr.db)
    eng.torch.cuda.synchronize()
    sb, T = pr.suffix, br.tensors
    n_slots = int(S.n_slots)
    assert n_slots == sb.cols["etype"].size and int(S.n_events) == sb.n_events
    got = {name: T["ev_" + name][:n_slots * np.dtype(t).itemsize].cpu().numpy().view(t) for name, t in abi.EVENT_COLUMNS}
    for name, _t in abi.EVENT_COLUMNS:
        if name != "aux":
            np.testing.assert_array_equal(got[name], sb.cols[name], err_msg=name)
    g_wf = T["loaded_wf"][:b.n_wf * abi.WORKFLOW.itemsize].cpu().numpy().view(abi.WORKFLOW)
    assert g_wf.tobytes() == sb.wf.tobytes()
    # long keys of the new batches that the loaded dictionaries already hold
    K = _prefix_key_count(b, pr.pre_wf)
    cnt = sb.wf["ev_count"].astype(np.int64)
    st = sb.wf_strides()
    wf_idx = np.repeat(np.arange(sb.n_wf), cnt)
    x = sb.wf["ev_begin"].astype(np.int64)[wf_idx] + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)) * st[wf_idx]
    key = got["key"][x].astype(np.int64)
    loaded = (key > 0) & (key <= K[wf_idx]) & (sb.key_len[x] > 16)
    new = (key > K[wf_idx]) & (sb.key_len[x] > 16)
    assert loaded.sum() >= n_added and new.sum() >= n_added, (int(loaded.sum()), int(new.sum()))
    assert int((K > 64).sum()) >= n_many      # the seeded hash table as well as the linear scan
    # the rows: the host path's step, byte for byte
    assert dev.exec.tobytes() == host.exec.tobytes()
    for name, *_r in abi.TABLES:
        if name != "tasks":
            assert dev.tables[name].tobytes() == host.tables[name].tobytes(), name


def test_json_transcode_of_populated_events(eng):
    """`full` JSON events (every attribute key of the schema present) of 150 workflows, and one JSON blob of 300
    events whose transcoded thriftrw form exceeds the 13 KB window: the ingest after the transcode walks it
    from HBM."""
    from test_gpu_json_ingest import _check
    rng = random.Random(8)
    hs = synth_mixed.mixed_histories(150, 64, multi_version=True, invalid_rate=0.2, can_rate=0.4)
    evs, _blob = F.many_events(40_000)
    evs = evs[:300]
    assert len(evs) == 300
    start = F._edge_workflow(0).batches[0]
    hs.append(WorkflowHistory(batches=[start, evs]))
    src = sources_of(hs)
    for h, s in zip(hs, src):
        s.blobs = [json.dumps([F.populate_json_event(event_json(e), "full", rng) for e in bt],
                              separators=(",", ":")).encode() if bt else b"" for bt in h.batches]
        s.encodings = ["json"] * len(s.blobs)
    ing, tdb = _check(eng, src, replay=True)
    assert int(ing.last_transcode.err) == 0
    off = ing.transcoded_blobs(tdb).blob_off
    path, _its = F.window_path(off)
    assert path[-1].kind == "hbm" and int(off[-1] - off[-2]) > F.K_STAGE_BYTES
