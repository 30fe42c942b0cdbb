"""The host decoders on real-shaped blobs (tests/full_event_cases.py): every field of the reference's event
schema present (real types, zero values, wrong wire types, a container of structs), as thriftrw and as
common/types JSON; and the two fixtures the device tests use -- the staging-window batch and the long-key
histories -- checked on the CPU: each edge they are built for is really there (window_path, key_statistics),
and both decode like flatten().  The host decoders are the device tests' byte-exact reference, so they are
pinned here first."""
import json
import random
import re

import numpy as np
import pytest

from cadence_amd import abi, synth_mixed
from cadence_amd.abi import EventType as ET
from cadence_amd.blobs import KNOWN_DOMAINS
from cadence_amd.decode import WorkflowSource, decode_histories
from cadence_amd.flatten import flatten
from cadence_amd.history import WorkflowHistory, events_from_json, load_json_history, split_batches_by_task_id
from cadence_amd.json_codec import event_json

import full_event_cases as F
from test_decode import ARCHIVAL, KNOWN, assert_same_batch, keys_of, sources_of
from thrift_tree import T_LIST, T_MAP, T_STRUCT, parse_blob


def _mixed():
    return synth_mixed.mixed_histories(300, 61, multi_version=True, invalid_rate=0.2, can_rate=0.4)


def _archival():
    ev = load_json_history(ARCHIVAL)
    return WorkflowHistory(batches=split_batches_by_task_id(ev), run_id="f2b360a0-d90a-4afa-ad88-ba041fad6a42",
                           branch_id="840307b9-9076-4ee2-82a0-45f21d61d719")


# ---- the schema table against what exists today -----------------------------------------------------------------
def test_schema_names_the_42_attribute_structs():
    attrs = [n for n in F.SCHEMA if n.endswith("EventAttributes")]
    assert len(attrs) == 42 == len(ET)
    assert sorted(F.ATTR_FIELD) == list(range(42)) and sorted(F.ATTR_FIELD.values()) == list(range(40, 460, 10))
    for fid, ty, name in F.SCHEMA["HistoryEvent"][1]:
        if fid >= 40:
            t = next(t for t, f in F.ATTR_FIELD.items() if f == fid)
            assert ty == "struct:" + F.attr_struct_name(t)
            assert name == ET(t).name[0].lower() + ET(t).name[1:] + "EventAttributes"
    # the ids follow the thrift struct, not the EventType values: TimerStarted sits at 180, before
    # ActivityTaskCancelRequested (200); the encoder writes each type's struct at the schema's id
    from cadence_amd.thrift_codec import ATTR_FIELD
    assert ATTR_FIELD == F.ATTR_FIELD
    assert (F.ATTR_FIELD[ET.TimerStarted], F.ATTR_FIELD[ET.ActivityTaskCancelRequested]) == (180, 200)
    assert [t for t in range(42) if F.ATTR_FIELD[t] != 40 + 10 * t] == list(range(14, 29))
    for n, (_line, fields) in F.SCHEMA.items():
        ids = [f[0] for f in fields]
        assert ids == sorted(set(ids)), n
        for _fid, ty, _name in fields:      # every struct a field names is in the table
            parts = ty.split(":")
            if parts[0] == "struct":
                assert parts[1] in F.SCHEMA
            if parts[:2] == ["list", "struct"]:
                assert parts[2] in F.SCHEMA


def _check_against_schema(fields, sname, seen):
    schema = {fid: ty for fid, ty, _n in F.SCHEMA[sname][1]}
    seen.add(sname)
    for ft, fid, v in fields:
        assert fid in schema, (sname, fid)
        ty = schema[fid]
        assert ft == F.wire_type(ty), (sname, fid, ft, ty)
        parts = ty.split(":")
        if parts[0] == "struct":
            _check_against_schema(v, parts[1], seen)
        elif parts[0] == "list":
            assert v[0] == (T_STRUCT if parts[1] == "struct" else F.WIRE[parts[1]])
            if parts[1] == "struct":
                for x in v[1]:
                    _check_against_schema(x, parts[2], seen)
        elif parts[0] == "map":
            assert (v[0], v[1]) == (F.WIRE[parts[1]], F.WIRE[parts[2]])


def test_schema_holds_every_field_the_encoder_writes():
    """Every id thrift_codec.attribute_fields writes (nested structs too) is in the table with that type."""
    seen = set()
    for s in sources_of(_mixed() + [_archival()]):
        for b in s.blobs:
            if not b:
                continue
            for ev in F._events_of(parse_blob(b))[2][1]:
                if F.attr_struct_name(F._event_type(ev)) is not None:
                    _check_against_schema(ev, "HistoryEvent", seen)
    assert len([n for n in seen if n.endswith("EventAttributes")]) == 42     # the walk emits every event type
    assert {"RetryPolicy", "ResetPoints", "ResetPointInfo", "TaskList", "WorkflowExecution"} <= seen


def test_schema_holds_every_field_the_decoder_reads():
    """Every `id == N && ft == T_X` of history_decode.cpp's read_attributes / read_retry_policy /
    read_reset_points is a schema field of that type, and DECODER_READS lists exactly those."""
    src = open("cadence_amd/csrc/history_decode.cpp").read()
    ev_of = {m.group(1): int(m.group(2)) for m in re.finditer(r"(CRR_EV_\w+)\s*=\s*(\d+)", open("include/cadence_replay.h").read())}
    wire = {"T_I32": 8, "T_I64": 10, "T_STRING": 11, "T_STRUCT": 12, "T_LIST": 15}
    body = src[src.index("void read_attributes("):src.index("// HistoryEvent struct.")]
    reads, labels, fresh = {}, [], True
    for line in body.splitlines():
        m = re.search(r"case (CRR_EV_\w+):", line)
        if m:
            if fresh:
                labels = []
            labels.append(F.attr_struct_name(ev_of[m.group(1)]))
            fresh = False
        for fid, t in re.findall(r"id == (\d+) && ft == (T_\w+)", line):
            fresh = True
            for n in labels:
                reads.setdefault(n, {})[int(fid)] = wire[t]
        if "break;" in line:
            fresh = True
    reads["RetryPolicy"] = {60: 8}          # read_retry_policy: id == 60 && want(ft, T_I32)
    assert "id == 60 && r.want(ft, T_I32)" in src
    reads["ResetPoints"] = {10: 15}         # read_reset_points
    assert "id == 10 && ft == T_LIST" in src
    reads["ResetPointInfo"] = {10: 11}
    assert "id2 == 10 && t2 == T_STRING" in src
    assert {n: set(v) for n, v in reads.items()} == F.DECODER_READS
    for n, fields in reads.items():
        schema = {fid: ty for fid, ty, _n in F.SCHEMA[n][1]}
        for fid, t in fields.items():
            assert F.wire_type(schema[fid]) == t, (n, fid)


def test_no_other_real_field_is_a_container_of_structs():
    """ResetPoints.points is the schema's only container of structs (the device's fast pass defers such a
    value to the general pass): with it read inline, a blob of real events stays on the fast pass."""
    found = [(n, fid) for n, (_l, fields) in F.SCHEMA.items() for fid, ty, _n in fields
             if ty.startswith("list:struct") or ty.startswith("map:") and "struct" in ty]
    assert found == [("ResetPoints", 10)]


# ---- populated blobs on the host decoder ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_case():
    hs = _mixed()
    return hs, sources_of(hs), flatten(hs, known_domains=KNOWN)


@pytest.mark.parametrize("mode", F.MODES)
def test_populated_thrift_decodes_like_flatten(mixed_case, mode):
    hs, src, want = mixed_case
    pop = F.populate_sources(src, mode, seed=5)
    n_structs = sum(F.check_populated(o, p, mode) for s, t in zip(src, pop) for o, p in zip(s.blobs, t.blobs))
    assert n_structs > 5000
    grown = sum(len(b) for s in pop for b in s.blobs) / sum(len(b) for s in src for b in s.blobs)
    assert grown > 1.0
    got = decode_histories(pop, known_domains=KNOWN)
    assert_same_batch(got, want)
    assert_same_batch(got, decode_histories(src, known_domains=KNOWN))


@pytest.mark.parametrize("mode", F.MODES)
def test_populated_archival_history_decodes_like_flatten(mode):
    h = _archival()
    src = sources_of([h])
    pop = F.populate_sources(src, mode, seed=6)
    assert sum(F.check_populated(o, p, mode) for o, p in zip(src[0].blobs, pop[0].blobs)) == 112
    got = decode_histories(pop)
    assert_same_batch(got, flatten([h]))
    assert_same_batch(got, decode_histories(src))


def test_populate_never_adds_a_read_field_with_its_own_type():
    """The rule that keeps a populated history's meaning: over every mode, a decoder-read field the original
    struct lacks is absent or of another wire type (check_populated), and `full` / `empty` add every other
    schema field -- e.g. the 25 of WorkflowExecutionStarted less the read ones the encoder left out."""
    hs = synth_mixed.mixed_histories(40, 62, multi_version=True)
    rng = random.Random(2)
    n_started = 0
    for s in sources_of(hs):
        for b in s.blobs:
            for mode in F.MODES:
                F.check_populated(b, F.populate(b, mode, rng), mode)
            for ev in F._events_of(parse_blob(F.populate(b, "full", rng)))[2][1] if b else []:
                if F._event_type(ev) == ET.WorkflowExecutionStarted:
                    ids = {f[1] for f in next(f for f in ev if f[1] == 40)[2]}
                    assert len(ids) >= 25 - 4 and {14, 16, 54, 56, 57, 58, 59, 61, 70, 100, 120, 121, 140} <= ids
                    n_started += 1
    assert n_started >= 40


def _json_blobs(h, mode, rng):
    return [json.dumps([F.populate_json_event(event_json(e), mode, rng) for e in b], separators=(",", ":")).encode()
            if b else b"" for b in h.batches]


@pytest.mark.parametrize("mode", ["full", "empty"])
def test_populated_json_decodes_like_flatten(mixed_case, mode):
    hs, src, want = mixed_case
    rng = random.Random(8)
    js = [WorkflowSource(**{**s.__dict__, "blobs": _json_blobs(h, mode, rng), "encodings": ["json"] * len(s.blobs)})
          for h, s in zip(hs, src)]
    # every attribute key of the schema is there
    ev0 = json.loads(js[0].blobs[0])[0]
    assert set(ev0["workflowExecutionStartedEventAttributes"]) >= {
        n for _f, _t, n in F.SCHEMA["WorkflowExecutionStartedEventAttributes"][1]}
    assert_same_batch(decode_histories(js, known_domains=KNOWN), want)


@pytest.mark.parametrize("mode", ["full", "empty"])
def test_populated_archival_json_decodes_like_flatten(mode):
    raw = json.load(open(ARCHIVAL))
    batches = split_batches_by_task_id(events_from_json(raw))
    rng = random.Random(9)
    blobs, i = [], 0
    for b in batches:
        blobs.append(json.dumps([F.populate_json_event(d, mode, rng) for d in raw[i:i + len(b)]]).encode())
        i += len(b)
    got = decode_histories([WorkflowSource(blobs=blobs, encodings=["json"] * len(blobs))])
    assert_same_batch(got, flatten([WorkflowHistory(batches=batches)]))


# ---- blobs of a chosen size -----------------------------------------------------------------------------------------
def test_pad_blob_and_many_events():
    hs = synth_mixed.mixed_histories(3, 63)
    src = sources_of(hs)
    first = src[0].blobs[0]                       # Started + DecisionTaskScheduled: padded through `input`
    for n in (len(first), len(first) + 1, 13 * 1024 + 7, 40_000):
        p = F.pad_blob(first, n)
        assert len(p) == n
        src[0].blobs[0] = p
        assert_same_batch(decode_histories(src), flatten(hs))
    with pytest.raises(AssertionError):
        F.pad_blob(first, len(first) - 1)
    evs, blob = F.many_events(20_000)
    assert len(blob) >= 20_000 and len(evs) > 100
    assert not F.can_pad(blob) and F.can_pad(first)
    h = WorkflowHistory(batches=[evs])
    assert_same_batch(decode_histories([WorkflowSource(blobs=[blob])]), flatten([h]))


# ---- the staging-window fixture: each edge it is built for, from window_path -------------------------------------
def test_window_path_restates_the_staging_loop():
    """Hand cases of the loop: a blob fits while ((b1 - 1) & ~15) + 32 <= lim, lim = s + 13 KB clipped to the
    wavefront's end; the first pending blob that does not fit is walked from HBM, a later one waits."""
    K = F.K_STAGE_BYTES
    assert K == 13 * 1024
    path, its = F.window_path([0, 100, 100, 300])
    assert [str(p) for p in path] == ["staged in window 0", "empty", "staged in window 0"] and its == [1]
    # 13296 bytes from a 16-aligned start fit with zero slack, one more byte does not
    path, _ = F.window_path([0, K - 16, K - 16 + 50, 2 * K + 100])
    assert (path[0].kind, path[0].slack) == ("staged", 0) and path[1].window == 1
    path, its = F.window_path([0, K - 15, K + 50])
    assert [p.kind for p in path] == ["hbm", "staged"] and its == [2]
    # an over-size blob in mid-wavefront: the small ones after it wait for their own window
    path, its = F.window_path([0, 200, 200 + 3 * K, 200 + 3 * K + 100])
    assert [(p.kind, p.window) for p in path] == [("staged", 0), ("hbm", 1), ("staged", 2)] and its == [3]
    # the last window is clipped to the end of the wavefront's bytes: a last blob under the window fits
    path, _ = F.window_path([0, 5])
    assert (path[0].kind, path[0].slack) == ("staged", 0)
    # a second wavefront starts its own windows
    path, its = F.window_path(list(range(0, 66 * 10, 10)))
    assert path[64].wave == 1 and path[64].lane == 0 and its == [1, 1]


def test_window_batch_reaches_every_edge():
    wb = F.window_batch()
    bs, path, R = wb.bs, wb.path, wb.roles
    off = bs.blob_off.astype(np.int64)
    assert 200 <= bs.n_blobs <= 260 and bs.n_blobs > 3 * 64
    hbm = [i for i, p in enumerate(path) if p.kind == "hbm"]
    # an HBM-walked blob at each residue of b0 mod 16
    assert {int(off[i]) % 16 for i in hbm} >= {0, 1, 8, 15}
    for name, r in (("hbm_res0", 0), ("hbm_res1", 1), ("hbm_res8", 8), ("hbm_res15", 15)):
        assert path[R[name]].kind == "hbm" and int(off[R[name]]) % 16 == r, name
    # one built by many_events, the others by pad_blob
    assert path[R["many_events"]].kind == "hbm" and not F.can_pad(bs.blob(R["many_events"]))
    assert F.can_pad(bs.blob(R["hbm_res1"]))
    # what the HBM-walked blobs hold
    assert set(hbm) & set(wb.has["act40"]) and R["hbm_res1"] in wb.has["act40"]
    assert set(hbm) & set(wb.has["prev_points"]) and R["hbm_res0"] in wb.has["prev_points"]
    assert set(hbm) & set(wb.has["checksum32"]) and R["hbm_res8"] in wb.has["checksum32"]
    # zero slack, and the same blob one 16-byte step longer
    p0, p16 = path[R["fit0"]], path[R["fit16"]]
    assert (p0.kind, p0.slack) == ("staged", 0)
    b1, s = int(off[R["fit0"] + 1]), int(off[R["fit0"]]) & ~15
    assert ((b1 - 1) & ~15) + 32 == s + F.K_STAGE_BYTES
    assert p16.kind == "hbm" and p16.slack == -16
    assert int(off[R["fit16"] + 1] - off[R["fit16"]]) == int(off[R["fit0"] + 1] - off[R["fit0"]]) + 16
    # an HBM-walked blob in mid-wavefront, small blobs after it in the same wavefront
    i = R["hbm_res15"]
    assert path[i].lane != 0
    after = [j for j in range(i + 1, (i // 64 + 1) * 64) if path[j].kind == "staged"]
    assert len(after) >= 5 and all(path[j].window > path[i].window for j in after)
    # a wavefront whose window is refilled at least three times
    assert max(wb.iterations) - 1 >= 3 and wb.iterations[path[i].wave] - 1 >= 3
    # an empty blob at a window boundary: the blob before it is the last of its window, the one after it the
    # first of the next
    e = R["edge_empty"]
    assert path[e].kind == "empty" and path[e - 1].kind == path[e + 1].kind == "staged"
    assert path[e + 1].window == path[e - 1].window + 1 and path[e - 1].wave == path[e + 1].wave
    assert not any(p.kind == "staged" and p.wave == path[e].wave and p.window == path[e - 1].window
                   for p in path[e + 1:])
    # the last blob HBM-walked, the buffer exactly n_bytes + CRR_INGEST_PAD
    from cadence_amd.ingest import INGEST_PAD
    assert hbm[-1] == bs.n_blobs - 1 and bs.bytes.size == bs.n_bytes + INGEST_PAD
    # one blob of 1 MB
    assert int(off[R["hbm_res8"] + 1] - off[R["hbm_res8"]]) == 1 << 20
    # (the figures the commit message quotes)
    print("window_batch: blobs", bs.n_blobs, "bytes", bs.n_bytes, "hbm-walked", len(hbm), "refills",
          sum(k - 1 for k in wb.iterations), "per wavefront", wb.iterations)


def test_window_batch_decodes_like_flatten():
    wb = F.window_batch()
    got = decode_histories(wb.bs.to_sources(), known_domains=KNOWN_DOMAINS)
    assert_same_batch(got, flatten(wb.hs, known_domains=set(KNOWN_DOMAINS)))


# ---- long and colliding keys -------------------------------------------------------------------------------------------
def test_str_hash_restatement_is_pinned():
    """Two values worked step by step from ingest_kernel.hip:136-144.
    "": the seed 0x811C9DC5 goes straight to the avalanche: ^>>16 0x811C1CD9, *0x85EBCA6B 0x5DB648B3, ^>>13
    0x5DB4A501, *0xC2B2AE35 0xAB3ED735, ^>>16 0xAB3E7C0B.
    "a": seed 0x811C9DC5 ^ 0x9E3779B1 = 0x1F2BE474; the step's low word (^0x61) * 16777619 = 0x27180D0F, its
    high word (^0) * 16777619 = 0x99DC8E9D; avalanche 0x99DC1741, 0x1702022B, 0x1702BA3B, 0xD12AA837,
    0xD12A791D."""
    assert F.str_hash_init(0) == 0x811C9DC5
    assert F.str_hash_init(1) == 0x811C9DC5 ^ 0x9E3779B1
    assert F.str_hash_step(0, 0) == 0
    assert F.str_hash_step(1, 0) == (16777619 * 16777619) & 0xFFFFFFFF
    assert F.str_hash(b"") == 0xAB3E7C0B
    assert F.str_hash(b"a") == 0xD12A791D
    # the tail is zero-padded and the length is in the seed: "a" and "a\0" differ
    assert F.str_hash(b"a") != F.str_hash(b"a\0")


def test_long_key_histories_cover_lengths_collisions_and_both_passes():
    hs = F.long_key_histories()
    st = F.key_statistics(hs)
    assert set(st["lengths"]) == set(F.KEY_LENGTHS) and min(st["lengths"].values()) >= 100
    assert st["longer_than_16"] > 1000 and st["colliding_pairs"] >= 100 and st["same_prefix_pairs"] > 1000
    # within a workflow: equal keys, keys differing only at the last byte, keys equal in their first 16 bytes
    n_equal = n_last = 0
    for h in hs:
        ks = F.workflow_keys(h)
        n_equal += len(ks) - len(set(ks))
        d = sorted(set(ks))
        n_last += sum(1 for a, b in zip(d, d[1:]) if len(a) == len(b) > 16 and a[:-1] == b[:-1])
    assert n_equal > 500 and n_last > 200
    # both interning passes: a wavefront per workflow (at most 64 events, under 64 batches, no previous reset
    # points) and a lane per workflow (the rest)
    n_ev = [len(h.events) for h in hs]
    has_prev = [any(isinstance(e.attrs.get("prev_auto_reset_points"), list) and e.attrs["prev_auto_reset_points"]
                    for e in h.events) for h in hs]
    wave = [n <= 64 and len(h.batches) < 64 and not p for n, h, p in zip(n_ev, hs, has_prev)]
    assert sum(wave) > 100 and sum(1 for w, n in zip(wave, n_ev) if not w and n > 64) >= 20
    assert sum(1 for w, p in zip(wave, has_prev) if not w and p) >= 20
    print("long_key_histories:", st)


def test_long_key_histories_decode_like_flatten():
    """And the helper's count of distinct byte strings per workflow is the number of key ids the host decoder
    assigns (ids 1..K in first-seen order)."""
    hs = F.long_key_histories()
    want = flatten(hs, known_domains=KNOWN)
    got = decode_histories(sources_of(hs), known_domains=KNOWN)
    assert_same_batch(got, want)
    cnt = got.wf["ev_count"].astype(np.int64)
    assert got.stride == 1 and got.wf["ev_begin"].tolist() == (np.cumsum(cnt) - cnt).tolist()   # canonical
    wf_idx = np.repeat(np.arange(got.n_wf), cnt)
    K = np.zeros(got.n_wf, np.int64)
    np.maximum.at(K, wf_idx, got.cols["key"][:int(cnt.sum())].astype(np.int64))
    st = (got.cols["etype"][:int(cnt.sum())] & abi.ETYPE_MASK) == ET.WorkflowExecutionStarted
    for x in np.nonzero(st)[0]:
        ss = got.start_side[int(got.cols["aux"][x])]
        c, o = max(int(ss["prev_reset_count"]), 0), int(ss["prev_reset_key_off"])
        if c:
            K[wf_idx[x]] = max(K[wf_idx[x]], int(got.reset_keys[o:o + c].max()))
    assert K.tolist() == [len(set(F.workflow_keys(h))) for h in hs]
    # the decoder's key table holds the long keys themselves
    assert sum(1 for k in set(keys_of(got)) if len(k) > 16) > 1000
