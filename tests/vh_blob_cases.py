"""Shared cases for the VersionHistories blob generated for routed replication tasks
(include/cadence_load_store_vh.h), used on the CPU (the host restatement) and on the GPU (the device against the host
and against the same expected bytes).

Expected bytes come from neither implementation under test: they are ``persisted.encode_version_histories`` (the
Python writer) over the histories the case wrote into the blobs, changed by ``store_cases.add_or_update`` on the
backfill route and by the oracle's (or the hand-written) ``vh`` rows on the current route.
"""
from __future__ import annotations

import functools
import struct
from typing import List, Optional

import numpy as np

from cadence_amd import abi, persisted

import ndc_load_cases as nc
import store_cases as sc
import thrift_tree as tt
import verify_cases as vc

O = abi.StoreOutcome
GENERATED = (int(O.APPLIED), int(O.BACKFILLED))


def expected_blob(current: int, histories) -> bytes:
    """The blob Go stores: VersionHistory.ToInternalType makes every token and items slice non-nil, so every field
    is written (an absent token with length 0, absent items as an empty list)."""
    return persisted.encode_version_histories(current, [(b"" if t is None else bytes(t), [] if it is None else list(it))
                                                        for t, it in histories])


def blob_length(histories) -> int:
    """The closed form of the header: 17 + sum(16 + token + 23 * items)."""
    return 17 + sum(16 + len(t or b"") + 23 * len(it or []) for t, it in histories)


def parse(blob: bytes):
    """(current, [(token, [(event id, version)])]) of a stored blob, every field required to be present."""
    fields = tt.parse_blob(blob)
    assert [(t, i) for t, i, _ in fields] == [(tt.T_I32, 10), (tt.T_LIST, 20)]
    current = struct.unpack(">i", fields[0][2])[0]
    et, hs = fields[1][2]
    assert et == tt.T_STRUCT
    out = []
    for h in hs:
        assert [(t, i) for t, i, _ in h] == [(tt.T_STRING, 10), (tt.T_LIST, 20)]
        it_t, items = h[1][2]
        assert it_t == tt.T_STRUCT
        rows = []
        for it in items:
            assert [(t, i) for t, i, _ in it] == [(tt.T_I64, 10), (tt.T_I64, 20)]
            rows.append((struct.unpack(">q", it[0][2])[0], struct.unpack(">q", it[1][2])[0]))
        out.append((bytes(h[0][2]), rows))
    return current, out


def blobs_of(rows: np.ndarray, blob_off: np.ndarray, data: np.ndarray) -> List[bytes]:
    return [data[int(blob_off[k]):int(blob_off[k + 1])].tobytes() for k in range(rows.shape[0])]


def assert_layout(rows: np.ndarray, blob_off: np.ndarray, data: np.ndarray):
    """len is 0 exactly for the tasks that are not generated; blob_off is the exclusive prefix of len."""
    assert rows.dtype == abi.VH_BLOB_ROW and blob_off.dtype == np.uint64 and data.dtype == np.uint8
    assert blob_off.shape == (rows.shape[0] + 1,)
    gen = np.isin(rows["outcome"], GENERATED)
    assert ((rows["len"] == 0) == ~gen).all() and (rows["reserved"] == 0).all()
    want = np.concatenate([[0], np.cumsum(rows["len"].astype(np.uint64))]).astype(np.uint64)
    assert (blob_off == want).all() and data.shape == (int(want[-1]),)


def assert_blobs(rows, blob_off, data, want: List[Optional[bytes]], what=""):
    assert_layout(rows, blob_off, data)
    got = blobs_of(rows, blob_off, data)
    for k, w in enumerate(want):
        assert got[k] == (w or b""), f"{what} task {k}: {got[k].hex()} vs {(w or b'').hex()}"


# ---- store_cases.hand_case ---------------------------------------------------------------------------------------
def _vh_rows(after, w: int):
    return [(int(x["event_id"]), int(x["version"])) for x in sc.rows_of(after, w)["vh"]]


def hand_histories(c: sc.StoreCase, k: int, outcome: int):
    """(current, histories) task k of the hand case commits, given its expected outcome."""
    w, b = int(c.tasks[k]["wf"]), int(c.results[k]["branch_index"])
    st = sc.HAND_STATES[w]
    hs = [(t, None if it is None else list(it)) for t, it in st["histories"]]
    if outcome == O.BACKFILLED:
        items, status = sc.add_or_update(hs[b][1] or [], int(c.last_events[k]["event_id"]), int(c.last_events[k]["version"]))
        assert status == 0
        hs[b] = (hs[b][0], items)
    else:
        hs[st["current"]] = (hs[st["current"]][0], _vh_rows(c.after, w))
    return st["current"], hs


def hand_expected(c: sc.StoreCase, want: np.ndarray) -> List[Optional[bytes]]:
    return [expected_blob(*hand_histories(c, k, int(want[k]["outcome"]))) if int(want[k]["outcome"]) in GENERATED else None
            for k in range(want.shape[0])]


def hand_modes(c: sc.StoreCase, want: np.ndarray):
    """What the generated tasks of the hand case cover: the AddOrUpdateItem modes and the token / items shapes."""
    seen = set()
    for k in range(want.shape[0]):
        if int(want[k]["outcome"]) not in GENERATED:
            continue
        w, b = int(c.tasks[k]["wf"]), int(c.results[k]["branch_index"])
        for t, it in sc.HAND_STATES[w]["histories"]:
            seen.add("token absent" if t is None else "token empty" if t == b"" else "token 300" if len(t) == 300 else "token")
            seen.add("items absent" if it is None else "items")
        if int(want[k]["outcome"]) == O.BACKFILLED:
            before = sc.HAND_STATES[w]["histories"][b][1] or []
            e = (int(c.last_events[k]["event_id"]), int(c.last_events[k]["version"]))
            seen.add("takes" if not before else "updates" if e[1] == before[-1][1] else "appends")
    return seen


# ---- store_cases.routed_case -------------------------------------------------------------------------------------
def routed_histories(c: sc.StoreCase, k: int, n_states: int = 130, n_tasks: int = 400, seed: int = 3, big: bool = True):
    case = nc.task_case(n_states, n_tasks, seed, big)
    w, b = int(c.tasks[k]["wf"]), int(c.results[k]["branch_index"])
    cur, local = case.locals_[w]
    hs = sc._written(w, local)
    items, status = sc.add_or_update(hs[b][1], int(c.last_events[k]["event_id"]), int(c.last_events[k]["version"]))
    assert status == 0
    hs[b] = (hs[b][0], items)
    return cur, hs


def routed_expected(c: sc.StoreCase, n_states: int = 130, n_tasks: int = 400, seed: int = 3, big: bool = True
                    ) -> List[Optional[bytes]]:
    """The blobs expected for ``c = store_cases.routed_case(...)`` of the same arguments."""
    return [expected_blob(*routed_histories(c, k, n_states, n_tasks, seed, big)) if int(c.want[k]["outcome"]) in GENERATED else None
            for k in range(c.want.shape[0])]


# ---- store_cases.replayed_case: the oracle's rows ------------------------------------------------------------------
def replayed_expected(rc: sc.ReplayedCase, want: np.ndarray, after) -> List[Optional[bytes]]:
    """``want``: store_cases.expected_replayed's rows (the outcome per task); ``after``: the oracle's replay of the
    tasks (canonical workflow order)."""
    out = []
    for k, t in enumerate(rc.tasks):
        w, outcome = int(t["wf"]), int(want[k]["outcome"])
        if outcome == O.APPLIED:
            out.append(expected_blob(*sc.histories_of(rc, w, _vh_rows(after, w))))
        elif outcome == O.BACKFILLED:
            items, status = sc.add_or_update(rc.local[w], int(rc.last_events[k]["event_id"]), int(rc.last_events[k]["version"]))
            assert status == 0
            out.append(expected_blob(*sc.histories_of(rc, w, items)))
        else:
            out.append(None)
    return out


# ---- one large state ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large_case():
    """A branch of 230 items behind a 300-byte token and a second branch: a blob of about 5.7 KB, which spans several
    wavefronts' chunks and puts an item seam at every offset inside a 16-byte chunk (23 is odd).  Three tasks: a
    backfill onto the long branch, one onto the short one, and one that is refused between them.
    -> (StoreCase-like tuple of arrays, expected blobs)."""
    long_items = [(3 * j + 2, 1 + j // 40) for j in range(230)]
    hs = [(sc.TOKEN_300, long_items), (b"second", [(4, 1), (9, 2)])]
    sbs = persisted.build_blob_set([vc.state(nei=700, current=0, histories=hs)[0]])
    n = 3
    tasks, last = np.zeros(n, abi.REPL_TASK), np.zeros(n, abi.LAST_EVENT)
    results, routes = np.zeros(n, abi.NDC_RESULT), np.zeros(n, abi.NDC_ROUTE)
    spec = [(0, (900, 9)), (0, (1, 1)), (1, (12, 2))]      # appends; a lower version: refused; updates
    want = []
    for k, (b, e) in enumerate(spec):
        last[k] = e
        results[k]["action"], results[k]["branch_index"], routes[k]["route"] = abi.NDC_APPEND, b, abi.ROUTE_NON_CURRENT
        items, status = sc.add_or_update(hs[b][1], *e)
        if status:
            want.append(None)
            continue
        new = list(hs)
        new[b] = (hs[b][0], items)
        want.append(expected_blob(0, new))
    return (sbs, tasks, last, results, routes), want


# ---- seams: conditions on a result, asserted so that a case cannot silently stop covering them -------------------
def assert_seams(rows: np.ndarray, blob_off: np.ndarray):
    """A blob is at least 33 bytes, so two non-empty blobs never begin in one 16-byte chunk: what a chunk can hold
    is the tail of one blob, the boundaries of the zero-length tasks behind it and the head of the next."""
    gen = np.nonzero(rows["len"] > 0)[0]
    starts = blob_off[gen].astype(np.int64)
    assert set(int(s) % 16 for s in starts) == set(range(16)), "the blob starts do not cover every residue mod 16"
    # a chunk that holds two or more task boundaries strictly inside it: one blob's tail, the next one's head
    inner = blob_off[1:-1].astype(np.int64)
    inner = inner[inner % 16 != 0]
    assert inner.size and np.bincount(inner // 16).max() >= 2, "no chunk holds two task boundaries"
    # three or more zero-length tasks in a row between two generated ones
    assert (np.diff(gen) >= 4).any(), "no run of three zero-length tasks between generated ones"


@functools.lru_cache(maxsize=None)
def seam_case():
    """States whose blobs are short and of many lengths (one branch with a token of 0..40 bytes, or none, and no items
    before the task), each with one backfill task, and runs of three refused tasks between them: the blob starts
    take every residue mod 16 and several chunks hold two boundaries or more (a 56-byte blob beside a 57-byte one).
    -> ((sbs, tasks, last, results, routes), expected blobs)."""
    wfs, hs_of = [], []
    for i in range(48):
        tok = None if i % 7 == 3 else bytes((5 * i + k) & 0xFF for k in range(i % 41))
        hs = [(tok, None if i % 2 else [])]
        if i % 5 == 0:
            hs.append((b"b", [(2, 1)]))
        wfs.append(vc.state(nei=30 + i, current=0, histories=hs)[0])
        hs_of.append(hs)
    sbs = persisted.build_blob_set(wfs)
    rows, want = [], []
    for i, hs in enumerate(hs_of):
        new = list(hs)
        new[0] = (hs[0][0], [(7 + i, 3)])
        rows.append((i, abi.ROUTE_NON_CURRENT, abi.NDC_APPEND, 0, (7 + i, 3)))
        want.append(expected_blob(0, new))
        if i % 6 == 2:      # three tasks in a row that generate nothing
            rows += [(i, abi.ROUTE_REBUILD, abi.NDC_APPEND, 0, (1, 1)), (i, abi.ROUTE_NON_CURRENT, abi.NDC_NEW_BRANCH, 1, (1, 1)),
                     (i, abi.ROUTE_NON_CURRENT, abi.NDC_APPEND, 9, (1, 1))]
            want += [None, None, None]
    n = len(rows)
    tasks, last = np.zeros(n, abi.REPL_TASK), np.zeros(n, abi.LAST_EVENT)
    results, routes = np.zeros(n, abi.NDC_RESULT), np.zeros(n, abi.NDC_ROUTE)
    for k, (w, route, action, b, e) in enumerate(rows):
        tasks[k]["wf"], last[k] = w, e
        results[k]["action"], results[k]["branch_index"], routes[k]["route"] = action, b, route
    return (sbs, tasks, last, results, routes), want


# ---- round trip: the generated blob as field 122, the generated checksum as stored -------------------------------
def with_vh_blob(workflow, blob: bytes):
    """A ``build_blob_set`` workflow with its execution blob's VersionHistories (field 122) replaced by ``blob``."""
    nei, blobs = workflow
    out = []
    for kind, bid, aux, s, raw in blobs:
        if kind == abi.STATE_EXECUTION:
            fields = tt._R(raw).value(tt.T_STRUCT)
            assert sum(1 for f in fields if f[1] == 122) == 1
            fields = [[t, i, blob if i == 122 else v] for t, i, v in fields]
            buf = bytearray()
            tt._w(buf, tt.T_STRUCT, fields)
            raw = bytes(buf)
        out.append((kind, bid, aux, s, raw))
    return nei, out


def stored_of(value: int):
    return abi.CHECKSUM_PAYLOAD_V1, abi.CHECKSUM_FLAVOR_CRC32, int(value).to_bytes(4, "big")
