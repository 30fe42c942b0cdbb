"""Shared cases for the checksum verification of loaded states (include/cadence_load_verify.h), used on the CPU
(the host restatement) and on the GPU (the device against the host).

Every expected value is ``oracle/checksum_py.encode_payload`` + ``zlib.crc32`` fed with the very values the case
put into the blobs; neither implementation under test takes part in it.
"""
from __future__ import annotations

import functools
import struct
import zlib
from typing import List, Optional, Sequence

import numpy as np

from cadence_amd import abi, persisted
from cadence_amd.history import thrift_history_branch_token
from cadence_amd.thrift_codec import T_LIST, T_STRUCT, W

import load_cases as lc
from oracle import checksum_py

LAST_UPDATED = 1_600_000_000_500_000_000      # persisted.execution_values' LastUpdatedTimeNanos
V1, CRC32 = abi.CHECKSUM_PAYLOAD_V1, abi.CHECKSUM_FLAVOR_CRC32
DEFAULT_HISTORIES = ((lc.TOKEN, ((19, 3),)),)
# (timers' StartedIDs, activities' ScheduleIDs, signals, request-cancels, children) of lc.good_workflow
GOOD_IDS = dict(timers=[7], acts=[5], sigs=[12], rcs=[11], children=[9])


def encode_vh(current: int, histories: Sequence) -> bytes:
    """persisted.encode_version_histories, but a history's token or items may be None: the field is left out."""
    w = W()
    w.b += b"\x59"
    w.i32(10, current)
    w.field(T_LIST, 20)
    w.b += bytes([T_STRUCT]) + struct.pack(">i", len(histories))
    for token, items in histories:
        if token is not None:
            w.string(10, token)
        if items is not None:
            w.field(T_LIST, 20)
            w.b += bytes([T_STRUCT]) + struct.pack(">i", len(items))
            for eid, ver in items:
                w.i64(10, eid)
                w.i64(20, ver)
                w.b += b"\x00"
        w.b += b"\x00"
    w.b += b"\x00"
    return bytes(w.b)


def payload(nei: int, exec_nei: int, sticky: str = "", current: int = 0, histories: Sequence = DEFAULT_HISTORIES,
            timers=(), acts=(), sigs=(), rcs=(), children=()) -> bytes:
    """The payload of a state built around ``lc.exec_blob(nei=exec_nei)`` whose next_event_id column is ``nei``
    (the scalar values are exec_blob's own)."""
    return checksum_py.encode_payload(
        cancel_requested=False, state=1, last_first_event_id=exec_nei - 2, next_event_id=nei,
        last_processed_event_id=exec_nei - 5, signal_count=2, decision_attempt=0, decision_version=3,
        decision_scheduled_id=exec_nei - 2, decision_started_id=abi.EMPTY_EVENT_ID,
        pending_timer_started_ids=timers, pending_activity_scheduled_ids=acts, pending_signal_initiated_ids=sigs,
        pending_req_cancel_initiated_ids=rcs, pending_child_initiated_ids=children, sticky_task_list=sticky,
        # VersionHistory.ToInternalType makes the token and the items: an absent one is empty, never nil
        version_histories=(current, [(b"" if t is None else bytes(t), [] if it is None else list(it)) for t, it in histories]))


def crc(p: bytes) -> int:
    return zlib.crc32(p) & 0xFFFFFFFF


def state(nei: int = 20, sticky: str = "", current: int = 0, histories: Sequence = DEFAULT_HISTORIES, pending: bool = False,
          points=(), **over):
    """-> (a workflow for build_blob_set, its expected payload): an execution blob with the given sticky task list
    and version histories; ``pending``: with lc.good_workflow's pending entries."""
    raw = lc.exec_blob(nei=nei, points=list(points), StickyTaskList=sticky, VersionHistories=encode_vh(current, histories), **over)
    blobs = [lc.execution(raw)]
    ids = {}
    if pending:
        blobs += [lc.activity_blob(5, "a5"), lc.timer_blob("t7", 7), lc.child_blob(9, 10), lc.initiated_blob(11, False),
                  lc.initiated_blob(12, True)]
        ids = GOOD_IDS
    return (nei, blobs), payload(nei, nei, sticky, current, histories, **ids)


@functools.lru_cache(maxsize=None)
def _batch(name: str):
    """-> (blob set, expected payload per workflow -- None: the workflow does not load)."""
    items = ((5, 1), (19, 3))
    if name == "plain":
        cases = [state()]
    elif name == "sticky":
        cases = [state(nei=30 + n, sticky="s" * n) for n in (0, 1, 9, 300)]
    elif name == "branches":
        cases = []
        for count, current in ((1, 0), (2, 0), (2, 1), (5, 0), (5, 2), (5, 4)):
            hs = [(b"token-%d" % b, [(3 + b, b), (10 + b, b + 1)][:1 + b % 2]) for b in range(count)]
            cases.append(state(nei=40 + len(cases), current=current, histories=hs))
        for n in (0, 95, 96, 97):
            tok = bytes((7 * k + n) & 0xFF for k in range(n))
            cases.append(state(nei=50, histories=[(tok, items)]))
            cases.append(state(nei=51, current=1, histories=[(b"x", [(1, 0)]), (tok, items), (tok[::-1], [(2, 2)])]))
        cases.append(state(nei=60, current=1, histories=[(b"with-no-items", []), (lc.TOKEN, items)]))
        cases.append(state(nei=61, current=0, histories=[(lc.TOKEN, []), (b"other", items)]))
        cases.append(state(nei=62, current=1, histories=[(None, items), (lc.TOKEN, items)]))
        cases.append(state(nei=63, current=0, histories=[(None, items)]))
        cases.append(state(nei=64, current=0, histories=[(lc.TOKEN, None), (None, None)]))
    elif name == "pending":
        big = lc.big_workflow()
        ids = dict(acts=[100 + 2 * ((k * 37) % 65) for k in range(65)], timers=[300 - k for k in range(5)])
        cases = [state(pending=True), (big, payload(400, 400, **ids)), state(nei=21, pending=True, sticky="sticky-tl")]
        # the same maps beside a sticky name and three branches
        raw = lc.exec_blob(nei=400, StickyTaskList="big-sticky", VersionHistories=encode_vh(2, [(b"a", items), (b"", []), (lc.TOKEN, items)]))
        blobs = [b for b in big[1] if b[0] != abi.STATE_EXECUTION]
        blobs.insert(11, lc.execution(raw))
        cases.append(((401, blobs), payload(401, 400, "big-sticky", 2, [(b"a", items), (b"", []), (lc.TOKEN, items)], **ids)))
    elif name == "outcomes":
        cases = [state(nei=70 + i) for i in range(7)]
        cases.append(((20, [lc.execution(lc.exec_blob()), lc.execution(lc.exec_blob())]), None))   # does not load
        cases += [state(nei=80 + i, sticky="tl") for i in range(3)]
    elif name.startswith("n_"):
        cases = [variant(i) for i in range(int(name[2:]))]
    else:
        raise KeyError(name)
    return persisted.build_blob_set([c[0] for c in cases]), [c[1] for c in cases]


def variant(i: int):
    """lc.good_workflow(i) with a sticky name and branch shapes that vary with i."""
    tok = bytes((i + k) & 0xFF for k in range(90 + i % 13))
    hs = [[(lc.TOKEN, ((19, 3),))], [(b"decoy", [(1, 0), (7, 3)]), (tok, [(19, 3)])], [(tok, [(4, 1), (19, 3)]), (None, []), (b"z", [(2, 2)])]][i % 3]
    return state(sticky=["", "s", "sticky-task-list-%d" % i][(i // 3) % 3], current=[0, 1, 0][i % 3], histories=hs, pending=True,
                 points=[("bin-%d" % i, True)])


BATCHES = ["plain", "sticky", "branches", "pending", "outcomes"]
SIZES = [1, 63, 64, 65, 257]


def batch(name: str):
    return _batch(name)


def expected_computed(payloads: List[Optional[bytes]]) -> np.ndarray:
    """abi.VERIFY_ROW's computed / payload_len per workflow; zeros where the workflow does not load."""
    out = np.zeros(len(payloads), abi.VERIFY_ROW)
    for w, p in enumerate(payloads):
        if p is not None:
            out["computed"][w], out["payload_len"][w] = crc(p), len(p)
    return out


def right_checksums(payloads) -> np.ndarray:
    """What the store holds for states written with their right checksum."""
    return persisted.stored_checksums([None if p is None else (V1, CRC32, checksum_py.checksum_value(p)) for p in payloads])


def outcome_matrix():
    """-> (blob set, payloads, stored, expected outcomes) of the "outcomes" batch (invalidate-before off)."""
    sbs, payloads = batch("outcomes")
    O = abi.VerifyOutcome
    good = [checksum_py.checksum_value(p) if p is not None else b"\0\0\0\0" for p in payloads]
    one_bit = struct.pack(">I", struct.unpack(">I", good[1])[0] ^ 0x00010000)
    rows = [((V1, CRC32, good[0]), O.MATCH),
            ((V1, CRC32, one_bit), O.MISMATCH),
            ((V1, CRC32, b""), O.NONE),
            ((V1, CRC32, good[3][:3]), O.MISMATCH),
            ((2, CRC32, good[4]), O.BAD_VERSION),
            ((V1, 0, good[5]), O.BAD_FLAVOR),
            ((0, 2, good[6]), O.BAD_VERSION),
            ((V1, CRC32, good[7]), O.NOT_LOADED),
            ((V1, CRC32, good[8]), O.MATCH),
            ((V1, CRC32, good[9] + b"\0"), O.MISMATCH),
            (None, O.NONE)]
    assert len(rows) == sbs.n_wf
    return sbs, payloads, persisted.stored_checksums([r[0] for r in rows]), np.array([int(r[1]) for r in rows], np.int32)


@functools.lru_cache(maxsize=None)
def replayed_case():
    """lc.prefix_case(3000, 61) persisted with every 7th loadable state sticky and every 11th multi-branch:
    (blob set, payload per workflow or None, the masks: loadable / sticky / multi-branch, the prefix replay)."""
    _hs, pre, _suf, _mask, pre_b, pre_r = lc.prefix_case(3000, 61)
    loaded = pre_r.to_loaded(pre_b)
    ok = np.nonzero(loaded.mask)[0]
    sticky, multi = set(ok[::7].tolist()), set(ok[::11].tolist())
    sbs = persisted.encode_states(pre_b, pre_r, pre, shuffle_seed=9, sticky=ok[::7], multi_branch=ok[::11])
    offs = {k: np.cumsum(loaded.counts(k)) - loaded.counts(k) for k in loaded.rows}
    payloads: List[Optional[bytes]] = []
    for w, h in enumerate(pre):
        if not loaded.mask[w]:
            payloads.append(None)
            continue
        ex = loaded.exec[w]

        def rows(name, n_f):
            o = int(offs[name][w])
            return loaded.rows[name][o:o + int(ex[n_f])]

        src = int(ex["token_src"])
        token = b"" if src == 0 else (thrift_history_branch_token(h.run_id, h.branch_id) if src == 1 else bytes(h.final_token))
        hist = [(token, [(int(r["event_id"]), int(r["version"])) for r in rows("vh", "n_vh_items")])]
        current = 0
        if w in multi:   # persisted.execution_values' decoy branch, in front of the current one
            hist = [(b"decoy-branch-token", [(1, 0), (7, 3)])] + hist
            current = 1
        payloads.append(checksum_py.encode_payload(
            cancel_requested=bool(int(ex["flags"]) & abi.EXEC_CANCEL_REQUESTED), state=int(ex["state"]),
            last_first_event_id=int(ex["last_first_event_id"]), next_event_id=int(ex["next_event_id"]),
            last_processed_event_id=int(ex["last_processed_event"]), signal_count=int(ex["signal_count"]),
            decision_attempt=int(ex["decision_attempt"]), decision_version=int(ex["decision_version"]),
            decision_scheduled_id=int(ex["decision_schedule_id"]), decision_started_id=int(ex["decision_started_id"]),
            pending_timer_started_ids=rows("timer", "n_timer")["started_id"],
            pending_activity_scheduled_ids=rows("act", "n_activity")["schedule_id"],
            pending_signal_initiated_ids=rows("sig", "n_signal")["initiated_id"],
            pending_req_cancel_initiated_ids=rows("rc", "n_rc")["initiated_id"],
            pending_child_initiated_ids=rows("child", "n_child")["initiated_id"],
            sticky_task_list="sticky-tl" if w in sticky else "", version_histories=(current, hist)))
    is_sticky = np.array([w in sticky for w in range(len(pre))])
    is_multi = np.array([w in multi for w in range(len(pre))])
    return sbs, payloads, loaded.mask.copy(), is_sticky, is_multi, pre_r


def check_replayed(got: np.ndarray):
    """The assertions of the replayed-states case on a result array (host or device): every loaded-OK workflow."""
    sbs, payloads, ok, is_sticky, is_multi, pre_r = replayed_case()
    assert (ok & is_sticky).sum() > 100 and (ok & is_multi).sum() > 100
    want = expected_computed(payloads)
    plain = ok & ~is_sticky & ~is_multi
    assert plain.sum() > 1000
    bad = np.nonzero(plain & (got["computed"] != pre_r.exec["checksum"]))[0]
    assert bad.size == 0, f"unflagged: {bad.size} differ from the replay's checksum, first {bad[:5]}"
    for what, sel in (("unflagged", plain), ("sticky", ok & is_sticky), ("multi-branch", ok & is_multi), ("all", ok)):
        for f in ("computed", "payload_len"):
            bad = np.nonzero(sel & (got[f] != want[f]))[0]
            assert bad.size == 0, f"{what}: {f} of {bad.size} workflows differ, first {bad[:5]}: {got[f][bad[:5]]} vs {want[f][bad[:5]]}"
    assert (got["outcome"][ok] == abi.VerifyOutcome.MATCH).all()
    assert (got["outcome"][~ok] == abi.VerifyOutcome.NOT_LOADED).all()
    assert (got["computed"][~ok] == 0).all() and (got["payload_len"][~ok] == 0).all() and (got["reserved"] == 0).all()
