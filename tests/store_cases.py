"""Shared cases for the checksum generated for routed replication tasks (include/cadence_load_store.h), used on the
CPU (the host restatement) and on the GPU (the device against the host and against the same expected values).

Every expected value is ``oracle/checksum_py.encode_payload`` + ``zlib.crc32`` over the values the case wrote into
the blobs, the oracle's rows for the replayed part and ``add_or_update`` below (VersionHistory.AddOrUpdateItem in a
few lines); neither implementation under test takes part in it.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Optional, Sequence, Tuple

import numpy as np

from cadence_amd import abi, persisted, synth_mixed
from cadence_amd.flatten import LoadedStates, flatten
from cadence_amd.history import thrift_history_branch_token

import load_cases as lc
import ndc_load_cases as nc
import verify_cases as vc
from oracle import checksum_py
from resume_cases import KNOWN, split_histories

O = abi.StoreOutcome
S = abi.Status
EMPTY_VERSION = -24     # common.EmptyVersion


def add_or_update(items: Sequence[Tuple[int, int]], event_id: int, version: int):
    """NewVersionHistoryItem (versionHistory.go:37-43) then AddOrUpdateItem (:193-226): (items after, status)."""
    if event_id < 0 or (version < 0 and version != EMPTY_VERSION):
        return None, int(S.VH_INVALID_ITEM)
    items = [tuple(x) for x in items]
    if not items:
        return [(event_id, version)], 0
    last_id, last_version = items[-1]
    if version < last_version:
        return None, int(S.VH_LOWER_VERSION)
    if event_id <= last_id:
        return None, int(S.VH_EVENT_ID_NOT_INCREASING)
    if version > last_version:
        return items + [(event_id, version)], 0
    return items[:-1] + [(event_id, last_version)], 0


def row_of(payload: Optional[bytes], outcome: int, status: int = 0):
    return (vc.crc(payload), int(outcome), len(payload), int(status)) if payload is not None else (0, int(outcome), 0, int(status))


def payload_of_rows(ex, rows, sticky: str, current: int, histories) -> bytes:
    """The payload of a state given as an exec row and its live rows by table name."""
    return checksum_py.encode_payload(
        cancel_requested=bool(int(ex["flags"]) & abi.EXEC_CANCEL_REQUESTED), state=int(ex["state"]),
        last_first_event_id=int(ex["last_first_event_id"]), next_event_id=int(ex["next_event_id"]),
        last_processed_event_id=int(ex["last_processed_event"]), signal_count=int(ex["signal_count"]),
        decision_attempt=int(ex["decision_attempt"]), decision_version=int(ex["decision_version"]),
        decision_scheduled_id=int(ex["decision_schedule_id"]), decision_started_id=int(ex["decision_started_id"]),
        pending_timer_started_ids=rows["timer"]["started_id"], pending_activity_scheduled_ids=rows["act"]["schedule_id"],
        pending_signal_initiated_ids=rows["sig"]["initiated_id"], pending_req_cancel_initiated_ids=rows["rc"]["initiated_id"],
        pending_child_initiated_ids=rows["child"]["initiated_id"], sticky_task_list=sticky,
        version_histories=(current, [(b"" if t is None else bytes(t), [] if it is None else list(it)) for t, it in histories]))


@dataclasses.dataclass
class StoreCase:
    sbs: persisted.StateBlobSet
    tasks: np.ndarray                 # abi.REPL_TASK
    last_events: np.ndarray           # abi.LAST_EVENT
    results: np.ndarray               # abi.NDC_RESULT
    routes: np.ndarray                # abi.NDC_ROUTE
    after: Optional[LoadedStates]     # the post-replay states given to the host restatement
    want: np.ndarray                  # abi.STORE_ROW expected with ``after``
    want_without: np.ndarray          # ... and without it: every task on the current route is not resumed


def _without(want: np.ndarray, routes: np.ndarray, loaded_task: np.ndarray) -> np.ndarray:
    out = want.copy()
    sel = (routes["route"] == abi.ROUTE_APPLY_CURRENT) & loaded_task & (out["outcome"] != O.NO_ROUTE)
    out[sel] = np.array([(0, int(O.NOT_RESUMED), 0, 0)], abi.STORE_ROW)
    return out


# ---- hand-built states, hand-made decisions: every outcome ---------------------------------------------------
TOKEN_300 = bytes((11 * k + 3) & 0xFF for k in range(300))
ITEMS = [(5, 1), (19, 3)]
HAND_STATES = [
    dict(nei=20, sticky="", current=0, histories=[(lc.TOKEN, [(19, 3)])]),
    dict(nei=21, sticky="s", current=1, histories=[(None, ITEMS), (TOKEN_300, [(3, 1), (20, 4)])]),
    dict(nei=22, sticky="sticky-tl", current=0, histories=[(b"", [(21, 3)]), (b"other", []), (b"no-items", None)], pending=True),
    dict(nei=23, sticky="n" * 300, current=0, histories=[(lc.TOKEN, [(22, 5)]), (TOKEN_300[::-1], ITEMS)], pending=True),
    None,                                                                    # two execution blobs: does not load
    dict(nei=25, sticky="", current=2, histories=[(b"a", ITEMS), (None, None), (b"cur", [(4, 1), (24, 6)])]),
]


def _after_hand() -> LoadedStates:
    """Post-replay states written by hand for the hand states: workflow 0 and 1 and 5 replayed OK with rows of their own,
    workflow 2 ended with status 7, workflow 3 was not resumed."""
    n = len(HAND_STATES)
    ex = np.zeros(n, abi.EXEC_ROW)
    counts = {0: dict(act=2, timer=1, vh=2), 1: dict(child=1, rc=2, sig=1, vh=3), 2: dict(vh=1), 5: dict(act=1, vh=1)}
    n_f = {t[0]: t[4] for t in abi.TABLES}
    rows = {name: [] for name in abi.LOAD_ROW_TABLES}
    id_f = dict(act="schedule_id", timer="started_id", child="initiated_id", rc="initiated_id", sig="initiated_id")
    dtypes = {t[0]: t[1] for t in abi.TABLES}
    for w in range(n):
        if w not in counts:
            continue
        ex[w]["state"], ex[w]["next_event_id"], ex[w]["last_first_event_id"] = 1 + w % 2, 40 + w, 37 + w
        ex[w]["last_processed_event"], ex[w]["signal_count"], ex[w]["decision_attempt"] = 30 + w, w, w % 2
        ex[w]["decision_version"], ex[w]["decision_schedule_id"], ex[w]["decision_started_id"] = 7, 38 + w, abi.EMPTY_EVENT_ID
        ex[w]["flags"] = abi.EXEC_CANCEL_REQUESTED if w == 1 else 0
        ex[w]["status"] = 7 if w == 2 else 0
        for name in abi.LOAD_ROW_TABLES:
            k = counts[w].get(name, 0)
            ex[w][n_f[name]] = k
            r = np.zeros(k, dtypes[name])
            if name == "vh":
                r["event_id"], r["version"] = [10 * (j + 1) + w for j in range(k)], [2 * j + 1 for j in range(k)]
            elif name in id_f:
                r[id_f[name]] = [6 + 3 * j + w for j in range(k)]
            rows[name].append(r)
    mask = np.array([w in counts for w in range(n)])
    return LoadedStates(ex, {name: (np.concatenate(rows[name]) if rows[name] else np.zeros(0, dtypes[name])) for name in rows}, mask)


@functools.lru_cache(maxsize=None)
def hand_case() -> StoreCase:
    wfs = []
    for st in HAND_STATES:
        wfs.append((20, [lc.execution(lc.exec_blob()), lc.execution(lc.exec_blob())]) if st is None else vc.state(**st)[0])
    sbs = persisted.build_blob_set(wfs)
    after = _after_hand()
    offs = {name: np.cumsum(after.counts(name)) - after.counts(name) for name in after.rows}

    def after_rows(w):
        return {name: after.rows[name][int(offs[name][w]):int(offs[name][w]) + int(after.counts(name)[w])] for name in after.rows}

    def stored(w, histories=None, **over):
        st = dict(HAND_STATES[w], **over)
        hs = st["histories"] if histories is None else histories
        ids = vc.GOOD_IDS if st.get("pending") else {}
        return vc.payload(st["nei"], st["nei"], st["sticky"], st["current"], hs, **ids)

    def backfill(w, branch, e):
        hs = list(HAND_STATES[w]["histories"])
        items, status = add_or_update(hs[branch][1] or [], *e)
        if status:
            return row_of(None, O.VH_ERROR, status)
        hs[branch] = (hs[branch][0], items)
        return row_of(stored(w, hs), O.BACKFILLED)

    def applied(w):
        st = HAND_STATES[w]
        r = after_rows(w)
        hs = list(st["histories"])
        hs[st["current"]] = (hs[st["current"]][0], [(int(x["event_id"]), int(x["version"])) for x in r["vh"]])
        return row_of(payload_of_rows(after.exec[w], r, "", st["current"], hs), O.APPLIED)

    A, N, RB, BR, NONE = abi.ROUTE_APPLY_CURRENT, abi.ROUTE_NON_CURRENT, abi.ROUTE_REBUILD, abi.ROUTE_BAD_REQUEST, abi.ROUTE_NONE
    APP, NEW, DUP = abi.NDC_APPEND, abi.NDC_NEW_BRANCH, abi.NDC_DUPLICATE
    # (wf, route, action, branch index, last event, expected row)
    rows = [
        (1, N, APP, 0, (25, 7), backfill(1, 0, (25, 7))),                    # a higher version appends
        (1, N, APP, 0, (30, 3), backfill(1, 0, (30, 3))),                    # an equal version updates the last event ID
        (2, N, APP, 2, (4, 2), backfill(2, 2, (4, 2))),                      # Items absent: the empty branch takes the item
        (2, N, APP, 1, (4, EMPTY_VERSION), backfill(2, 1, (4, EMPTY_VERSION))),   # Items empty; EmptyVersion is a valid version
        (3, N, APP, 1, (20, 3), backfill(3, 1, (20, 3))),                    # a 300-byte sticky name and token
        (5, N, APP, 1, (0, 0), backfill(5, 1, (0, 0))),                      # neither token nor items, event ID 0
        (5, N, APP, 0, (1 << 40, 1 << 41), backfill(5, 0, (1 << 40, 1 << 41))),
        (1, N, APP, 0, (40, 2), row_of(None, O.VH_ERROR, S.VH_LOWER_VERSION)),
        (1, N, APP, 0, (40, EMPTY_VERSION), row_of(None, O.VH_ERROR, S.VH_LOWER_VERSION)),
        (1, N, APP, 0, (19, 3), row_of(None, O.VH_ERROR, S.VH_EVENT_ID_NOT_INCREASING)),
        (1, N, APP, 0, (10, 5), row_of(None, O.VH_ERROR, S.VH_EVENT_ID_NOT_INCREASING)),
        (1, N, APP, 0, (-1, 3), row_of(None, O.VH_ERROR, S.VH_INVALID_ITEM)),
        (2, N, APP, 2, (5, -2), row_of(None, O.VH_ERROR, S.VH_INVALID_ITEM)),
        (1, N, APP, 9, (-1, 3), row_of(None, O.VH_ERROR, S.VH_INVALID_ITEM)),   # NewVersionHistoryItem comes first
        (1, N, APP, 2, (25, 7), row_of(None, O.VH_ERROR, S.NDC_BAD_INDEX)),
        (1, N, APP, -1, (25, 7), row_of(None, O.VH_ERROR, S.NDC_BAD_INDEX)),
        (1, A, APP, 0, (25, 7), row_of(None, O.VH_ERROR, S.NDC_BAD_INDEX)),  # the current route, not the current branch
        (0, NONE, DUP, 0, (25, 7), row_of(None, O.NO_ROUTE)),
        (0, RB, APP, 0, (25, 7), row_of(None, O.NO_ROUTE)),
        (1, BR, APP, 0, (25, 7), row_of(None, O.NO_ROUTE)),
        (1, 77, APP, 0, (25, 7), row_of(None, O.NO_ROUTE)),
        (0, N, NEW, 1, (25, 7), row_of(None, O.NEW_BRANCH)),
        (0, A, NEW, 1, (25, 7), row_of(None, O.NEW_BRANCH)),
        (4, N, APP, 0, (25, 7), row_of(None, O.NOT_LOADED)),
        (4, A, APP, 0, (25, 7), row_of(None, O.NOT_LOADED)),
        (len(HAND_STATES), N, APP, 0, (25, 7), row_of(None, O.NOT_LOADED)),
        (0xFFFFFFFF, A, APP, 0, (25, 7), row_of(None, O.NOT_LOADED)),
        (0, A, APP, 0, (0, 0), applied(0)),
        (1, A, APP, 1, (0, 0), applied(1)),
        (5, A, APP, 2, (0, 0), applied(5)),
        (2, A, APP, 0, (0, 0), row_of(None, O.REPLAY_FAILED, 7)),
        (2, A, NEW, 3, (0, 0), row_of(None, O.REPLAY_FAILED, 7)),
        (3, A, APP, 0, (0, 0), row_of(None, O.NOT_RESUMED)),
        (3, A, NEW, 2, (0, 0), row_of(None, O.NOT_RESUMED)),
    ]
    n = len(rows)
    tasks, last = np.zeros(n, abi.REPL_TASK), np.zeros(n, abi.LAST_EVENT)
    results, routes = np.zeros(n, abi.NDC_RESULT), np.zeros(n, abi.NDC_ROUTE)
    want = np.zeros(n, abi.STORE_ROW)
    for k, (w, route, action, branch, e, row) in enumerate(rows):
        tasks[k]["wf"], last[k] = w, e
        results[k]["action"], results[k]["branch_index"], routes[k]["route"] = action, branch, route
        want[k] = row
    loaded_task = np.array([w < len(HAND_STATES) and HAND_STATES[w] is not None for w, *_ in rows])
    return StoreCase(sbs, tasks, last, results, routes, after, want, _without(want, routes, loaded_task))


# ---- ndc_load_cases.task_case with the expected decisions ---------------------------------------------------
def last_event_of(task, k: int):
    """A task's last event: its version is the task's, its ID at or past the first event's."""
    return int(task["first_event_id"]) + k % 3, int(task["first_event_version"])


def _written(w: int, local):
    """The branches of task_case's state w as they were written, absent fields read as Load makes them."""
    return [(b"token-%d-%d" % (w, b) if (w + b) % 5 else None, list(items)) for b, items in enumerate(local)]


@functools.lru_cache(maxsize=None)
def routed_case(n_states: int = 130, n_tasks: int = 400, seed: int = 3, big: bool = True) -> StoreCase:
    """ndc_load_cases.task_case of the same arguments with the expected decisions and the expected rows."""
    case = nc.task_case(n_states, n_tasks, seed, big)
    results, routes, _new = nc.expected_routes(case)
    n = case.tasks.shape[0]
    last = np.array([last_event_of(case.tasks[k], k) for k in range(n)], abi.LAST_EVENT)
    want = np.zeros(n, abi.STORE_ROW)
    for k in range(n):
        t = case.ndc_tasks[k]
        route, action = int(routes[k]["route"]), int(results[k]["action"])
        if t is None:
            want[k] = row_of(None, O.NOT_LOADED)
        elif route not in (abi.ROUTE_APPLY_CURRENT, abi.ROUTE_NON_CURRENT):
            want[k] = row_of(None, O.NO_ROUTE)
        elif route == abi.ROUTE_APPLY_CURRENT:
            want[k] = row_of(None, O.NOT_RESUMED)
        elif action == abi.NDC_NEW_BRANCH:
            want[k] = row_of(None, O.NEW_BRANCH)
        else:
            w, b = int(case.tasks[k]["wf"]), int(results[k]["branch_index"])
            cur, local = case.locals_[w]
            hs = _written(w, local)
            items, status = add_or_update(hs[b][1], int(last[k]["event_id"]), int(last[k]["version"]))
            if status:
                want[k] = row_of(None, O.VH_ERROR, status)
                continue
            hs[b] = (hs[b][0], items)
            ids = dict(acts=[5] if w % 3 >= 1 else [], timers=[7] if w % 3 == 2 else [])
            want[k] = row_of(vc.payload(20, 20, "", cur, hs, **ids), O.BACKFILLED)
    return StoreCase(case.sbs, case.tasks, last, results, routes, None, want, want)


# ---- replayed states: the setup of test_gpu_load_ndc.test_apply_current_tasks_resume_to_the_oracle -----------------
def vh_items(batch, res):
    loaded = res.to_loaded(batch)
    c = loaded.counts("vh")
    o = np.cumsum(c) - c
    rows = loaded.rows["vh"]
    return [[(int(r["event_id"]), int(r["version"])) for r in rows[int(o[w]):int(o[w]) + int(c[w])]] if loaded.mask[w] else None
            for w in range(c.shape[0])]


STALE = b"stale-branch-token"


@dataclasses.dataclass
class ReplayedCase:
    hs: list
    pre: list
    suf: list
    split: np.ndarray
    pre_b: object
    pre_r: object
    one_b: object                 # the whole histories flattened: its oracle replay is the state after the task
    one_r: object
    sbs: persisted.StateBlobSet
    branches: dict                # workflow -> (histories as encode_states takes them, current index)
    tasks: np.ndarray
    incoming: np.ndarray
    last_events: np.ndarray
    two_branch: np.ndarray        # bool per workflow
    tokens: list                  # per workflow: its own branch's token
    local: list                   # per workflow: its own branch's items before the task (None: not loadable)
    after: list                   # ... and after it


def replayed_case_of(hs, split_seed: int, second_every: int, shuffle_seed: int = 8, last_only: bool = True) -> ReplayedCase:
    """Histories split before a task, the prefixes persisted: every ``second_every``-th selected state gets a second
    branch; on a third of those that branch is current with a last version above the task's, so the task routes
    NON_CURRENT; on the others it is a stale branch ``[(1, v0)]`` in front of or behind the state's own,
    which stays current.  Every selected workflow gets one task: its suffix."""
    from oracle import oracle
    pre, suf, split = split_histories(hs, split_seed, last_only=last_only)
    pre_b, one_b = flatten(pre, known_domains=KNOWN), flatten(hs, known_domains=KNOWN)
    pre_r, one_r = oracle.replay(pre_b, 0), oracle.replay(one_b, 0)
    local, after = vh_items(pre_b, pre_r), vh_items(one_b, one_r)
    sel = np.array([bool(split[w]) and local[w] is not None and after[w] is not None for w in range(len(hs))])
    branches, two = {}, np.zeros(len(hs), bool)
    for i, w in enumerate(np.nonzero(sel)[0][::second_every]):
        if local[w][0][0] < 2:
            continue
        task_version = suf[w].batches[0][0].version
        if i % 3 == 0:
            # (it shares the first version with the state's own branch: FindLCAItem needs a joint point)
            branches[int(w)] = ([None, (STALE, [(1, local[w][0][1]), (2, task_version + 5)])], 1)
        else:
            branches[int(w)] = ([(STALE, [(1, local[w][0][1])]), None][::1 if i % 2 else -1], i % 2)
        two[w] = True
    sbs = persisted.encode_states(pre_b, pre_r, pre, shuffle_seed=shuffle_seed, branches=branches)
    tasks, incoming, last = np.zeros(int(sel.sum()), abi.REPL_TASK), [], np.zeros(int(sel.sum()), abi.LAST_EVENT)
    for k, w in enumerate(np.nonzero(sel)[0]):
        first, final = suf[w].batches[0][0], suf[w].batches[-1][-1]
        tasks[k] = (w, len(incoming), len(after[w]), 0, first.id, first.version)
        last[k] = (final.id, final.version)
        incoming.extend(after[w])
    order = np.random.default_rng(5).permutation(tasks.shape[0])
    loaded = pre_r.to_loaded(pre_b)
    tokens = []
    for w, h in enumerate(pre):
        src = int(loaded.exec[w]["token_src"])
        tokens.append(b"" if src == 0 else (thrift_history_branch_token(h.run_id, h.branch_id) if src == 1 else bytes(h.final_token)))
    return ReplayedCase(hs, pre, suf, split, pre_b, pre_r, one_b, one_r, sbs, branches, tasks[order],
                        np.array(incoming, abi.VH_ITEM), last[order], two, tokens, local, after)


@functools.lru_cache(maxsize=None)
def replayed_case() -> ReplayedCase:
    return replayed_case_of(synth_mixed.mixed_histories(64, 81, multi_version=True), 82, 2)


@functools.lru_cache(maxsize=None)
def replayed_case_large() -> ReplayedCase:
    """replayed_case's recipe over 1400 histories: 1400 states and 1366 tasks, so the loader's 1024-thread scans hold
    more than one element per thread and APPLIED and BACKFILLED tasks lie past task 1024."""
    return replayed_case_of(synth_mixed.mixed_histories(1400, 81, multi_version=True), 82, 2)


def histories_of(rc: ReplayedCase, w: int, own_items):
    """(current index, [(token, items)]) of workflow w with ``own_items`` on its own branch."""
    own = (rc.tokens[w], list(own_items))
    if w not in rc.branches:
        return 0, [own]
    hs, cur = rc.branches[w]
    return cur, [own if h is None else (h[0], list(h[1])) for h in hs]


def rows_of(loaded: LoadedStates, w: int):
    out = {}
    for name in loaded.rows:
        c = loaded.counts(name)
        o = int((np.cumsum(c) - c)[w])
        out[name] = loaded.rows[name][o:o + int(c[w])]
    return out


def decided(rc: ReplayedCase):
    """(results, routes) of the case's tasks: ``oracle.ndc_prepare`` on NdcTasks of the values written, then
    ndc_load_cases' restatement of prepareMutableState."""
    from oracle import oracle
    from cadence_amd import ndc
    tasks = []
    for t in rc.tasks:
        w, b = int(t["wf"]), int(t["incoming_begin"])
        cur, hs = histories_of(rc, w, rc.local[w])
        inc = [(int(x["event_id"]), int(x["version"])) for x in rc.incoming[b:b + int(t["incoming_count"])]]
        tasks.append(ndc.NdcTask([list(items) for _tok, items in hs], cur, inc, int(t["first_event_id"]), int(t["first_event_version"])))
    batch = ndc.pack(tasks)
    res, out = oracle.ndc_prepare(batch)
    routes = np.zeros(len(tasks), abi.NDC_ROUTE)
    for k, t in enumerate(tasks):
        routes[k] = nc.route_of(t, res[k], ndc.new_branch_items(batch, res, out, k))
    return res, routes


def expected_replayed(rc: ReplayedCase, routes: np.ndarray, results: np.ndarray, resumed: np.ndarray, after: LoadedStates) -> np.ndarray:
    """abi.STORE_ROW per task from the values written and the oracle's rows: APPLIED from ``after``, the oracle's
    replay of the task onto the state (canonical order, the exec rows of every resumed workflow kept), BACKFILLED
    from the persisted prefix state with the task's last event on its own branch.  ``resumed``: the workflows whose
    task was replayed."""
    before = rc.pre_r.to_loaded(rc.pre_b)
    want = np.zeros(rc.tasks.shape[0], abi.STORE_ROW)
    for k, t in enumerate(rc.tasks):
        w, route = int(t["wf"]), int(routes[k]["route"])
        own = 0 if w not in rc.branches else [i for i, h in enumerate(rc.branches[w][0]) if h is None][0]
        if route == abi.ROUTE_APPLY_CURRENT:
            if not resumed[w]:
                want[k] = row_of(None, O.NOT_RESUMED)
            elif int(after.exec[w]["status"]) != 0:
                want[k] = row_of(None, O.REPLAY_FAILED, int(after.exec[w]["status"]))
            else:
                r = rows_of(after, w)
                cur, hs = histories_of(rc, w, [(int(x["event_id"]), int(x["version"])) for x in r["vh"]])
                want[k] = row_of(payload_of_rows(after.exec[w], r, "", cur, hs), O.APPLIED)
        elif route == abi.ROUTE_NON_CURRENT and int(results[k]["action"]) == abi.NDC_APPEND:
            assert int(results[k]["branch_index"]) == own
            items, status = add_or_update(rc.local[w], int(rc.last_events[k]["event_id"]), int(rc.last_events[k]["version"]))
            assert status == 0
            cur, hs = histories_of(rc, w, items)
            want[k] = row_of(payload_of_rows(before.exec[w], rows_of(before, w), "", cur, hs), O.BACKFILLED)
        else:
            want[k] = row_of(None, O.NO_ROUTE if route != abi.ROUTE_NON_CURRENT else O.NEW_BRANCH)
    return want


def reencoded_applied(rc: ReplayedCase, applied: np.ndarray) -> persisted.StateBlobSet:
    """The states after their task as the store would hold them: the whole histories' replay persisted with each
    two-branch state's other branch beside the replay's items (``applied``: the workflows to keep)."""
    ok = rc.one_r.to_loaded(rc.one_b).mask
    assert ok[applied].all()
    return persisted.encode_states(rc.one_b, rc.one_r, rc.hs, shuffle_seed=3, branches={w: b for w, b in rc.branches.items() if applied[w]})
