"""Shared cases for the pending-entry mutation of a committed replication task (include/cadence_load_mutation.h), used
on the CPU (the host restatement) and on the GPU (the device against the host and against the same expected values).

``classify`` is the header's semantics restated in Python over sets and dictionaries -- matching by key, no merge walk
-- so neither implementation under test takes part in an expected value.  The state before is the expected loaded
image (``load_cases.expected_image``) for the replayed cases and the host loader's image for the hand states (the
loader is pinned by test_load_states, it is not what these tests are about); the state after is the oracle's resumed
replay, or rows written by hand.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional

import numpy as np

from cadence_amd import abi, persisted
from cadence_amd.flatten import LoadedStates, flatten

import load_cases as lc
import store_cases as sc
from resume_cases import KNOWN

O = abi.StoreOutcome
MAPS = abi.MUTATION_MAPS
DTYPES = {t[0]: t[1] for t in abi.TABLES}
COUNT_F = {t[0]: t[4] for t in abi.TABLES}
# what an entry is matched by: the store's key column
KEY_F = dict(act="schedule_id", timer="key", child="initiated_id", rc="initiated_id", sig="initiated_id")
# the fields that are not persisted: derived by Load, or padding
DERIVED = dict(act=("last_hb_timeout_vis_s",), timer=(), child=("reserved",), rc=(), sig=())


def same_persisted(name: str, a, b) -> bool:
    for f in DTYPES[name].names:
        if f in DERIVED[name]:
            continue
        x, y = int(a[f]), int(b[f])
        if name == "act" and f == "flags":
            x, y = x & ~abi.ROW_MAPPED, y & ~abi.ROW_MAPPED
        if x != y:
            return False
    return True


def classify(name: str, before: np.ndarray, after: np.ndarray):
    """(indices into ``after`` of the rows to upsert, the keys to delete in the order of ``before``, the indices of
    the untouched rows, of the new rows, of the changed rows)."""
    kf = KEY_F[name]
    old = {int(r[kf]): r for r in before}
    assert len(old) == before.shape[0] and len(set(int(r[kf]) for r in after)) == after.shape[0]
    new = [j for j, r in enumerate(after) if int(r[kf]) not in old]
    changed = [j for j, r in enumerate(after) if int(r[kf]) in old and not same_persisted(name, old[int(r[kf])], r)]
    untouched = [j for j, r in enumerate(after) if int(r[kf]) in old and same_persisted(name, old[int(r[kf])], r)]
    live = set(int(r[kf]) for r in after)
    deleted = [int(r[kf]) for r in before if int(r[kf]) not in live]
    return sorted(new + changed), deleted, untouched, new, changed


def reset_points_differ(before: np.ndarray, after: np.ndarray) -> bool:
    return before.shape[0] != after.shape[0] or before.tobytes() != after.tobytes()


@dataclasses.dataclass
class Tally:
    """What the expected mutations of the APPLIED tasks hold, per map."""
    new: Dict[str, int]
    changed: Dict[str, int]
    deleted: Dict[str, int]
    untouched: Dict[str, int]
    restarted: int = 0            # TimerIDs live before and after under another started_id
    status_only: int = 0          # timers upserted whose only persisted difference is task_status
    applied_tasks: List[int] = dataclasses.field(default_factory=list)


def expected_mutation(tasks: np.ndarray, store_rows: np.ndarray, before: LoadedStates, after: Optional[LoadedStates]):
    """(persisted.Mutation, Tally) for tasks whose expected ``abi.STORE_ROW`` rows are ``store_rows`` (their outcome and
    status are the mutation's), from the states before and after in canonical workflow order."""
    n = tasks.shape[0]
    rows = np.zeros(n, abi.MUTATION_ROW)
    ex, up, de = [], {m: [] for m in MAPS}, {m: [] for m in MAPS}
    n_up, n_de = {m: 0 for m in MAPS}, {m: 0 for m in MAPS}
    tally = Tally(*({m: 0 for m in MAPS} for _ in range(4)))
    for k in range(n):
        rows[k]["outcome"], rows[k]["status"] = store_rows[k]["outcome"], store_rows[k]["status"]
        rows[k]["exec_index"] = abi.MUTATION_NO_EXEC
        applied = int(rows[k]["outcome"]) == O.APPLIED
        if applied:
            w = int(tasks[k]["wf"])
            B, A = sc.rows_of(before, w), sc.rows_of(after, w)
            rows[k]["exec_index"] = len(ex)
            ex.append(after.exec[w])
            if reset_points_differ(B["rp"], A["rp"]):
                rows[k]["flags"] = abi.MUTATION_RESET_POINTS_CHANGED
            tally.applied_tasks.append(k)
        for t, m in enumerate(MAPS):
            rows[k]["map"][t]["upsert_begin"], rows[k]["map"][t]["delete_begin"] = n_up[m], n_de[m]
            if not applied:
                continue
            ups, dels, untouched, new, changed = classify(m, B[m], A[m])
            rows[k]["map"][t]["n_upsert"], rows[k]["map"][t]["n_delete"] = len(ups), len(dels)
            up[m].append(A[m][ups])
            de[m].append(np.array(dels, np.int64))
            n_up[m] += len(ups)
            n_de[m] += len(dels)
            tally.new[m] += len(new)
            tally.changed[m] += len(changed)
            tally.deleted[m] += len(dels)
            tally.untouched[m] += len(untouched)
            if m == "timer":
                old = {int(r["key"]): r for r in B[m]}
                for j in changed:
                    r, o = A[m][j], old[int(A[m][j]["key"])]
                    if int(r["started_id"]) != int(o["started_id"]):
                        tally.restarted += 1
                    elif all(int(r[f]) == int(o[f]) for f in r.dtype.names if f != "task_status"):
                        tally.status_only += 1

    def cat(parts, dt):
        return np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    m = persisted.Mutation(rows, np.array(ex, abi.EXEC_ROW) if ex else np.zeros(0, abi.EXEC_ROW),
                           {x: cat(up[x], DTYPES[x]) for x in MAPS}, {x: cat(de[x], np.int64) for x in MAPS})
    return m, tally


def assert_mutation(got: persisted.Mutation, want: persisted.Mutation, what: str = ""):
    for f in ("outcome", "status", "flags", "exec_index"):
        bad = np.nonzero(got.rows[f] != want.rows[f])[0]
        assert bad.size == 0, f"{what} rows.{f}: tasks {bad[:5]}: {got.rows[f][bad[:5]]} vs {want.rows[f][bad[:5]]}"
    for f in abi.MUTATION_MAP.names:
        bad = np.nonzero((got.rows["map"][f] != want.rows["map"][f]).any(axis=1))[0]
        assert bad.size == 0, f"{what} rows.map.{f}: tasks {bad[:5]}: {got.rows['map'][f][bad[:5]]} vs {want.rows['map'][f][bad[:5]]}"
    a, b = got.image_bytes(), want.image_bytes()
    for f in a:
        assert len(a[f]) == len(b[f]), f"{what} {f}: {len(a[f])} bytes vs {len(b[f])}"
        assert a[f] == b[f], f"{what} {f} differs"


# ---- hand states: every classification per map ------------------------------------------------------------------
def _hand_state(i: int):
    pts = [("bin-a", True), ("bin-b", False)]
    return (40, [lc.execution(lc.exec_blob(nei=40, items=((39, 3),), points=pts)),
                 lc.activity_blob(5, "a5"), lc.activity_blob(6, "a6"), lc.activity_blob(8, "a8"),
                 lc.timer_blob("t7", 7), lc.timer_blob("t9", 9), lc.timer_blob("t11", 11), lc.timer_blob("t13", 13),
                 lc.child_blob(9), lc.child_blob(13, 14), lc.child_blob(17),
                 lc.initiated_blob(11, False), lc.initiated_blob(15, False),
                 lc.initiated_blob(12, True), lc.initiated_blob(16, True)])


@dataclasses.dataclass
class HandCase:
    sbs: persisted.StateBlobSet
    tasks: np.ndarray
    last_events: np.ndarray
    results: np.ndarray
    routes: np.ndarray
    before: LoadedStates
    after: LoadedStates
    store_rows: np.ndarray        # the expected outcome and status per task
    want: Dict[int, dict]         # workflow -> map -> (upserted keys, deleted keys), written out by hand


def _new_row(name, **kw):
    r = np.zeros(1, DTYPES[name])
    for k, v in kw.items():
        r[k] = v
    return r


@functools.lru_cache(maxsize=None)
def hand_classification_case() -> HandCase:
    """Four copies of one state with pending entries of every kind, each with one task on the current route:
    workflow 0 -- per map something new, changed, deleted and untouched, a restarted TimerID, a timer whose
    task_status alone changed, and rows that differ in a derived field only; workflow 1 -- nothing touched, the exec
    row alone; workflow 2 -- everything deleted and one reset point changed; workflow 3 -- one timer deleted under a
    TimerID that another started_id of the same state takes over, and a reset point added."""
    n_wf = 4
    sbs = persisted.build_blob_set([_hand_state(i) for i in range(n_wf)])
    before = persisted.load_states_host(sbs)
    assert before.mask.all()
    ex = before.exec.copy()
    ex["next_event_id"] += 10
    ex["last_first_event_id"] += 9
    rows = {m: [] for m in abi.LOAD_ROW_TABLES}
    want = {}
    for w in range(n_wf):
        B = {m: r.copy() for m, r in sc.rows_of(before, w).items()}
        key = before.interners[w]
        A = dict(B)
        if w == 0:
            act = B["act"].copy()
            act["flags"][0] ^= abi.ROW_MAPPED              # derived only: not an upsert
            act["last_hb_timeout_vis_s"][0] = 77
            act["started_id"][1], act["started_src"][1] = 41, 16   # changed
            A["act"] = np.concatenate([act[:2], _new_row("act", schedule_id=44, version=3, key=len(key), flags=abi.ROW_LIVE,
                                                         sched_src=17, started_src=-1, started_id=abi.EMPTY_EVENT_ID)])
            tm = B["timer"].copy()                           # rows by started_id: t7@7, t9@9, t11@11, t13@13
            t9 = tm[1:2].copy()
            t9["started_id"], t9["src"] = 45, 18             # fired and started again under the same TimerID
            t13 = tm[3:4].copy()
            t13["task_status"] = 0                           # the status alone
            A["timer"] = np.concatenate([tm[:1], t13, t9, _new_row("timer", started_id=46, version=3, key=len(key) + 1,
                                                                   src=19, flags=abi.ROW_LIVE, expiry_time=5)])
            ch = B["child"].copy()                           # 9, 13, 17
            ch["started_id"][0], ch["started_src"][0] = 47, 20
            ch["reserved"][2] = 5                            # padding only: not an upsert
            A["child"] = np.concatenate([ch[:1], ch[2:], _new_row("child", initiated_id=48, version=3, initiated_batch_id=47,
                                                                  started_id=abi.EMPTY_EVENT_ID, src=21, started_src=-1,
                                                                  flags=abi.ROW_LIVE)])
            A["rc"] = np.concatenate([B["rc"][:1], _new_row("rc", initiated_id=49, version=3, initiated_batch_id=47, src=22,
                                                            flags=abi.ROW_LIVE)])
            sig = B["sig"].copy()
            sig["version"][0] = 4
            A["sig"] = np.concatenate([sig[:1], _new_row("sig", initiated_id=50, version=3, initiated_batch_id=47, src=23,
                                                         flags=abi.ROW_LIVE)])
            A["rp"] = B["rp"][:1]
            want[w] = dict(act=([6, 44], [8]), timer=([key["t13"], key["t9"], len(key) + 1], [key["t11"]]),
                           child=([9, 48], [13]), rc=([49], [15]), sig=([12, 50], [16]), flag=True)
        elif w == 1:
            want[w] = dict(act=([], []), timer=([], []), child=([], []), rc=([], []), sig=([], []), flag=False)
        elif w == 2:
            for m in MAPS:
                A[m] = B[m][:0]
            rp = B["rp"].copy()
            rp["flags"][1] ^= abi.ROW_RESETTABLE
            A["rp"] = rp
            want[w] = dict(act=([], [5, 6, 8]), timer=([], [key["t7"], key["t9"], key["t11"], key["t13"]]),
                           child=([], [9, 13, 17]), rc=([], [11, 15]), sig=([], [12, 16]), flag=True)
        else:
            tm = B["timer"].copy()
            t7 = tm[0:1].copy()
            t7["started_id"], t7["src"] = 12, 16             # restarted between two rows that stay
            A["timer"] = np.concatenate([tm[1:3], t7, tm[3:]])   # 9, 11, 12, 13
            A["rp"] = np.concatenate([B["rp"], B["rp"][:1]])
            want[w] = dict(act=([], []), timer=([key["t7"]], []), child=([], []), rc=([], []), sig=([], []), flag=True)
        for m in abi.LOAD_ROW_TABLES:
            rows[m].append(A[m])
            ex[COUNT_F[m]][w] = A[m].shape[0]
    after = LoadedStates(ex, {m: np.concatenate(rows[m]) for m in rows}, np.ones(n_wf, bool), None)
    order = [2, 0, 3, 1, 0]                                  # workflow 0 twice: tasks do not see one another
    n = len(order)
    tasks, last = np.zeros(n, abi.REPL_TASK), np.zeros(n, abi.LAST_EVENT)
    results, routes = np.zeros(n, abi.NDC_RESULT), np.zeros(n, abi.NDC_ROUTE)
    tasks["wf"] = order
    results["action"], routes["route"] = abi.NDC_APPEND, abi.ROUTE_APPLY_CURRENT
    store_rows = np.zeros(n, abi.STORE_ROW)
    store_rows["outcome"] = int(O.APPLIED)
    return HandCase(sbs, tasks, last, results, routes, before, after, store_rows, want)


# ---- replayed states ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Replayed:
    rc: sc.ReplayedCase
    results: np.ndarray
    routes: np.ndarray
    mask: np.ndarray              # the workflows whose task is replayed
    before: LoadedStates          # load_cases.expected_image of the persisted prefix states
    lay: object                   # the canonical resumed batch
    after: LoadedStates           # the oracle's resumed replay
    store_rows: np.ndarray        # sc.expected_replayed
    want: persisted.Mutation
    tally: Tally


def replayed(rc: sc.ReplayedCase) -> Replayed:
    """The case decided by the oracle and the restated routing, its tasks replayed by the oracle onto the states the
    host loader gives (canonical order), and the expected mutation."""
    from oracle import oracle
    res, routes = sc.decided(rc)
    mask = persisted.apply_mask(routes, rc.tasks, rc.sbs.n_wf)
    lay = flatten(rc.suf, known_domains=KNOWN, loaded=persisted.load_states_host(rc.sbs).resumable(mask))
    after = oracle.replay(lay, 0).to_loaded(lay, mask=mask)
    store_rows = sc.expected_replayed(rc, routes, res, mask, after)
    before = lc.expected_image(rc.pre_r.to_loaded(rc.pre_b), rc.sbs)
    want, tally = expected_mutation(rc.tasks, store_rows, before, after)
    return Replayed(rc, res, routes, mask, before, lay, after, store_rows, want, tally)


@functools.lru_cache(maxsize=None)
def replayed_small() -> Replayed:
    """store_cases.replayed_case's histories, each split anywhere (not only before its last batch): the suffixes
    schedule, start, complete and cancel entries."""
    from cadence_amd import synth_mixed
    return replayed(sc.replayed_case_of(synth_mixed.mixed_histories(64, 81, multi_version=True), 82, 2, last_only=False))


@functools.lru_cache(maxsize=None)
def replayed_tail() -> Replayed:
    hs = lc.prefix_case(150, 62, long_tail=True)[0]
    return replayed(sc.replayed_case_of(hs, 63, 3, shuffle_seed=6, last_only=False))


def after_on(r: Replayed, after: LoadedStates) -> persisted.Mutation:
    """The expected mutation of the same case from another image of the states after (the device's resumed replay in
    canonical order: key ids and provenance are those of its own layout)."""
    return expected_mutation(r.rc.tasks, sc.expected_replayed(r.rc, r.routes, r.results, r.mask, after), r.before, after)[0]


# ---- the round trip ------------------------------------------------------------------------------------------------
def reset_points_of(after: LoadedStates, w: int):
    names = persisted._inverse(after.interners[w])
    return [(names[int(p["key"])], bool(int(p["flags"]) & abi.ROW_RESETTABLE)) for p in sc.rows_of(after, w)["rp"]]


def persisted_view(img, w: int):
    """Workflow w of a loaded image in a form that does not depend on the order of its blobs: provenance reduced to
    whether there is one, key ids replaced by their strings."""
    names = [""] + img.keys(w)
    ex = {f: int(img.exec[f][w]) for f in abi.EXEC_ROW.names if f not in ("start_src", "src_next")}
    ex["decision_request_src"] = min(ex["decision_request_src"], 0)
    out = {"exec": ex, "token": img.token(w), "status": int(img.status[w]), "flags": int(img.flags[w])}
    for m, rows in sc.rows_of(img, w).items():
        out[m] = []
        for r in rows:
            d = {}
            for f in r.dtype.names:
                v = int(r[f])
                if f in ("src", "sched_src"):
                    continue
                if f == "started_src":
                    v = min(v, 0)
                if f == "key":
                    v = names[v]
                d[f] = v
            out[m].append(d)
    return out
