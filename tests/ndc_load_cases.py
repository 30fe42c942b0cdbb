"""Shared cases for the branch table of persisted states and the replication tasks decided against it
(include/cadence_load_ndc.h): states with arbitrary branch sets written through ``persisted`` and by hand,
test_ndc.random_tasks' shapes written into such states, and conflictResolverImpl.prepareMutableState
(ndc/conflict_resolver.go:75-120) restated in Python.  Everything expected here comes from the values written,
never from the loader's output.
"""
from __future__ import annotations

import dataclasses
import functools
import random
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

from cadence_amd import abi, ndc, persisted
from cadence_amd.ndc import NdcTask
from cadence_amd.thrift_codec import T_LIST, T_STRUCT, W

import load_cases as lc

Items = List[Tuple[int, int]]
# a written branch: (token, items); None for either: the field is absent from its VersionHistory struct
Branch = Tuple[Optional[bytes], Optional[Items]]


def version_histories_blob(current: int, branches: Sequence[Branch]) -> bytes:
    """shared.VersionHistories behind the 0x59 preamble, written field by field with thrift_codec.W: a branch's
    token / Items field is left out where it is None."""
    w = W()
    w.b += b"\x59"
    w.i32(10, current)
    w.field(T_LIST, 20)
    w.b += bytes([T_STRUCT]) + struct.pack(">i", len(branches))
    for token, items in branches:
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


def hand_state(current: int, branches: Sequence[Branch], extra=(), nei: int = 20, raw: Optional[bytes] = None):
    """A hand-built workflow whose execution blob holds ``branches`` (``raw``: these VersionHistories bytes)."""
    vh = version_histories_blob(current, branches) if raw is None else raw
    return (nei, list(extra) + [lc.execution(lc.exec_blob(nei=nei, VersionHistories=vh))])


def workflows_of(sbs: persisted.StateBlobSet):
    """``build_blob_set``'s input back from a blob set."""
    out = []
    for W_ in sbs.wf:
        blobs = []
        for b in range(int(W_["blob_begin"]), int(W_["blob_begin"]) + int(W_["blob_count"])):
            B = sbs.blob[b]
            s = sbs.strings[int(B["str_off"]):int(B["str_off"]) + int(B["str_len"])].tobytes()
            blobs.append((int(B["kind"]), int(B["id"]), int(B["aux_time"]), s, sbs.blob_bytes(b)))
        out.append((int(W_["next_event_id"]), blobs))
    return out


def expected_of(current: int, branches: Sequence[Branch]):
    """What the branch table must hold for a loaded state: (current, [(items, token bytes)])."""
    return current, [(list(items or []), bytes(token or b"")) for token, items in branches]


def table_of(sbs: persisted.StateBlobSet, br: persisted.Branches):
    """The table as values: per workflow None (no branches) or (current, [(items, token bytes)])."""
    out = []
    for w in range(sbs.n_wf):
        hs = br.of(w)
        if not hs:
            assert int(br.current[w]) == 0
            out.append(None)
            continue
        toks = []
        for b in range(int(br.branch_begin[w]), int(br.branch_begin[w + 1])):
            assert int(br.tokens[b]["wf"]) == w
            toks.append(sbs.bytes[int(br.tokens[b]["off"]):int(br.tokens[b]["off"]) + int(br.tokens[b]["len"])].tobytes())
        out.append((int(br.current[w]), [(items, tok) for (items, _rng), tok in zip(hs, toks)]))
    return out


def random_branches(rng: random.Random) -> Tuple[int, List[Branch]]:
    n = rng.randint(1, 4)
    out = []
    for _ in range(n):
        e, v, items = 0, rng.randint(0, 3), []
        for _ in range(rng.randint(1, 6)):
            e += rng.randint(1, 30)
            v += rng.randint(0, 50)
            items.append((e, v))
        out.append((bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 1, 7, 8, 9, 40, 97]))), items))
    return (rng.randrange(n) if n > 1 and rng.random() < 0.8 else 0), out


@functools.lru_cache(maxsize=None)
def replayed_branch_states(n: int = 200, seed: int = 71):
    """``n`` replayed states written through ``encode_states(branches=...)`` with random branch sets, their blobs
    shuffled, plus hand-built ones (branches without an Items field, without a token) and three that do not load
    (a truncated VersionHistories blob, a current index out of range, two execution blobs), spread among them:
    (blob set, expected table per workflow)."""
    rng = random.Random(seed)
    _hs, pre, _suf, _mask, pre_b, pre_r = lc.prefix_case(n, seed)
    ok = pre_r.to_loaded(pre_b).mask
    sets = {w: random_branches(rng) for w in range(ok.shape[0]) if ok[w]}
    if all(cur == 0 for cur, _ in sets.values()):
        raise AssertionError("no state with a current index other than 0: change the seed")
    sbs = persisted.encode_states(pre_b, pre_r, pre, shuffle_seed=seed, branches={w: (b, cur) for w, (cur, b) in sets.items()})
    wfs = workflows_of(sbs)
    want = [expected_of(*sets[w]) if ok[w] else None for w in range(ok.shape[0])]
    full = version_histories_blob(1, [(b"tok-a", [(3, 1), (9, 4)]), (b"tok-b", [(3, 1), (12, 7)])])
    hand = [
        (1, [(b"token-only", None), (b"both", [(4, 2), (8, 5)]), (None, [(4, 2)])], True),
        (0, [(None, None)], True),
        (2, [(None, [(1, 0)]), (b"", []), (b"cur", None)], True),
        (0, [], full[:len(full) - 7]),                                       # truncated nested blob
        (2, [(b"t", [(5, 1)]), (b"u", [(5, 1), (6, 2)])], False),            # current index out of range
    ]
    for i, (cur, branches, how) in enumerate(hand):
        at = (i + 1) * len(wfs) // (len(hand) + 2)
        wfs.insert(at, hand_state(cur, branches, extra=[lc.timer_blob("t7", 7)], raw=how if isinstance(how, bytes) else None))
        want.insert(at, expected_of(cur, branches) if how is True else None)
    at = len(wfs) // 2
    wfs.insert(at, (20, [lc.execution(lc.exec_blob()), lc.execution(lc.exec_blob())]))   # two execution blobs
    want.insert(at, None)
    return persisted.build_blob_set(wfs), want


# ---- replication tasks against states (test_ndc.random_tasks' shapes) -----------------------------------------
@dataclasses.dataclass
class TaskCase:
    sbs: persisted.StateBlobSet
    loaded: np.ndarray            # bool per workflow: the state is written to load
    locals_: list                 # per workflow: (current, [items per branch]) as written
    tasks: np.ndarray             # abi.REPL_TASK
    incoming: np.ndarray          # abi.VH_ITEM
    ndc_tasks: List[Optional[NdcTask]]   # per task: the NdcTask of the values written (None: not decided)
    known: dict                   # name -> task index of a known answer


def _chain(rng):
    chain, eid, ver = [], 0, rng.randint(0, 3)
    for _ in range(rng.randint(1, 6)):
        eid += rng.randint(1, 30)
        ver += rng.randint(1, 50)
        chain.append((eid, ver))
    return chain


def _branch_from(rng, ch):
    k = rng.randint(1, len(ch))
    b = [list(x) for x in ch[:k]]
    if rng.random() < 0.5:
        b[-1][0] = max(b[-2][0] + 1 if len(b) > 1 else 1, b[-1][0] - rng.randint(0, 5))
    e, v = b[-1]
    for _ in range(rng.randint(0, 3)):
        e += rng.randint(1, 20)
        v += rng.randint(1, 40)
        b.append([e, v])
    return [tuple(x) for x in b]


def _incoming(rng, chain):
    incoming = _branch_from(rng, chain) if rng.random() < 0.9 else [(rng.randint(1, 9), 999)]
    if rng.random() < 0.03:
        incoming = [(5, 3), (4, 7)]                                  # malformed
    first = incoming[-1][0] - rng.choice([0, 0, 1, 2, 3, 10]) + rng.choice([0, 1])
    return incoming, first, incoming[-1][1]


def _extending(rng, local):
    """A task in order on one of the state's branches (random_tasks' own tasks are mostly duplicates or out of
    order, which never reach prepareMutableState): the branch's next event at its last version or a newer one,
    or a fork one event before its end."""
    b = rng.choice([x for x in local if x] or [[(rng.randint(1, 9), 1)]])
    e, v = b[-1]
    how = rng.random()
    if how < 0.4:
        incoming = b[:-1] + [(e + rng.randint(1, 5), v)]
    elif how < 0.8 or e < 2 or (len(b) > 1 and b[-2][0] >= e - 1):
        incoming = b + [(e + rng.randint(1, 5), v + rng.randint(1, 30))]
    else:
        e -= 1
        incoming = b[:-1] + [(e, v), (e + rng.randint(1, 5), v + rng.randint(1, 30))]
    return incoming, e + 1, incoming[-1][1]


# the reference's own cases (conflict_resolver_test.go:171-187, :189-260) as (local, current, the branch index
# prepareMutableState is called with, incoming version)
KNOWN_NO_REBUILD = ([[(2, 12)]], 0, 0, 12)
KNOWN_REBUILD = ([[(2, 12)], [(1, 12)]], 0, 1, 13)


@functools.lru_cache(maxsize=None)
def task_case(n_states: int = 130, n_tasks: int = 400, seed: int = 3, big: bool = True) -> TaskCase:
    """``n_states`` hand-built states whose branch sets have test_ndc.random_tasks' shapes (empty branches
    included: written without an Items field), three of them made not to load in the middle of the second
    wavefront, with ``big`` one state with a 600-item branch and one with 70 branches; about ``n_tasks`` tasks
    in shuffled order, several per workflow and none for some, two with ``wf >= n_wf``, and the two known
    answers."""
    rng = random.Random(seed)
    states, chains = [], []
    for w in range(n_states):
        chain = _chain(rng)
        local = [_branch_from(rng, chain) for _ in range(rng.randint(1, 4))]
        if rng.random() < 0.08:
            local.insert(rng.randrange(len(local) + 1), [])               # an empty branch
        states.append([rng.randrange(len(local)), local])
        chains.append(chain)
    known_at = {"no_rebuild": 7, "rebuild": 71}
    states[7] = [KNOWN_NO_REBUILD[1], KNOWN_NO_REBUILD[0]]
    states[71] = [KNOWN_REBUILD[1], KNOWN_REBUILD[0]]
    if big:
        chain = [(3 * i + 3, 2 * i + 1) for i in range(600)]
        states[40], chains[40] = [0, [chain, chain[:300] + [(2000, 5000)]]], chain
        chain = _chain(rng)
        states[100], chains[100] = [33, [_branch_from(rng, chain) for _ in range(70)]], chain
    bad = {n_states // 2 + 31: "truncated", n_states // 2 + 32: "index", n_states // 2 + 33: "two"} if n_states > 100 else {}
    wfs, loaded = [], np.ones(n_states, bool)
    for w, (cur, local) in enumerate(states):
        branches = [(b"token-%d-%d" % (w, b) if (w + b) % 5 else None, items if items or (w % 2) else None)
                    for b, items in enumerate(local)]
        extra = [lc.activity_blob(5, "a5"), lc.timer_blob("t7", 7)][: w % 3]
        if bad.get(w) == "truncated":
            full = version_histories_blob(cur, branches)
            wfs.append(hand_state(cur, branches, extra, raw=full[:len(full) - 5]))
        elif bad.get(w) == "index":
            wfs.append(hand_state(len(local), branches, extra))
        elif bad.get(w) == "two":
            wfs.append((20, [lc.execution(lc.exec_blob()), lc.execution(lc.exec_blob())]))
        else:
            wfs.append(hand_state(cur, branches, extra))
        loaded[w] = w not in bad
    sbs = persisted.build_blob_set(wfs)
    # tasks: workflows 0, 3, 6 ... get none; the not-loaded ones and the known answers always get one
    rows = []
    rows.append((7, [(3, 12)], 3, 12))               # extends branch 0, the current one, at version 12
    rows.append((71, [(1, 12), (2, 13)], 2, 13))     # event 2 at version 13 on top of (1, 12)
    for w in bad:
        rows.append((w,) + _incoming(rng, chains[w]))
    pool = [w for w in range(n_states) if w % 3 and w not in (7, 71)]
    while len(rows) < n_tasks - 2:
        w = rng.choice(pool)
        rows.append((w,) + (_incoming(rng, chains[w]) if rng.random() < 0.5 else _extending(rng, states[w][1])))
    rows.append((n_states, [(1, 1)], 2, 1))
    rows.append((0xFFFFFFFF, [(1, 1)], 2, 1))
    order = list(range(len(rows)))
    rng.shuffle(order)
    rows = [rows[i] for i in order]
    known = {"no_rebuild": order.index(0), "rebuild": order.index(1)}
    tasks = np.zeros(len(rows), abi.REPL_TASK)
    items, ndc_tasks = [], []
    for k, (w, incoming, first, ver) in enumerate(rows):
        tasks[k] = (w, len(items), len(incoming), 0, first, ver)
        items.extend(incoming)
        ok = w < n_states and loaded[w]
        ndc_tasks.append(NdcTask([list(b) for b in states[w][1]], states[w][0], list(incoming), first, ver) if ok else None)
    return TaskCase(sbs, loaded, states, tasks, np.array(items, abi.VH_ITEM), ndc_tasks, known)


# task_case sizes past one element per thread of the loader's 1024-thread scans (per = ceil(n / 1024) consecutive
# elements each, over the states' branch and item counts and over the tasks' rooms, blob lengths and marks):
# (1300, 2500): states per = 2, threads from 650 up idle; tasks per = 3, 2500 = 833 * 3 + 1, so thread 833 holds
#               one element and the threads behind it none
# (1025, 1025): the first size with per = 2; thread 512 holds the one last element
LARGE_CASES = ((1300, 2500), (1025, 1025))


def written_table(case: TaskCase):
    """``table_of``'s value for the branch table of ``case``'s states, from the values task_case wrote."""
    return [expected_of(cur, [(b"token-%d-%d" % (w, b) if (w + b) % 5 else None, items) for b, items in enumerate(local)])
            if case.loaded[w] else None for w, (cur, local) in enumerate(case.locals_)]


def oracle_decisions(case: TaskCase):
    """``oracle.ndc_prepare`` on ``ndc.pack`` of the decided tasks: (indices of the decided tasks, batch, results,
    out items)."""
    from oracle import oracle
    idx = [k for k, t in enumerate(case.ndc_tasks) if t is not None]
    batch = ndc.pack([case.ndc_tasks[k] for k in idx])
    res, out = oracle.ndc_prepare(batch)
    return idx, batch, res, out


def route_of(task: NdcTask, r, new_items: Items):
    """prepareMutableState (conflict_resolver.go:75-120) and what rebuild (:122-158) is called with, over the
    histories as prepareVersionHistory left them: (route, status, branch, branch_is_local, last event ID, last
    version)."""
    if int(r["status"]) != 0 or int(r["action"]) == abi.NDC_DUPLICATE:
        return (abi.ROUTE_NONE, int(r["status"]), 0, 0, 0, 0)
    branch, cur = int(r["branch_index"]), int(r["new_current_index"])
    if branch == cur:                                                         # :88-90
        return (abi.ROUTE_APPLY_CURRENT, 0, 0, 0, 0, 0)
    hist = [list(b) for b in task.local] + ([list(new_items)] if int(r["action"]) == abi.NDC_NEW_BRANCH else [])
    if not hist[cur]:                                                         # GetLastItem :96-99
        return (abi.ROUTE_NONE, int(abi.Status.VH_EMPTY), 0, 0, 0, 0)
    last_version = hist[cur][-1][1]
    if task.first_event_version < last_version:                               # :102-104
        return (abi.ROUTE_NON_CURRENT, 0, 0, 0, 0, 0)
    if task.first_event_version == last_version:                              # :106-110
        return (abi.ROUTE_BAD_REQUEST, 0, 0, 0, 0, 0)
    if not hist[branch]:                                                      # :136-139
        return (abi.ROUTE_NONE, int(abi.Status.VH_EMPTY), 0, 0, 0, 0)
    return (abi.ROUTE_REBUILD, 0, branch, int(branch < len(task.local)), hist[branch][-1][0], hist[branch][-1][1])


def expected_routes(case: TaskCase):
    """(results, routes, new-branch items per task) expected for every task of ``case``: the oracle's decision
    and the restated routing for the decided ones, the not-decided row for the others."""
    idx, batch, res, out = oracle_decisions(case)
    n = len(case.ndc_tasks)
    results = np.zeros(n, abi.NDC_RESULT)
    results["status"] = abi.Status.NDC_STATE_NOT_LOADED
    results["action"] = abi.NDC_DUPLICATE
    routes = np.zeros(n, abi.NDC_ROUTE)
    routes["status"] = abi.Status.NDC_STATE_NOT_LOADED
    new_items = [[] for _ in range(n)]
    for j, k in enumerate(idx):
        results[k] = res[j]
        new_items[k] = ndc.new_branch_items(batch, res, out, j)
        routes[k] = route_of(case.ndc_tasks[k], res[j], new_items[k])
    return results, routes, new_items
