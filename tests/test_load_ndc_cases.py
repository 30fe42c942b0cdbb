"""The inputs of the GPU test of cadence_load_ndc.h, checked on the CPU: the replication tasks written into
persisted states (test_ndc.random_tasks' shapes, ndc_load_cases.task_case) reach every outcome of
prepareVersionHistory under the oracle and every route of prepareMutableState under its Python restatement
(ndc_load_cases.route_of, written from ndc/conflict_resolver.go:75-120), and that restatement gives the
reference's own two answers (conflict_resolver_test.go:171-187, :189-260).
"""
import numpy as np
import pytest

from cadence_amd import abi
from cadence_amd.abi import Status
from cadence_amd.ndc import NdcTask
from cadence_amd.persisted import load_branches_host

import ndc_load_cases as nc


def test_the_tasks_cover_every_decision():
    case = nc.task_case()
    assert case.sbs.n_wf == 130 and 380 <= len(case.tasks) <= 420
    _idx, _batch, res, _out = nc.oracle_decisions(case)
    st = set(int(s) for s in res["status"])
    assert {0, int(Status.NDC_NO_LCA), int(Status.NDC_RETRY_TASK)} <= st
    acts = set(int(a) for a, s in zip(res["action"], res["status"]) if s == 0)
    assert acts == {abi.NDC_APPEND, abi.NDC_NEW_BRANCH, abi.NDC_DUPLICATE}


def test_the_tasks_cover_every_route():
    case = nc.task_case()
    results, routes, _items = nc.expected_routes(case)
    assert set(int(r) for r in routes["route"]) == {abi.ROUTE_NONE, abi.ROUTE_APPLY_CURRENT, abi.ROUTE_NON_CURRENT,
                                                    abi.ROUTE_REBUILD, abi.ROUTE_BAD_REQUEST}
    not_decided = np.array([t is None for t in case.ndc_tasks])
    assert not_decided.sum() >= 5 and (results["status"][not_decided] == Status.NDC_STATE_NOT_LOADED).all()
    assert (routes["route"][not_decided] == abi.ROUTE_NONE).all()
    assert (case.tasks["wf"] >= case.sbs.n_wf).sum() == 2
    # several tasks per workflow, none for some, shuffled
    per_wf = np.bincount(case.tasks["wf"][case.tasks["wf"] < case.sbs.n_wf], minlength=case.sbs.n_wf)
    assert per_wf.max() >= 4 and (per_wf == 0).sum() >= 30
    assert (np.diff(case.tasks["wf"].astype(np.int64)) < 0).sum() > 100
    # rebuilds from a stored branch and from the new one
    rb = routes[routes["route"] == abi.ROUTE_REBUILD]
    assert set(int(x) for x in rb["branch_is_local"]) == {0, 1}


# per size: (tasks per route NONE / APPLY_CURRENT / NON_CURRENT / REBUILD / BAD_REQUEST, branches, tasks not decided,
# items of new-branch room)
LARGE_COUNTS = {(1300, 2500): ([1346, 521, 233, 388, 12], 3392, 11, 12323),
                (1025, 1025): ([570, 199, 89, 165, 2], 2699, 7, 4779)}


@pytest.mark.parametrize("n_states,n_tasks", nc.LARGE_CASES)
def test_the_large_cases_cover_every_decision_and_route(n_states, n_tasks):
    """The sizes the GPU tests use past 1024 states and tasks are not degenerate: every decision, every route, both
    kinds of rebuild, and the states are what the tasks were built from."""
    case = nc.task_case(n_states, n_tasks)
    assert case.sbs.n_wf == n_states > 1024 and len(case.tasks) == n_tasks > 1024
    # the chunk of a 1024-thread scan: more than one element and idle threads behind the last one, over the states
    # and over the tasks; the tasks' last chunk is not full
    for n in (n_states, n_tasks):
        per = -(-n // 1024)
        assert per >= 2 and -(-n // per) < 1024
    assert n_tasks % -(-n_tasks // 1024) != 0
    _idx, _batch, res, _out = nc.oracle_decisions(case)
    assert {0, int(Status.NDC_NO_LCA), int(Status.NDC_RETRY_TASK)} <= set(int(s) for s in res["status"])
    assert set(int(a) for a, s in zip(res["action"], res["status"]) if s == 0) == {abi.NDC_APPEND, abi.NDC_NEW_BRANCH, abi.NDC_DUPLICATE}
    results, routes, _items = nc.expected_routes(case)
    host = load_branches_host(case.sbs)
    room = sum(max(len(b) for b in t.local) for t in case.ndc_tasks if t is not None)
    not_decided = sum(t is None for t in case.ndc_tasks)
    assert (np.bincount(routes["route"], minlength=5).tolist(), host.branches.shape[0], not_decided, room) == LARGE_COUNTS[(n_states, n_tasks)]
    rb = routes[routes["route"] == abi.ROUTE_REBUILD]
    assert set(int(x) for x in rb["branch_is_local"]) == {0, 1}
    assert nc.table_of(case.sbs, host) == nc.written_table(case)
    assert tuple(routes[case.known["rebuild"]]) == (abi.ROUTE_REBUILD, 0, 2, 0, 1, 12)


def test_an_empty_current_branch_is_vh_empty():
    """GetLastItem on an empty current branch (conflict_resolver.go:96-99).  No task reaches it through
    prepareVersionHistory, whose LCA search fails on the empty branch first (NDC_NO_LCA), so it is stated on a
    decision given directly."""
    task = NdcTask([[], [(4, 2)]], 0, [(4, 2), (9, 5)], 5, 5)
    r = _decision(action=abi.NDC_APPEND, branch_index=1, new_current_index=0)
    assert nc.route_of(task, r, []) == (abi.ROUTE_NONE, int(Status.VH_EMPTY), 0, 0, 0, 0)
    from oracle import oracle
    from cadence_amd import ndc
    res, _ = oracle.ndc_prepare(ndc.pack([task]))
    assert res[0]["status"] == Status.NDC_NO_LCA


def test_the_states_are_what_the_tasks_were_built_from():
    case = nc.task_case()
    got = nc.table_of(case.sbs, load_branches_host(case.sbs))
    for w, (cur, local) in enumerate(case.locals_):
        if not case.loaded[w]:
            assert got[w] is None
        else:
            assert got[w][0] == cur and [items for items, _tok in got[w][1]] == [list(b) for b in local], w
    assert max(len(b) for _c, loc in case.locals_ for b in loc) == 600
    assert max(len(loc) for _c, loc in case.locals_) == 70


def _decision(**kw):
    r = np.zeros(1, abi.NDC_RESULT)[0]
    for k, v in kw.items():
        r[k] = v
    return r


def test_known_answer_no_rebuild():
    """TestPrepareMutableState_NoRebuild: one branch, prepareMutableState(0, 12) -> the state as it is."""
    local, cur, branch, version = nc.KNOWN_NO_REBUILD
    task = NdcTask(local, cur, [(3, version)], 3, version)
    r = _decision(action=abi.NDC_APPEND, branch_index=branch, new_current_index=cur)
    assert nc.route_of(task, r, []) == (abi.ROUTE_APPLY_CURRENT, 0, 0, 0, 0, 0)
    # and through the decision itself: the task extends branch 0
    case = nc.task_case()
    results, routes, _ = nc.expected_routes(case)
    k = case.known["no_rebuild"]
    assert (results[k]["status"], results[k]["action"], results[k]["branch_index"]) == (0, abi.NDC_APPEND, 0)
    assert routes[k]["route"] == abi.ROUTE_APPLY_CURRENT


def test_known_answer_rebuild():
    """TestPrepareMutableState_Rebuild: branches [(2, 12)] (current) and [(1, 12)], prepareMutableState(1, 13) ->
    Rebuild from branch 1 with its last item (1, 12)."""
    local, cur, branch, version = nc.KNOWN_REBUILD
    task = NdcTask(local, cur, [(1, 12), (2, version)], 2, version)
    r = _decision(action=abi.NDC_APPEND, branch_index=branch, new_current_index=cur)
    assert nc.route_of(task, r, []) == (abi.ROUTE_REBUILD, 0, 1, 1, 1, 12)
    # Through the decision the same state routes to a rebuild from (1, 12) too, but prepareVersionHistory does not
    # hand out index 1 for it: both branches meet the incoming history at event 1 and are equally long, so
    # FindLCAVersionHistoryIndexAndItem (versionHistory.go:501-528) keeps branch 0, which is not appendable there,
    # and the task forks a new branch [(1, 12)] (index 2) -- the items of branch 1 again.
    case = nc.task_case()
    results, routes, items = nc.expected_routes(case)
    k = case.known["rebuild"]
    assert (results[k]["status"], results[k]["action"], results[k]["branch_index"]) == (0, abi.NDC_NEW_BRANCH, 2)
    assert items[k] == [(1, 12)]
    assert tuple(routes[k]) == (abi.ROUTE_REBUILD, 0, 2, 0, 1, 12)
