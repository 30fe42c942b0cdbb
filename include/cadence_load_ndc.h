/*
 * cadence_load_ndc.h -- the branch decision and the conflict resolver's routing decision for replication
 * tasks against persisted states, from the persisted bytes, on the device.
 *
 * Between mutableStateBuilder.Load and ApplyEvents, historyReplicatorImpl.applyEvents
 * (service/history/ndc/history_replicator.go:234-258) asks
 *   branchManager.prepareVersionHistory   (ndc/branch_manager.go:87-149)    which branch the task belongs to
 *   conflictResolver.prepareMutableState  (ndc/conflict_resolver.go:75-120) whether the state continues as it is
 * and only then reaches applyNonStartEventsToCurrentBranch.  The loader (cadence_load.h) decodes the current
 * branch alone; this interface walks every history of every loaded state's VersionHistories blob (the execution
 * blob's field 122) into the branch table crr_ndc_prepare takes, runs crr_ndc_prepare as it is over a batch of
 * replication tasks against those states, and then routes every task.  The branch table stays resident in the
 * caller's buffers.
 *
 * Each task is decided against the persisted state alone: two tasks that name one workflow do not see one
 * another's outcome (a new branch one of them would add is not a local branch of the other).  The caller
 * applies them in its own order and decides the later ones again where an earlier one changed the histories.
 *
 * What stays on the host: the buffered-events flush (branch_manager.go:169-196), ForkHistoryBranch (the new
 * branch's token; the base branch's token is in the token table), the rebuild itself (state_rebuilder.go) and
 * the append of a non-current branch's events.
 *
 * This header is an addition to ABI version 8: CRR_ABI_VERSION and every existing struct and entry point are
 * unchanged; crr_sizeof(22..26) report the structs below.  The calls read the loader's scratch and change
 * nothing in it; they work in a buffer of their own (crr_load_ndc_scratch_bytes).
 */
#ifndef CADENCE_LOAD_NDC_H_
#define CADENCE_LOAD_NDC_H_

#include <stddef.h>
#include <stdint.h>

#include "cadence_load.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A task is not decided when its workflow did not load (status != CRR_LOAD_OK) or its `wf` is at or beyond the
 * batch's n_wf: crr_status_code CRR_ERR_NDC_STATE_NOT_LOADED (25, the one value this interface adds to the enum). */

/* One replication task (32 B).  Any number of tasks may name one workflow, in any order. */
typedef struct crr_repl_task {
    uint32_t wf;                    /* index into the state batch */
    uint32_t incoming_begin;        /* the task's VersionHistoryItems (ndc/replication_task.go:113) =  */
    uint32_t incoming_count;        /*   incoming[incoming_begin, +incoming_count)                     */
    uint32_t reserved;              /* 0 */
    int64_t  first_event_id;        /* the task's first event */
    int64_t  first_event_version;   /* and its version: the task's version (replication_task.go:118) */
} crr_repl_task;

/* Where a branch's token lies in the state batch's `bytes` (16 B); an absent token has length 0. */
typedef struct crr_branch_token {
    uint64_t off;
    uint32_t len;
    uint32_t wf;
} crr_branch_token;

/* The branch table (device buffers of the caller, sized from the plan; host buffers for
 * crr_load_branches_host).  Workflow w's histories, in stored order, are
 * branches[branch_begin[w] .. branch_begin[w + 1]) with their tokens at the same indices; a branch's items are
 * items[item_begin, +item_count), an absent Items field giving an empty branch.  A workflow that did not load
 * has no branches and current 0.  items has room for n_items + n_incoming rows: the device calls copy the
 * tasks' incoming items behind the local ones, so that crr_ndc_prepare sees one items array. */
typedef struct crr_load_branches {
    crr_ndc_branch*   branches;     /* [n_branches] */
    crr_vh_item*      items;        /* [n_items (+ n_incoming)] */
    crr_branch_token* tokens;       /* [n_branches] */
    int64_t*          branch_begin; /* [n_wf + 1] exclusive prefix, [n_wf] = n_branches */
    int32_t*          current;      /* [n_wf] CurrentVersionHistoryIndex as stored */
} crr_load_branches;

/* What the planning call reports (a host struct, valid when the call returns). */
typedef struct crr_load_ndc_sizes {
    int32_t  err;                   /* 0, or CRR_INGEST_SCRATCH_TOO_SMALL (-100): `work` smaller than work_needed */
    uint32_t n_wf;
    uint32_t n_tasks;
    uint32_t n_incoming;
    uint64_t n_branches;            /* histories of all loaded workflows */
    uint64_t n_items;               /* their items */
    uint64_t n_out_items;           /* room for new-branch items: per task, the longest local branch of its workflow */
    uint64_t work_needed;           /* crr_load_ndc_scratch_bytes(n_wf, n_tasks) */
} crr_load_ndc_sizes;

#define CRR_ROUTE_NONE          0   /* status not OK, or the task is a duplicate: nothing to apply */
#define CRR_ROUTE_APPLY_CURRENT 1   /* the task's branch is the current one (conflict_resolver.go:88-90): the only
                                       route on which the task's events are replayed onto the placed rows */
#define CRR_ROUTE_NON_CURRENT   2   /* incoming version below the current branch's last version (:102-104):
                                       history is appended, no replay */
#define CRR_ROUTE_REBUILD       3   /* above it (:112-119): the state is rebuilt from branch `branch` */
#define CRR_ROUTE_BAD_REQUEST   4   /* equal (:106-110): BadRequestError */

/* Per task (32 B).  Fields past `status` are set for CRR_ROUTE_REBUILD (what Rebuild is called with,
 * conflict_resolver.go:132-158) and zero otherwise. */
typedef struct crr_ndc_route {
    int32_t route;                  /* CRR_ROUTE_* */
    int32_t status;                 /* the decision's status; CRR_ERR_VH_EMPTY where GetLastItem fails on an empty
                                       branch (the current one, or the one to rebuild from) */
    int32_t branch;                 /* index of the branch to rebuild from (the decision's branch_index) */
    int32_t branch_is_local;        /* 1: a stored branch, its token is tokens[branch_begin[wf] + branch]; 0: the new
                                       branch, whose token ForkHistoryBranch returns */
    int64_t last_event_id;          /* that branch's last item */
    int64_t last_version;
} crr_ndc_route;

/* Bytes of the work buffer for a batch of n_wf states and n_tasks tasks. */
size_t crr_load_ndc_scratch_bytes(uint32_t n_wf, uint32_t n_tasks);

/* Size the branch table and the new-branch items: counts every loaded workflow's histories and items from the
 * persisted bytes, and the prefix of the tasks' new-branch room.  `in`, `scratch`, `scratch_bytes` and
 * `summary_host` are those of a finished crr_load_states_plan; `tasks` is device [n_tasks] (NULL with
 * n_tasks == 0: the branch table alone); `work` is device, 16-byte aligned.  Synchronises `stream` once, to
 * read the totals back.  Returns 0, -1 on an invalid argument (`in` not the planned batch's shape, or totals
 * past what crr_ndc_branch's 32-bit indices hold), else the hipError_t. */
int crr_load_ndc_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                      const crr_load_summary* summary_host, const crr_repl_task* tasks, uint32_t n_tasks,
                      uint32_t n_incoming, void* work, size_t work_bytes, crr_load_ndc_sizes* plan, void* stream);

/* Emit the branch table into `dst`, then decide and route every task.  `plan_host` is the finished plan of the
 * same arguments; `incoming` is device [n_incoming]; `results` and `routes` are device [n_tasks], `out_items`
 * device [n_out_items], a valid pointer even when that is 0 (task k's new-branch items at the out_begin the plan gave it: ascending with k, the
 * prefix of the tasks' room); all three may be NULL when n_tasks == 0.  A task that is not decided gets status
 * CRR_ERR_NDC_STATE_NOT_LOADED (an incoming range outside `incoming`: CRR_ERR_NDC_BAD_INDEX), action
 * CRR_NDC_DUPLICATE, zeros in every other result field and CRR_ROUTE_NONE.  `out_begin` (device [n_tasks],
 * may be NULL) receives each task's offset into out_items.  Enqueued on `stream`, no synchronisation.
 * Returns 0, -1 on an invalid argument, else the hipError_t. */
int crr_load_ndc_run(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                     const crr_load_summary* summary_host, const crr_repl_task* tasks, const crr_vh_item* incoming,
                     void* work, size_t work_bytes, const crr_load_ndc_sizes* plan_host, const crr_load_branches* dst,
                     crr_ndc_result* results, crr_ndc_route* routes, crr_vh_item* out_items, uint32_t* out_begin,
                     void* stream);

/* Host restatement of the branch table (libcadence_host.so): host pointers; decodes `in` as
 * crr_load_states_host does, then runs the same walk.  `dst` (or any buffer of it) may be NULL: call once to
 * size the buffers from `plan` (n_wf, n_branches, n_items), then again with them.  There is no host restatement
 * of the decision.  Returns 0, -1 on an invalid argument, -2 out of memory. */
int crr_load_branches_host(const crr_state_batch* in, const crr_load_branches* dst, crr_load_ndc_sizes* plan,
                           int threads);

#ifdef __cplusplus
}
#endif
#endif /* CADENCE_LOAD_NDC_H_ */
