/*
 * cadence_load_store.h -- the checksum to store with a persisted state after a routed replication task was
 * committed, on the device.
 *
 * cadence_load.h decodes the states, cadence_load_verify.h checks the checksum they were stored with,
 * cadence_load_ndc.h decides and routes every replication task, and crr_replay continues the states whose task
 * was routed to the current branch.  What Go writes back with the state when it commits the task is
 * generateChecksum's value (CloseTransactionAsMutation, service/history/execution/mutable_state_builder.go:3959-3996
 * and :4641-4651; payload execution/checksum.go:36-114).  Under the passive policy nothing between ApplyEvents
 * (or the backfill's AddOrUpdateItem) and generateChecksum changes a field of the payload (DESIGN.md §4 lists the
 * lines), so the value follows from data that is resident after those calls: the loader's scratch, the branch
 * table crr_load_ndc_run left, and the rows the resumed replay wrote.
 *
 * Two routes commit a state.
 *
 *   CRR_ROUTE_APPLY_CURRENT + CRR_NDC_APPEND (ndc/history_replicator.go:385-460): the state as the resumed
 *   replay left it.  Scalars from the post-replay exec row at the workflow's device position; the five ID lists
 *   from the first field of the live rows in slots 0..n-1 of each pending map (ascending by ID after a call),
 *   addressed base + j * stride, stride 1 at or past wave_begin, as crr_load_states_place addresses them -- the
 *   rows, not the live-ID sidecar; StickyTaskListName "" (ApplyEvents clears stickiness, state_builder.go:108);
 *   VersionHistories: CurrentVersionHistoryIndex as stored and every stored branch in stored order, each token
 *   from the persisted bytes, a non-current branch's items from the branch table, the current branch's items
 *   the replay's vh rows.
 *
 *   CRR_ROUTE_NON_CURRENT + CRR_NDC_APPEND (history_replicator.go:490-542): nothing is replayed.  Scalars, ID
 *   lists and the sticky name as stored (the fields crr_load_states_verify reads); every branch from the table,
 *   with AddOrUpdateItem(the task's last event) applied to branch `branch_index` (common/persistence/
 *   versionHistory.go:193-226): an empty branch takes the item, an equal version updates the last item's event
 *   ID, a higher version appends.  This is the passive backfill.  When the backfilled events have to be
 *   reapplied to the current branch (case 1 of backfillWorkflowEventsReapply, ndc/transaction_manager.go:270-310)
 *   the state changes through the active path: that commit, and its checksum, are the host's.
 *
 * Whether a domain samples generation at all (shouldGenerateChecksum, mutable_state_builder.go:4653-4658) is the
 * caller's decision.  The caller stores `value` as four big-endian bytes with CRR_CHECKSUM_PAYLOAD_V1 /
 * CRR_CHECKSUM_FLAVOR_CRC32 (cadence_load_verify.h); the next Load of the state then verifies it.
 *
 * Tasks are independent, as in cadence_load_ndc.h: two tasks that name one workflow do not see one another.
 *
 * What stays on the host: tasks that fork a new branch (its token comes from ForkHistoryBranch, a persistence
 * write), the rebuild route, the active-side reapply of a backfill, continue-as-new's new run, and encoding the
 * state blobs for the store (the updated VersionHistories blob is cadence_load_store_vh.h's).
 *
 * This header is an addition to ABI version 8: CRR_ABI_VERSION and every existing struct and entry point are
 * unchanged; crr_sizeof(27) / (28) report the two structs below.
 */
#ifndef CADENCE_LOAD_STORE_H_
#define CADENCE_LOAD_STORE_H_

#include <stddef.h>
#include <stdint.h>

#include "cadence_load.h"
#include "cadence_load_ndc.h"
#include "cadence_load_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A task's last event (16 B): task.getLastEvent() (ndc/replication_task.go), not the last incoming item. */
typedef struct crr_last_event {
    int64_t event_id;
    int64_t version;
} crr_last_event;

/* Precedence, in the order the calls of the path come: NOT_LOADED, NO_ROUTE, on the current route NOT_RESUMED and
 * REPLAY_FAILED, then NEW_BRANCH and VH_ERROR; a task that passes them all is generated. */
enum crr_store_outcome {
    CRR_STORE_APPLIED = 0,          /* generated from the state the resumed replay left */
    CRR_STORE_BACKFILLED = 1,       /* generated from the stored state with the task's last event on its branch */
    CRR_STORE_NOT_LOADED = 2,       /* the state's load status is not CRR_LOAD_OK, or the task's wf is past the batch */
    CRR_STORE_NO_ROUTE = 3,         /* CRR_ROUTE_NONE, CRR_ROUTE_REBUILD or CRR_ROUTE_BAD_REQUEST: nothing committed here */
    CRR_STORE_NEW_BRANCH = 4,       /* CRR_NDC_NEW_BRANCH: the branch's token is ForkHistoryBranch's */
    CRR_STORE_VH_ERROR = 5,         /* the branch update fails: status = CRR_ERR_VH_INVALID_ITEM (NewVersionHistoryItem,
                                       versionHistory.go:37-43), CRR_ERR_VH_LOWER_VERSION or
                                       CRR_ERR_VH_EVENT_ID_NOT_INCREASING (AddOrUpdateItem); CRR_ERR_NDC_BAD_INDEX: the
                                       decision's branch_index is not a stored branch (GetVersionHistory), or on the
                                       current route not the current one */
    CRR_STORE_NOT_RESUMED = 6,      /* CRR_ROUTE_APPLY_CURRENT, but the workflow is not in the resumed batch, its
                                       descriptor lacks CRR_WF_FLAG_RESUME, or no replay outputs were given */
    CRR_STORE_REPLAY_FAILED = 7     /* the resumed replay's exec row has a status other than CRR_OK: status carries it */
};

/* Per task (16 B).  value and payload_len are zero unless the outcome is APPLIED or BACKFILLED; status is zero
 * but for CRR_STORE_VH_ERROR and CRR_STORE_REPLAY_FAILED. */
typedef struct crr_store_row {
    uint32_t value;                 /* CRC32-IEEE of 0x59 + the thriftrw MutableStateChecksumPayload */
    int32_t  outcome;               /* crr_store_outcome */
    uint32_t payload_len;           /* bytes of the payload, the 0x59 preamble included */
    int32_t  status;                /* crr_status_code */
} crr_store_row;

/* Generate the checksum to store for every task.  `in`, `scratch`, `scratch_bytes` and `summary_host` are those
 * of a finished crr_load_states_plan; `tasks`, `results`, `routes` (device, [n_tasks]) and `branches` with
 * `ndc_plan_host` are the arguments and outputs of the crr_load_ndc_run that decided these tasks (n_tasks may be a
 * prefix of them); `last_events` is device [n_tasks].  For the tasks routed to the current branch: `replay_in`
 * and `replay_out` are the crr_inputs the resumed replay ran with and its crr_outputs (both NULL: none was run),
 * `position` a device uint32[in->n_wf] giving each workflow's position in that batch -- the inverse of the
 * `perm` crr_load_states_place took; UINT32_MAX: not in the batch; NULL: workflow w at position w.  `result` is
 * device [n_tasks].
 *
 * Everything but `result` is only read.  Each count taken from a post-replay exec row is clamped to the
 * descriptor's capacity before a row is addressed, and every index taken from a task, a decision or the branch
 * table is checked against the sizes of `ndc_plan_host` first.
 *
 * Enqueued on `stream` behind the replay, no synchronisation; n_tasks == 0 launches nothing.  Returns 0, -1 on an
 * invalid argument (`in` not the planned batch's shape included), else the hipError_t. */
int crr_load_store_checksums(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                             const crr_load_summary* summary_host, const crr_repl_task* tasks,
                             const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                             const crr_ndc_route* routes, const crr_load_branches* branches,
                             const crr_load_ndc_sizes* ndc_plan_host, const crr_inputs* replay_in,
                             const crr_outputs* replay_out, const uint32_t* position, crr_store_row* result,
                             void* stream);

/* Host restatement (libcadence_host.so): host pointers; decodes `in` as crr_load_states_host does and walks its
 * branches as crr_load_branches_host does, then runs the same payload code.  The post-replay state is a dense
 * image indexed by workflow, as crr_load_states_host writes one (exec, rows[0..5] and offsets are read;
 * `status`, when set, marks with a non-zero value the workflows that were not resumed); NULL: no task can be
 * CRR_STORE_APPLIED.  Returns 0, -1 on an invalid argument, -2 out of memory. */
int crr_load_store_checksums_host(const crr_state_batch* in, const crr_repl_task* tasks,
                                  const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                                  const crr_ndc_route* routes, const crr_load_image* after, crr_store_row* result,
                                  int threads);

#ifdef __cplusplus
}
#endif
#endif /* CADENCE_LOAD_STORE_H_ */
