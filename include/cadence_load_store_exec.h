/*
 * cadence_load_store_exec.h -- the execution blob to store with a persisted state after a routed replication task
 * was committed, on the device.
 *
 * cadence_load_store.h generates the checksum Go writes back with the state, cadence_load_store_vh.h the updated
 * VersionHistories blob and cadence_load_mutation.h the pending-entry mutation.  The one blob every committed task
 * writes is ExecutionInfo (CloseTransactionAsMutation, service/history/execution/mutable_state_builder.go:3998-3999):
 * sqlblobs.WorkflowExecutionInfo as workflowExecutionInfoToThrift fills it
 * (common/persistence/serialization/thrift_mapper.go:186-250).  Every thrift scalar is fixed-width and thriftrw
 * writes the set fields in ascending id, so the new blob is the stored blob with a bounded number of edits, and the
 * strings, the memo and the search attributes the replay never touches are copied, not parsed.
 *
 * One result per task, the arguments and the independence of crr_load_store_checksums: two tasks naming one
 * workflow do not see one another.  Outcome and status are load_decode.h's store_decide with the branch-table check
 * of store_task, so they equal crr_store_row's for the same inputs.  Only CRR_STORE_APPLIED and
 * CRR_STORE_BACKFILLED produce a blob; every other outcome has length 0.
 *
 * The splice.  The stored execution blob is walked field by field at top level:
 *   - a field that is not overridden is copied verbatim (unknown ids, lists and maps included);
 *   - an overridden field takes its new value in place;
 *   - an overridden field the stored blob lacks is inserted before the first stored field with a greater id, or
 *     before the stop byte when there is none (several at one place in ascending id);
 *   - a field to be omitted is dropped.
 * For a blob Go wrote (fields ascending, each once) the result is byte-equal to the full re-encoding (DESIGN.md
 * section 4, "The execution blob to store").
 *
 * Overrides of CRR_STORE_BACKFILLED (nothing is replayed; ndc/history_replicator.go:490-542):
 *    56 LastUpdatedTimeNanos   the task's now_ns (mutable_state_builder.go:3989)
 *   108 HistorySize            the stored value (absent: 0) + the task's history_size_delta
 *   122 VersionHistories       the task's bytes from crr_load_store_vh_run
 * Overrides of CRR_STORE_APPLIED: those three, and from the post-replay exec row at the workflow's device position
 *    34 State, 36 CloseStatus, 48 LastEventTaskID, 50 LastFirstEventID, 52 LastProcessedEvent, 58 DecisionVersion,
 *    60 DecisionScheduleID, 62 DecisionStartedID, 64 DecisionTimeout, 66 DecisionAttempt, 70 CancelRequested,
 *   106 SignalCount;
 *    68 / 69 / 71 the decision's started / scheduled / original scheduled times, CRR_ZERO_TIME written as
 *       time.Time{}.UnixNano();
 *    18 CompletionEventBatchID: written (inserted when absent) when the row's value is not EmptyEventID, omitted
 *       otherwise (thrift_mapper.go:195 hands the *int64 on as it is and thriftrw leaves a nil one out; DESIGN.md
 *       section 4 says which writers set it always);
 *    78 / 110 / 112 / 114 become empty strings and 80 becomes 0 (ClearStickyness, state_builder.go:108 ->
 *       mutable_state_builder.go:1504-1510);
 *    74 DecisionRequestID by the row's decision_request_src: CRR_SRC_EMPTY_UUID "emptyUuid"; CRR_SRC_NONE "";
 *       below the state's blob_count the stored field as it is; at or above it the RequestId of event number
 *       src - blob_count of the task (field 30 of its decisionTaskStartedEventAttributes, field 90 of the event),
 *       counted across the workflow's blobs in `task_blobs`.
 * Everything else, 115 AutoResetPoints included: as stored.
 *
 * Left to the host: the outcome stays as decided, the length is 0 and crr_exec_blob_row.flags says why.
 *   CRR_EXEC_BLOB_HOST_RESET_POINTS       the reset points changed: addBinaryCheckSumIfNotExists
 *                                         (mutable_state_builder.go:1911-1971) also rewrites
 *                                         SearchAttributes["BinaryChecksums"] and stamps the point with the host clock
 *   CRR_EXEC_BLOB_HOST_SEARCH_ATTRIBUTES  the task's events hold an UpsertWorkflowSearchAttributes (:2933 merges
 *                                         the map)
 *   CRR_EXEC_BLOB_HOST_REQUEST_ID         the request id comes from the task and no task blobs were given, or the
 *                                         event is not found or is not a DecisionTaskStarted
 *   CRR_EXEC_BLOB_HOST_STORED_SHAPE       the stored blob holds an overridden field with another thrift type or
 *                                         twice, or needs more edits than a script holds
 *
 * Two calls, as crr_load_store_vh_plan / _run.  The plan leaves per task an edit script in the work buffer: copy
 * segments (from the stored bytes, the VersionHistories bytes, the task's blob or a literal of at most 8 bytes) and
 * scalar patches (offset, width, big-endian value); the run call takes the same work buffer.
 *
 * This header is an addition to ABI version 8: CRR_ABI_VERSION and every existing struct and entry point are
 * unchanged; crr_sizeof(36) / (37) / (38) report crr_exec_blob_task, crr_exec_blob_row and crr_exec_blob_sizes (29
 * and 32 stay unassigned and report 0).
 */
#ifndef CADENCE_LOAD_STORE_EXEC_H_
#define CADENCE_LOAD_STORE_EXEC_H_

#include <stddef.h>
#include <stdint.h>

#include "cadence_ingest.h"
#include "cadence_load_store_vh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRR_EXEC_BLOB_HOST_RESET_POINTS      1u
#define CRR_EXEC_BLOB_HOST_SEARCH_ATTRIBUTES 2u
#define CRR_EXEC_BLOB_HOST_REQUEST_ID        4u
#define CRR_EXEC_BLOB_HOST_STORED_SHAPE      8u

/* What a task brings beside crr_repl_task (16 B). */
typedef struct crr_exec_blob_task {
    int64_t now_ns;                   /* the commit's clock: LastUpdatedTimeNanos */
    int64_t history_size_delta;       /* bytes of history the task appended (may be negative) */
} crr_exec_blob_task;

/* Per task (24 B). */
typedef struct crr_exec_blob_row {
    int32_t  outcome;                 /* crr_store_outcome, cadence_load_store.h: same values, same precedence */
    int32_t  status;                  /* as crr_store_row.status */
    uint32_t flags;                   /* CRR_EXEC_BLOB_HOST_* */
    uint32_t len;                     /* bytes of the blob, 0 unless generated on the device */
    int64_t  next_event_id;           /* the executions.next_event_id column to write beside the blob: the
                                         post-replay row's for APPLIED, the stored one for BACKFILLED, else 0 */
} crr_exec_blob_row;

/* Host struct, valid when the plan returns. */
typedef struct crr_exec_blob_sizes {
    int32_t  err;                     /* 0 or CRR_INGEST_SCRATCH_TOO_SMALL */
    uint32_t n_tasks;
    uint64_t n_bytes;                 /* blob_off[n_tasks] */
    uint64_t n_blobs;                 /* tasks with a blob */
    uint64_t n_host;                  /* APPLIED / BACKFILLED tasks left to the host (flags != 0) */
    uint64_t work_needed;             /* bytes of work buffer the plan needs */
    uint64_t run_work_needed;         /* bytes of it the run call reads (the same buffer) */
} crr_exec_blob_sizes;

/* Bytes of the work buffer (device, 16-byte aligned). */
size_t crr_load_store_exec_scratch_bytes(uint32_t n_tasks);

/* Decide every task exactly as crr_load_store_checksums does, size its blob and leave its edit script in `work`.
 * The read-only arguments up to `position` are those of crr_load_mutation_plan, with the same meaning and checks.
 * `exec_tasks` is device [n_tasks].  `vh_rows` / `vh_off` / `vh_plan_host` are what crr_load_store_vh_plan left for
 * the same tasks.  `task_blobs` (optional, a host struct of device pointers) holds the tasks' event blobs: workflow
 * p of it is device position p, the batch crr_ingest_plan_resume took; only bytes, blob_off, n_blobs, n_wf and
 * wf[].blob_begin / blob_count are read.  `rows` is device [n_tasks]; `blob_off` device [n_tasks + 1], the
 * exclusive prefix of the rows' lengths.  Synchronises `stream` once to read the totals into `plan`; a work buffer
 * that is too small gives plan->err = CRR_INGEST_SCRATCH_TOO_SMALL with work_needed set, and nothing is launched.
 * n_tasks == 0 launches nothing (blob_off[0] is set to 0 when blob_off is given).  Returns 0; -1 on an invalid
 * argument or when a VersionHistories row disagrees with a task's outcome (another length than its offsets give,
 * or none for a generated task); else the hipError_t. */
int crr_load_store_exec_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                             const crr_load_summary* summary_host, const crr_repl_task* tasks,
                             const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                             const crr_ndc_route* routes, const crr_load_branches* branches,
                             const crr_load_ndc_sizes* ndc_plan_host, const crr_inputs* replay_in,
                             const crr_outputs* replay_out, const uint32_t* position,
                             const crr_exec_blob_task* exec_tasks, const crr_vh_blob_row* vh_rows,
                             const uint64_t* vh_off, const crr_vh_blob_sizes* vh_plan_host,
                             const crr_blob_batch* task_blobs, crr_exec_blob_row* rows, uint64_t* blob_off, void* work,
                             size_t work_bytes, crr_exec_blob_sizes* plan, void* stream);

/* Emit every blob at out_bytes + blob_off[k]: the plan's arguments again (`rows`, `blob_off` and `work` as it left
 * them, `plan_host` the finished plan), `vh_bytes` what crr_load_store_vh_run writes -- the call is enqueued behind
 * it on the same stream -- and `out_bytes`, device, 16-byte aligned, with `out_capacity` bytes.  Exactly
 * plan_host->n_bytes bytes are written.  Each lane of the kernel owns 16 bytes of the output and stores them at
 * once (the lane that owns a shorter tail stores that tail byte by byte); which bytes a lane owns follows from its
 * index alone.  Every offset a script, the stored blob or the task's blob gives is checked against the buffer it
 * indexes; a byte whose lookup fails is zero.  No synchronisation; n_bytes == 0 launches nothing.  Returns 0, -1
 * on an invalid argument or when out_capacity < n_bytes (nothing is launched), else the hipError_t. */
int crr_load_store_exec_run(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                            const crr_load_summary* summary_host, const crr_repl_task* tasks,
                            const crr_last_event* last_events, const crr_ndc_result* results, const crr_ndc_route* routes,
                            const crr_load_branches* branches, const crr_load_ndc_sizes* ndc_plan_host,
                            const crr_inputs* replay_in, const crr_outputs* replay_out, const uint32_t* position,
                            const crr_exec_blob_task* exec_tasks, const crr_vh_blob_row* vh_rows, const uint64_t* vh_off,
                            const crr_vh_blob_sizes* vh_plan_host, const crr_blob_batch* task_blobs,
                            const crr_exec_blob_row* rows, const uint64_t* blob_off, const void* work, size_t work_bytes,
                            const crr_exec_blob_sizes* plan_host, const uint8_t* vh_bytes, uint8_t* out_bytes,
                            size_t out_capacity, void* stream);

/* Host restatement (libcadence_host.so): host pointers and the dense after-image, as crr_load_mutation_host; the
 * VersionHistories blobs are generated inside (crr_load_store_vh_host's), the blobs written by the plain sequential
 * writer.  `task_blobs`: host pointers, workflow w of it is workflow w of `in` (NULL: none).  `upserts`: per
 * workflow of `in`, nonzero when the task's events hold an UpsertWorkflowSearchAttributes (NULL: none do) -- the
 * host has no event columns to read it from.  `rows`, `blob_off` and `out` may each be NULL: call once to size the
 * buffers from `plan`, then again with them.  With `out`: -1 and nothing written when out_capacity < n_bytes.
 * Returns 0, -1 on an invalid argument, -2 out of memory. */
int crr_load_store_exec_host(const crr_state_batch* in, const crr_repl_task* tasks, const crr_last_event* last_events,
                             uint32_t n_tasks, const crr_ndc_result* results, const crr_ndc_route* routes,
                             const crr_load_image* after, const crr_exec_blob_task* exec_tasks,
                             const crr_blob_batch* task_blobs, const uint8_t* upserts, crr_exec_blob_row* rows,
                             uint64_t* blob_off, uint8_t* out, size_t out_capacity, crr_exec_blob_sizes* plan,
                             int threads);

#ifdef __cplusplus
}
#endif
#endif /* CADENCE_LOAD_STORE_EXEC_H_ */
