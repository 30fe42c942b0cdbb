/*
 * cadence_load_mutation.h -- the pending-entry mutation to store with a persisted state after a routed replication
 * task was committed, on the device.
 *
 * cadence_load_store.h generates the checksum Go writes back with the state and cadence_load_store_vh.h the updated
 * VersionHistories blob.  The rest of the write is not the state again: CloseTransactionAsMutation
 * (service/history/execution/mutable_state_builder.go:3959-4031) writes ExecutionInfo, always, and per pending map
 * the entries to upsert and the IDs to delete (:4002-4011), which the SQL store applies as one REPLACE per upserted
 * entry and one DELETE per deleted ID (common/persistence/sql/workflowStateMaps.go:35-120, 212-265, 329-395,
 * 468-520, 579-635).  crr_compact_rows is the snapshot (CloseTransactionAsSnapshot): every live row of every
 * workflow.  This header is its mutation counterpart: per committed task the post-replay exec row, the rows to
 * upsert gathered dense, and the IDs to delete, so that only those cross to the host.  Which entries changed carries
 * no strings; the host materialises the strings of the gathered rows from their *_src fields, as for any row.
 *
 * One result per task, the arguments and the independence of crr_load_store_checksums: two tasks naming one
 * workflow do not see one another.  The outcome is the decision crr_load_store_checksums makes (load_decode.h's
 * store_decide and the same branch-table check), so outcome and status equal crr_store_row's for the same inputs.
 *
 *   CRR_STORE_APPLIED.  The state before is the loader's dense image of the workflow (what crr_load_states_verify
 *   reads).  The state after is what the resumed replay left at the workflow's device position: the exec row, and
 *   slots 0..n-1 of each pending map at base + j * stride (stride 1 at or past wave_begin), each count clamped to
 *   the descriptor's capacity first, exactly as crr_load_store_checksums addresses them.
 *
 *   Entries are matched per map: activities by schedule_id; children, request-cancels and signals by initiated_id;
 *   timers by `key`, the interned TimerID, which is the store's key column (a timer that fired and was started
 *   again under the same TimerID inside the task is one upsert and no delete).
 *     upsert  a row live after that has no match before, or differs from its match in a persisted field.  The
 *             persisted fields are every field of the row image filled from a blob or a key column, and every
 *             *_src; the derived ones do not count: the activity's CRR_ROW_MAPPED flag and last_hb_timeout_vis_s
 *             (and the child row's reserved word).
 *     delete  a key live before with no match after.
 *   An entry created and removed inside the task, and an entry the task did not touch, are in neither list.
 *   Both sides are ascending by their first field (the ID; a timer's started_id), so the four ID-keyed maps are one
 *   merge walk.  For timers the walk over started_id gives the candidates: equal started_id and key is a match; a
 *   row only after is an upsert; a row only before is a delete unless a row after carries its key.  On states whose
 *   TimerIDs and started_ids are unique on each side (the loader refuses others, CRR_LOAD_DUPLICATE_ID) that is
 *   matching by key.  Work per task: the rows of both sides once, plus (timers only before) x (timers after) key
 *   compares -- bounded by CRR_LOAD_MAX_BLOBS and the descriptor's capacities.
 *
 *   The exec row of an APPLIED task is always part of the mutation.  CRR_MUTATION_RESET_POINTS_CHANGED is set when
 *   the reset points differ between before and after (count or any row): the host re-encodes AutoResetPoints only
 *   then.
 *
 *   CRR_STORE_BACKFILLED: nothing pending changes and no exec row is gathered; the mutation is the VersionHistories
 *   blob and the checksum of the two other headers.  The outcome is reported with zero counts.
 *   Every other outcome: zero counts, the status as in crr_store_row.
 *
 * Against Go's own sets: Go's delete sets also hold IDs created and deleted inside the
 * transaction (a no-op on the store); Go upserts every touched entry even when no persisted field changed; Go puts
 * a restarted TimerID into both sets.  What is reported here is the state-equivalent mutation: the store after
 * applying it equals the store of the post-task snapshot.  Signal-requested IDs and buffered events stay the host's.
 *
 * Order.  Exec rows dense in task order.  Per map the upserted rows dense in task order and within a task in slot
 * order (ascending by ID; timers by started_id), as full row images; the deleted keys in task order and within a task
 * in the order of the rows before (ascending by ID; timers by started_id), as int64 (a timer's `key` widened).
 *
 * Two calls, as crr_load_store_vh_plan / _run: the plan counts per task, turns the counts into offsets and fills the
 * rows (one synchronisation, to read the totals back); the caller sizes the outputs from the plan; the run call
 * writes them and does not synchronise.
 *
 * This header is an addition to ABI version 8: CRR_ABI_VERSION and every existing struct and entry point are
 * unchanged; crr_sizeof(33) / (34) / (35) report crr_mutation_row, crr_mutation_sizes and crr_mutation_out (32 stays
 * unassigned and reports 0).
 */
#ifndef CADENCE_LOAD_MUTATION_H_
#define CADENCE_LOAD_MUTATION_H_

#include <stddef.h>
#include <stdint.h>

#include "cadence_load_store.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The pending maps in crr_compact_rows' order: 0 activity, 1 timer, 2 child, 3 request-cancel, 4 signal. */
#define CRR_MUTATION_MAPS 5

#define CRR_MUTATION_RESET_POINTS_CHANGED 1u   /* crr_mutation_row.flags */

/* One map's share of a task's mutation (16 B): ranges of the run call's dense outputs for that map. */
typedef struct crr_mutation_map {
    uint32_t upsert_begin, n_upsert;   /* rows [upsert_begin, + n_upsert) of the map's upserted rows */
    uint32_t delete_begin, n_delete;   /* keys [delete_begin, + n_delete) of the map's deleted keys */
} crr_mutation_map;

/* Per task (96 B).  Counts are zero unless the outcome is CRR_STORE_APPLIED; the begins are the exclusive prefixes
 * over the tasks whatever the outcome. */
typedef struct crr_mutation_row {
    int32_t  outcome;                  /* crr_store_outcome, cadence_load_store.h: same values, same precedence */
    int32_t  status;                   /* as crr_store_row.status */
    uint32_t flags;                    /* CRR_MUTATION_* */
    uint32_t exec_index;               /* rank among the tasks with an exec row; UINT32_MAX: none */
    crr_mutation_map map[CRR_MUTATION_MAPS];
} crr_mutation_row;

/* Host struct, valid when the plan returns. */
typedef struct crr_mutation_sizes {
    int32_t  err;                      /* 0 or CRR_INGEST_SCRATCH_TOO_SMALL */
    uint32_t n_tasks;
    uint64_t n_exec;                   /* exec rows: the tasks with outcome APPLIED */
    uint64_t n_upsert[CRR_MUTATION_MAPS];   /* upserted rows per map */
    uint64_t n_delete[CRR_MUTATION_MAPS];   /* deleted keys per map */
    uint64_t work_needed;              /* bytes of work buffer the plan needs */
    uint64_t run_work_needed;          /* bytes of work buffer the run call needs (its directory) */
} crr_mutation_sizes;

/* The run call's outputs: device buffers, 8-byte aligned, with their capacities in rows / keys.  A buffer whose
 * total is zero may be NULL. */
typedef struct crr_mutation_out {
    crr_exec_row* exec;
    uint64_t      exec_capacity;
    void*         upsert[CRR_MUTATION_MAPS];          /* crr_activity_row / crr_timer_row / crr_child_row /
                                                         crr_initiated_row / crr_initiated_row */
    uint64_t      upsert_capacity[CRR_MUTATION_MAPS];
    int64_t*      deleted[CRR_MUTATION_MAPS];
    uint64_t      delete_capacity[CRR_MUTATION_MAPS];
} crr_mutation_out;

/* Bytes of the plan's work buffer (device, 16-byte aligned). */
size_t crr_load_mutation_scratch_bytes(uint32_t n_tasks);

/* Decide every task exactly as crr_load_store_checksums does, classify the pending entries of the APPLIED ones and
 * fill `rows` (device [n_tasks]).  The read-only arguments are those of crr_load_store_checksums, with the same
 * meaning and the same checks; `work` / `work_bytes` the work buffer.  Synchronises `stream` once to read the totals
 * into `plan`; a work buffer that is too small gives plan->err = CRR_INGEST_SCRATCH_TOO_SMALL with work_needed set,
 * and nothing is launched.  n_tasks == 0 launches nothing.  Returns 0, -1 on an invalid argument or when a total
 * does not fit 32 bits, else the hipError_t. */
int crr_load_mutation_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                           const crr_load_summary* summary_host, const crr_repl_task* tasks,
                           const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                           const crr_ndc_route* routes, const crr_load_branches* branches,
                           const crr_load_ndc_sizes* ndc_plan_host, const crr_inputs* replay_in,
                           const crr_outputs* replay_out, const uint32_t* position, crr_mutation_row* rows,
                           void* work, size_t work_bytes, crr_mutation_sizes* plan, void* stream);

/* Write the planned mutation: the same read-only arguments, `rows` as the plan left them, `plan_host` the finished
 * plan (n_tasks is its n_tasks), `work` a device buffer (16-byte aligned) of at least plan_host->run_work_needed
 * bytes, which may be the plan's.  Exactly n_exec exec rows, n_upsert[t] rows and n_delete[t] keys are written and
 * nothing else.  One lane per task repeats the walk, writes the deleted keys and a directory -- the source slot of
 * each exec row and of each upserted row -- into `work`; then one lane per 8-byte word of each output finds its row
 * through the directory and stores the word, so which word a lane writes follows from its index alone.  A row whose
 * directory entry was not written (the inputs changed since the plan) is zeros, as is a key past what the walk finds
 * now.  Enqueued on `stream`, no synchronisation; n_tasks == 0 launches nothing.  Returns 0, -1 on an invalid
 * argument, a capacity below the plan's total or too small a work buffer (nothing is launched), else the
 * hipError_t. */
int crr_load_mutation_run(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                          const crr_load_summary* summary_host, const crr_repl_task* tasks,
                          const crr_last_event* last_events, const crr_ndc_result* results, const crr_ndc_route* routes,
                          const crr_load_branches* branches, const crr_load_ndc_sizes* ndc_plan_host,
                          const crr_inputs* replay_in, const crr_outputs* replay_out, const uint32_t* position,
                          const crr_mutation_row* rows, const crr_mutation_sizes* plan_host, const crr_mutation_out* out,
                          void* work, size_t work_bytes, void* stream);

/* Host restatement (libcadence_host.so): host pointers and the dense after-image, as crr_load_store_checksums_host
 * (rows[6], the reset points, is read too when set).  `rows` and `out` may each be NULL: call once to size the
 * buffers from `plan`, then again with them.  With `out`: -1 and nothing written when a capacity is below its total.
 * Returns 0, -1 on an invalid argument, -2 out of memory. */
int crr_load_mutation_host(const crr_state_batch* in, const crr_repl_task* tasks, const crr_last_event* last_events,
                           uint32_t n_tasks, const crr_ndc_result* results, const crr_ndc_route* routes,
                           const crr_load_image* after, crr_mutation_row* rows, const crr_mutation_out* out,
                           crr_mutation_sizes* plan, int threads);

#ifdef __cplusplus
}
#endif
#endif /* CADENCE_LOAD_MUTATION_H_ */
