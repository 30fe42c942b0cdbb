/*
 * cadence_load_resume.h -- the resumed replay of routed replication tasks planned on the device from the persisted
 * states the loader decoded.
 *
 * cadence_load.h decodes persisted states into a dense image in its scratch, cadence_load_ndc.h routes replication
 * tasks against them, and crr_ingest_plan_resume / crr_ingest_layout_resume (cadence_ingest.h) decode a task's event
 * blobs onto loaded rows.  Between them a caller had to download the whole image (crr_load_states_read), lay the
 * tasks' events out on the host with the loaded counts added in, and upload the result.  This header is that link on
 * the device: which task is applied onto which state, the tasks' blobs and the states' key dictionaries gathered as
 * the blob batch and the seeds crr_ingest_plan_resume takes, and -- once that plan has counted this call's inserts --
 * the crr_workflow descriptors crr_ingest_layout_resume continues in place, with the loaded branch tokens in an arena.
 *
 * Layout.  The canonical one only: stride 1, no wave tail (crr_ingest_resume.wave_begin 0), no tiers.  Device
 * position p is loaded workflow p: `perm` is NULL for crr_load_states_place and `position` is the identity for the
 * store calls of cadence_load_store.h and its siblings.  Every state has a position; only applied ones carry events.
 *
 * Outcome per task (crr_load_resume_row.outcome), in this precedence:
 *   CRR_RESUME_NOT_ROUTED   its route is not CRR_ROUTE_APPLY_CURRENT
 *   CRR_RESUME_NOT_LOADED   its workflow index is out of range, or that state's load status is not CRR_LOAD_OK
 *   CRR_RESUME_SHADOWED     another task of a lower index is applied onto the same workflow
 *   CRR_RESUME_APPLIED      its events are replayed onto the state at `position` (its workflow index)
 * `position` is UINT32_MAX unless the outcome is APPLIED or SHADOWED.
 *
 * The gathered batch.  `bytes`: the applied tasks' blobs in position order, each byte-identical to its source;
 * zeros up to the next multiple of 16 (seed_base); then the applied states' dictionary strings in position order.
 * Exactly sizes.n_bytes = seed_base + key_bytes bytes are written; the buffer must be readable CRR_INGEST_PAD
 * bytes past them, which are not written.  `wf[p]`: the winning task's crr_blob_wf (workflow k of `task_blobs` is
 * task k) with blob_begin / blob_count rewritten so that ranges stay consecutive and new_run_wf mapped to the
 * position its task is applied at (-1 when it is not); a position without a task holds zeros with blob_begin the
 * prefix, blob_count 0, new_run_wf -1 and final_token_len UINT32_MAX.  The strings, domains and n_domains of the
 * gathered batch are those of `task_blobs`.  Seeds: key_begin / key_count per position, key_off / key_len per
 * entry, offsets into the new `bytes`, ids the loader's (1..K in the loader's order).  task_of[p]: the applied
 * task's index, -1 for none.  A task whose blob range or offsets do not lie inside `task_blobs` is applied with no
 * blobs.
 *
 * The descriptors (crr_load_resume_finalize, after crr_ingest_plan_resume over the gathered batch).  Per position:
 * each of the seven table capacities is the loaded count of that table (zero unless applied) plus the ingest plan's
 * insert count of this call; task_cap is the ingest plan's; bases are the exclusive prefixes of the capacities over
 * the positions (flatten.assign_canonical_tables); start_token_off / _len name the loaded current-branch token
 * copied into `arena` (each padded to 8 bytes with zeros; length 0 unless applied); final_token_len is UINT32_MAX;
 * init_version, now_ns, retention_days and flags come from wf[p], with CRR_WF_FLAG_RESUME on applied positions;
 * ev_count and empty_batch_at are the ingest plan's (0 and -1 at a position without blobs), ev_begin is left 0 for
 * crr_ingest_layout_resume to write.  That call sets CRR_WF_FLAG_RESUME on every descriptor it continues:
 * crr_load_resume_settle, enqueued behind it, clears it again at the positions without a task.
 *
 * Plan / run semantics, argument checks and error returns follow cadence_load_mutation.h.  This header is an
 * addition to ABI version 8: CRR_ABI_VERSION and every existing struct and entry point are unchanged;
 * crr_sizeof(40..43) report crr_load_resume_row, crr_load_resume_sizes, crr_load_resume_out and
 * crr_load_resume_totals (39 stays unassigned and reports 0).
 */
#ifndef CADENCE_LOAD_RESUME_H_
#define CADENCE_LOAD_RESUME_H_

#include <stddef.h>
#include <stdint.h>

#include "cadence_ingest.h"
#include "cadence_load.h"
#include "cadence_load_ndc.h"

#ifdef __cplusplus
extern "C" {
#endif

enum crr_resume_outcome {
    CRR_RESUME_APPLIED = 0,
    CRR_RESUME_SHADOWED = 1,
    CRR_RESUME_NOT_ROUTED = 2,
    CRR_RESUME_NOT_LOADED = 3
};

/* Per task (8 B). */
typedef struct crr_load_resume_row {
    int32_t  outcome;                  /* crr_resume_outcome */
    uint32_t position;                 /* APPLIED / SHADOWED: the device position (the workflow index); else UINT32_MAX */
} crr_load_resume_row;

/* Host struct, valid when the plan returns. */
typedef struct crr_load_resume_sizes {
    int32_t  err;                      /* 0 or CRR_INGEST_SCRATCH_TOO_SMALL */
    uint32_t n_tasks;
    uint32_t n_wf;                     /* positions: the loaded workflows */
    uint32_t reserved;
    uint64_t n_applied;                /* applied tasks = positions with a task */
    uint64_t n_blobs;                  /* their blobs */
    uint64_t blob_bytes;               /* ... and those blobs' bytes */
    uint64_t n_keys;                   /* dictionary entries of the applied states */
    uint64_t key_bytes;                /* ... and their string bytes */
    uint64_t token_bytes;              /* the applied states' current-branch tokens, each padded to 8: the arena */
    uint64_t n_bytes;                  /* what the gather writes to `bytes`: blob_bytes rounded up to 16 + key_bytes */
    uint64_t work_needed;              /* bytes of work buffer the three calls need */
} crr_load_resume_sizes;

/* The gather's outputs: device buffers.  bytes 16-byte aligned, the others 8-byte aligned. */
typedef struct crr_load_resume_out {
    uint8_t*     bytes;                /* [n_bytes] written, readable to n_bytes + CRR_INGEST_PAD */
    uint64_t     bytes_capacity;       /* bytes that may be written (>= n_bytes) */
    uint64_t*    blob_off;             /* [n_blobs + 1] */
    uint64_t     blob_capacity;        /* blobs (>= n_blobs; blob_off holds one more entry) */
    crr_blob_wf* wf;                   /* [n_wf] */
    uint32_t*    key_begin;            /* [n_wf] */
    uint32_t*    key_count;            /* [n_wf] */
    uint64_t*    key_off;              /* [n_keys] */
    uint32_t*    key_len;              /* [n_keys] */
    uint64_t     key_capacity;         /* entries (>= n_keys) */
    int32_t*     task_of;              /* [n_wf] */
} crr_load_resume_out;

/* Host struct, valid when the finalize returns: what sizes crr_outputs and the arena. */
typedef struct crr_load_resume_totals {
    uint64_t table_rows[8];            /* act, timer, child, rc, sig, vh, rp, tasks slot-table rows */
    uint64_t arena_bytes;              /* = sizes.token_bytes */
} crr_load_resume_totals;

/* Rows of the per-workflow counts crr_ingest_resume_counts exposes and crr_load_resume_finalize / _host read:
 * ev_count, empty_batch_at, then this call's inserts per table (act, timer, child, rc, sig, vh, rp, tasks). */
#define CRR_RESUME_COUNT_ROWS 10

/* The per-workflow pass of the last crr_ingest_plan_resume (or crr_ingest_plan) that used `scratch` with this batch
 * shape: *counts is a device pointer to int32 [CRR_RESUME_COUNT_ROWS][*stride] inside the scratch, workflow w of
 * row r at counts[r * stride + w].  Nothing is launched or copied.  Returns 0, -1 on an invalid argument. */
int crr_ingest_resume_counts(const crr_blob_batch* in, void* scratch, size_t scratch_bytes, const int32_t** counts,
                             uint64_t* stride);

/* Bytes of the work buffer the three calls share (device, 16-byte aligned). */
size_t crr_load_resume_scratch_bytes(uint32_t n_wf, uint32_t n_tasks);

/* Decide every task and size the gather.  `in`, `scratch`, `summary_host`: the planned state batch
 * (crr_load_states_plan); `tasks`, `routes` (device [n_tasks]) as crr_load_ndc_run left them; `task_blobs`: a host
 * struct of device pointers, the tasks' event blobs in task order (workflow k of it is task k; a task past its n_wf
 * has no blobs).  Fills `rows` (device [n_tasks]) and the per-position counts and offsets in `work`.  Counts become
 * offsets through block sums and one scan; nothing is scanned serially over tasks or positions.  Synchronises `stream` once to read the totals into
 * `plan`; a work buffer that is too small gives plan->err = CRR_INGEST_SCRATCH_TOO_SMALL with work_needed set, and
 * nothing is launched.  Returns 0, -1 on an invalid argument or when a total does not fit 32 bits, else the
 * hipError_t. */
int crr_load_resume_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                         const crr_load_summary* summary_host, const crr_repl_task* tasks, const crr_ndc_route* routes,
                         uint32_t n_tasks, const crr_blob_batch* task_blobs, crr_load_resume_row* rows, void* work,
                         size_t work_bytes, crr_load_resume_sizes* plan, void* stream);

/* Write the gathered batch, the seeds and task_of: the same read-only arguments and `work` as the plan left it
 * (`rows` is not read: the winners are in `work`; it may be NULL), `plan_host` the finished plan.  The byte gather is output-stationary: lane i owns bytes [16 i, 16 i + 16) of
 * `bytes`, finds its sources by an upper-bound search over the planned offsets and stores one dwordx4; the lane that
 * owns a short tail stores it byte by byte, so exactly n_bytes bytes are written.  A source range that no longer
 * lies where the plan found it reads as zeros.  Enqueued on `stream`, no synchronisation.  Returns 0, -1 on an
 * invalid argument or a capacity below the plan's total (nothing is launched), else the hipError_t. */
int crr_load_resume_gather(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                           const crr_load_summary* summary_host, const crr_repl_task* tasks,
                           const crr_blob_batch* task_blobs, const crr_load_resume_row* rows, const void* work,
                           size_t work_bytes, const crr_load_resume_sizes* plan_host, const crr_load_resume_out* out,
                           void* stream);

/* Write the descriptors and the token arena.  `gathered_wf`: the gather's wf[n_wf]; `counts` / `count_stride`: what
 * crr_ingest_resume_counts gave after crr_ingest_plan_resume over the gathered batch (wave_begin 0, the gather's
 * seeds); `wf` (device [n_wf]) the descriptors, `arena` a device buffer of which `arena_capacity` (>=
 * plan_host->token_bytes) bytes may be written.  A capacity is clamped to INT32_MAX, the descriptor's field.
 * Synchronises `stream` once to read `totals`, which is written only when the call returns 0.  Returns 0, -1 on an
 * invalid argument, else the hipError_t. */
int crr_load_resume_finalize(const void* scratch, size_t scratch_bytes, const crr_load_summary* summary_host,
                             const crr_blob_wf* gathered_wf, const int32_t* counts, uint64_t count_stride, void* work,
                             size_t work_bytes, const crr_load_resume_sizes* plan_host, crr_workflow* wf, uint8_t* arena,
                             size_t arena_capacity, crr_load_resume_totals* totals, void* stream);

/* After crr_ingest_layout_resume has continued the descriptors in place -- it sets CRR_WF_FLAG_RESUME on every one it
 * is given -- clear that flag again at the positions without a task (task_of[p] < 0), so that only applied workflows
 * resume and the others are plain workflows without events.  `task_of` (the gather's) and `wf` are device [n_wf].
 * Enqueued on `stream`, no synchronisation.  Returns 0, -1 on an invalid argument, else the hipError_t. */
int crr_load_resume_settle(const int32_t* task_of, crr_workflow* wf, uint32_t n_wf, void* stream);

/* Host restatement (libcadence_host.so): host pointers throughout.  `counts` (int32 [CRR_RESUME_COUNT_ROWS][n_wf],
 * stride n_wf) may be NULL: the descriptors are then not written and `totals` holds only arena_bytes.  `rows`, `out`,
 * `wf` and `arena` may each be NULL: call once to size the buffers from `plan`, then again with them; the descriptors
 * are written when `counts`, `out` (they read its wf) and `wf` are all given.  With `out`, `wf` or `arena`: -1 and
 * nothing written when a capacity is below its total.  Returns 0, -1 on an invalid argument, -2 out of
 * memory. */
int crr_load_resume_host(const crr_state_batch* in, const crr_repl_task* tasks, const crr_ndc_route* routes,
                         uint32_t n_tasks, const crr_blob_batch* task_blobs, const int32_t* counts,
                         crr_load_resume_row* rows, const crr_load_resume_out* out, crr_workflow* wf, uint8_t* arena,
                         size_t arena_capacity, crr_load_resume_sizes* plan, crr_load_resume_totals* totals, int threads);

#ifdef __cplusplus
}
#endif
#endif /* CADENCE_LOAD_RESUME_H_ */
