/*
 * cadence_load_store_vh.h -- the VersionHistories blob to store with a persisted state after a routed replication
 * task was committed, on the device.
 *
 * cadence_load_store.h generates the four bytes of the checksum Go writes back with the state.  What Go writes
 * with them on both routes that commit a loaded state is the updated VersionHistories: CloseTransactionAsMutation
 * leads to SerializeVersionHistories (common/persistence/serializer.go:178-183), whose thriftrw DataBlob is field
 * 122 of the execution blob (encoding "thriftrw", field 124).  On the current route every committed task changes
 * it (at the least the last item's event ID); on the backfill route it is the only thing that changes.
 *
 * thriftrw is thrift binary, and Go always writes every field of the three structs (FromVersionHistories takes the
 * address of the index; VersionHistory.ToInternalType always makes a non-nil token and a non-nil items slice,
 * versionHistory.go:125-139; FromVersionHistoryItem takes both addresses), so the blob is exactly
 *
 *   59                                   preambleVersion0
 *   08 00 0a  <i32 current index>
 *   0f 00 14  0c  <i32 n histories>
 *     per history:  0b 00 0a <i32 len> <token bytes>
 *                   0f 00 14 0c <i32 n items>
 *                   per item: 0a 00 0a <i64 event id> 0a 00 14 <i64 version> 00      (23 B)
 *                   00
 *   00
 *
 * and its length 17 + sum over the histories of (16 + token length + 23 * items).  After the 0x59 it is byte for
 * byte the VersionHistories struct crr_load_store_checksums streams into the CRC inside field 56 of the checksum
 * payload: the same decision and the same per-branch rules give both ("The value to store").
 *
 *   CRR_STORE_APPLIED: the stored current index; the current branch's items are the replay's vh rows, their count
 *   clamped to the descriptor's capacity; every other branch comes from the branch table.
 *   CRR_STORE_BACKFILLED: every branch from the table, AddOrUpdateItem(the task's last event) applied to
 *   `branch_index`.
 *   Tokens always come from the persisted bytes; an absent token is written with length 0, absent items as an
 *   empty list.
 *
 * Every other outcome generates nothing (length 0); a task that forks a new branch stays with the host, because its
 * token is ForkHistoryBranch's.
 *
 * Two calls, as crr_load_ndc_plan / crr_load_ndc_run: the plan decides every task, writes its row and scans the
 * lengths into offsets (one synchronisation, to read the totals back); the caller sizes `out` from the plan; the run
 * call emits every blob and does not synchronise.
 *
 * This header is an addition to ABI version 8: CRR_ABI_VERSION and every existing struct and entry point are
 * unchanged; crr_sizeof(30) / (31) report the two structs below (29 stays unassigned and reports 0).
 */
#ifndef CADENCE_LOAD_STORE_VH_H_
#define CADENCE_LOAD_STORE_VH_H_

#include <stddef.h>
#include <stdint.h>

#include "cadence_load_store.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per task (16 B). */
typedef struct crr_vh_blob_row {
    uint32_t len;                     /* bytes of the blob, 0 unless generated */
    int32_t  outcome;                 /* crr_store_outcome, cadence_load_store.h: same values, same precedence */
    int32_t  status;                  /* as crr_store_row.status */
    uint32_t reserved;                /* 0 */
} crr_vh_blob_row;

/* Host struct, valid when the plan returns. */
typedef struct crr_vh_blob_sizes {
    int32_t  err;                     /* 0 or CRR_INGEST_SCRATCH_TOO_SMALL */
    uint32_t n_tasks;
    uint64_t n_generated;             /* tasks with outcome APPLIED or BACKFILLED */
    uint64_t n_bytes;                 /* blob_off[n_tasks] */
    uint64_t work_needed;
} crr_vh_blob_sizes;

/* Bytes of the plan's work buffer (device, 16-byte aligned). */
size_t crr_load_store_vh_scratch_bytes(uint32_t n_tasks);

/* Decide every task exactly as crr_load_store_checksums does and size its blob.  The read-only arguments are those
 * of crr_load_store_checksums, with the same meaning and the same checks.  `rows` is device [n_tasks]; `blob_off`
 * device [n_tasks + 1], the exclusive prefix of the rows' lengths (a task that is not generated occupies no
 * bytes); `work` / `work_bytes` the work buffer.  Synchronises `stream` once to read the totals into `plan`; a work
 * buffer that is too small gives plan->err = CRR_INGEST_SCRATCH_TOO_SMALL with work_needed set, and nothing is
 * launched.  n_tasks == 0 launches nothing (blob_off[0] is set to 0 when blob_off is given).  Returns 0, -1 on an
 * invalid argument, else the hipError_t. */
int crr_load_store_vh_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                           const crr_load_summary* summary_host, const crr_repl_task* tasks,
                           const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                           const crr_ndc_route* routes, const crr_load_branches* branches,
                           const crr_load_ndc_sizes* ndc_plan_host, const crr_inputs* replay_in,
                           const crr_outputs* replay_out, const uint32_t* position, crr_vh_blob_row* rows,
                           uint64_t* blob_off, void* work, size_t work_bytes, crr_vh_blob_sizes* plan, void* stream);

/* Emit every generated blob at out + blob_off[k]: the same read-only arguments, `rows` and `blob_off` as the plan
 * left them, `plan_host` the finished plan (n_tasks is its n_tasks).  `out` is device, 16-byte aligned, with
 * `out_capacity` bytes; bytes [0, round_up(n_bytes, 16)) are written and no others, the tail past n_bytes as zeros.
 * Each lane of the kernel produces 16 bytes of `out` and stores them at once; which bytes a lane owns follows from
 * its index alone, so nothing a task, a decision or a post-replay row holds can move a store.  A byte whose lookup
 * fails (the inputs changed since the plan) is written as zero.  Enqueued on `stream`, no synchronisation;
 * n_bytes == 0 launches nothing.  Returns 0, -1 on an invalid argument or when out_capacity <
 * round_up(n_bytes, 16) (nothing is launched), else the hipError_t. */
int crr_load_store_vh_run(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                          const crr_load_summary* summary_host, const crr_repl_task* tasks,
                          const crr_last_event* last_events, const crr_ndc_result* results, const crr_ndc_route* routes,
                          const crr_load_branches* branches, const crr_load_ndc_sizes* ndc_plan_host,
                          const crr_inputs* replay_in, const crr_outputs* replay_out, const uint32_t* position,
                          const crr_vh_blob_row* rows, const uint64_t* blob_off, const crr_vh_blob_sizes* plan_host,
                          uint8_t* out, size_t out_capacity, void* stream);

/* Host restatement (libcadence_host.so): host pointers and the dense after-image, as crr_load_store_checksums_host;
 * the blobs are written by the plain sequential writer.  `rows`, `blob_off` and `out` may each be NULL: call once to
 * size the buffers from `plan` (n_tasks, n_bytes), then again with them.  With `out`: -1 and nothing written when
 * out_capacity < round_up(n_bytes, 16); else bytes [0, round_up(n_bytes, 16)) are written, the tail as zeros.
 * Returns 0, -1 on an invalid argument, -2 out of memory. */
int crr_load_store_vh_host(const crr_state_batch* in, const crr_repl_task* tasks, const crr_last_event* last_events,
                           uint32_t n_tasks, const crr_ndc_result* results, const crr_ndc_route* routes,
                           const crr_load_image* after, crr_vh_blob_row* rows, uint64_t* blob_off, uint8_t* out,
                           size_t out_capacity, crr_vh_blob_sizes* plan, int threads);

#ifdef __cplusplus
}
#endif
#endif /* CADENCE_LOAD_STORE_VH_H_ */
