/*
 * cadence_load.h -- persisted mutable-state blobs -> the engine's resumable rows.
 *
 * What a history service doing passive replication reads from the SQL store before
 * mutableStateBuilder.Load (service/history/execution/mutable_state_builder.go:306-349) is, per execution,
 *   one sqlblobs.WorkflowExecutionInfo blob            (+ the next_event_id column)
 *   one sqlblobs.ActivityInfo blob per pending activity (+ schedule_id, last_heartbeat_updated_time)
 *   one sqlblobs.TimerInfo blob per pending timer       (+ the timer_id string)
 *   one sqlblobs.ChildExecutionInfo / RequestCancelInfo / SignalInfo blob per pending entry (+ initiated_id)
 * (common/persistence/sql/workflowStateMaps.go:144-187, :234-302; sqlExecutionStore.go:1423-1441).  The state
 * blobs are plain thrift binary without a preamble (serialization/thrift_decoder.go:161-165), field IDs of
 * .gen/go/sqlblobs/sqlblobs.go, semantics of serialization/thrift_mapper.go:252-512; VersionHistories and
 * AutoResetPoints inside the execution blob are thriftrw DataBlobs with the 0x59 preamble.
 *
 * This interface decodes a batch of such states into the rows a CRR_WF_FLAG_RESUME replay continues
 * (cadence_replay.h), on the device (crr_load_states_plan / _read / _place) or on the host
 * (crr_load_states_host, libcadence_host.so: the specification the device is compared with byte for byte).
 * DESIGN.md §4 ("Persisted mutable states on the device") has the field-by-field mapping table.
 *
 * Provenance.  A persisted state has no event steps: every *_src of a loaded row is the index, within its
 * workflow, of the blob that holds the strings (sched_src / started_src / src of a pending entry: its own
 * blob; start_src, a reset point's src and a real DecisionRequestID: the execution blob), and src_next is
 * blob_count, so the steps of the call that continues the state follow the blob indices.
 *
 * Keys.  One dictionary per workflow, 0 = "": ids from 1 in first-seen order walking the workflow's blobs in
 * the given order -- an activity's ActivityID, a timer's timer_id, the execution blob's reset points'
 * BinaryChecksums in list order.
 */
#ifndef CADENCE_LOAD_H_
#define CADENCE_LOAD_H_

#include <stddef.h>
#include <stdint.h>

#include "cadence_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

enum crr_state_blob_kind {
    CRR_STATE_EXECUTION = 0,        /* sqlblobs.WorkflowExecutionInfo                                      */
    CRR_STATE_ACTIVITY = 1,         /* sqlblobs.ActivityInfo:   id = schedule_id, aux_time = last heartbeat */
    CRR_STATE_TIMER = 2,            /* sqlblobs.TimerInfo:      str = timer_id (its StartedID is in the blob) */
    CRR_STATE_CHILD = 3,            /* sqlblobs.ChildExecutionInfo: id = initiated_id                       */
    CRR_STATE_REQUEST_CANCEL = 4,   /* sqlblobs.RequestCancelInfo:  id = initiated_id                       */
    CRR_STATE_SIGNAL = 5            /* sqlblobs.SignalInfo:         id = initiated_id                       */
};

/* The key columns stored beside one blob (32 B). */
typedef struct crr_state_blob {
    uint32_t kind;                  /* crr_state_blob_kind */
    uint32_t str_len;               /* timer: the timer_id column, bytes at strings + str_off */
    int64_t  id;                    /* activity: schedule_id; child / request-cancel / signal: initiated_id */
    int64_t  aux_time;              /* activity: last_heartbeat_updated_time, Unix ns (the Go zero time as
                                       time.Time{}.UnixNano() or CRR_ZERO_TIME) */
    uint64_t str_off;
} crr_state_blob;

/* One execution (16 B).  Blob ranges are consecutive as in crr_blob_batch: wf[0].blob_begin == 0 and
 * wf[w + 1].blob_begin == wf[w].blob_begin + wf[w].blob_count.  A workflow's blobs come in any order;
 * exactly one of them is its execution blob. */
typedef struct crr_state_wf {
    uint32_t blob_begin;
    uint32_t blob_count;
    int64_t  next_event_id;         /* executions.next_event_id */
} crr_state_wf;

typedef struct crr_state_batch {
    const uint8_t*        bytes;    /* every blob, concatenated; 16-byte aligned, readable CRR_INGEST_PAD (32)
                                       bytes past the end of the last blob */
    const uint64_t*       blob_off; /* [n_blobs + 1] byte offsets into `bytes` */
    const crr_state_blob* blob;     /* [n_blobs] */
    const crr_state_wf*   wf;       /* [n_wf] */
    const uint8_t*        strings;  /* timer_id columns */
    uint32_t              n_blobs;
    uint32_t              n_wf;
} crr_state_batch;

/* Per-workflow outcome.  A failed workflow gets a zero exec row, zero counts, no token and no keys, and is
 * not to be resumed; it never fails the rest of the batch. */
enum crr_load_status {
    CRR_LOAD_OK = 0,
    CRR_LOAD_MALFORMED = 1,         /* a blob (or a nested blob) is truncated or not thrift binary */
    CRR_LOAD_NESTED_ENCODING = 2,   /* VersionHistories / AutoResetPoints encoding other than "thriftrw" */
    CRR_LOAD_DUPLICATE_ID = 3,      /* two entries of one map share their ID (timers: StartedID or timer_id) */
    CRR_LOAD_VERSION_HISTORIES = 4, /* no version histories, or the current index out of range */
    CRR_LOAD_EXECUTION_COUNT = 5,   /* not exactly one execution blob */
    CRR_LOAD_TOO_LARGE = 6          /* more than CRR_LOAD_MAX_BLOBS blobs, or reset points: left to the host */
};
/* A workflow is decoded by one lane, and ordering its entries, finding duplicate IDs and interning its keys
 * compare them pairwise: the bound keeps one pathological state from holding a kernel for long (at the
 * bound, about 10^7 comparisons for that lane). */
#define CRR_LOAD_MAX_BLOBS 4096
/* Per-workflow flags.  The mutable-state checksum payload (execution/checksum.go:56-114) covers the sticky
 * task list's name and every branch's token and items; the rows hold neither, so crr_checksum on placed rows
 * still does not apply to a workflow with one of these flags.  The verification Load makes of a state it has
 * just materialised is cadence_load_verify.h: it builds the payload from the loader's scratch and the persisted
 * bytes and covers every workflow that loaded OK, flagged or not. */
#define CRR_LOAD_FLAG_STICKY        1u   /* StickyTaskList is non-empty */
#define CRR_LOAD_FLAG_MULTI_BRANCH  2u   /* more than one version history; only the current one is loaded */

/* Dense image tables: the seven row tables (crr_compact_rows' order: activity, timer, child, request-cancel,
 * signal, version-history items, reset points), then the per-workflow byte / entry ranges. */
#define CRR_LOAD_T_TOKEN      7     /* current branch token bytes */
#define CRR_LOAD_T_KEYS       8     /* dictionary entries (key ids 1..count) */
#define CRR_LOAD_T_KEY_BYTES  9     /* dictionary string bytes */
#define CRR_LOAD_TABLES      10

/* What the plan reports (a host struct, valid when the call returns). */
typedef struct crr_load_summary {
    int32_t  err;                   /* 0, or CRR_INGEST_SCRATCH_TOO_SMALL (-100): plan again with scratch_needed */
    uint32_t n_failed;              /* workflows whose status is not CRR_LOAD_OK */
    int64_t  err_blob;              /* lowest index of a malformed blob, -1: none */
    uint64_t totals[CRR_LOAD_TABLES];  /* rows per table, token bytes, dictionary entries, dictionary bytes */
    uint64_t staging[2];            /* internal: the plan's sizing of its key staging (read / place rebuild the
                                       scratch layout from it) */
    uint64_t scratch_needed;        /* bytes this batch needs */
    uint32_t n_blobs;
    uint32_t n_wf;
} crr_load_summary;

/* The dense loaded image (flatten.LoadedStates): caller buffers sized from the summary.  exec[w] is the
 * workflow's exec row; table t's rows of workflow w are rows[t][offsets[t][w] .. offsets[t][w + 1]), live
 * rows ascending by ID; offsets is [CRR_LOAD_TABLES][n_wf + 1] (exclusive prefixes, [t][n_wf] = the total).
 * Token of w: tokens[offsets[7][w] ..); dictionary of w: key_begin = offsets[8][w], key_count the
 * difference, key id k (1..count) = key_bytes[key_off[key_begin + k - 1] .. + key_len[...]) -- the
 * key_begin / key_count / key_off / key_len form of crr_ingest_resume once the caller adds the offset it
 * uploads key_bytes at.  Any pointer may be NULL (not copied). */
typedef struct crr_load_image {
    crr_exec_row* exec;             /* [n_wf] */
    void*         rows[7];
    int64_t*      offsets;          /* [CRR_LOAD_TABLES][n_wf + 1] */
    uint8_t*      tokens;
    uint64_t*     key_off;
    uint32_t*     key_len;
    uint8_t*      key_bytes;
    int32_t*      status;           /* [n_wf] crr_load_status */
    uint32_t*     flags;            /* [n_wf] CRR_LOAD_FLAG_* */
} crr_load_image;

/* Device scratch for a batch: the fixed part plus room for a typical dense image; a batch that needs more
 * reports CRR_INGEST_SCRATCH_TOO_SMALL with summary.scratch_needed, as crr_ingest_plan does. */
size_t crr_load_scratch_bytes(uint32_t n_blobs, uint32_t n_wf);

/* Decode every blob of `in` (device pointers) and leave the dense image in `scratch` (device, 16-byte
 * aligned).  Synchronises `stream` twice: to size the dense image, and to read the summary back.
 * Returns 0, -1 on an invalid argument -- the workflows' blob ranges not consecutive or not covering the
 * blobs included, which the plan checks on the device (nothing of such a batch is to be read or placed) --
 * else the hipError_t. */
int crr_load_states_plan(const crr_state_batch* in, void* scratch, size_t scratch_bytes, crr_load_summary* summary,
                         void* stream);

/* Copy the dense image out of the scratch into `dst` (host or device buffers), enqueued on `stream`. */
int crr_load_states_read(const void* scratch, size_t scratch_bytes, const crr_load_summary* summary_host,
                         const crr_load_image* dst, void* stream);

/* Scatter the dense image into a replay's outputs.  `layout` is the crr_inputs the resumed replay runs with
 * (device descriptors wf[n_wf], stride, CRR_IN_WAVE_TAIL / wave_begin); device position p takes loaded
 * workflow perm[p] (device uint32[n_wf]; NULL: p).  For every position whose descriptor carries
 * CRR_WF_FLAG_RESUME and whose loaded status is CRR_LOAD_OK: the exec row, and row j of each table at
 * base + j * stride.  With out->live_ids set the five pending maps' IDs go to the sidecar at the same
 * indices, so crr_checksum is valid on the placed rows before any replay.  A workflow with more rows in a
 * table than that table's capacity is left with zero counts and status CRR_ERR_CAPACITY (fail_step =
 * src_next) and none of its rows written.  Other positions, and slots past a workflow's count, are not
 * touched. */
int crr_load_states_place(const void* scratch, size_t scratch_bytes, const crr_load_summary* summary_host,
                          const crr_inputs* layout, const uint32_t* perm, const crr_outputs* out, void* stream);

/* Host restatement (libcadence_host.so): `in` and `dst` are host pointers; any buffer of `dst` (or `dst`
 * itself) may be NULL -- call once without buffers to size them from the summary, then again with them.
 * `threads` <= 1: single-threaded.  Returns 0, -1 on an invalid argument, -2 out of memory. */
int crr_load_states_host(const crr_state_batch* in, const crr_load_image* dst, crr_load_summary* summary, int threads);

#ifdef __cplusplus
}
#endif
#endif /* CADENCE_LOAD_H_ */
