/*
 * cadence_load_verify.h -- the checksum check mutableStateBuilder.Load makes on a state it has just
 * materialised (service/history/execution/mutable_state_builder.go:334-348 -> checksum.go:45-54 ->
 * common/checksum/crc.go:59-78), for a batch of persisted states decoded by cadence_load.h.
 *
 * The payload (execution/checksum.go:56-114) is built from the loader's own scratch and the persisted bytes,
 * not from placed rows, so it is right for every workflow whose load status is CRR_LOAD_OK -- the ones
 * flagged CRR_LOAD_FLAG_STICKY / CRR_LOAD_FLAG_MULTI_BRANCH included, which crr_checksum on placed rows
 * does not cover:
 *   scalars                     the dense image's exec row (NextEventID: crr_state_wf.next_event_id)
 *   the five pending-ID lists   the dense rows' ID columns, ascending by ID
 *   StickyTaskListName          the execution blob's field 78 bytes (absent: "")
 *   VersionHistories            CurrentVersionHistoryIndex as stored and every history of the nested blob in
 *                               stored order, each with its BranchToken (absent: zero length) and its Items
 *                               (absent: an empty list) -- VersionHistory.ToInternalType makes both
 *                               (common/persistence/versionHistory.go:125-139), so neither is ever nil
 * DESIGN.md §4 has the paragraph on these sources.
 *
 * This header is an addition to ABI version 8: CRR_ABI_VERSION, the structs and the entry points of
 * cadence_load.h are unchanged; crr_sizeof(20) / (21) report the two structs below.
 */
#ifndef CADENCE_LOAD_VERIFY_H_
#define CADENCE_LOAD_VERIFY_H_

#include <stddef.h>
#include <stdint.h>

#include "cadence_load.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the store keeps beside an execution: checksum.Checksum (common/checksum/defs.go). */
typedef struct crr_stored_checksum {
    int32_t  version;               /* Checksum.Version */
    int32_t  flavor;                /* Checksum.Flavor */
    uint32_t value;                 /* Checksum.Value read big-endian, when value_len == 4 */
    uint32_t value_len;             /* len(Checksum.Value); 0: none stored, or this execution was not sampled
                                       for verification (MutableStateChecksumVerifyProbability) */
} crr_stored_checksum;              /* 16 B */

#define CRR_CHECKSUM_PAYLOAD_V1   1 /* mutableStateChecksumPayloadV1 (execution/checksum.go:33) */
#define CRR_CHECKSUM_FLAVOR_CRC32 1 /* FlavorIEEECRC32OverThriftBinary (common/checksum/defs.go) */

/* Precedence, as Go tests them: NOT_LOADED, NONE, INVALIDATED, BAD_VERSION (checksum.go:49), BAD_FLAVOR
 * (crc.go:64), then MATCH or MISMATCH. */
enum crr_verify_outcome {
    CRR_VERIFY_MATCH = 0,
    CRR_VERIFY_MISMATCH = 1,        /* checksum.ErrMismatch (also value_len not 0 and not 4) */
    CRR_VERIFY_NONE = 2,            /* len(Value) == 0: Load does nothing */
    CRR_VERIFY_INVALIDATED = 3,     /* shouldInvalidateChecksum: LastUpdatedTimestamp before the cut-off */
    CRR_VERIFY_BAD_VERSION = 4,     /* Version != mutableStateChecksumPayloadV1 */
    CRR_VERIFY_BAD_FLAVOR = 5,      /* Flavor != FlavorIEEECRC32OverThriftBinary */
    CRR_VERIFY_NOT_LOADED = 6       /* load status != CRR_LOAD_OK */
};

/* Per workflow (16 B).  computed / payload_len are written for every loaded workflow whatever the outcome;
 * a workflow that is not loaded gets zeros beside its outcome. */
typedef struct crr_verify_row {
    uint32_t computed;              /* CRC32-IEEE of the generated payload */
    int32_t  outcome;               /* crr_verify_outcome */
    uint32_t payload_len;           /* bytes of the payload, the 0x59 preamble included */
    uint32_t reserved;              /* 0 */
} crr_verify_row;

/* Generate every loaded workflow's payload and compare it with `stored` (device, [n_wf]; NULL: compute only,
 * every loaded workflow's outcome is then CRR_VERIFY_NONE).  `in`, `scratch` and `summary_host` are those of a
 * finished crr_load_states_plan; the call is valid before or after crr_load_states_read / _place and changes
 * nothing in the scratch.  invalidate_before_ns: MutableStateChecksumInvalidateBefore as Unix ns -- a state
 * whose LastUpdatedTimeNanos (execution blob field 56) is strictly less is CRR_VERIFY_INVALIDATED; <= 0: off.
 * `result` is device [n_wf].  Enqueued on `stream`, no synchronisation.  Returns 0, -1 on an invalid argument
 * (`in` not the planned batch's shape included), else the hipError_t. */
int crr_load_states_verify(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                           const crr_load_summary* summary_host, const crr_stored_checksum* stored,
                           int64_t invalidate_before_ns, crr_verify_row* result, void* stream);

/* Host restatement (libcadence_host.so): host pointers; decodes `in` as crr_load_states_host does, then runs the
 * same payload code.  Returns 0, -1 on an invalid argument, -2 out of memory. */
int crr_load_states_verify_host(const crr_state_batch* in, const crr_stored_checksum* stored,
                                int64_t invalidate_before_ns, crr_verify_row* result, int threads);

#ifdef __cplusplus
}
#endif
#endif /* CADENCE_LOAD_VERIFY_H_ */
