// load_kernel.hip -- persisted mutable-state blobs -> resumable rows on the GPU (include/cadence_load.h).
//
// The decoder is load_decode.h (its own bounds-checked thrift reader; shared with the host restatement so
// the two cannot drift); this file holds the launches:
//   load_parse_kernel   one lane per blob: a pending entry's struct -> its row image in the scratch
//   load_count_kernel   one lane per workflow: the execution blob -> the exec row, the nested blobs walked
//                       to validate and count, duplicate IDs, status / flags, the per-table counts
//   load_scan_kernel    one block: exclusive prefixes of the counts over workflows (compact_kernel.hip's pattern)
//   load_emit_kernel    one lane per workflow: rows to their rank by ID, keys interned, MAPPED, items, tokens
//   load_dict_kernel    one lane per workflow: the key dictionary
//   load_place_kernel   one lane per device position: the dense rows scattered into a replay's slot tables
//   load_verify_kernel  one lane per workflow: the mutable-state checksum payload generated from the dense image
//                       and the persisted bytes, its CRC compared with the stored checksum (cadence_load_verify.h)
//   load_branches_count_kernel / load_branches_emit_kernel   one lane per workflow: every history of the nested
//                       VersionHistories blob counted, then written as the branch table crr_ndc_prepare takes
//                       (cadence_load_ndc.h); load_ndc_scan_kernel between them, load_scan_kernel's pattern
//   load_task_room_kernel / load_task_rows_kernel / load_route_kernel   one lane per replication task: its room for
//                       new-branch items, its crr_ndc_task row, and after crr_ndc_prepare the routing decision
//   load_store_kernel   one lane per replication task: the checksum to store once the task is committed, its payload
//                       generated from the rows the resumed replay left or from the loaded image (cadence_load_store.h)
//   load_store_vh_size_kernel / load_store_vh_emit_kernel   the VersionHistories blob to store for the same tasks
//                       (cadence_load_store_vh.h): one lane per task sizes it, load_ndc_scan_kernel gives the offsets,
//                       then one lane per 16 bytes of the output writes them with one dwordx4 store
//   load_mutation_count_kernel / load_mutation_offsets_kernel / load_mutation_emit_kernel / load_mutation_gather_kernel
//                       the pending-entry mutation to store for the same tasks (cadence_load_mutation.h): one lane per
//                       task classifies its entries by a merge walk and counts, the block sums are scanned by
//                       load_ndc_scan_kernel and one pass turns the counts into offsets; then one lane per task writes
//                       the deleted keys and a directory, and one lane per 8-byte word gathers the rows through it
//   load_store_exec_size_kernel / load_store_exec_offsets_kernel / load_store_exec_emit_kernel
//                       the execution blob to store for the same tasks (cadence_load_store_exec.h): one lane per task
//                       decides, walks the stored blob's top-level fields and leaves an edit script (copy segments and
//                       scalar patches); block sums through load_ndc_scan_kernel and one pass give the offsets; then
//                       one lane per 16 bytes of the output follows its task's script and stores them at once
//   load_resume_bid_kernel / load_resume_rows_kernel / load_resume_count_kernel / load_resume_offsets_kernel /
//   load_resume_index_kernel / load_resume_gather_kernel / load_resume_caps_kernel / load_resume_descriptor_kernel
//                       the resumed replay of the same tasks planned from the loaded states (cadence_load_resume.h):
//                       one lane per task bids for its workflow (the lowest index wins), one lane per position counts
//                       what it contributes, block sums through load_ndc_scan_kernel and one pass give the offsets;
//                       then the gathered batch's small arrays, and one lane per 16 bytes of its bytes; after the
//                       ingest's plan, the capacities summed the same way and one lane per position writes its
//                       descriptor and copies its token into the arena
// Divergence is inherent on the skip paths (every lane walks its own blob); the lane state is the reader
// (pointer, cursor, end) and the row being built, and the skip stack for nested containers lives in LDS.
// A workflow is one lane whatever its size: the ordering, duplicate and MAPPED passes are quadratic in its
// pending entries, which the states of the replication path keep small (a wavefront-per-workflow variant
// for large states is not built).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cadence_ingest.h"
#include "cadence_load.h"
#include "cadence_load_verify.h"
#include "load_decode.h"
#include "stream_device.h"

namespace crr_load {
namespace {

constexpr int kBlock = 128;
constexpr int kScanBlock = 1024;

__global__ void __launch_bounds__(kBlock) load_parse_kernel(Ctx c) {
  __shared__ Frame stk[kBlock][kMaxDepth];
  const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
  if (b < c.in.n_blobs) parse_blob(c, b, stk[threadIdx.x]);
}

__global__ void __launch_bounds__(kBlock) load_count_kernel(Ctx c) {
  __shared__ Frame stk[kBlock][kMaxDepth];
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w >= c.in.n_wf) return;
  if (!range_ok(c, w)) c.err()[2 + kCounters] = 1;   // (every writer stores the same value)
  count_wf(c, w, stk[threadIdx.x]);
}

__global__ void __launch_bounds__(kBlock) load_emit_kernel(Ctx c) {
  __shared__ Frame stk[kBlock][kMaxDepth];
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w < c.in.n_wf) emit_wf(c, w, stk[threadIdx.x]);
}

__global__ void __launch_bounds__(kBlock) load_dict_kernel(Ctx c) {
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w < c.in.n_wf) dict_wf(c, w);
}

// one block: counters [first, last) scanned in place over the n_wf workflows (each thread a contiguous chunk,
// Hillis-Steele over the 1024 chunk sums); the totals also go to totals[t] for the host to read in one copy
__global__ void __launch_bounds__(kScanBlock) load_scan_kernel(Ctx c, uint32_t mask, uint64_t* totals) {
  __shared__ int64_t part[kScanBlock];
  const uint32_t n = c.in.n_wf;
  const uint32_t per = (n + kScanBlock - 1) / kScanBlock;
  for (int t = 0; t < kCounters; ++t) {
    if (!((mask >> t) & 1u)) continue;
    int64_t* p = c.cnt(t);
    const uint32_t lo = min((uint64_t)threadIdx.x * per, (uint64_t)n), hi = min((uint64_t)lo + per, (uint64_t)n);
    int64_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += p[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < kScanBlock; d <<= 1) {
      const int64_t o = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
      __syncthreads();
      part[threadIdx.x] += o;
      __syncthreads();
    }
    int64_t run = part[threadIdx.x] - s;
    for (uint32_t i = lo; i < hi; ++i) {
      const int64_t x = p[i];
      p[i] = run;
      run += x;
    }
    if (threadIdx.x == kScanBlock - 1) {
      p[n] = part[kScanBlock - 1];
      totals[t] = (uint64_t)part[kScanBlock - 1];
    }
    __syncthreads();
  }
}

struct PlaceArgs {
  const crr_workflow* wf;
  const uint32_t* perm;
  uint32_t n_pos, stride, wave_begin, n_loaded;
  crr_outputs out;
};

__global__ void __launch_bounds__(kBlock) load_place_kernel(Ctx c, PlaceArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.n_pos) return;
  const crr_workflow& D = a.wf[p];
  if (!(D.flags & CRR_WF_FLAG_RESUME)) return;
  const uint32_t w = a.perm ? a.perm[p] : p;
  if (w >= a.n_loaded || c.status()[w] != CRR_LOAD_OK) return;
  const int64_t st = p >= a.wave_begin ? 1 : (int64_t)a.stride;
  const crr_exec_row& R = c.exec()[w];
  crr_exec_row& X = a.out.exec[p];
  // each table by name (no arrays indexed by table: everything stays in registers)
  auto count = [&](int t) { return c.cnt(t)[w + 1] - c.cnt(t)[w]; };
  auto fits1 = [&](int t, int32_t cap, const void* dst) {
    const int64_t n = count(t);
    return n <= (int64_t)(cap < 0 ? 0 : cap) && (n == 0 || dst != nullptr);
  };
  const bool fits = fits1(0, D.act_cap, a.out.act) && fits1(1, D.timer_cap, a.out.timer) && fits1(2, D.child_cap, a.out.child) &&
                    fits1(3, D.rc_cap, a.out.rc) && fits1(4, D.sig_cap, a.out.sig) && fits1(5, D.vh_cap, a.out.vh) &&
                    fits1(6, D.rp_cap, a.out.rp);
  if (!fits) {   // sized too small by the host: nothing of it written but the exec row's verdict
    X = R;
    X.status = CRR_ERR_CAPACITY;
    X.fail_step = R.src_next;
    X.n_activity = X.n_timer = X.n_child = X.n_rc = X.n_signal = X.n_vh_items = X.n_reset_points = 0;
    return;
  }
  X = R;
  auto put = [&](int t, int64_t base, void* dst, int64_t* ids) {
    const uint32_t words = kRowBytes[t] / 8;   // every row type is a multiple of 8 bytes
    const int64_t off = c.cnt(t)[w], n = count(t);
    const uint64_t* s = reinterpret_cast<const uint64_t*>(c.rows(t) + (uint64_t)off * kRowBytes[t]);
    for (int64_t j = 0; j < n; ++j) {
      uint64_t* q = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(dst) + (uint64_t)(base + j * st) * kRowBytes[t]);
      for (uint32_t k = 0; k < words; ++k) q[k] = s[(uint64_t)j * words + k];
      // the live-ID sidecar: each pending map's ID is its row's first field
      if (ids) ids[base + j * st] = (int64_t)s[(uint64_t)j * words];
    }
  };
  put(0, D.act_base, a.out.act, a.out.live_ids[0]);
  put(1, D.timer_base, a.out.timer, a.out.live_ids[1]);
  put(2, D.child_base, a.out.child, a.out.live_ids[2]);
  put(3, D.rc_base, a.out.rc, a.out.live_ids[3]);
  put(4, D.sig_base, a.out.sig, a.out.live_ids[4]);
  put(5, D.vh_base, a.out.vh, nullptr);
  put(6, D.rp_base, a.out.rp, nullptr);
}

// the slicing-by-8 CRC tables of load_decode.h's Crc, built by the block in LDS (replay_kernel.hip's
// build_crc_tables restated): table 0 the byte-wise reflected CRC32, tables 1..7 its extensions
__device__ void build_crc_tables(uint32_t* T) {
  for (int i = threadIdx.x; i < 256; i += kBlock) {
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    T[i] = c;
  }
  __syncthreads();
  for (int t = 1; t < 8; ++t) {
    for (int i = threadIdx.x; i < 256; i += kBlock) {
      const uint32_t p = T[(t - 1) * 256 + i];
      T[t * 256 + i] = (p >> 8) ^ T[p & 0xff];
    }
    __syncthreads();
  }
}

// one lane per workflow: the checksum payload streamed through the CRC (nothing of it is stored), then Load's
// decision; 16 KB of LDS per block (the tables and the skip stacks)
__global__ void __launch_bounds__(kBlock) load_verify_kernel(Ctx c, const crr_stored_checksum* stored,
                                                             int64_t invalidate_before_ns, crr_verify_row* result) {
  __shared__ uint32_t crc_tables[8 * 256];
  __shared__ Frame stk[kBlock][kMaxDepth];
  build_crc_tables(crc_tables);
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w < c.in.n_wf) verify_wf(c, w, crc_tables, stored, invalidate_before_ns, result, stk[threadIdx.x]);
}

// ---- cadence_load_ndc.h: every branch of every loaded state, the tasks' rows, the routing decision ------------
__global__ void __launch_bounds__(kBlock) load_branches_count_kernel(Ctx c, NdcWork k) {
  __shared__ Frame stk[kBlock][kMaxDepth];
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w < c.in.n_wf) branches_count_wf(c, k, w, stk[threadIdx.x]);
}

__global__ void __launch_bounds__(kBlock) load_branches_emit_kernel(Ctx c, NdcWork k, crr_load_branches dst) {
  __shared__ Frame stk[kBlock][kMaxDepth];
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w < c.in.n_wf) branches_emit_wf(c, k, w, dst, stk[threadIdx.x]);
}

// load_scan_kernel's pattern over plain rows: `rows` arrays of n + 1 int64 each, scanned in place to exclusive
// prefixes ([n] = the total, which also goes to totals[row])
__global__ void __launch_bounds__(kScanBlock) load_ndc_scan_kernel(int64_t* base, uint32_t n, int rows, uint64_t* totals) {
  __shared__ int64_t part[kScanBlock];
  const uint32_t per = (n + kScanBlock - 1) / kScanBlock;
  for (int t = 0; t < rows; ++t) {
    int64_t* p = base + (uint64_t)t * ((uint64_t)n + 1);
    const uint32_t lo = min((uint64_t)threadIdx.x * per, (uint64_t)n), hi = min((uint64_t)lo + per, (uint64_t)n);
    int64_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += p[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < kScanBlock; d <<= 1) {
      const int64_t o = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
      __syncthreads();
      part[threadIdx.x] += o;
      __syncthreads();
    }
    int64_t run = part[threadIdx.x] - s;
    for (uint32_t i = lo; i < hi; ++i) {
      const int64_t x = p[i];
      p[i] = run;
      run += x;
    }
    if (threadIdx.x == kScanBlock - 1) {
      p[n] = part[kScanBlock - 1];
      totals[t] = (uint64_t)part[kScanBlock - 1];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kBlock) load_task_room_kernel(NdcWork k, const crr_repl_task* tasks) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < k.n_tasks) k.out_off()[i] = task_room(k, tasks[i]);
}

__global__ void __launch_bounds__(kBlock) load_task_rows_kernel(NdcWork k, const crr_repl_task* tasks, uint32_t n_incoming,
                                                                uint64_t n_items, const int32_t* current, uint32_t* out_begin) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= k.n_tasks) return;
  const crr_ndc_task r = task_row(k, tasks[i], i, n_incoming, n_items, current);
  k.rows()[i] = r;
  if (out_begin) out_begin[i] = r.out_begin;
}

__global__ void __launch_bounds__(kBlock) load_route_kernel(NdcWork k, const crr_repl_task* tasks, uint32_t n_incoming,
                                                            const crr_ndc_branch* branches, const crr_vh_item* items,
                                                            const crr_vh_item* out_items, crr_ndc_result* results,
                                                            crr_ndc_route* routes) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < k.n_tasks) route_task(k, tasks[i], i, n_incoming, branches, items, out_items, results, routes);
}

// ---- cadence_load_store.h: the checksum to store for every routed task -----------------------------------------
// one lane per task, load_verify_kernel's shape: the payload streamed through the CRC, nothing of it stored, the
// tables built by the block in LDS (8 KB).  It walks no blob -- the branches come from the resident table -- so
// it needs no skip stack.
__global__ void __launch_bounds__(kBlock) load_store_kernel(Ctx c, StoreIn a, ReplayAfter after, crr_store_row* result) {
  __shared__ uint32_t crc_tables[8 * 256];
  build_crc_tables(crc_tables);
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.n_tasks) store_task(c, a, after, crc_tables, i, result);
}

// ---- cadence_load_store_vh.h: the VersionHistories blob to store for every routed task --------------------------
// one lane per task, load_store_kernel's launch: the decision, the blob's length from the branch table's token
// lengths and item counts (nothing is walked), the row; the length goes to blob_off[i] for the scan, the
// generated mark to the work buffer
__global__ void __launch_bounds__(kBlock) load_store_vh_size_kernel(Ctx c, StoreIn a, ReplayAfter after, crr_vh_blob_row* rows,
                                                                    int64_t* lens, int64_t* generated) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_tasks) return;
  const uint64_t len = vh_size_task(c, a, after, i, rows);
  lens[i] = (int64_t)len;
  generated[i] = len != 0;
}

// output-stationary: lane i owns bytes [16 i, 16 i + 16) of `out` and stores them as one dwordx4, whatever blobs
// they belong to (load_decode.h's vh_emit_chunk); no LDS, no blob-size limit, and no store whose address depends
// on anything but the lane's index
__global__ void __launch_bounds__(kBlock) load_store_vh_emit_kernel(Ctx c, StoreIn a, ReplayAfter after, const uint64_t* blob_off,
                                                                    uint64_t n_bytes, uint64_t n_chunks, ulonglong2* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_chunks) return;
  uint64_t lo, hi;
  vh_emit_chunk(c, a, after, blob_off, n_bytes, i, lo, hi);
  out[i] = make_ulonglong2(lo, hi);
}

// ---- cadence_load_mutation.h: the pending-entry mutation to store for every routed task ------------------------
// The columns that are counted, scanned and turned into offsets: the exec rows, then per map its upserted rows and
// its deleted keys.
constexpr int kMutCols = 1 + 2 * CRR_MUTATION_MAPS;

__device__ inline uint32_t mut_col(const crr_mutation_row& o, int col) {
  if (col == 0) return o.exec_index != 0xFFFFFFFFu ? 1u : 0u;
  const crr_mutation_map& m = o.map[(col - 1) / 2];
  return (col & 1) ? m.n_upsert : m.n_delete;
}

// one lane per task, load_store_kernel's launch without the CRC: the decision, then one merge walk per pending map
// over the rows before (the loader's dense image) and after (the replay's slots); the row with its counts, and the
// block's column sums (LDS atomics: most lanes add to two or three columns) for the offsets
__global__ void __launch_bounds__(kBlock) load_mutation_count_kernel(Ctx c, StoreIn a, ReplayAfter after, crr_mutation_row* rows,
                                                                     int64_t* block_sums, uint32_t n_blocks) {
  __shared__ uint32_t sums[kMutCols];
  if (threadIdx.x < kMutCols) sums[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.n_tasks) {
    crr_mutation_row o;
    mutation_count_task(c, a, after, i, o);
    rows[i] = o;
#pragma unroll
    for (int col = 0; col < kMutCols; ++col) {
      const uint32_t v = mut_col(o, col);
      if (v) atomicAdd(&sums[col], v);
    }
  }
  __syncthreads();
  if (threadIdx.x < kMutCols) block_sums[(uint64_t)threadIdx.x * ((uint64_t)n_blocks + 1) + blockIdx.x] = sums[threadIdx.x];
}

__device__ inline uint32_t wave_inclusive_scan(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// one pass over the packed count rows: block_base is the scanned block sums ([kMutCols][n_blocks + 1]); within the
// block each column is a wavefront scan, the first wavefront's total handed over in LDS.  Every lane of the block
// takes part in the scans, a lane past the last task with zeros.
__global__ void __launch_bounds__(kBlock) load_mutation_offsets_kernel(crr_mutation_row* rows, uint32_t n_tasks,
                                                                       const int64_t* block_base, uint32_t n_blocks) {
  static_assert(kBlock == 128, "two wavefronts of 64");
  __shared__ uint32_t first_wave[kMutCols];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool have = i < n_tasks;
  crr_mutation_row o;
  if (have) o = rows[i];
  uint32_t excl[kMutCols];
#pragma unroll
  for (int col = 0; col < kMutCols; ++col) {
    const uint32_t v = have ? mut_col(o, col) : 0u;
    const uint32_t incl = wave_inclusive_scan(v);
    if (threadIdx.x == 63) first_wave[col] = incl;
    excl[col] = incl - v;
  }
  __syncthreads();
  if (!have) return;
#pragma unroll
  for (int col = 0; col < kMutCols; ++col) {
    excl[col] += (uint32_t)block_base[(uint64_t)col * ((uint64_t)n_blocks + 1) + blockIdx.x];
    if (threadIdx.x >= 64) excl[col] += first_wave[col];
  }
  if (o.exec_index != 0xFFFFFFFFu) o.exec_index = excl[0];
#pragma unroll
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) {
    o.map[t].upsert_begin = excl[1 + 2 * t];
    o.map[t].delete_begin = excl[2 + 2 * t];
  }
  rows[i] = o;
}

// one lane per task: the walk again, the deleted keys to their planned ranges and the directory to the work buffer
__global__ void __launch_bounds__(kBlock) load_mutation_emit_kernel(Ctx c, StoreIn a, ReplayAfter after, const crr_mutation_row* rows,
                                                                    MutDst d) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.n_tasks) mutation_emit_task(c, a, after, i, rows, d);
}

// output-stationary, compact_gather_kernel's reasoning: lane g owns 8-byte word g of a dense output and finds its
// row through the directory, so a wavefront's stores are one contiguous 512 bytes and no store address depends on
// anything but the lane's index
__global__ void __launch_bounds__(kBlock) load_mutation_gather_kernel(const uint64_t* table, const uint64_t* dir, uint32_t words,
                                                                      uint64_t n_words, uint64_t* out) {
  const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g < n_words) out[g] = mutation_gather_word(table, dir, words, g);
}

// ---- cadence_load_store_exec.h: the execution blob to store for every routed task ------------------------------
// The columns that are summed per block and scanned: the blobs' bytes, the tasks with a blob, the generated tasks
// left to the host, the tasks whose VersionHistories row disagrees.
constexpr int kExecCols = 4;

// one lane per task, load_mutation_count_kernel's launch with the skip stack of the walking kernels: the decision,
// the stored blob's top-level fields twice (which overridden fields it holds, then the splice), for a request id
// of this task the task's events; the row, the edit script, and the block's column sums for the offsets
__global__ void __launch_bounds__(kBlock) load_store_exec_size_kernel(Ctx c, StoreIn a, ReplayAfter after, ExecIn x,
                                                                      crr_exec_blob_row* rows, ExecScript* scripts,
                                                                      int64_t* block_sums, uint32_t n_blocks) {
  __shared__ Frame stk[kBlock][kMaxDepth];
  __shared__ unsigned long long sums[kExecCols];
  if (threadIdx.x < kExecCols) sums[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.n_tasks) {
    bool vh_bad;
    const uint32_t len = exec_size_task(c, a, after, x, i, rows, scripts + i, vh_bad, stk[threadIdx.x]);
    const crr_exec_blob_row o = rows[i];
    if (len) {
      atomicAdd(&sums[0], (unsigned long long)len);
      atomicAdd(&sums[1], 1ull);
    } else if (o.flags) {
      atomicAdd(&sums[2], 1ull);
    }
    if (vh_bad) atomicAdd(&sums[3], 1ull);
  }
  __syncthreads();
  if (threadIdx.x < kExecCols) block_sums[(uint64_t)threadIdx.x * ((uint64_t)n_blocks + 1) + blockIdx.x] = (int64_t)sums[threadIdx.x];
}

// load_mutation_offsets_kernel's scheme for the one column that becomes offsets: block_base is the scanned block
// sums; within the block a wavefront scan of the lengths, the first wavefront's total handed over in LDS
__global__ void __launch_bounds__(kBlock) load_store_exec_offsets_kernel(const crr_exec_blob_row* rows, uint32_t n_tasks,
                                                                         const int64_t* block_base, uint64_t* blob_off) {
  static_assert(kBlock == 128, "two wavefronts of 64");
  __shared__ unsigned long long first_wave;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool have = i < n_tasks;
  const unsigned long long v = have ? rows[i].len : 0u;
  unsigned long long incl = v;
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (threadIdx.x == 63) first_wave = incl;
  __syncthreads();
  if (!have) return;
  unsigned long long excl = incl - v + (unsigned long long)block_base[blockIdx.x];
  if (threadIdx.x >= 64) excl += first_wave;
  blob_off[i] = excl;
  if (i + 1 == n_tasks) blob_off[n_tasks] = excl + v;
}

// output-stationary, load_store_vh_emit_kernel's shape: lane i owns bytes [16 i, 16 i + 16) of `out` and stores them
// as one dwordx4; the lane that owns the tail past the last whole 16 stores its n_bytes - 16 i bytes one by one.
// Which bytes a lane writes follows from its index and n_bytes alone.
__global__ void __launch_bounds__(kBlock) load_store_exec_emit_kernel(const ExecScript* scripts, const uint8_t* stored,
                                                                      const uint64_t* stored_off, uint32_t n_stored_blobs,
                                                                      const uint8_t* vh, uint64_t n_vh, const uint8_t* task,
                                                                      const uint64_t* task_off, uint32_t n_task_blobs,
                                                                      const uint64_t* blob_off, uint32_t n_tasks,
                                                                      uint64_t n_bytes, uint64_t n_chunks, uint8_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_chunks) return;
  const uint64_t n_stored = stored_off ? stored_off[n_stored_blobs] : 0, n_task = task_off ? task_off[n_task_blobs] : 0;
  const ExecSrc q = {stored, vh, task, n_stored, n_vh, n_task};
  uint64_t lo, hi;
  exec_emit_chunk(scripts, q, blob_off, n_tasks, n_bytes, i, lo, hi);
  if (16 * i + 16 <= n_bytes) {
    reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(lo, hi);
  } else {
    const uint32_t n = (uint32_t)(n_bytes - 16 * i);
    for (uint32_t b = 0; b < n; ++b) out[16 * i + b] = (uint8_t)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xffu);
  }
}

// ---- cadence_load_resume.h: the resumed replay of routed tasks planned from the loaded states -------------------
static_assert(kResBlock == kBlock, "one block sum per launch block");

// an exclusive scan of N columns over the block's 128 lanes: a wavefront scan per column, the first wavefront's
// totals handed over in LDS (load_mutation_offsets_kernel's scheme).  Every lane of the block takes part.
template <int N>
__device__ inline void block_exclusive_scan(const uint64_t (&v)[N], uint64_t (&excl)[N], unsigned long long* first_wave) {
  static_assert(kBlock == 128, "two wavefronts of 64");
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int col = 0; col < N; ++col) {
    unsigned long long incl = v[col];
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (threadIdx.x == 63) first_wave[col] = incl;
    excl[col] = incl - v[col];
  }
  __syncthreads();
  if (threadIdx.x >= 64) {
#pragma unroll
    for (int col = 0; col < N; ++col) excl[col] += first_wave[col];
  }
}

// one lane per task: a task that may be applied bids for its workflow with its index; the lowest wins
__global__ void __launch_bounds__(kBlock) load_resume_bid_kernel(Ctx c, ResumeIn r, ResumeWork k) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= r.n_tasks) return;
  if (resume_candidate(c, r, i) == CRR_RESUME_APPLIED) atomicMin(&k.winner()[r.tasks[i].wf], i);
}

// one lane per task: its row, once every bid is in
__global__ void __launch_bounds__(kBlock) load_resume_rows_kernel(Ctx c, ResumeIn r, ResumeWork k, crr_load_resume_row* rows) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < r.n_tasks) rows[i] = resume_row(c, r, k.winner(), i);
}

// one lane per position: its counts to off(col)[p] and the block's column sums
__global__ void __launch_bounds__(kBlock) load_resume_count_kernel(Ctx c, ResumeIn r, ResumeWork k) {
  __shared__ unsigned long long sums[kResCols];
  if (threadIdx.x < kResCols) sums[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p < k.n_wf) {
    uint64_t v[kResCols];
    resume_counts(c, r, k.winner()[p], p, v);
#pragma unroll
    for (int col = 0; col < kResCols; ++col) {
      k.off(col)[p] = v[col];
      if (v[col]) atomicAdd(&sums[col], (unsigned long long)v[col]);
    }
  }
  __syncthreads();
  if (threadIdx.x < kResCols)
    k.sums()[(uint64_t)threadIdx.x * ((uint64_t)k.L.n_blocks + 1) + blockIdx.x] = (int64_t)sums[threadIdx.x];
}

// one pass over the counts: the scanned block sums plus the scan within the block, in place
__global__ void __launch_bounds__(kBlock) load_resume_offsets_kernel(ResumeWork k) {
  __shared__ unsigned long long first_wave[kResCols];
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const bool have = p < k.n_wf;
  uint64_t v[kResCols], excl[kResCols];
#pragma unroll
  for (int col = 0; col < kResCols; ++col) v[col] = have ? k.off(col)[p] : 0;
  block_exclusive_scan<kResCols>(v, excl, first_wave);
  if (!have) return;
#pragma unroll
  for (int col = 0; col < kResCols; ++col) {
    const uint64_t e = excl[col] + (uint64_t)k.sums()[(uint64_t)col * ((uint64_t)k.L.n_blocks + 1) + blockIdx.x];
    k.off(col)[p] = e;
    if (p + 1 == k.n_wf) k.off(col)[k.n_wf] = e + v[col];
  }
}

// the gathered batch's small arrays, one lane per element of the longest: position p's crr_blob_wf, seeds' range and
// task; blob j's offset; dictionary entry e.  Each lane's store addresses follow from its index and the plan's totals.
__global__ void __launch_bounds__(kBlock) load_resume_index_kernel(Ctx c, ResumeIn r, ResumeWork k, ResumeTotals T,
                                                                   crr_load_resume_out out) {
  const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g < k.n_wf) {
    const uint32_t p = (uint32_t)g;
    out.wf[p] = resume_blob_wf(r, k, p);
    out.key_begin[p] = (uint32_t)k.off(kResKeys)[p];
    out.key_count[p] = (uint32_t)(k.off(kResKeys)[p + 1] - k.off(kResKeys)[p]);
    const uint32_t task = k.winner()[p];
    out.task_of[p] = task == kResNoTask ? -1 : (int32_t)task;
  }
  if (g <= T.n_blobs) out.blob_off[g] = resume_blob_off(r, k, T, g);
  if (g < T.n_keys) {
    uint64_t off;
    uint32_t len;
    resume_key(c, k, T, g, off, len);
    out.key_off[g] = off;
    out.key_len[g] = len;
  }
}

// output-stationary, load_store_exec_emit_kernel's shape: lane i owns bytes [16 i, 16 i + 16) of `out` and stores them
// as one dwordx4; the lane that owns the tail past the last whole 16 stores its n_bytes - 16 i bytes one by one
__global__ void __launch_bounds__(kBlock) load_resume_gather_kernel(Ctx c, ResumeIn r, ResumeWork k, ResumeTotals T,
                                                                    uint64_t n_chunks, uint8_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_chunks) return;
  uint64_t lo, hi;
  resume_gather_chunk(c, r, k, T, i, lo, hi);
  if (16 * i + 16 <= T.n_bytes) {
    reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(lo, hi);
  } else {
    const uint32_t n = (uint32_t)(T.n_bytes - 16 * i);
    for (uint32_t b = 0; b < n; ++b) out[16 * i + b] = (uint8_t)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xffu);
  }
}

// one lane per position: the block's sums of the eight capacities
__global__ void __launch_bounds__(kBlock) load_resume_caps_kernel(Ctx c, ResumeWork k, const int32_t* counts, uint64_t stride) {
  __shared__ unsigned long long sums[kResCaps];
  if (threadIdx.x < kResCaps) sums[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p < k.n_wf) {
    uint64_t cap[kResCaps];
    resume_caps(c, k, counts, stride, p, cap);
#pragma unroll
    for (int t = 0; t < kResCaps; ++t)
      if (cap[t]) atomicAdd(&sums[t], (unsigned long long)cap[t]);
  }
  __syncthreads();
  if (threadIdx.x < kResCaps)
    k.cap_sums()[(uint64_t)threadIdx.x * ((uint64_t)k.L.n_blocks + 1) + blockIdx.x] = (int64_t)sums[threadIdx.x];
}

// one lane per position: the capacities again, their prefixes, the descriptor and the token's bytes into the arena
// (a position's arena range is the plan's, checked against the capacity before anything is stored)
__global__ void __launch_bounds__(kBlock) load_resume_descriptor_kernel(Ctx c, ResumeWork k, const crr_blob_wf* gathered_wf,
                                                                        const int32_t* counts, uint64_t stride, crr_workflow* wf,
                                                                        uint8_t* arena, uint64_t arena_capacity) {
  __shared__ unsigned long long first_wave[kResCaps];
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const bool have = p < k.n_wf;
  uint64_t cap[kResCaps], base[kResCaps];
#pragma unroll
  for (int t = 0; t < kResCaps; ++t) cap[t] = 0;
  if (have) resume_caps(c, k, counts, stride, p, cap);
  block_exclusive_scan<kResCaps>(cap, base, first_wave);
  if (!have) return;
#pragma unroll
  for (int t = 0; t < kResCaps; ++t) base[t] += (uint64_t)k.cap_sums()[(uint64_t)t * ((uint64_t)k.L.n_blocks + 1) + blockIdx.x];
  wf[p] = resume_descriptor(c, k, gathered_wf, counts, stride, p, cap, base, arena, arena_capacity);
}

// one lane per position: a descriptor without a task does not resume (the layout's in-place pass set the flag on all)
__global__ void __launch_bounds__(kBlock) load_resume_settle_kernel(const int32_t* task_of, crr_workflow* wf, uint32_t n_wf) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p < n_wf && task_of[p] < 0) wf[p].flags &= ~CRR_WF_FLAG_RESUME;
}

inline dim3 grid_of(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

// every entry point that takes a stream, once its arguments are checked: the stream as `s`, its device selected
// until the function returns (stream_device.h), or hipErrorInvalidHandle returned
#define CRR_ON_STREAM(s, stream)                           \
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);   \
  crr_internal::StreamDevice on_dev_(s);                   \
  if (!on_dev_.ok) return (int)hipErrorInvalidHandle

// what the launches before it left, then the n totals of a plan on the host: the one synchronisation of a plan call
inline hipError_t read_totals(hipStream_t s, const uint64_t* dev, uint64_t* host, size_t n) {
  hipError_t e;
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(host, dev, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  return hipStreamSynchronize(s);
}

constexpr uint32_t kScanA = 0xFFFu & ~((1u << CRR_LOAD_T_KEYS) | (1u << CRR_LOAD_T_KEY_BYTES));
constexpr uint32_t kScanB = (1u << CRR_LOAD_T_KEYS) | (1u << CRR_LOAD_T_KEY_BYTES);

}  // namespace
}  // namespace crr_load

extern "C" {

using namespace crr_load;

size_t crr_load_scratch_bytes(uint32_t n_blobs, uint32_t n_wf) {
  uint64_t tot[kCounters] = {0};
  tot[0] = n_blobs;   // the widest row type for every pending entry
  tot[5] = tot[6] = 8ull * n_wf;
  tot[CRR_LOAD_T_TOKEN] = 128ull * n_wf;
  tot[kCand] = (uint64_t)n_blobs + 8ull * n_wf;
  tot[kCandBytes] = 32ull * tot[kCand];
  return (size_t)carve(n_blobs, n_wf, tot).end;
}

int crr_load_states_plan(const crr_state_batch* in, void* scratch, size_t scratch_bytes, crr_load_summary* summary,
                         void* stream) {
  if (!in || !summary || !scratch || ((uintptr_t)scratch & 15u)) return -1;
  if (in->n_blobs && (!in->bytes || !in->blob_off || !in->blob)) return -1;
  if (in->n_wf && !in->wf) return -1;
  CRR_ON_STREAM(s, stream);
  Ctx c;
  c.in = *in;
  c.s = static_cast<uint8_t*>(scratch);
  c.L = carve(in->n_blobs, in->n_wf, nullptr);
  memset(summary, 0, sizeof *summary);
  summary->err_blob = -1;
  summary->n_blobs = in->n_blobs;
  summary->n_wf = in->n_wf;
  if (c.L.end > scratch_bytes) {
    summary->err = CRR_INGEST_SCRATCH_TOO_SMALL;
    summary->scratch_needed = crr_load_scratch_bytes(in->n_blobs, in->n_wf);
    return 0;
  }
  if (in->n_wf == 0) return 0;
  hipError_t e;
  // err()[0] = no malformed blob, [1] = failed workflows, [2..] = the scans' totals, then the bad-ranges mark
  if ((e = hipMemsetAsync(c.err(), 0xFF, sizeof(uint64_t), s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(c.err() + 1, 0, (2 + kCounters) * sizeof(uint64_t), s)) != hipSuccess) return (int)e;
  uint64_t* d_tot = c.err() + 2;
  if (in->n_blobs) hipLaunchKernelGGL(load_parse_kernel, grid_of(in->n_blobs), dim3(kBlock), 0, s, c);
  hipLaunchKernelGGL(load_count_kernel, grid_of(in->n_wf), dim3(kBlock), 0, s, c);
  hipLaunchKernelGGL(load_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, c, kScanA, d_tot);
  uint64_t h[3 + kCounters];
  if ((e = read_totals(s, c.err(), h, sizeof h / sizeof h[0])) != hipSuccess) return (int)e;
  if (h[2 + kCounters]) return -1;   // blob ranges not consecutive or not covering the blobs
  c.L = carve(in->n_blobs, in->n_wf, h + 2);
  if (c.L.end > scratch_bytes) {
    summary->err = CRR_INGEST_SCRATCH_TOO_SMALL;
    summary->scratch_needed = c.L.end;
    return 0;
  }
  hipLaunchKernelGGL(load_emit_kernel, grid_of(in->n_wf), dim3(kBlock), 0, s, c);
  hipLaunchKernelGGL(load_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, c, kScanB, d_tot);
  hipLaunchKernelGGL(load_dict_kernel, grid_of(in->n_wf), dim3(kBlock), 0, s, c);
  if ((e = read_totals(s, c.err(), h, sizeof h / sizeof h[0])) != hipSuccess) return (int)e;
  int64_t totals[kCounters];
  for (int t = 0; t < kCounters; ++t) totals[t] = (int64_t)h[2 + t];
  fill_summary(summary, c, totals, h[0], h[1], c.L.end);
  return 0;
}

static bool plan_usable(const void* scratch, size_t scratch_bytes, const crr_load_summary* S, Ctx& c) {
  if (!scratch || !S || S->err != 0 || ((uintptr_t)scratch & 15u)) return false;
  c.s = const_cast<uint8_t*>(static_cast<const uint8_t*>(scratch));
  c.L = layout_of(*S);
  memset(&c.in, 0, sizeof c.in);
  c.in.n_blobs = S->n_blobs;
  c.in.n_wf = S->n_wf;
  return c.L.end <= scratch_bytes && c.L.end == S->scratch_needed;
}

int crr_load_states_read(const void* scratch, size_t scratch_bytes, const crr_load_summary* summary_host,
                         const crr_load_image* dst, void* stream) {
  Ctx c;
  if (!dst || !plan_usable(scratch, scratch_bytes, summary_host, c)) return -1;
  CRR_ON_STREAM(s, stream);
  const crr_load_summary& S = *summary_host;
  const size_t n = S.n_wf;
  if (n == 0) return 0;
  hipError_t e = hipSuccess;
  auto copy = [&](void* d, const void* src, size_t bytes) {
    if (d && bytes && e == hipSuccess) e = hipMemcpyAsync(d, src, bytes, hipMemcpyDefault, s);
  };
  copy(dst->exec, c.exec(), n * sizeof(crr_exec_row));
  for (int t = 0; t < 7; ++t) copy(dst->rows[t], c.rows(t), (size_t)S.totals[t] * kRowBytes[t]);
  copy(dst->offsets, c.cnt(0), (size_t)CRR_LOAD_TABLES * (n + 1) * sizeof(int64_t));
  copy(dst->tokens, c.tokens(), (size_t)S.totals[CRR_LOAD_T_TOKEN]);
  copy(dst->key_off, c.key_off(), (size_t)S.totals[CRR_LOAD_T_KEYS] * sizeof(uint64_t));
  copy(dst->key_len, c.key_len(), (size_t)S.totals[CRR_LOAD_T_KEYS] * sizeof(uint32_t));
  copy(dst->key_bytes, c.key_bytes(), (size_t)S.totals[CRR_LOAD_T_KEY_BYTES]);
  copy(dst->status, c.status(), n * sizeof(int32_t));
  copy(dst->flags, c.flags(), n * sizeof(uint32_t));
  return (int)e;
}

int crr_load_states_place(const void* scratch, size_t scratch_bytes, const crr_load_summary* summary_host,
                          const crr_inputs* layout, const uint32_t* perm, const crr_outputs* out, void* stream) {
  Ctx c;
  if (!layout || !out || !out->exec || !plan_usable(scratch, scratch_bytes, summary_host, c)) return -1;
  if (layout->n_wf && !layout->wf) return -1;
  if (layout->stride == 0 || ((layout->flags & CRR_IN_WAVE_TAIL) && layout->wave_begin > layout->n_wf)) return -1;
  int ids = 0;
  for (int t = 0; t < 5; ++t) ids += out->live_ids[t] != nullptr;
  if (ids != 0 && ids != 5) return -1;   // all five set or none
  CRR_ON_STREAM(s, stream);
  if (layout->n_wf == 0 || summary_host->n_wf == 0) return 0;
  PlaceArgs a;
  a.wf = layout->wf;
  a.perm = perm;
  a.n_pos = layout->n_wf;
  a.stride = layout->stride;
  a.wave_begin = (layout->flags & CRR_IN_WAVE_TAIL) ? layout->wave_begin : layout->n_wf;
  a.n_loaded = summary_host->n_wf;
  a.out = *out;
  hipLaunchKernelGGL(load_place_kernel, grid_of(a.n_pos), dim3(kBlock), 0, s, c, a);
  return (int)hipGetLastError();
}

int crr_load_states_verify(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                           const crr_load_summary* summary_host, const crr_stored_checksum* stored,
                           int64_t invalidate_before_ns, crr_verify_row* result, void* stream) {
  Ctx c;
  if (!in || !result || !plan_usable(scratch, scratch_bytes, summary_host, c)) return -1;
  if (in->n_blobs != summary_host->n_blobs || in->n_wf != summary_host->n_wf) return -1;   // not the planned batch
  if (in->n_blobs && (!in->bytes || !in->blob_off)) return -1;
  CRR_ON_STREAM(s, stream);
  if (in->n_wf == 0) return 0;
  c.in = *in;
  hipLaunchKernelGGL(load_verify_kernel, grid_of(in->n_wf), dim3(kBlock), 0, s, c, stored, invalidate_before_ns, result);
  return (int)hipGetLastError();
}

size_t crr_load_ndc_scratch_bytes(uint32_t n_wf, uint32_t n_tasks) { return (size_t)carve_ndc(n_wf, n_tasks).end; }

// the loader's context for the branch walk (a batch without workflows has no plan to read) and the work buffer
static bool ndc_usable(const crr_state_batch* in, const void* scratch, size_t scratch_bytes, const crr_load_summary* S,
                       void* work, uint32_t n_tasks, Ctx& c, NdcWork& k) {
  if (!in || !S || !work || ((uintptr_t)work & 15u)) return false;
  if (in->n_blobs != S->n_blobs || in->n_wf != S->n_wf) return false;   // not the planned batch
  if (in->n_wf) {
    if (!plan_usable(scratch, scratch_bytes, S, c)) return false;
    if (in->n_blobs && (!in->bytes || !in->blob_off)) return false;
  } else {
    memset(&c, 0, sizeof c);
  }
  c.in = *in;
  k.s = static_cast<uint8_t*>(work);
  k.L = carve_ndc(in->n_wf, n_tasks);
  k.n_wf = in->n_wf;
  k.n_tasks = n_tasks;
  return true;
}

int crr_load_ndc_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                      const crr_load_summary* summary_host, const crr_repl_task* tasks, uint32_t n_tasks,
                      uint32_t n_incoming, void* work, size_t work_bytes, crr_load_ndc_sizes* plan, void* stream) {
  Ctx c;
  NdcWork k;
  if (!plan || (n_tasks && !tasks) || !ndc_usable(in, scratch, scratch_bytes, summary_host, work, n_tasks, c, k)) return -1;
  CRR_ON_STREAM(s, stream);
  memset(plan, 0, sizeof *plan);
  plan->n_wf = in->n_wf;
  plan->n_tasks = n_tasks;
  plan->n_incoming = n_incoming;
  plan->work_needed = k.L.end;
  if (k.L.end > work_bytes) {
    plan->err = CRR_INGEST_SCRATCH_TOO_SMALL;
    return 0;
  }
  hipError_t e;
  if ((e = hipMemsetAsync(k.totals(), 0, 4 * sizeof(uint64_t), s)) != hipSuccess) return (int)e;
  if (in->n_wf) {
    hipLaunchKernelGGL(load_branches_count_kernel, grid_of(in->n_wf), dim3(kBlock), 0, s, c, k);
    hipLaunchKernelGGL(load_ndc_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, k.cnt(0), in->n_wf, 2, k.totals());
  } else if ((e = hipMemsetAsync(k.cnt(0), 0, kBrCounters * sizeof(int64_t), s)) != hipSuccess) {
    return (int)e;
  }
  if (n_tasks) {
    hipLaunchKernelGGL(load_task_room_kernel, grid_of(n_tasks), dim3(kBlock), 0, s, k, tasks);
    hipLaunchKernelGGL(load_ndc_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, k.out_off(), n_tasks, 1, k.totals() + 2);
  } else if ((e = hipMemsetAsync(k.out_off(), 0, sizeof(int64_t), s)) != hipSuccess) {
    return (int)e;
  }
  uint64_t h[4];
  if ((e = read_totals(s, k.totals(), h, sizeof h / sizeof h[0])) != hipSuccess) return (int)e;
  plan->n_branches = h[0];
  plan->n_items = h[1];
  plan->n_out_items = h[2];
  // crr_ndc_branch / crr_ndc_task index with 32 bits
  if (h[0] > 0xFFFFFFFFull || h[1] + n_incoming > 0xFFFFFFFFull || h[2] > 0xFFFFFFFFull) return -1;
  return 0;
}

int crr_load_ndc_run(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                     const crr_load_summary* summary_host, const crr_repl_task* tasks, const crr_vh_item* incoming,
                     void* work, size_t work_bytes, const crr_load_ndc_sizes* plan_host, const crr_load_branches* dst,
                     crr_ndc_result* results, crr_ndc_route* routes, crr_vh_item* out_items, uint32_t* out_begin,
                     void* stream) {
  Ctx c;
  NdcWork k;
  if (!plan_host || plan_host->err != 0 || !dst || !dst->branch_begin) return -1;
  const crr_load_ndc_sizes& P = *plan_host;
  if (!ndc_usable(in, scratch, scratch_bytes, summary_host, work, P.n_tasks, c, k)) return -1;
  if (P.n_wf != in->n_wf || P.work_needed != k.L.end || k.L.end > work_bytes) return -1;
  if (P.n_branches > 0xFFFFFFFFull || P.n_items + P.n_incoming > 0xFFFFFFFFull || P.n_out_items > 0xFFFFFFFFull) return -1;
  if (in->n_wf && !dst->current) return -1;
  if (P.n_branches && (!dst->branches || !dst->tokens)) return -1;
  if ((P.n_items || (P.n_tasks && P.n_incoming)) && !dst->items) return -1;
  if (P.n_tasks && (!tasks || !results || !routes || !out_items || !dst->branches || !dst->items || !dst->current)) return -1;
  if (P.n_tasks && P.n_incoming && !incoming) return -1;
  CRR_ON_STREAM(s, stream);
  hipError_t e;
  if (in->n_wf) hipLaunchKernelGGL(load_branches_emit_kernel, grid_of(in->n_wf), dim3(kBlock), 0, s, c, k, *dst);
  else if ((e = hipMemsetAsync(dst->branch_begin, 0, sizeof(int64_t), s)) != hipSuccess) return (int)e;
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if (P.n_tasks == 0) return 0;
  // the incoming items behind the local ones: one items array for crr_ndc_prepare
  if (P.n_incoming && (e = hipMemcpyAsync(dst->items + P.n_items, incoming, (size_t)P.n_incoming * sizeof(crr_vh_item),
                                          hipMemcpyDeviceToDevice, s)) != hipSuccess)
    return (int)e;
  hipLaunchKernelGGL(load_task_rows_kernel, grid_of(P.n_tasks), dim3(kBlock), 0, s, k, tasks, P.n_incoming, P.n_items,
                     dst->current, out_begin);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  crr_ndc_inputs ni;
  ni.tasks = k.rows();
  ni.branches = dst->branches;
  ni.items = dst->items;
  ni.n_tasks = P.n_tasks;
  ni.reserved = 0;
  const int rc = crr_ndc_prepare(&ni, results, out_items, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(load_route_kernel, grid_of(P.n_tasks), dim3(kBlock), 0, s, k, tasks, P.n_incoming, dst->branches,
                     dst->items, out_items, results, routes);
  return (int)hipGetLastError();
}

// the read-only arguments crr_load_store_checksums and the two calls of cadence_load_store_vh.h share, checked
// and packed for the kernels: 0, or -1 on an invalid argument
static int store_setup(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                       const crr_load_summary* summary_host, const crr_repl_task* tasks,
                       const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                       const crr_ndc_route* routes, const crr_load_branches* branches,
                       const crr_load_ndc_sizes* ndc_plan_host, const crr_inputs* replay_in,
                       const crr_outputs* replay_out, const uint32_t* position, Ctx& c, StoreIn& a, ReplayAfter& after) {
  if (!in || !summary_host || !ndc_plan_host || ndc_plan_host->err != 0) return -1;
  const crr_load_ndc_sizes& P = *ndc_plan_host;
  if (in->n_blobs != summary_host->n_blobs || in->n_wf != summary_host->n_wf || P.n_wf != in->n_wf) return -1;   // not the planned batch
  if (n_tasks > P.n_tasks) return -1;
  if (in->n_wf) {
    if (!plan_usable(scratch, scratch_bytes, summary_host, c)) return -1;
    if (in->n_blobs && (!in->bytes || !in->blob_off)) return -1;
  } else {
    memset(&c, 0, sizeof c);   // a batch without workflows has no plan to read: every task is not loaded
  }
  c.in = *in;
  if ((replay_in == nullptr) != (replay_out == nullptr)) return -1;
  if (replay_in) {
    if (replay_in->n_wf && (!replay_in->wf || !replay_out->exec)) return -1;
    if (replay_in->stride == 0 || ((replay_in->flags & CRR_IN_WAVE_TAIL) && replay_in->wave_begin > replay_in->n_wf)) return -1;
  }
  memset(&a, 0, sizeof a);
  memset(&after, 0, sizeof after);
  if (n_tasks) {
    if (!tasks || !last_events || !results || !routes || !branches) return -1;
    if (in->n_wf && (!branches->branch_begin || !branches->current)) return -1;
    if (P.n_branches && (!branches->branches || !branches->tokens)) return -1;
    if (P.n_items && !branches->items) return -1;
    a.br = *branches;
  }
  a.tasks = tasks;
  a.last = last_events;
  a.results = results;
  a.routes = routes;
  a.n_branches = P.n_branches;
  a.n_items = P.n_items;
  a.n_tasks = n_tasks;
  after.have = replay_in != nullptr;
  if (replay_in) {
    after.wf = replay_in->wf;
    after.position = position;
    after.out = *replay_out;
    after.n_pos = replay_in->n_wf;
    after.stride = replay_in->stride;
    after.wave_begin = (replay_in->flags & CRR_IN_WAVE_TAIL) ? replay_in->wave_begin : replay_in->n_wf;
  }
  return 0;
}

int crr_load_store_checksums(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                             const crr_load_summary* summary_host, const crr_repl_task* tasks,
                             const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                             const crr_ndc_route* routes, const crr_load_branches* branches,
                             const crr_load_ndc_sizes* ndc_plan_host, const crr_inputs* replay_in,
                             const crr_outputs* replay_out, const uint32_t* position, crr_store_row* result,
                             void* stream) {
  Ctx c;
  StoreIn a;
  ReplayAfter after;
  if (store_setup(in, scratch, scratch_bytes, summary_host, tasks, last_events, n_tasks, results, routes, branches,
                  ndc_plan_host, replay_in, replay_out, position, c, a, after) != 0)
    return -1;
  if (n_tasks && !result) return -1;
  CRR_ON_STREAM(s, stream);
  if (n_tasks == 0) return 0;
  hipLaunchKernelGGL(load_store_kernel, grid_of(n_tasks), dim3(kBlock), 0, s, c, a, after, result);
  return (int)hipGetLastError();
}

// the plan's work buffer: the generated marks [n_tasks + 1] (scanned to their count), then the two totals
struct VhLayout {
  uint64_t marks, totals, end;
};
static VhLayout carve_vh(uint32_t n_tasks) {
  VhLayout L;
  uint64_t o = 0;
  L.marks = o;   o = align16(o + ((uint64_t)n_tasks + 1) * sizeof(int64_t));
  L.totals = o;  o = align16(o + 2 * sizeof(uint64_t));
  L.end = o;
  return L;
}

size_t crr_load_store_vh_scratch_bytes(uint32_t n_tasks) { return (size_t)carve_vh(n_tasks).end; }

int crr_load_store_vh_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                           const crr_load_summary* summary_host, const crr_repl_task* tasks,
                           const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                           const crr_ndc_route* routes, const crr_load_branches* branches,
                           const crr_load_ndc_sizes* ndc_plan_host, const crr_inputs* replay_in,
                           const crr_outputs* replay_out, const uint32_t* position, crr_vh_blob_row* rows,
                           uint64_t* blob_off, void* work, size_t work_bytes, crr_vh_blob_sizes* plan, void* stream) {
  Ctx c;
  StoreIn a;
  ReplayAfter after;
  if (!plan || store_setup(in, scratch, scratch_bytes, summary_host, tasks, last_events, n_tasks, results, routes, branches,
                           ndc_plan_host, replay_in, replay_out, position, c, a, after) != 0)
    return -1;
  if (n_tasks && (!rows || !blob_off || !work || ((uintptr_t)work & 15u) || ((uintptr_t)blob_off & 7u))) return -1;
  CRR_ON_STREAM(s, stream);
  const VhLayout L = carve_vh(n_tasks);
  memset(plan, 0, sizeof *plan);
  plan->n_tasks = n_tasks;
  plan->work_needed = L.end;
  hipError_t e;
  if (n_tasks == 0) {
    if (blob_off && (e = hipMemsetAsync(blob_off, 0, sizeof(uint64_t), s)) != hipSuccess) return (int)e;
    return 0;
  }
  if (L.end > work_bytes) {
    plan->err = CRR_INGEST_SCRATCH_TOO_SMALL;
    return 0;
  }
  int64_t* marks = reinterpret_cast<int64_t*>(static_cast<uint8_t*>(work) + L.marks);
  uint64_t* totals = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(work) + L.totals);
  int64_t* lens = reinterpret_cast<int64_t*>(blob_off);
  hipLaunchKernelGGL(load_store_vh_size_kernel, grid_of(n_tasks), dim3(kBlock), 0, s, c, a, after, rows, lens, marks);
  hipLaunchKernelGGL(load_ndc_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, lens, n_tasks, 1, totals);
  hipLaunchKernelGGL(load_ndc_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, marks, n_tasks, 1, totals + 1);
  uint64_t h[2];
  if ((e = read_totals(s, totals, h, sizeof h / sizeof h[0])) != hipSuccess) return (int)e;
  plan->n_bytes = h[0];
  plan->n_generated = h[1];
  return 0;
}

int crr_load_store_vh_run(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                          const crr_load_summary* summary_host, const crr_repl_task* tasks,
                          const crr_last_event* last_events, const crr_ndc_result* results, const crr_ndc_route* routes,
                          const crr_load_branches* branches, const crr_load_ndc_sizes* ndc_plan_host,
                          const crr_inputs* replay_in, const crr_outputs* replay_out, const uint32_t* position,
                          const crr_vh_blob_row* rows, const uint64_t* blob_off, const crr_vh_blob_sizes* plan_host,
                          uint8_t* out, size_t out_capacity, void* stream) {
  Ctx c;
  StoreIn a;
  ReplayAfter after;
  if (!plan_host || plan_host->err != 0) return -1;
  const uint32_t n_tasks = plan_host->n_tasks;
  if (store_setup(in, scratch, scratch_bytes, summary_host, tasks, last_events, n_tasks, results, routes, branches,
                  ndc_plan_host, replay_in, replay_out, position, c, a, after) != 0)
    return -1;
  if (n_tasks && (!rows || !blob_off)) return -1;
  if (n_tasks == 0 && plan_host->n_bytes != 0) return -1;
  const uint64_t padded = align16(plan_host->n_bytes);
  if (padded < plan_host->n_bytes || (uint64_t)out_capacity < padded) return -1;
  if (padded && (!out || ((uintptr_t)out & 15u))) return -1;
  const uint64_t n_chunks = padded / 16, blocks = (n_chunks + kBlock - 1) / kBlock;
  if (blocks > 0x7FFFFFFFull) return -1;
  CRR_ON_STREAM(s, stream);
  if (n_chunks == 0) return 0;
  hipLaunchKernelGGL(load_store_vh_emit_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s, c, a, after, blob_off,
                     plan_host->n_bytes, n_chunks, reinterpret_cast<ulonglong2*>(out));
  return (int)hipGetLastError();
}

// ---- cadence_load_mutation.h ----------------------------------------------------------------------------------
// the plan's work buffer: the block sums [kMutCols][n_blocks + 1] (scanned in place), then the totals
struct MutPlanLayout {
  uint64_t sums, totals, end;
  uint32_t n_blocks;
};
static MutPlanLayout carve_mut_plan(uint32_t n_tasks) {
  MutPlanLayout L;
  L.n_blocks = (uint32_t)(((uint64_t)n_tasks + kBlock - 1) / kBlock);
  uint64_t o = 0;
  L.sums = o;    o = align16(o + (uint64_t)kMutCols * ((uint64_t)L.n_blocks + 1) * sizeof(int64_t));
  L.totals = o;  o = align16(o + kMutCols * sizeof(uint64_t));
  L.end = o;
  return L;
}
// the run's work buffer: the directory -- the exec rows' slots, then each map's upserted rows' slots
struct MutRunLayout {
  uint64_t dir_exec, dir[CRR_MUTATION_MAPS], end;
};
static MutRunLayout carve_mut_run(const crr_mutation_sizes& P) {
  MutRunLayout L;
  uint64_t o = 0;
  L.dir_exec = o;  o = align16(o + P.n_exec * sizeof(uint64_t));
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) { L.dir[t] = o; o = align16(o + P.n_upsert[t] * sizeof(uint64_t)); }
  L.end = o;
  return L;
}

size_t crr_load_mutation_scratch_bytes(uint32_t n_tasks) { return (size_t)carve_mut_plan(n_tasks).end; }

int crr_load_mutation_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                           const crr_load_summary* summary_host, const crr_repl_task* tasks,
                           const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                           const crr_ndc_route* routes, const crr_load_branches* branches,
                           const crr_load_ndc_sizes* ndc_plan_host, const crr_inputs* replay_in,
                           const crr_outputs* replay_out, const uint32_t* position, crr_mutation_row* rows,
                           void* work, size_t work_bytes, crr_mutation_sizes* plan, void* stream) {
  Ctx c;
  StoreIn a;
  ReplayAfter after;
  if (!plan || store_setup(in, scratch, scratch_bytes, summary_host, tasks, last_events, n_tasks, results, routes, branches,
                           ndc_plan_host, replay_in, replay_out, position, c, a, after) != 0)
    return -1;
  if (n_tasks && (!rows || !work || ((uintptr_t)work & 15u) || ((uintptr_t)rows & 3u))) return -1;
  CRR_ON_STREAM(s, stream);
  const MutPlanLayout L = carve_mut_plan(n_tasks);
  memset(plan, 0, sizeof *plan);
  plan->n_tasks = n_tasks;
  plan->work_needed = L.end;
  if (n_tasks == 0) return 0;
  if (L.end > work_bytes) {
    plan->err = CRR_INGEST_SCRATCH_TOO_SMALL;
    return 0;
  }
  int64_t* sums = reinterpret_cast<int64_t*>(static_cast<uint8_t*>(work) + L.sums);
  uint64_t* totals = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(work) + L.totals);
  hipLaunchKernelGGL(load_mutation_count_kernel, dim3(L.n_blocks), dim3(kBlock), 0, s, c, a, after, rows, sums, L.n_blocks);
  hipLaunchKernelGGL(load_ndc_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, sums, L.n_blocks, kMutCols, totals);
  hipLaunchKernelGGL(load_mutation_offsets_kernel, dim3(L.n_blocks), dim3(kBlock), 0, s, rows, n_tasks, sums, L.n_blocks);
  hipError_t e;
  uint64_t h[kMutCols];
  if ((e = read_totals(s, totals, h, sizeof h / sizeof h[0])) != hipSuccess) return (int)e;
  plan->n_exec = h[0];
  bool fits = true;
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) {
    plan->n_upsert[t] = h[1 + 2 * t];
    plan->n_delete[t] = h[2 + 2 * t];
    fits = fits && h[1 + 2 * t] <= 0xFFFFFFFFull && h[2 + 2 * t] <= 0xFFFFFFFFull;
  }
  plan->run_work_needed = carve_mut_run(*plan).end;
  return fits ? 0 : -1;
}

int crr_load_mutation_run(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                          const crr_load_summary* summary_host, const crr_repl_task* tasks,
                          const crr_last_event* last_events, const crr_ndc_result* results, const crr_ndc_route* routes,
                          const crr_load_branches* branches, const crr_load_ndc_sizes* ndc_plan_host,
                          const crr_inputs* replay_in, const crr_outputs* replay_out, const uint32_t* position,
                          const crr_mutation_row* rows, const crr_mutation_sizes* plan_host, const crr_mutation_out* out,
                          void* work, size_t work_bytes, void* stream) {
  Ctx c;
  StoreIn a;
  ReplayAfter after;
  if (!plan_host || plan_host->err != 0 || !out) return -1;
  const crr_mutation_sizes& P = *plan_host;
  const uint32_t n_tasks = P.n_tasks;
  if (store_setup(in, scratch, scratch_bytes, summary_host, tasks, last_events, n_tasks, results, routes, branches,
                  ndc_plan_host, replay_in, replay_out, position, c, a, after) != 0)
    return -1;
  if (n_tasks && !rows) return -1;
  // every total is a sum of 32-bit counts over at most n_tasks tasks, and none exists without an exec row
  if (P.n_exec > n_tasks || (P.n_exec && !replay_out)) return -1;
  auto usable = [](const void* p, uint64_t capacity, uint64_t total) {
    return capacity >= total && (total == 0 || (p && !((uintptr_t)p & 7u)));
  };
  if (!usable(out->exec, out->exec_capacity, P.n_exec)) return -1;
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) {
    if (P.n_upsert[t] > 0xFFFFFFFFull || P.n_delete[t] > 0xFFFFFFFFull) return -1;
    if ((P.n_upsert[t] || P.n_delete[t]) && !P.n_exec) return -1;
    if (!usable(out->upsert[t], out->upsert_capacity[t], P.n_upsert[t])) return -1;
    if (!usable(out->deleted[t], out->delete_capacity[t], P.n_delete[t])) return -1;
  }
  const MutRunLayout L = carve_mut_run(P);
  if (L.end > work_bytes || (L.end && (!work || ((uintptr_t)work & 15u)))) return -1;
  CRR_ON_STREAM(s, stream);
  if (n_tasks == 0 || P.n_exec == 0) return 0;
  const void* tables[CRR_MUTATION_MAPS] = {replay_out->act, replay_out->timer, replay_out->child, replay_out->rc, replay_out->sig};
  MutDst d;
  memset(&d, 0, sizeof d);
  uint8_t* w = static_cast<uint8_t*>(work);
  d.dir_exec = reinterpret_cast<uint64_t*>(w + L.dir_exec);
  d.n_exec = P.n_exec;
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) {
    if (P.n_upsert[t] && !tables[t]) return -1;
    d.dir[t] = reinterpret_cast<uint64_t*>(w + L.dir[t]);
    d.keys[t] = out->deleted[t];
    d.base[t] = static_cast<const uint8_t*>(tables[t]);
    d.n_upsert[t] = P.n_upsert[t];
    d.n_delete[t] = P.n_delete[t];
  }
  hipError_t e;
  if ((e = hipMemsetAsync(work, 0xFF, (size_t)L.end, s)) != hipSuccess) return (int)e;   // kMutNoSlot everywhere
  hipLaunchKernelGGL(load_mutation_emit_kernel, grid_of(n_tasks), dim3(kBlock), 0, s, c, a, after, rows, d);
  auto gather = [&](const void* table, const uint64_t* dir, uint32_t row_bytes, uint64_t n_rows, void* dst) {
    const uint32_t words = row_bytes / 8;
    const uint64_t n_words = n_rows * words, blocks = (n_words + kBlock - 1) / kBlock;   // < 2^32 * 26 / 128
    if (n_words == 0) return;
    hipLaunchKernelGGL(load_mutation_gather_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                       static_cast<const uint64_t*>(table), dir, words, n_words, static_cast<uint64_t*>(dst));
  };
  gather(replay_out->exec, d.dir_exec, sizeof(crr_exec_row), P.n_exec, out->exec);
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) gather(tables[t], d.dir[t], kRowBytes[t], P.n_upsert[t], out->upsert[t]);
  return (int)hipGetLastError();
}

// ---- cadence_load_store_exec.h --------------------------------------------------------------------------------
// the work buffer: the block sums [kExecCols][n_blocks + 1] (scanned in place), the totals, then a script per task
struct ExecLayout {
  uint64_t sums, totals, scripts, end;
  uint32_t n_blocks;
};
static ExecLayout carve_exec(uint32_t n_tasks) {
  ExecLayout L;
  L.n_blocks = (uint32_t)(((uint64_t)n_tasks + kBlock - 1) / kBlock);
  uint64_t o = 0;
  L.sums = o;     o = align16(o + (uint64_t)kExecCols * ((uint64_t)L.n_blocks + 1) * sizeof(int64_t));
  L.totals = o;   o = align16(o + kExecCols * sizeof(uint64_t));
  L.scripts = o;  o = align16(o + (uint64_t)n_tasks * sizeof(ExecScript));
  L.end = o;
  return L;
}

size_t crr_load_store_exec_scratch_bytes(uint32_t n_tasks) { return (size_t)carve_exec(n_tasks).end; }

// the arguments the two calls share beside store_setup's, checked and packed: 0, or -1
static int exec_setup(uint32_t n_tasks, const crr_inputs* replay_in, const crr_exec_blob_task* exec_tasks,
                      const crr_vh_blob_row* vh_rows, const uint64_t* vh_off, const crr_vh_blob_sizes* vh_plan_host,
                      const crr_blob_batch* task_blobs, ExecIn& x) {
  memset(&x, 0, sizeof x);
  if (!vh_plan_host || vh_plan_host->err != 0 || vh_plan_host->n_tasks != n_tasks) return -1;
  if (n_tasks && (!exec_tasks || !vh_rows || !vh_off || ((uintptr_t)vh_off & 7u))) return -1;
  x.xt = exec_tasks;
  x.vh_rows = vh_rows;
  x.vh_off = vh_off;
  x.vh_total = vh_plan_host->n_bytes;
  if (task_blobs) {
    const crr_blob_batch& B = *task_blobs;
    if (B.n_wf && !B.wf) return -1;
    if (B.n_blobs && (!B.bytes || !B.blob_off)) return -1;
    // (a batch without offsets has no total to check against: it reads as absent)
    if (B.n_wf && B.blob_off) pack_task_blobs(x, B);
  }
  if (replay_in) {
    x.etype = replay_in->ev.etype;
    x.ev_wf = replay_in->wf;
    x.ev_n_wf = replay_in->n_wf;
    x.ev_stride = replay_in->stride;
    x.ev_wave_begin = (replay_in->flags & CRR_IN_WAVE_TAIL) ? replay_in->wave_begin : replay_in->n_wf;
  }
  return 0;
}

int crr_load_store_exec_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                             const crr_load_summary* summary_host, const crr_repl_task* tasks,
                             const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                             const crr_ndc_route* routes, const crr_load_branches* branches,
                             const crr_load_ndc_sizes* ndc_plan_host, const crr_inputs* replay_in,
                             const crr_outputs* replay_out, const uint32_t* position,
                             const crr_exec_blob_task* exec_tasks, const crr_vh_blob_row* vh_rows,
                             const uint64_t* vh_off, const crr_vh_blob_sizes* vh_plan_host,
                             const crr_blob_batch* task_blobs, crr_exec_blob_row* rows, uint64_t* blob_off, void* work,
                             size_t work_bytes, crr_exec_blob_sizes* plan, void* stream) {
  Ctx c;
  StoreIn a;
  ReplayAfter after;
  ExecIn x;
  if (!plan || store_setup(in, scratch, scratch_bytes, summary_host, tasks, last_events, n_tasks, results, routes, branches,
                           ndc_plan_host, replay_in, replay_out, position, c, a, after) != 0)
    return -1;
  if (exec_setup(n_tasks, replay_in, exec_tasks, vh_rows, vh_off, vh_plan_host, task_blobs, x) != 0) return -1;
  if (n_tasks && (!rows || !blob_off || !work || ((uintptr_t)work & 15u) || ((uintptr_t)blob_off & 7u) || ((uintptr_t)rows & 7u)))
    return -1;
  CRR_ON_STREAM(s, stream);
  const ExecLayout L = carve_exec(n_tasks);
  memset(plan, 0, sizeof *plan);
  plan->n_tasks = n_tasks;
  plan->work_needed = plan->run_work_needed = L.end;
  hipError_t e;
  if (n_tasks == 0) {
    if (blob_off && (e = hipMemsetAsync(blob_off, 0, sizeof(uint64_t), s)) != hipSuccess) return (int)e;
    return 0;
  }
  if (L.end > work_bytes) {
    plan->err = CRR_INGEST_SCRATCH_TOO_SMALL;
    return 0;
  }
  uint8_t* w = static_cast<uint8_t*>(work);
  int64_t* sums = reinterpret_cast<int64_t*>(w + L.sums);
  uint64_t* totals = reinterpret_cast<uint64_t*>(w + L.totals);
  ExecScript* scripts = reinterpret_cast<ExecScript*>(w + L.scripts);
  hipLaunchKernelGGL(load_store_exec_size_kernel, dim3(L.n_blocks), dim3(kBlock), 0, s, c, a, after, x, rows, scripts, sums,
                     L.n_blocks);
  hipLaunchKernelGGL(load_ndc_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, sums, L.n_blocks, kExecCols, totals);
  hipLaunchKernelGGL(load_store_exec_offsets_kernel, dim3(L.n_blocks), dim3(kBlock), 0, s, rows, n_tasks, sums, blob_off);
  uint64_t h[kExecCols];
  if ((e = read_totals(s, totals, h, sizeof h / sizeof h[0])) != hipSuccess) return (int)e;
  plan->n_bytes = h[0];
  plan->n_blobs = h[1];
  plan->n_host = h[2];
  return h[3] ? -1 : 0;
}

int crr_load_store_exec_run(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                            const crr_load_summary* summary_host, const crr_repl_task* tasks,
                            const crr_last_event* last_events, const crr_ndc_result* results, const crr_ndc_route* routes,
                            const crr_load_branches* branches, const crr_load_ndc_sizes* ndc_plan_host,
                            const crr_inputs* replay_in, const crr_outputs* replay_out, const uint32_t* position,
                            const crr_exec_blob_task* exec_tasks, const crr_vh_blob_row* vh_rows, const uint64_t* vh_off,
                            const crr_vh_blob_sizes* vh_plan_host, const crr_blob_batch* task_blobs,
                            const crr_exec_blob_row* rows, const uint64_t* blob_off, const void* work, size_t work_bytes,
                            const crr_exec_blob_sizes* plan_host, const uint8_t* vh_bytes, uint8_t* out_bytes,
                            size_t out_capacity, void* stream) {
  Ctx c;
  StoreIn a;
  ReplayAfter after;
  ExecIn x;
  if (!plan_host || plan_host->err != 0) return -1;
  const uint32_t n_tasks = plan_host->n_tasks;
  if (store_setup(in, scratch, scratch_bytes, summary_host, tasks, last_events, n_tasks, results, routes, branches,
                  ndc_plan_host, replay_in, replay_out, position, c, a, after) != 0)
    return -1;
  if (exec_setup(n_tasks, replay_in, exec_tasks, vh_rows, vh_off, vh_plan_host, task_blobs, x) != 0) return -1;
  const ExecLayout L = carve_exec(n_tasks);
  if (n_tasks && (!rows || !blob_off || !work || ((uintptr_t)work & 15u) || L.end > work_bytes)) return -1;
  const uint64_t n_bytes = plan_host->n_bytes;
  if ((n_tasks == 0 && n_bytes != 0) || (uint64_t)out_capacity < n_bytes) return -1;
  if (n_bytes && (!out_bytes || ((uintptr_t)out_bytes & 15u))) return -1;
  if (x.vh_total && !vh_bytes) return -1;
  const uint64_t n_chunks = (n_bytes + 15) / 16, blocks = (n_chunks + kBlock - 1) / kBlock;
  if (n_chunks < n_bytes / 16 || blocks > 0x7FFFFFFFull) return -1;
  CRR_ON_STREAM(s, stream);
  if (n_chunks == 0) return 0;
  const ExecScript* scripts = reinterpret_cast<const ExecScript*>(static_cast<const uint8_t*>(work) + L.scripts);
  hipLaunchKernelGGL(load_store_exec_emit_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s, scripts, in->bytes,
                     in->n_blobs ? in->blob_off : nullptr, in->n_blobs, vh_bytes, x.vh_total, x.tb_bytes, x.tb_off,
                     x.tb_n_blobs, blob_off, n_tasks, n_bytes, n_chunks, out_bytes);
  return (int)hipGetLastError();
}

// ---- cadence_load_resume.h ------------------------------------------------------------------------------------
size_t crr_load_resume_scratch_bytes(uint32_t n_wf, uint32_t n_tasks) {
  (void)n_tasks;   // (the work is per position: the tasks only bid for one)
  return (size_t)carve_resume(n_wf).end;
}

// the arguments the plan and the gather share, checked and packed: 0, or -1
static int resume_setup(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                        const crr_load_summary* summary_host, const crr_repl_task* tasks, const crr_ndc_route* routes,
                        uint32_t n_tasks, const crr_blob_batch* task_blobs, const void* work, Ctx& c, ResumeIn& r,
                        ResumeWork& k) {
  if (!in || !summary_host || in->n_blobs != summary_host->n_blobs || in->n_wf != summary_host->n_wf) return -1;
  if (in->n_wf) {
    if (!plan_usable(scratch, scratch_bytes, summary_host, c)) return -1;
  } else {
    memset(&c, 0, sizeof c);   // a batch without workflows has no plan to read: every task is not loaded
  }
  c.in = *in;
  memset(&r, 0, sizeof r);
  if (n_tasks && (!tasks || !task_blobs)) return -1;   // (the plan checks its routes itself)
  r.tasks = tasks;
  r.routes = routes;
  r.n_tasks = n_tasks;
  if (task_blobs) {
    const crr_blob_batch& B = *task_blobs;
    if (B.n_wf && !B.wf) return -1;
    if (!B.blob_off || (B.n_blobs && !B.bytes)) return -1;
    pack_task_blobs(r, B);
  }
  k.s = const_cast<uint8_t*>(static_cast<const uint8_t*>(work));
  k.L = carve_resume(in->n_wf);
  k.n_wf = in->n_wf;
  return 0;
}

int crr_load_resume_plan(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                         const crr_load_summary* summary_host, const crr_repl_task* tasks, const crr_ndc_route* routes,
                         uint32_t n_tasks, const crr_blob_batch* task_blobs, crr_load_resume_row* rows, void* work,
                         size_t work_bytes, crr_load_resume_sizes* plan, void* stream) {
  Ctx c;
  ResumeIn r;
  ResumeWork k;
  if (!plan || resume_setup(in, scratch, scratch_bytes, summary_host, tasks, routes, n_tasks, task_blobs, work, c, r, k) != 0)
    return -1;
  if (n_tasks && (!routes || !rows || ((uintptr_t)rows & 3u))) return -1;
  if (in->n_wf && (!work || ((uintptr_t)work & 15u))) return -1;
  CRR_ON_STREAM(s, stream);
  memset(plan, 0, sizeof *plan);
  plan->n_tasks = n_tasks;
  plan->n_wf = in->n_wf;
  plan->work_needed = k.L.end;
  hipError_t e;
  if (in->n_wf == 0) {   // no position: every task is not routed or not loaded
    if (n_tasks) hipLaunchKernelGGL(load_resume_rows_kernel, grid_of(n_tasks), dim3(kBlock), 0, s, c, r, k, rows);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    return (int)hipStreamSynchronize(s);
  }
  if (k.L.end > work_bytes) {
    plan->err = CRR_INGEST_SCRATCH_TOO_SMALL;
    return 0;
  }
  if ((e = hipMemsetAsync(k.winner(), 0xFF, (size_t)in->n_wf * sizeof(uint32_t), s)) != hipSuccess) return (int)e;
  if (n_tasks) {
    hipLaunchKernelGGL(load_resume_bid_kernel, grid_of(n_tasks), dim3(kBlock), 0, s, c, r, k);
    hipLaunchKernelGGL(load_resume_rows_kernel, grid_of(n_tasks), dim3(kBlock), 0, s, c, r, k, rows);
  }
  hipLaunchKernelGGL(load_resume_count_kernel, dim3(k.L.n_blocks), dim3(kBlock), 0, s, c, r, k);
  hipLaunchKernelGGL(load_ndc_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, k.sums(), k.L.n_blocks, kResCols, k.totals());
  hipLaunchKernelGGL(load_resume_offsets_kernel, dim3(k.L.n_blocks), dim3(kBlock), 0, s, k);
  uint64_t h[kResCols];
  if ((e = read_totals(s, k.totals(), h, sizeof h / sizeof h[0])) != hipSuccess) return (int)e;
  plan->n_applied = h[kResApplied];
  plan->n_blobs = h[kResBlobs];
  plan->blob_bytes = h[kResBlobBytes];
  plan->n_keys = h[kResKeys];
  plan->key_bytes = h[kResKeyBytes];
  plan->token_bytes = h[kResTokenBytes];
  plan->n_bytes = align16(h[kResBlobBytes]) + h[kResKeyBytes];
  // crr_blob_wf, the seeds and the descriptors' token offsets index with 32 bits
  return h[kResBlobs] < 0xFFFFFFFFull && h[kResKeys] <= 0xFFFFFFFFull && h[kResTokenBytes] <= 0xFFFFFFFFull ? 0 : -1;
}

// the plan as a call after it may use it: its work buffer laid out for the planned batch
static bool resume_plan_usable(const crr_load_resume_sizes* P, uint32_t n_wf, const void* work, size_t work_bytes) {
  if (!P || P->err != 0 || P->n_wf != n_wf) return false;
  const ResumeLayout L = carve_resume(n_wf);
  if (P->work_needed != L.end) return false;
  if (n_wf && (!work || ((uintptr_t)work & 15u) || L.end > work_bytes)) return false;
  return P->n_blobs < 0xFFFFFFFFull && P->n_keys <= 0xFFFFFFFFull && P->token_bytes <= 0xFFFFFFFFull &&
         P->n_bytes == align16(P->blob_bytes) + P->key_bytes && P->n_applied <= n_wf;
}

int crr_load_resume_gather(const crr_state_batch* in, const void* scratch, size_t scratch_bytes,
                           const crr_load_summary* summary_host, const crr_repl_task* tasks,
                           const crr_blob_batch* task_blobs, const crr_load_resume_row* rows, const void* work,
                           size_t work_bytes, const crr_load_resume_sizes* plan_host, const crr_load_resume_out* out,
                           void* stream) {
  Ctx c;
  ResumeIn r;
  ResumeWork k;
  if (!plan_host || !out || !in || !resume_plan_usable(plan_host, in->n_wf, work, work_bytes)) return -1;
  const crr_load_resume_sizes& P = *plan_host;
  (void)rows;   // (neither the rows nor the routes are read again: the winners are in `work`)
  if (resume_setup(in, scratch, scratch_bytes, summary_host, tasks, nullptr, P.n_tasks, task_blobs, work, c, r, k) != 0) return -1;
  auto usable = [](const void* p, uint64_t capacity, uint64_t total, uintptr_t align) {
    return capacity >= total && (total == 0 || (p && !((uintptr_t)p & align)));
  };
  if (!usable(out->bytes, out->bytes_capacity, P.n_bytes, 15u)) return -1;
  if (!out->blob_off || ((uintptr_t)out->blob_off & 7u) || out->blob_capacity < P.n_blobs) return -1;
  if (!usable(out->key_off, out->key_capacity, P.n_keys, 7u) || !usable(out->key_len, out->key_capacity, P.n_keys, 3u)) return -1;
  if (in->n_wf && (!out->wf || ((uintptr_t)out->wf & 7u) || !out->key_begin || !out->key_count || !out->task_of)) return -1;
  const uint64_t n_chunks = (P.n_bytes + 15) / 16, blocks = (n_chunks + kBlock - 1) / kBlock;
  if (n_chunks < P.n_bytes / 16 || blocks > 0x7FFFFFFFull) return -1;
  CRR_ON_STREAM(s, stream);
  hipError_t e;
  if (in->n_wf == 0) return (int)hipMemsetAsync(out->blob_off, 0, sizeof(uint64_t), s);
  const ResumeTotals T = {P.n_blobs, P.blob_bytes, P.n_keys, P.key_bytes, P.n_bytes};
  uint64_t longest = in->n_wf;
  if (P.n_blobs + 1 > longest) longest = P.n_blobs + 1;
  if (P.n_keys > longest) longest = P.n_keys;
  hipLaunchKernelGGL(load_resume_index_kernel, dim3((uint32_t)((longest + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, c, r, k, T,
                     *out);
  if (n_chunks)
    hipLaunchKernelGGL(load_resume_gather_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s, c, r, k, T, n_chunks, out->bytes);
  e = hipGetLastError();
  return (int)e;
}

int crr_load_resume_finalize(const void* scratch, size_t scratch_bytes, const crr_load_summary* summary_host,
                             const crr_blob_wf* gathered_wf, const int32_t* counts, uint64_t count_stride, void* work,
                             size_t work_bytes, const crr_load_resume_sizes* plan_host, crr_workflow* wf, uint8_t* arena,
                             size_t arena_capacity, crr_load_resume_totals* totals, void* stream) {
  Ctx c;
  if (!summary_host || !totals || !resume_plan_usable(plan_host, summary_host->n_wf, work, work_bytes)) return -1;
  const crr_load_resume_sizes& P = *plan_host;
  const uint32_t n_wf = P.n_wf;
  if ((uint64_t)arena_capacity < P.token_bytes || (P.token_bytes && !arena)) return -1;
  if (n_wf) {
    if (!plan_usable(scratch, scratch_bytes, summary_host, c)) return -1;
    if (!gathered_wf || !counts || count_stride < n_wf || !wf || ((uintptr_t)wf & 7u) || ((uintptr_t)gathered_wf & 7u)) return -1;
  }
  CRR_ON_STREAM(s, stream);
  if (n_wf == 0) {
    memset(totals, 0, sizeof *totals);
    return 0;
  }
  ResumeWork k;
  k.s = static_cast<uint8_t*>(work);
  k.L = carve_resume(n_wf);
  k.n_wf = n_wf;
  hipLaunchKernelGGL(load_resume_caps_kernel, dim3(k.L.n_blocks), dim3(kBlock), 0, s, c, k, counts, count_stride);
  hipLaunchKernelGGL(load_ndc_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, k.cap_sums(), k.L.n_blocks, kResCaps, k.cap_totals());
  hipLaunchKernelGGL(load_resume_descriptor_kernel, dim3(k.L.n_blocks), dim3(kBlock), 0, s, c, k, gathered_wf, counts,
                     count_stride, wf, arena, (uint64_t)arena_capacity);
  hipError_t e;
  uint64_t h[kResCaps];
  if ((e = read_totals(s, k.cap_totals(), h, sizeof h / sizeof h[0])) != hipSuccess) return (int)e;
  memset(totals, 0, sizeof *totals);
  totals->arena_bytes = P.token_bytes;
  for (int t = 0; t < kResCaps; ++t) totals->table_rows[t] = h[t];
  return 0;
}

int crr_load_resume_settle(const int32_t* task_of, crr_workflow* wf, uint32_t n_wf, void* stream) {
  if (n_wf && (!task_of || !wf || ((uintptr_t)task_of & 3u) || ((uintptr_t)wf & 7u))) return -1;
  CRR_ON_STREAM(s, stream);
  if (n_wf == 0) return 0;
  hipLaunchKernelGGL(load_resume_settle_kernel, grid_of(n_wf), dim3(kBlock), 0, s, task_of, wf, n_wf);
  return (int)hipGetLastError();
}

}  // extern "C"
