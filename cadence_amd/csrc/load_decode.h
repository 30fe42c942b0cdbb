// load_decode.h -- the persisted mutable-state decoder (include/cadence_load.h), written once for both
// builds: load_states.cpp compiles it for the host (crr_load_states_host, the specification) and
// load_kernel.hip for gfx950 (crr_load_states_plan).  The phases are plain functions over one scratch
// buffer; a host loop or a kernel calls them per blob / per workflow, with a prefix scan between them:
//
//   parse_blob   per blob      a pending entry's sqlblobs struct -> its row image (Rec)
//   count_wf     per workflow  the execution blob -> the exec row; nested VersionHistories / ResetPoints
//                              walked once to validate and count; duplicate IDs; the workflow's status
//   (scan A)                   rows per table, token bytes, key candidates -> exclusive offsets
//   emit_wf      per workflow  rows into the dense tables at their rank by ID, keys interned in blob order,
//                              CRR_ROW_MAPPED, version-history items, token bytes, reset points
//   (scan B)                   dictionary entries and bytes
//   dict_wf      per workflow  the dictionary's key_off / key_len / bytes
//   verify_wf    per workflow  (on request, cadence_load_verify.h) the mutable-state checksum payload's CRC from
//                              the dense image and the persisted bytes, compared with the stored checksum
//   branches_count_wf / branches_emit_wf   per workflow  (on request, cadence_load_ndc.h) every history of the
//                              VersionHistories blob -> the branch table crr_ndc_prepare takes; task_row /
//                              route_task per replication task around that call
//   store_task   per task      (on request, cadence_load_store.h) the checksum to store once the routed task is
//                              committed: the payload written once behind a state view (payload_head ...), from the
//                              rows a resumed replay left or from the loaded image with the task's last event
//   mutation_count_task / mutation_emit_task   per task  (on request, cadence_load_mutation.h) the pending entries
//                              to upsert and the keys to delete for the same decision: one merge walk per pending
//                              map (mutation_walk) over the loaded image before and the state view after
//   exec_plan_task / exec_walk / exec_emit_chunk   per task  (on request, cadence_load_store_exec.h) the execution blob
//                              to store for the same decision: the stored blob's top-level fields spliced with the
//                              task's overrides, through an emitter (an edit script, or the sequential byte sink)
//
// Wire format: thrift binary (big-endian; field header = type byte + i16 id, 0 ends a struct), field IDs of
// .gen/go/sqlblobs/sqlblobs.go restated below (tests/golden/sqlblobs_fields.json pins them); a field whose
// wire type is not the expected one is skipped like an unknown one, as thriftrw's FromWire does.
// Every read is checked against the blob's end: a cursor that would pass it marks the reader bad, which
// ends the blob with CRR_LOAD_MALFORMED.
#ifndef CADENCE_LOAD_DECODE_H_
#define CADENCE_LOAD_DECODE_H_

#include <stdint.h>
#include <string.h>

#include "cadence_load.h"
#include "cadence_load_ndc.h"
#include "cadence_load_store.h"
#include "cadence_load_mutation.h"
#include "cadence_load_store_vh.h"
#include "cadence_load_store_exec.h"
#include "cadence_load_resume.h"
#include "cadence_load_verify.h"

#if defined(__HIPCC__)
#define CRR_HD __host__ __device__ inline
#else
#define CRR_HD inline
#endif

namespace crr_load {

// time.Time{}.UnixNano() (serialization/thrift_mapper.go:702, zeroTimeNanos): timeFromUnixNano maps it back
// to the zero time, which rows hold as CRR_ZERO_TIME
constexpr int64_t kGoZeroTimeNanos = -6795364578871345152LL;
constexpr uint64_t kInStrings = 1ull << 63;  // string offset: into crr_state_batch.strings, not .bytes

// counters per workflow, scanned in place to exclusive offsets ([t][n_wf] = the total); 0..9 are the image's
// offsets (CRR_LOAD_T_*), 10 / 11 the staging of key candidates (an upper bound of the dictionary)
constexpr int kCand = 10, kCandBytes = 11, kCounters = 12;
constexpr uint32_t kRowBytes[7] = {sizeof(crr_activity_row), sizeof(crr_timer_row), sizeof(crr_child_row),
                                   sizeof(crr_initiated_row), sizeof(crr_initiated_row), sizeof(crr_vh_item),
                                   sizeof(crr_reset_point_row)};

// thrift binary type bytes
enum : uint8_t { T_STOP = 0, T_BOOL = 2, T_BYTE = 3, T_DOUBLE = 4, T_I16 = 6, T_I32 = 8, T_I64 = 10, T_STRING = 11,
                 T_STRUCT = 12, T_MAP = 13, T_SET = 14, T_LIST = 15 };

// ---- bounds-checked reader --------------------------------------------------------------------------------
struct Rd {
  const uint8_t* p;
  uint64_t pos, end;  // pos <= end always
  bool bad;
};

CRR_HD bool need(Rd& r, uint64_t n) {
  if (r.bad || n > r.end - r.pos) {
    r.bad = true;
    return false;
  }
  return true;
}
CRR_HD uint8_t rd_u8(Rd& r) {
  if (!need(r, 1)) return 0;
  return r.p[r.pos++];
}
CRR_HD int16_t rd_i16(Rd& r) {
  if (!need(r, 2)) return 0;
  const uint16_t v = (uint16_t)((r.p[r.pos] << 8) | r.p[r.pos + 1]);
  r.pos += 2;
  return (int16_t)v;
}
CRR_HD int32_t rd_i32(Rd& r) {
  if (!need(r, 4)) return 0;
  uint32_t v;
  memcpy(&v, r.p + r.pos, 4);
  r.pos += 4;
  return (int32_t)__builtin_bswap32(v);
}
CRR_HD int64_t rd_i64(Rd& r) {
  if (!need(r, 8)) return 0;
  uint64_t v;
  memcpy(&v, r.p + r.pos, 8);
  r.pos += 8;
  return (int64_t)__builtin_bswap64(v);
}
// thriftrw's binary reader rejects a bool byte other than 0 / 1
CRR_HD bool rd_bool(Rd& r) {
  const uint8_t b = rd_u8(r);
  if (b > 1) r.bad = true;
  return b == 1;
}
CRR_HD bool rd_str(Rd& r, uint64_t& off, uint32_t& len) {
  const int32_t n = rd_i32(r);
  off = r.pos;
  len = 0;
  if (r.bad) return false;
  if (n < 0 || !need(r, (uint64_t)n)) {
    r.bad = true;
    return false;
  }
  len = (uint32_t)n;
  r.pos += (uint64_t)n;
  return true;
}

// Skipping a value of any type without recursion: containers push a frame; nesting past kMaxDepth (the
// persisted structs nest two deep: list<string>, map<string, binary>) is reported as malformed.
constexpr int kMaxDepth = 8;
struct Frame {
  uint32_t remaining;
  uint8_t mode, t1, t2, pad;  // mode 0 struct, 1 list / set (t1 element), 2 map (t1 key, t2 value)
};

CRR_HD void skip(Rd& r, uint8_t t, Frame* stk) {
  int sp = 0;
  uint8_t cur = t;
  bool have = true;
  for (;;) {
    if (r.bad) return;
    if (have) {
      have = false;
      Frame f = {0, 0, 0, 0, 0};
      bool push = false;
      switch (cur) {
        case T_BOOL: case T_BYTE: if (need(r, 1)) r.pos += 1; break;
        case T_I16: if (need(r, 2)) r.pos += 2; break;
        case T_I32: if (need(r, 4)) r.pos += 4; break;
        case T_DOUBLE: case T_I64: if (need(r, 8)) r.pos += 8; break;
        case T_STRING: {
          uint64_t o;
          uint32_t l;
          rd_str(r, o, l);
          break;
        }
        case T_STRUCT: push = true; break;
        case T_SET: case T_LIST: {
          f.mode = 1;
          f.t1 = rd_u8(r);
          const int32_t n = rd_i32(r);
          // every element takes at least one byte: a count past the blob's end is malformed
          if (n < 0 || (uint64_t)n > r.end - r.pos) r.bad = true;
          f.remaining = (uint32_t)n;
          push = true;
          break;
        }
        case T_MAP: {
          f.mode = 2;
          f.t1 = rd_u8(r);
          f.t2 = rd_u8(r);
          const int32_t n = rd_i32(r);
          if (n < 0 || 2 * (uint64_t)n > r.end - r.pos) r.bad = true;
          f.remaining = 2u * (uint32_t)n;
          push = true;
          break;
        }
        default: r.bad = true;
      }
      if (push && !r.bad) {
        if (sp == kMaxDepth) {
          r.bad = true;
          return;
        }
        stk[sp++] = f;
      }
      continue;
    }
    if (sp == 0) return;
    Frame& f = stk[sp - 1];
    if (f.mode == 0) {
      const uint8_t ft = rd_u8(r);
      if (r.bad) return;
      if (ft == T_STOP) {
        --sp;
        continue;
      }
      rd_i16(r);
      cur = ft;
      have = true;
    } else if (f.remaining == 0) {
      --sp;
    } else {
      cur = (f.mode == 2 && (f.remaining & 1u)) ? f.t2 : f.t1;  // 2n left: a key next
      --f.remaining;
      have = true;
    }
  }
}

CRR_HD bool next_field(Rd& r, uint8_t& t, int16_t& id) {
  t = rd_u8(r);
  if (r.bad || t == T_STOP) return false;
  id = rd_i16(r);
  return !r.bad;
}

CRR_HD int64_t from_unix_nano(int64_t v) { return v == kGoZeroTimeNanos ? CRR_ZERO_TIME : v; }

// ---- scratch layout ---------------------------------------------------------------------------------------
// a pending entry's parsed blob: its row image (src / key fields set by emit_wf) and where its key string is
struct Rec {
  int64_t id;        // the ID its map is keyed and ordered by
  uint64_t str_off;  // ActivityID (in bytes) / timer_id (kInStrings | offset in strings)
  uint32_t str_len;
  int32_t bad;       // the blob is malformed
  union {
    crr_activity_row act;
    crr_timer_row timer;
    crr_child_row child;
    crr_initiated_row init;
  } row;
};

// what count_wf learnt about the execution blob's nested blobs (absolute offsets into bytes)
struct ExecAux {
  uint64_t vh_off, rp_off;
  uint32_t vh_len, rp_len;
  int32_t exec_idx;   // index of the execution blob within the workflow
  int32_t current;    // current version-history index
  // what only the checksum payload needs (verify_wf): the sticky task list's name, every branch, the cut-off's time
  uint64_t sticky_off;
  int64_t last_updated;   // LastUpdatedTimeNanos as stored (absent: 0)
  uint32_t sticky_len;
  int32_t n_hist;
};

CRR_HD uint64_t align16(uint64_t x) { return (x + 15u) & ~15ull; }

struct Layout {
  uint64_t rec, aux, cnt, status, flags, err, exec, fixed_end;  // fixed part
  uint64_t rows[7], tokens, cand_off, cand_len, key_off, key_len, key_bytes, end;  // sized by scan A's totals
};

// `tot`: scan A's totals indexed like the counters (0..7, kCand, kCandBytes used); NULL: the fixed part only
inline Layout carve(uint32_t n_blobs, uint32_t n_wf, const uint64_t* tot) {
  Layout L;
  memset(&L, 0, sizeof L);
  uint64_t o = 0;
  L.rec = o;     o = align16(o + (uint64_t)n_blobs * sizeof(Rec));
  L.aux = o;     o = align16(o + (uint64_t)n_wf * sizeof(ExecAux));
  L.cnt = o;     o = align16(o + (uint64_t)kCounters * ((uint64_t)n_wf + 1) * sizeof(int64_t));
  L.status = o;  o = align16(o + (uint64_t)n_wf * sizeof(int32_t));
  L.flags = o;   o = align16(o + (uint64_t)n_wf * sizeof(uint32_t));
  L.err = o;     o = align16(o + (3 + kCounters) * sizeof(uint64_t));
  L.exec = o;    o = align16(o + (uint64_t)n_wf * sizeof(crr_exec_row));
  L.fixed_end = o;
  if (tot) {
    for (int t = 0; t < 7; ++t) { L.rows[t] = o; o = align16(o + tot[t] * kRowBytes[t]); }
    L.tokens = o;    o = align16(o + tot[CRR_LOAD_T_TOKEN]);
    L.cand_off = o;  o = align16(o + tot[kCand] * sizeof(uint64_t));
    L.cand_len = o;  o = align16(o + tot[kCand] * sizeof(uint32_t));
    L.key_off = o;   o = align16(o + tot[kCand] * sizeof(uint64_t));
    L.key_len = o;   o = align16(o + tot[kCand] * sizeof(uint32_t));
    L.key_bytes = o; o = align16(o + tot[kCandBytes]);
  }
  L.end = o;
  return L;
}

struct Ctx {
  crr_state_batch in;
  uint8_t* s;  // the scratch
  Layout L;
  CRR_HD Rec* rec() const { return reinterpret_cast<Rec*>(s + L.rec); }
  CRR_HD ExecAux* aux() const { return reinterpret_cast<ExecAux*>(s + L.aux); }
  CRR_HD int64_t* cnt(int t) const { return reinterpret_cast<int64_t*>(s + L.cnt) + (uint64_t)t * ((uint64_t)in.n_wf + 1); }
  CRR_HD int32_t* status() const { return reinterpret_cast<int32_t*>(s + L.status); }
  CRR_HD uint32_t* flags() const { return reinterpret_cast<uint32_t*>(s + L.flags); }
  CRR_HD uint64_t* err() const { return reinterpret_cast<uint64_t*>(s + L.err); }  // [0] lowest malformed blob, [1] failed, [2..] totals, [2 + kCounters] bad ranges
  CRR_HD crr_exec_row* exec() const { return reinterpret_cast<crr_exec_row*>(s + L.exec); }
  CRR_HD uint8_t* rows(int t) const { return s + L.rows[t]; }
  CRR_HD uint8_t* tokens() const { return s + L.tokens; }
  CRR_HD uint64_t* cand_off() const { return reinterpret_cast<uint64_t*>(s + L.cand_off); }
  CRR_HD uint32_t* cand_len() const { return reinterpret_cast<uint32_t*>(s + L.cand_len); }
  CRR_HD uint64_t* key_off() const { return reinterpret_cast<uint64_t*>(s + L.key_off); }
  CRR_HD uint32_t* key_len() const { return reinterpret_cast<uint32_t*>(s + L.key_len); }
  CRR_HD uint8_t* key_bytes() const { return s + L.key_bytes; }
  CRR_HD const uint8_t* str(uint64_t off) const { return (off & kInStrings) ? in.strings + (off & ~kInStrings) : in.bytes + off; }
  CRR_HD Rd blob(uint32_t b) const {
    Rd r = {in.bytes, in.blob_off[b], in.blob_off[b + 1], false};
    if (r.end < r.pos || r.end > in.blob_off[in.n_blobs]) {   // offsets not ascending within the batch's bytes
      r.end = r.pos;
      r.bad = true;
    }
    return r;
  }
};

CRR_HD void note_malformed(const Ctx& c, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(reinterpret_cast<unsigned long long*>(c.err()), (unsigned long long)b);
#else
  uint64_t* p = c.err();
  uint64_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (b < cur && !__atomic_compare_exchange_n(p, &cur, b, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
#endif
}
CRR_HD void note_failed(const Ctx& c) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(reinterpret_cast<unsigned long long*>(c.err() + 1), 1ull);
#else
  __atomic_fetch_add(c.err() + 1, 1ull, __ATOMIC_RELAXED);
#endif
}

// ---- pending entries: sqlblobs.ActivityInfo / TimerInfo / ChildExecutionInfo / RequestCancelInfo / SignalInfo
#define CRR_F(ID, TYPE, STMT) \
  case ID:                    \
    if (t == TYPE) {          \
      STMT;                   \
    } else {                  \
      skip(r, t, stk);        \
    }                         \
    break;

CRR_HD void parse_blob(const Ctx& c, uint32_t b, Frame* stk) {
  const crr_state_blob B = c.in.blob[b];
  Rec o;
  memset(&o, 0, sizeof o);
  o.id = B.id;
  if (B.kind == CRR_STATE_EXECUTION || B.kind > CRR_STATE_SIGNAL) {  // execution blobs: count_wf
    o.bad = B.kind > CRR_STATE_SIGNAL;
    c.rec()[b] = o;
    return;
  }
  Rd r = c.blob(b);
  uint8_t t;
  int16_t id;
  if (B.kind == CRR_STATE_ACTIVITY) {
    crr_activity_row& a = o.row.act;   // absent fields: the Go getters' zero values (times: Unix 0)
    a.schedule_id = B.id;
    a.flags = CRR_ROW_LIVE;
    a.last_heartbeat_time = from_unix_nano(B.aux_time);
    while (next_field(r, t, id)) {
      switch (id) {
        CRR_F(10, T_I64, a.version = rd_i64(r))
        CRR_F(12, T_I64, a.scheduled_batch_id = rd_i64(r))
        CRR_F(18, T_I64, a.scheduled_time = from_unix_nano(rd_i64(r)))
        CRR_F(20, T_I64, a.started_id = rd_i64(r))
        CRR_F(26, T_I64, a.started_time = from_unix_nano(rd_i64(r)))
        CRR_F(28, T_STRING, rd_str(r, o.str_off, o.str_len))
        CRR_F(32, T_I32, a.schedule_to_start = rd_i32(r))
        CRR_F(34, T_I32, a.schedule_to_close = rd_i32(r))
        CRR_F(36, T_I32, a.start_to_close = rd_i32(r))
        CRR_F(38, T_I32, a.heartbeat = rd_i32(r))
        CRR_F(40, T_BOOL, a.flags = (a.flags & ~CRR_ROW_CANCEL_REQUESTED) | (rd_bool(r) ? CRR_ROW_CANCEL_REQUESTED : 0u))
        CRR_F(42, T_I64, a.cancel_request_id = rd_i64(r))
        CRR_F(44, T_I32, a.timer_task_status = rd_i32(r))
        CRR_F(46, T_I32, a.attempt = rd_i32(r))
        CRR_F(52, T_BOOL, a.flags = (a.flags & ~CRR_ROW_HAS_RETRY) | (rd_bool(r) ? CRR_ROW_HAS_RETRY : 0u))
        default: skip(r, t, stk);
      }
    }
  } else if (B.kind == CRR_STATE_TIMER) {
    crr_timer_row& m = o.row.timer;
    m.flags = CRR_ROW_LIVE;
    o.str_off = kInStrings | B.str_off;
    o.str_len = B.str_len;
    while (next_field(r, t, id)) {
      switch (id) {
        CRR_F(10, T_I64, m.version = rd_i64(r))
        CRR_F(12, T_I64, m.started_id = rd_i64(r))
        CRR_F(14, T_I64, m.expiry_time = from_unix_nano(rd_i64(r)))
        CRR_F(16, T_I64, m.task_status = (int32_t)rd_i64(r))   // TaskID carries TaskStatus (workflowStateMaps.go:296-299)
        default: skip(r, t, stk);
      }
    }
    o.id = m.started_id;
  } else if (B.kind == CRR_STATE_CHILD) {
    crr_child_row& m = o.row.child;
    m.initiated_id = B.id;
    m.flags = CRR_ROW_LIVE;
    while (next_field(r, t, id)) {
      switch (id) {
        CRR_F(10, T_I64, m.version = rd_i64(r))
        CRR_F(12, T_I64, m.initiated_batch_id = rd_i64(r))
        CRR_F(14, T_I64, m.started_id = rd_i64(r))
        default: skip(r, t, stk);
      }
    }
  } else {  // RequestCancelInfo / SignalInfo: the same two numeric fields
    crr_initiated_row& m = o.row.init;
    m.initiated_id = B.id;
    m.flags = CRR_ROW_LIVE;
    while (next_field(r, t, id)) {
      switch (id) {
        CRR_F(10, T_I64, m.version = rd_i64(r))
        CRR_F(11, T_I64, m.initiated_batch_id = rd_i64(r))
        default: skip(r, t, stk);
      }
    }
  }
  o.bad = r.bad;
  c.rec()[b] = o;
}

// ---- nested DataBlobs ---------------------------------------------------------------------------------------
CRR_HD bool str_is(const uint8_t* p, uint32_t len, const char* lit, uint32_t n) {
  if (len != n) return false;
  for (uint32_t i = 0; i < n; ++i)
    if (p[i] != (uint8_t)lit[i]) return false;
  return true;
}

struct VhWalk {
  int32_t current;     // CurrentVersionHistoryIndex (absent: 0)
  int32_t n_hist;
  int32_t n_items;     // of history `target`
  uint64_t tok_off;    // its branch token
  uint32_t tok_len;
};

// one shared.VersionHistoryItem{10 eventID, 20 version}, the cursor at its first field
CRR_HD crr_vh_item read_vh_item(Rd& r, Frame* stk) {
  crr_vh_item it = {0, 0};
  uint8_t t;
  int16_t id;
  while (next_field(r, t, id)) {
    if (id == 10 && t == T_I64) it.event_id = rd_i64(r);
    else if (id == 20 && t == T_I64) it.version = rd_i64(r);
    else skip(r, t, stk);
  }
  return it;
}

struct VhNoVisit {
  CRR_HD void operator()(uint64_t, uint32_t, uint64_t, int32_t) const {}
};

// shared.VersionHistories{10 currentVersionHistoryIndex, 20 list<VersionHistory{10 branchToken,
// 20 list<VersionHistoryItem{10 eventID, 20 version}>}>} behind the 0x59 preamble; items of history `target`
// go to `items` (NULL: counted only).  false: malformed (a repeated list field included, so that every
// index written here stays below the count an earlier walk returned).
// `vis(token offset, token length, items position, item count)` is called once per history, in stored order,
// when its struct ends: the token as its last field 10 gave it (absent: length 0), the items as the cursor
// behind the list's header and the element count (absent: 0), to be read again with read_vh_item.
template <class Vis>
CRR_HD bool walk_vh(Rd r, int32_t target, crr_vh_item* items, VhWalk& out, Frame* stk, Vis&& vis) {
  out.current = 0;
  out.n_hist = 0;
  out.n_items = 0;
  out.tok_off = 0;
  out.tok_len = 0;
  if (rd_u8(r) != 0x59) return false;
  uint8_t t, t2;
  int16_t id, id2;
  bool seen_histories = false;
  while (next_field(r, t, id)) {
    if (id == 10 && t == T_I32) {
      out.current = rd_i32(r);
    } else if (id == 20 && t == T_LIST) {
      if (seen_histories) return false;   // thriftrw never writes a field twice: a repeated list is malformed
      seen_histories = true;
      const uint8_t et = rd_u8(r);
      const int32_t n = rd_i32(r);
      if (r.bad || et != T_STRUCT || n < 0 || (uint64_t)n > r.end - r.pos) return false;
      for (int32_t h = 0; h < n; ++h) {
        const bool mine = out.n_hist == target;
        bool seen_items = false;
        uint64_t tok_off = 0, items_pos = 0;
        uint32_t tok_len = 0;
        int32_t n_items = 0;
        while (next_field(r, t2, id2)) {
          if (id2 == 10 && t2 == T_STRING) {
            rd_str(r, tok_off, tok_len);
            if (mine) {
              out.tok_off = tok_off;
              out.tok_len = tok_len;
            }
          } else if (id2 == 20 && t2 == T_LIST) {
            const uint8_t et2 = rd_u8(r);
            const int32_t m = rd_i32(r);
            if (r.bad || seen_items || et2 != T_STRUCT || m < 0 || (uint64_t)m > r.end - r.pos) return false;
            seen_items = true;
            items_pos = r.pos;
            n_items = m;
            for (int32_t k = 0; k < m; ++k) {
              const crr_vh_item it = read_vh_item(r, stk);
              if (r.bad) return false;
              if (mine) {
                if (items) items[out.n_items] = it;
                ++out.n_items;
              }
            }
          } else {
            skip(r, t2, stk);
          }
        }
        if (r.bad) return false;
        vis(tok_off, tok_len, items_pos, n_items);
        ++out.n_hist;
      }
    } else {
      skip(r, t, stk);
    }
  }
  return !r.bad;
}

CRR_HD bool walk_vh(Rd r, int32_t target, crr_vh_item* items, VhWalk& out, Frame* stk) {
  return walk_vh(r, target, items, out, stk, VhNoVisit());
}

// shared.ResetPoints{10 list<ResetPointInfo{10 binaryChecksum, 20 runID, 30 firstDecisionCompletedID,
// 40 createdTimeNano, 50 expiringTimeNano, 60 resettable}>} behind the 0x59 preamble.  `F(index, checksum
// offset, length, resettable)` is called per point.  false: malformed.
template <class Fn>
CRR_HD bool walk_reset_points(Rd r, Frame* stk, Fn&& fn) {
  if (rd_u8(r) != 0x59) return false;
  uint8_t t, t2;
  int16_t id, id2;
  bool seen_points = false;
  while (next_field(r, t, id)) {
    if (id == 10 && t == T_LIST) {
      if (seen_points) return false;   // as in walk_vh: so the count pass and the emit pass see one list
      seen_points = true;
      const uint8_t et = rd_u8(r);
      const int32_t n = rd_i32(r);
      if (r.bad || et != T_STRUCT || n < 0 || (uint64_t)n > r.end - r.pos) return false;
      for (int32_t k = 0; k < n; ++k) {
        uint64_t off = 0;
        uint32_t len = 0;
        bool resettable = false;
        while (next_field(r, t2, id2)) {
          if (id2 == 10 && t2 == T_STRING) rd_str(r, off, len);
          else if (id2 == 60 && t2 == T_BOOL) resettable = rd_bool(r);
          else skip(r, t2, stk);
        }
        if (r.bad) return false;
        fn(k, off, len, resettable);
      }
    } else {
      skip(r, t, stk);
    }
  }
  return !r.bad;
}

// ---- per workflow: the execution blob, the counts, the status ---------------------------------------------
struct ExecParse {
  uint64_t vh_enc_off, rp_enc_off;
  uint32_t vh_enc_len, rp_enc_len;
};

// sqlblobs.WorkflowExecutionInfo -> the exec row (persistence_mapper.go ToInternalWorkflowExecutionInfo)
CRR_HD bool parse_execution(Rd& r, Frame* stk, int32_t idx, crr_exec_row& R, ExecAux& A, ExecParse& P) {
  uint8_t t;
  int16_t id;
  R.fail_step = -1;
  R.completion_event_batch_id = CRR_EMPTY_EVENT_ID;   // persistence_mapper.go:32, kept when the field is absent
  R.current_version = CRR_EMPTY_VERSION;              // Load, mutable_state_builder.go:325
  R.flags = CRR_EXEC_RESET_POINTS_SET;                // DeserializeResetPoints never returns nil (serializer.go:144-148)
  R.decision_request_src = CRR_SRC_NONE;
  R.start_src = idx;
  while (next_field(r, t, id)) {
    switch (id) {
      CRR_F(18, T_I64, R.completion_event_batch_id = rd_i64(r))
      CRR_F(30, T_I32, R.decision_start_to_close = rd_i32(r))
      CRR_F(34, T_I32, R.state = rd_i32(r))
      CRR_F(36, T_I32, R.close_status = rd_i32(r))
      CRR_F(48, T_I64, R.last_event_task_id = rd_i64(r))
      CRR_F(50, T_I64, R.last_first_event_id = rd_i64(r))
      CRR_F(52, T_I64, R.last_processed_event = rd_i64(r))
      CRR_F(56, T_I64, A.last_updated = rd_i64(r))
      CRR_F(58, T_I64, R.decision_version = rd_i64(r))
      CRR_F(60, T_I64, R.decision_schedule_id = rd_i64(r))
      CRR_F(62, T_I64, R.decision_started_id = rd_i64(r))
      CRR_F(64, T_I32, R.decision_timeout = rd_i32(r))
      CRR_F(66, T_I64, R.decision_attempt = rd_i64(r))
      CRR_F(68, T_I64, R.decision_started_ts = from_unix_nano(rd_i64(r)))
      CRR_F(69, T_I64, R.decision_scheduled_ts = from_unix_nano(rd_i64(r)))
      CRR_F(70, T_BOOL, R.flags = (R.flags & ~CRR_EXEC_CANCEL_REQUESTED) | (rd_bool(r) ? CRR_EXEC_CANCEL_REQUESTED : 0u))
      CRR_F(71, T_I64, R.decision_orig_scheduled_ts = from_unix_nano(rd_i64(r)))
      case 74:
        if (t == T_STRING) {
          uint64_t o;
          uint32_t l;
          if (rd_str(r, o, l))
            R.decision_request_src = l == 0 ? CRR_SRC_NONE : (str_is(r.p + o, l, "emptyUuid", 9) ? CRR_SRC_EMPTY_UUID : idx);
        } else {
          skip(r, t, stk);
        }
        break;
      CRR_F(78, T_STRING, rd_str(r, A.sticky_off, A.sticky_len))
      case 94:   // ExpirationTime: 0 in the row when unset or the zero time
        if (t == T_I64) {
          const int64_t v = rd_i64(r);
          R.expiration_ns = v == kGoZeroTimeNanos ? 0 : v;
        } else {
          skip(r, t, stk);
        }
        break;
      CRR_F(106, T_I64, R.signal_count = (int32_t)rd_i64(r))
      CRR_F(115, T_STRING, rd_str(r, A.rp_off, A.rp_len))
      CRR_F(116, T_STRING, rd_str(r, P.rp_enc_off, P.rp_enc_len))
      CRR_F(122, T_STRING, rd_str(r, A.vh_off, A.vh_len))
      CRR_F(124, T_STRING, rd_str(r, P.vh_enc_off, P.vh_enc_len))
      default: skip(r, t, stk);
    }
  }
  return !r.bad;
}
#undef CRR_F

CRR_HD bool bytes_equal(const uint8_t* a, const uint8_t* b, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

// the workflows' blob ranges are consecutive and cover the blobs (cadence_load.h): checked per workflow against
// its predecessor, so the device plan refuses the batches the host entry point refuses
CRR_HD bool range_ok(const Ctx& c, uint32_t w) {
  const crr_state_wf W = c.in.wf[w];
  const uint64_t begin = w ? (uint64_t)c.in.wf[w - 1].blob_begin + c.in.wf[w - 1].blob_count : 0;
  if (W.blob_begin != begin) return false;
  return w + 1 < c.in.n_wf || (uint64_t)W.blob_begin + W.blob_count == c.in.n_blobs;
}

CRR_HD void count_wf(const Ctx& c, uint32_t w, Frame* stk) {
  const crr_state_wf W = c.in.wf[w];
  const uint32_t b0 = W.blob_begin;
  const uint32_t n = (uint64_t)b0 + W.blob_count <= c.in.n_blobs ? W.blob_count : 0;   // a range outside the batch: no blobs
  crr_exec_row R;
  memset(&R, 0, sizeof R);
  ExecAux A;
  memset(&A, 0, sizeof A);
  ExecParse P;
  memset(&P, 0, sizeof P);
  int64_t cnt[kCounters];
  for (int t = 0; t < kCounters; ++t) cnt[t] = 0;
  int32_t n_exec = 0;
  bool malformed = false;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t k = c.in.blob[b0 + i].kind;
    if (k == CRR_STATE_EXECUTION) {
      ++n_exec;
      A.exec_idx = (int32_t)i;
    } else {
      const Rec& rc = c.rec()[b0 + i];
      if (rc.bad) {
        malformed = true;
        note_malformed(c, b0 + i);
      } else {
        ++cnt[k - 1];
        if (k == CRR_STATE_ACTIVITY || k == CRR_STATE_TIMER) {
          ++cnt[kCand];
          cnt[kCandBytes] += rc.str_len;
        }
      }
    }
  }
  int32_t st = CRR_LOAD_OK;
  uint32_t fl = 0;
  if (W.blob_count > CRR_LOAD_MAX_BLOBS) st = CRR_LOAD_TOO_LARGE;
  else if (n_exec != 1) st = CRR_LOAD_EXECUTION_COUNT;
  VhWalk V;
  memset(&V, 0, sizeof V);
  if (st == CRR_LOAD_OK) {
    const uint32_t eb = b0 + (uint32_t)A.exec_idx;
    Rd r = c.blob(eb);
    bool ok = parse_execution(r, stk, A.exec_idx, R, A, P);
    bool enc_ok = true, vh_ok = true;
    if (ok && A.vh_len) {   // an empty nested blob: the field is absent
      if (!str_is(r.p + P.vh_enc_off, P.vh_enc_len, "thriftrw", 8)) enc_ok = false;
      else {
        Rd v = {c.in.bytes, A.vh_off, A.vh_off + A.vh_len, false};
        VhWalk V0;
        ok = walk_vh(v, -1, nullptr, V0, stk);
        if (ok) {
          if (V0.n_hist == 0 || V0.current < 0 || V0.current >= V0.n_hist) vh_ok = false;
          else ok = walk_vh(v, V0.current, nullptr, V, stk);
        }
      }
    } else if (ok) {
      vh_ok = false;
    }
    if (ok && A.rp_len) {
      if (!str_is(r.p + P.rp_enc_off, P.rp_enc_len, "thriftrw", 8)) enc_ok = false;
      else {
        Rd v = {c.in.bytes, A.rp_off, A.rp_off + A.rp_len, false};
        int64_t n_rp = 0, rp_bytes = 0, n_keyed = 0;
        ok = walk_reset_points(v, stk, [&](int32_t, uint64_t, uint32_t len, bool) {
          ++n_rp;
          n_keyed += len != 0;
          rp_bytes += len;
        });
        cnt[6] = n_rp;
        cnt[kCand] += n_keyed;
        cnt[kCandBytes] += rp_bytes;
      }
    }
    if (!ok) {
      malformed = true;
      note_malformed(c, eb);
    }
    if (malformed) st = CRR_LOAD_MALFORMED;
    else if (!enc_ok) st = CRR_LOAD_NESTED_ENCODING;
    else if (!vh_ok) st = CRR_LOAD_VERSION_HISTORIES;
    else if (cnt[6] > CRR_LOAD_MAX_BLOBS) st = CRR_LOAD_TOO_LARGE;   // reset points: interned one against the other
  }
  if (st == CRR_LOAD_OK) {   // duplicate IDs within a map (timers: StartedID, or the timer_id the store keys them by)
    for (uint32_t i = 0; i < n && st == CRR_LOAD_OK; ++i) {
      const uint32_t k = c.in.blob[b0 + i].kind;
      if (k == CRR_STATE_EXECUTION) continue;
      const Rec& a = c.rec()[b0 + i];
      for (uint32_t j = i + 1; j < n; ++j) {
        if (c.in.blob[b0 + j].kind != k) continue;
        const Rec& b = c.rec()[b0 + j];
        if (a.id == b.id || (k == CRR_STATE_TIMER && a.str_len == b.str_len &&
                             bytes_equal(c.str(a.str_off), c.str(b.str_off), a.str_len))) {
          st = CRR_LOAD_DUPLICATE_ID;
          break;
        }
      }
    }
  }
  if (st == CRR_LOAD_OK) {
    A.current = V.current;
    A.n_hist = V.n_hist;
    cnt[5] = V.n_items;
    cnt[CRR_LOAD_T_TOKEN] = V.tok_len;
    R.next_event_id = W.next_event_id;
    R.n_activity = (int32_t)cnt[0];
    R.n_timer = (int32_t)cnt[1];
    R.n_child = (int32_t)cnt[2];
    R.n_rc = (int32_t)cnt[3];
    R.n_signal = (int32_t)cnt[4];
    R.n_vh_items = (int32_t)cnt[5];
    R.n_reset_points = (int32_t)cnt[6];
    R.token_src = V.tok_len ? 1 : 0;
    R.src_next = (int32_t)n;
    if (A.sticky_len) fl |= CRR_LOAD_FLAG_STICKY;
    if (V.n_hist > 1) fl |= CRR_LOAD_FLAG_MULTI_BRANCH;
  } else {
    memset(&R, 0, sizeof R);
    for (int t = 0; t < kCounters; ++t) cnt[t] = 0;
    note_failed(c);
  }
  c.exec()[w] = R;
  c.aux()[w] = A;
  c.status()[w] = st;
  c.flags()[w] = fl;
  for (int t = 0; t < kCounters; ++t) c.cnt(t)[w] = cnt[t];
  c.cnt(CRR_LOAD_T_KEYS)[w] = 0;   // emit_wf's
  c.cnt(CRR_LOAD_T_KEY_BYTES)[w] = 0;
}

// ---- per workflow: the dense rows ---------------------------------------------------------------------------
struct Interner {
  const Ctx& c;
  uint64_t base;   // the workflow's candidate region: its distinct strings in first-seen order
  uint32_t n;
  uint64_t bytes;
  CRR_HD uint32_t operator()(uint64_t off, uint32_t len) {
    if (len == 0) return 0;
    const uint8_t* s = c.str(off);
    for (uint32_t k = 0; k < n; ++k)
      if (c.cand_len()[base + k] == len && bytes_equal(c.str(c.cand_off()[base + k]), s, len)) return k + 1;
    c.cand_off()[base + n] = off;
    c.cand_len()[base + n] = len;
    bytes += len;
    return ++n;
  }
};

CRR_HD void emit_wf(const Ctx& c, uint32_t w, Frame* stk) {
  if (c.status()[w] != CRR_LOAD_OK) return;   // (its counters are zero)
  const crr_state_wf W = c.in.wf[w];
  const uint32_t b0 = W.blob_begin, n = W.blob_count;
  const ExecAux A = c.aux()[w];
  // (named scalars, not an array indexed by the blob's kind: the offsets stay in registers)
  const int64_t o0 = c.cnt(0)[w], o1 = c.cnt(1)[w], o2 = c.cnt(2)[w], o3 = c.cnt(3)[w], o4 = c.cnt(4)[w], o5 = c.cnt(5)[w],
                o6 = c.cnt(6)[w], o7 = c.cnt(CRR_LOAD_T_TOKEN)[w];
  Interner intern = {c, (uint64_t)c.cnt(kCand)[w], 0, 0};
  const Rec* recs = c.rec() + b0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t k = c.in.blob[b0 + i].kind;
    if (k == CRR_STATE_EXECUTION) {
      crr_reset_point_row* rp = reinterpret_cast<crr_reset_point_row*>(c.rows(6)) + o6;
      if (A.rp_len) {
        Rd v = {c.in.bytes, A.rp_off, A.rp_off + A.rp_len, false};
        walk_reset_points(v, stk, [&](int32_t j, uint64_t off, uint32_t len, bool resettable) {
          crr_reset_point_row row = {(int32_t)i, j, intern(off, len), CRR_ROW_LIVE | (resettable ? CRR_ROW_RESETTABLE : 0u)};
          rp[j] = row;
        });
      }
      Rd v = {c.in.bytes, A.vh_off, A.vh_off + A.vh_len, false};
      VhWalk V;
      walk_vh(v, A.current, reinterpret_cast<crr_vh_item*>(c.rows(5)) + o5, V, stk);
      uint8_t* tok = c.tokens() + o7;
      for (uint32_t q = 0; q < V.tok_len; ++q) tok[q] = c.in.bytes[V.tok_off + q];
      continue;
    }
    const Rec& rc = recs[i];
    int64_t rank = 0;   // rows ascending by ID: the order the checksum and the replay's finalize use
    const int64_t my_id = rc.id;
    for (uint32_t j = 0; j < n; ++j)
      rank += (c.in.blob[b0 + j].kind == k && recs[j].id < my_id) ? 1 : 0;
    // the row image goes to its slot as parsed; the fields this pass owns are then set in place
    if (k == CRR_STATE_ACTIVITY) {
      crr_activity_row& row = reinterpret_cast<crr_activity_row*>(c.rows(0))[o0 + rank];
      row = rc.row.act;
      row.key = intern(rc.str_off, rc.str_len);
      row.sched_src = (int32_t)i;
      row.started_src = rc.row.act.started_id == CRR_EMPTY_EVENT_ID ? -1 : (int32_t)i;
    } else if (k == CRR_STATE_TIMER) {
      crr_timer_row& row = reinterpret_cast<crr_timer_row*>(c.rows(1))[o1 + rank];
      row = rc.row.timer;
      row.key = intern(rc.str_off, rc.str_len);
      row.src = (int32_t)i;
    } else if (k == CRR_STATE_CHILD) {
      crr_child_row& row = reinterpret_cast<crr_child_row*>(c.rows(2))[o2 + rank];
      row = rc.row.child;
      row.src = (int32_t)i;
      row.started_src = rc.row.child.started_id == CRR_EMPTY_EVENT_ID ? -1 : (int32_t)i;
    } else {
      crr_initiated_row& row = k == CRR_STATE_REQUEST_CANCEL ? reinterpret_cast<crr_initiated_row*>(c.rows(3))[o3 + rank]
                                                             : reinterpret_cast<crr_initiated_row*>(c.rows(4))[o4 + rank];
      row = rc.row.init;
      row.src = (int32_t)i;
    }
  }
  // Load maps every activity by its ActivityID, a later ScheduleID overwriting an earlier one
  // (mutable_state_builder.go:311-314; Go ranges over a map there: the header's rule for
  // CRR_WF_FLAG_RESUME fixes the order -- the greatest ScheduleID wins)
  crr_activity_row* act = reinterpret_cast<crr_activity_row*>(c.rows(0)) + o0;
  const int64_t na = c.cnt(0)[w + 1] - o0;
  for (int64_t i = 0; i < na; ++i) {
    bool mapped = true;
    const uint32_t key = act[i].key;
    for (int64_t j = i + 1; j < na; ++j)
      if (act[j].key == key) {
        mapped = false;
        break;
      }
    if (mapped) act[i].flags |= CRR_ROW_MAPPED;
  }
  c.cnt(CRR_LOAD_T_KEYS)[w] = intern.n;
  c.cnt(CRR_LOAD_T_KEY_BYTES)[w] = (int64_t)intern.bytes;
}

CRR_HD void dict_wf(const Ctx& c, uint32_t w) {
  const int64_t k0 = c.cnt(CRR_LOAD_T_KEYS)[w], k1 = c.cnt(CRR_LOAD_T_KEYS)[w + 1];
  uint64_t run = (uint64_t)c.cnt(CRR_LOAD_T_KEY_BYTES)[w];
  const uint64_t base = (uint64_t)c.cnt(kCand)[w];
  for (int64_t k = 0; k < k1 - k0; ++k) {
    const uint32_t len = c.cand_len()[base + k];
    const uint8_t* s = c.str(c.cand_off()[base + k]);
    c.key_off()[k0 + k] = run;
    c.key_len()[k0 + k] = len;
    uint8_t* d = c.key_bytes() + run;
    for (uint32_t q = 0; q < len; ++q) d[q] = s[q];
    run += len;
  }
}

// ---- per workflow: the checksum Load verifies (cadence_load_verify.h) --------------------------------------
// CRC32-IEEE (hash/crc32.ChecksumIEEE, common/checksum/crc.go:46), slicing-by-8: the streaming writer of
// replay_kernel.hip's payload_crc restated for both builds.  The tables are 8 x 256 words: in LDS on the
// device (build_crc_tables in load_kernel.hip), a constant on the host (make_crc_tab).
struct CrcTab {
  uint32_t v[8 * 256];
};
constexpr CrcTab make_crc_tab() {
  CrcTab T{};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    T.v[i] = c;
  }
  for (int t = 1; t < 8; ++t)
    for (int i = 0; i < 256; ++i) {
      const uint32_t p = T.v[(t - 1) * 256 + i];
      T.v[t * 256 + i] = (p >> 8) ^ T.v[p & 0xff];
    }
  return T;
}

struct Crc {
  const uint32_t* T;
  uint32_t crc;
  uint64_t buf;   // the bytes not yet folded in, in arrival order from the low byte
  int nbuf;
  uint32_t len;

  CRR_HD void init(const uint32_t* tables) {
    T = tables;
    crc = 0xFFFFFFFFu;
    buf = 0;
    nbuf = 0;
    len = 0;
  }
  CRR_HD void block8(uint64_t b) {
    const uint32_t lo = (uint32_t)b ^ crc, hi = (uint32_t)(b >> 32);
    crc = T[7 * 256 + (lo & 0xff)] ^ T[6 * 256 + ((lo >> 8) & 0xff)] ^ T[5 * 256 + ((lo >> 16) & 0xff)] ^
          T[4 * 256 + (lo >> 24)] ^ T[3 * 256 + (hi & 0xff)] ^ T[2 * 256 + ((hi >> 8) & 0xff)] ^
          T[1 * 256 + ((hi >> 16) & 0xff)] ^ T[0 * 256 + (hi >> 24)];
  }
  // k (1..8) bytes held in arrival order in the low bytes of d
  CRR_HD void push(uint64_t d, int k) {
    len += (uint32_t)k;
    if (k < 8) d &= (1ull << (8 * k)) - 1ull;
    if (nbuf + k < 8) {
      buf |= d << (8 * nbuf);
      nbuf += k;
      return;
    }
    const int take = 8 - nbuf;
    block8(nbuf ? (buf | (d << (8 * nbuf))) : d);
    const int rem = k - take;
    buf = rem ? (d >> (8 * take)) : 0ull;
    nbuf = rem;
  }
  CRR_HD void u8(uint32_t b) { push(b & 0xff, 1); }
  CRR_HD void be16(uint32_t v) { push(((v >> 8) & 0xff) | ((v & 0xff) << 8), 2); }
  CRR_HD void be32(uint32_t v) { push(__builtin_bswap32(v), 4); }
  CRR_HD void be64(int64_t v) { push(__builtin_bswap64((uint64_t)v), 8); }
  // thrift binary field header: type byte + big-endian i16 id
  CRR_HD void field(uint32_t type, uint32_t id) { push(type | (((id >> 8) & 0xff) << 8) | ((id & 0xff) << 16), 3); }
  CRR_HD void list_header(uint32_t id, uint32_t elem, uint32_t n) {
    field(T_LIST, id);
    push(elem | ((uint64_t)__builtin_bswap32(n) << 8), 5);
  }
  // a binary value: its length, then its bytes (eight at a time while eight are left: no read past p + n)
  CRR_HD void binary(const uint8_t* p, uint32_t n) {
    be32(n);
    uint32_t i = 0;
    for (; i + 8 <= n; i += 8) {
      uint64_t d;
      memcpy(&d, p + i, 8);
      push(d, 8);
    }
    for (; i < n; ++i) u8(p[i]);
  }
  CRR_HD uint32_t finish() {
    for (int i = 0; i < nbuf; ++i) crc = T[(crc ^ (uint32_t)(buf >> (8 * i))) & 0xff] ^ (crc >> 8);
    nbuf = 0;
    return ~crc;
  }
};

// generateMutableStateChecksum (execution/checksum.go:36-114) for a workflow that loaded OK: 0x59 +
// MutableStateChecksumPayload.Encode (.gen/go/checksum/checksum.go:539-821), fields and order as payload_crc
// writes them, from the sources cadence_load_verify.h lists; then Load's decision
// (mutable_state_builder.go:334-348).  `stored`: NULL: compute only.  Every offset used here was checked
// against its blob's end when count_wf parsed the execution blob of the same `in`; a workflow whose recorded
// ranges do not lie within this batch's bytes (not the planned batch) is reported as not loaded.
CRR_HD void verify_wf(const Ctx& c, uint32_t w, const uint32_t* tables, const crr_stored_checksum* stored,
                      int64_t invalidate_before_ns, crr_verify_row* result, Frame* stk) {
  crr_verify_row out = {0, CRR_VERIFY_NOT_LOADED, 0, 0};
  if (c.status()[w] != CRR_LOAD_OK) {   // (a batch without blobs, whose blob_off may be NULL, has only such workflows)
    result[w] = out;
    return;
  }
  const ExecAux A = c.aux()[w];
  const uint64_t total = c.in.blob_off[c.in.n_blobs];
  if (A.vh_off > total || A.vh_len > total - A.vh_off || A.sticky_off > total || A.sticky_len > total - A.sticky_off) {
    result[w] = out;
    return;
  }
  const crr_exec_row R = c.exec()[w];
  Crc K;
  K.init(tables);
  K.u8(0x59);                                                                   // preambleVersion0
  K.field(T_BOOL, 10); K.u8((R.flags & CRR_EXEC_CANCEL_REQUESTED) ? 1 : 0);     // CancelRequested
  K.field(T_I16, 15); K.be16((uint32_t)(uint16_t)(int16_t)R.state);             // State
  K.field(T_I64, 23); K.be64(R.last_first_event_id);
  K.field(T_I64, 24); K.be64(R.next_event_id);
  K.field(T_I64, 25); K.be64(R.last_processed_event);
  K.field(T_I64, 26); K.be64((int64_t)R.signal_count);
  K.field(T_I32, 35); K.be32((uint32_t)(int32_t)R.decision_attempt);
  K.field(T_I64, 36); K.be64(R.decision_version);
  K.field(T_I64, 37); K.be64(R.decision_schedule_id);
  K.field(T_I64, 38); K.be64(R.decision_started_id);
  // the pending-ID lists: each dense table's rows are ascending by ID (emit_wf), the ID a row's first field
  auto ids = [&](uint32_t field_id, int t) {
    const int64_t o = c.cnt(t)[w], n = c.cnt(t)[w + 1] - o;
    K.list_header(field_id, T_I64, (uint32_t)n);
    const uint8_t* row = c.rows(t) + (uint64_t)o * kRowBytes[t];
    for (int64_t j = 0; j < n; ++j) K.be64(*reinterpret_cast<const int64_t*>(row + (uint64_t)j * kRowBytes[t]));
  };
  ids(45, 1);   // PendingTimerStartedIDs
  ids(46, 0);   // PendingActivityScheduledIDs
  ids(47, 4);   // PendingSignalInitiatedIDs
  ids(48, 3);   // PendingReqCancelInitiatedIDs
  ids(49, 2);   // PendingChildInitiatedIDs
  K.field(T_STRING, 55); K.binary(c.in.bytes + A.sticky_off, A.sticky_len);      // StickyTaskListName
  K.field(T_STRUCT, 56);                                                        // VersionHistories
  K.field(T_I32, 10); K.be32((uint32_t)A.current);                              //   CurrentVersionHistoryIndex
  K.list_header(20, T_STRUCT, (uint32_t)A.n_hist);                              //   Histories
  const Rd v = {c.in.bytes, A.vh_off, A.vh_off + A.vh_len, false};
  VhWalk V;
  const bool ok = walk_vh(v, -1, nullptr, V, stk, [&](uint64_t tok_off, uint32_t tok_len, uint64_t items_pos, int32_t n_items) {
    K.field(T_STRING, 10); K.binary(c.in.bytes + tok_off, tok_len);             //   VersionHistory.BranchToken
    K.list_header(20, T_STRUCT, (uint32_t)n_items);                             //   VersionHistory.Items
    Rd it = {v.p, items_pos, v.end, false};
    for (int32_t k = 0; k < n_items; ++k) {
      const crr_vh_item x = read_vh_item(it, stk);
      K.field(T_I64, 10); K.be64(x.event_id);
      K.field(T_I64, 20); K.be64(x.version);
      K.u8(0);
    }
    K.u8(0);   // VersionHistory stop
  });
  if (!ok || V.n_hist != A.n_hist) {   // not the bytes the plan walked
    result[w] = out;
    return;
  }
  K.u8(0);   // VersionHistories stop
  K.u8(0);   // payload stop
  out.payload_len = K.len;
  out.computed = K.finish();
  out.outcome = CRR_VERIFY_NONE;
  if (stored) {
    const crr_stored_checksum S = stored[w];
    if (S.value_len == 0) out.outcome = CRR_VERIFY_NONE;
    else if (invalidate_before_ns > 0 && A.last_updated < invalidate_before_ns) out.outcome = CRR_VERIFY_INVALIDATED;
    else if (S.version != CRR_CHECKSUM_PAYLOAD_V1) out.outcome = CRR_VERIFY_BAD_VERSION;
    else if (S.flavor != CRR_CHECKSUM_FLAVOR_CRC32) out.outcome = CRR_VERIFY_BAD_FLAVOR;
    else out.outcome = (S.value_len == 4 && S.value == out.computed) ? CRR_VERIFY_MATCH : CRR_VERIFY_MISMATCH;
  }
  result[w] = out;
}

// ---- per workflow: every branch of the VersionHistories blob (cadence_load_ndc.h) --------------------------
// the walk's own work buffer: per-workflow counters [3][n_wf + 1] (histories and items scanned in place to
// exclusive offsets, the longest branch as counted), the tasks' new-branch prefix [n_tasks + 1], the
// crr_ndc_task rows built for crr_ndc_prepare, and the totals the planning call reads back
constexpr int kBrHist = 0, kBrItems = 1, kBrLongest = 2, kBrCounters = 3;
struct NdcLayout {
  uint64_t cnt, out_off, rows, totals, end;
};
inline NdcLayout carve_ndc(uint32_t n_wf, uint32_t n_tasks) {
  NdcLayout L;
  uint64_t o = 0;
  L.cnt = o;      o = align16(o + (uint64_t)kBrCounters * ((uint64_t)n_wf + 1) * sizeof(int64_t));
  L.out_off = o;  o = align16(o + ((uint64_t)n_tasks + 1) * sizeof(int64_t));
  L.rows = o;     o = align16(o + (uint64_t)n_tasks * sizeof(crr_ndc_task));
  L.totals = o;   o = align16(o + 4 * sizeof(uint64_t));
  L.end = o;
  return L;
}
struct NdcWork {
  uint8_t* s;
  NdcLayout L;
  uint32_t n_wf, n_tasks;
  CRR_HD int64_t* cnt(int t) const { return reinterpret_cast<int64_t*>(s + L.cnt) + (uint64_t)t * ((uint64_t)n_wf + 1); }
  CRR_HD int64_t* out_off() const { return reinterpret_cast<int64_t*>(s + L.out_off); }
  CRR_HD crr_ndc_task* rows() const { return reinterpret_cast<crr_ndc_task*>(s + L.rows); }
  CRR_HD uint64_t* totals() const { return reinterpret_cast<uint64_t*>(s + L.totals); }   // branches, items, out items
};

// Every offset used by the two branch passes was checked against its blob's end when count_wf parsed the
// execution blob of the same `in` and walked this nested blob (so walk_vh cannot fail here on the planned
// batch); a workflow whose recorded range does not lie within this batch's bytes, or whose walk does not give
// the histories the plan counted (not the planned batch), has no branches, like one that did not load.
CRR_HD bool branches_range_ok(const Ctx& c, const ExecAux& A) {
  if (c.in.n_blobs == 0) return false;
  const uint64_t total = c.in.blob_off[c.in.n_blobs];
  return A.vh_len != 0 && A.vh_off <= total && A.vh_len <= total - A.vh_off;
}

// count phase: histories, items over all histories, the longest branch
CRR_HD void branches_count_wf(const Ctx& c, const NdcWork& k, uint32_t w, Frame* stk) {
  int64_t n_hist = 0, n_items = 0, longest = 0;
  if (c.status()[w] == CRR_LOAD_OK) {
    const ExecAux A = c.aux()[w];
    if (branches_range_ok(c, A)) {
      const Rd v = {c.in.bytes, A.vh_off, A.vh_off + A.vh_len, false};
      VhWalk V;
      const bool ok = walk_vh(v, -1, nullptr, V, stk, [&](uint64_t, uint32_t, uint64_t, int32_t m) {
        ++n_hist;
        n_items += m;
        if (m > longest) longest = m;
      });
      if (!ok || V.n_hist != A.n_hist) n_hist = n_items = longest = 0;
    }
  }
  k.cnt(kBrHist)[w] = n_hist;
  k.cnt(kBrItems)[w] = n_items;
  k.cnt(kBrLongest)[w] = longest;
}

// emit phase (after the scan of the first two counters): the branch descriptors, the tokens' positions, every
// item, the stored current index.  Nothing is written past what the count phase counted for this workflow.
CRR_HD void branches_emit_wf(const Ctx& c, const NdcWork& k, uint32_t w, const crr_load_branches& dst, Frame* stk) {
  const int64_t b0 = k.cnt(kBrHist)[w], nb = k.cnt(kBrHist)[w + 1] - b0;
  const int64_t i0 = k.cnt(kBrItems)[w], ni = k.cnt(kBrItems)[w + 1] - i0;
  if (dst.branch_begin) {
    dst.branch_begin[w] = b0;
    if (w + 1 == c.in.n_wf) dst.branch_begin[w + 1] = b0 + nb;
  }
  if (nb == 0) {
    if (dst.current) dst.current[w] = 0;
    return;
  }
  const ExecAux A = c.aux()[w];
  if (dst.current) dst.current[w] = A.current;
  const Rd v = {c.in.bytes, A.vh_off, A.vh_off + A.vh_len, false};
  VhWalk V;
  int64_t h = 0, run = 0;
  walk_vh(v, -1, nullptr, V, stk, [&](uint64_t tok_off, uint32_t tok_len, uint64_t items_pos, int32_t m) {
    if (h >= nb || run + m > ni) {   // not the bytes the plan counted
      h = nb;
      return;
    }
    if (dst.branches) {
      const crr_ndc_branch br = {(uint32_t)(i0 + run), (uint32_t)m};
      dst.branches[b0 + h] = br;
    }
    if (dst.tokens) {
      const crr_branch_token tk = {tok_len ? tok_off : 0, tok_len, w};
      dst.tokens[b0 + h] = tk;
    }
    if (dst.items) {
      Rd it = {v.p, items_pos, v.end, false};
      for (int32_t q = 0; q < m; ++q) dst.items[i0 + run + q] = read_vh_item(it, stk);
    }
    run += m;
    ++h;
  });
}

// the new-branch room of task k: the longest local branch of its workflow (0: not decided)
CRR_HD int64_t task_room(const NdcWork& k, const crr_repl_task& t) {
  return t.wf < k.n_wf ? k.cnt(kBrLongest)[t.wf] : 0;
}

// whether task `t` is decided, and if not the status it carries
CRR_HD int32_t task_refusal(const NdcWork& k, const crr_repl_task& t, uint32_t n_incoming) {
  if (t.wf >= k.n_wf || k.cnt(kBrHist)[t.wf + 1] == k.cnt(kBrHist)[t.wf]) return CRR_ERR_NDC_STATE_NOT_LOADED;
  if (t.incoming_begin > n_incoming || t.incoming_count > n_incoming - t.incoming_begin) return CRR_ERR_NDC_BAD_INDEX;
  return CRR_OK;
}

// the crr_ndc_task row of task `t` (after both scans): the workflow's branches and stored current index, the
// incoming items where the run call copies them (behind the n_items local ones), its room in out_items
CRR_HD crr_ndc_task task_row(const NdcWork& k, const crr_repl_task& t, uint32_t idx, uint32_t n_incoming,
                             uint64_t n_items, const int32_t* current) {
  crr_ndc_task r;
  memset(&r, 0, sizeof r);
  r.out_begin = (uint32_t)k.out_off()[idx];
  r.first_event_id = t.first_event_id;
  r.first_event_version = t.first_event_version;
  if (task_refusal(k, t, n_incoming) != CRR_OK) return r;   // no branches: crr_ndc_prepare reads nothing for it
  r.branch_begin = (uint32_t)k.cnt(kBrHist)[t.wf];
  r.branch_count = (uint32_t)(k.cnt(kBrHist)[t.wf + 1] - k.cnt(kBrHist)[t.wf]);
  r.current_index = current[t.wf];
  r.incoming_begin = (uint32_t)(n_items + t.incoming_begin);
  r.incoming_count = t.incoming_count;
  return r;
}

// conflictResolverImpl.prepareMutableState (ndc/conflict_resolver.go:75-120) for task `idx`, over the histories
// as prepareVersionHistory left them: `res` is crr_ndc_prepare's row (rewritten here for a task that was not
// decided), `row` the task's crr_ndc_task
CRR_HD void route_task(const NdcWork& k, const crr_repl_task& t, uint32_t idx, uint32_t n_incoming,
                       const crr_ndc_branch* branches, const crr_vh_item* items, const crr_vh_item* out_items,
                       crr_ndc_result* results, crr_ndc_route* routes) {
  crr_ndc_route o;
  memset(&o, 0, sizeof o);
  o.route = CRR_ROUTE_NONE;
  const int32_t refusal = task_refusal(k, t, n_incoming);
  if (refusal != CRR_OK) {
    crr_ndc_result z;
    memset(&z, 0, sizeof z);
    z.status = refusal;
    z.action = CRR_NDC_DUPLICATE;
    results[idx] = z;
    o.status = refusal;
    routes[idx] = o;
    return;
  }
  const crr_ndc_result r = results[idx];
  const crr_ndc_task row = k.rows()[idx];
  o.status = r.status;
  if (r.status != CRR_OK || r.action == CRR_NDC_DUPLICATE) {
    routes[idx] = o;
    return;
  }
  if (r.branch_index == r.new_current_index) {   // :88-90
    o.route = CRR_ROUTE_APPLY_CURRENT;
    routes[idx] = o;
    return;
  }
  // a branch's last item (GetLastItem): local branches from the table, the new one from the task's out_items run
  auto last_item = [&](int32_t b, crr_vh_item& it) {
    if (b >= 0 && (uint32_t)b < row.branch_count) {
      const crr_ndc_branch br = branches[row.branch_begin + (uint32_t)b];
      if (br.item_count == 0) return false;
      it = items[br.item_begin + br.item_count - 1];
      return true;
    }
    if (b != (int32_t)row.branch_count || r.action != CRR_NDC_NEW_BRANCH || r.new_item_count <= 0) return false;
    it = out_items[row.out_begin + (uint32_t)r.new_item_count - 1];
    return true;
  };
  crr_vh_item cur_last = {0, 0};
  if (!last_item(r.new_current_index, cur_last)) {   // :92-99
    o.status = CRR_ERR_VH_EMPTY;
    routes[idx] = o;
    return;
  }
  const int64_t version = t.first_event_version;
  if (version < cur_last.version) {
    o.route = CRR_ROUTE_NON_CURRENT;                 // :102-104
  } else if (version == cur_last.version) {
    o.route = CRR_ROUTE_BAD_REQUEST;                 // :106-110
  } else {                                           // :112-119 -> rebuild (:122-158)
    crr_vh_item last = {0, 0};
    if (!last_item(r.branch_index, last)) {
      o.status = CRR_ERR_VH_EMPTY;
    } else {
      o.route = CRR_ROUTE_REBUILD;
      o.branch = r.branch_index;
      o.branch_is_local = (uint32_t)r.branch_index < row.branch_count ? 1 : 0;
      o.last_event_id = last.event_id;
      o.last_version = last.version;
    }
  }
  routes[idx] = o;
}

// ---- per task: the checksum to store once the routed task is committed (cadence_load_store.h) ---------------
// The payload writer of generateMutableStateChecksum, written once behind a state view: the exec row, the ID of
// live row j of pending map t, version-history item j of the current branch.  Every source of a state is this
// one view -- the loader's scratch, a dense image, the slot tables a resumed replay wrote -- as a row pointer
// and a stride per table (each table by name: with the constant table indices of the writer everything stays
// in registers).  The counts are the caller's, already bounded by what the tables hold.
struct StateView {
  crr_exec_row R;
  const uint8_t *act, *timer, *child, *rc, *sig;   // live row 0 of each pending map
  const crr_vh_item* vh;                           // item 0 of the current branch
  uint32_t n_act, n_timer, n_child, n_rc, n_sig, n_vh;
  uint64_t stride;                                 // rows between two live rows
  // what only the mutation reads (cadence_load_mutation.h): the reset points, and where the exec row lies in its
  // table (the device position, or the workflow for a dense image)
  const uint8_t* rp;
  uint32_t n_rp;
  uint64_t exec_slot;

  CRR_HD uint32_t count(int t) const { return t == 0 ? n_act : t == 1 ? n_timer : t == 2 ? n_child : t == 3 ? n_rc : n_sig; }
  CRR_HD const uint8_t* rows_of(int t) const { return t == 0 ? act : t == 1 ? timer : t == 2 ? child : t == 3 ? rc : sig; }
  CRR_HD int64_t id(int t, uint32_t j) const {     // the ID a row's first field
    const uint8_t* p = rows_of(t);
    int64_t v;
    memcpy(&v, p + (uint64_t)j * stride * kRowBytes[t], sizeof v);
    return v;
  }
  CRR_HD crr_vh_item item(uint32_t j) const { return vh[(uint64_t)j * stride]; }
};

// a count read from an exec row, bounded by the rows its table holds (none without a table)
CRR_HD uint32_t bounded_count(int32_t n, int64_t room, const void* table) {
  if (!table || n <= 0 || room <= 0) return 0;
  return (uint32_t)((int64_t)n < room ? (int64_t)n : room);
}

// the state of workflow w as loaded: the fields verify_wf reads
CRR_HD StateView scratch_view(const Ctx& c, uint32_t w) {
  StateView S;
  S.R = c.exec()[w];
  auto row0 = [&](int t) { return c.rows(t) + (uint64_t)c.cnt(t)[w] * kRowBytes[t]; };
  auto n = [&](int t) { return (uint32_t)(c.cnt(t)[w + 1] - c.cnt(t)[w]); };
  S.act = row0(0), S.timer = row0(1), S.child = row0(2), S.rc = row0(3), S.sig = row0(4);
  S.vh = reinterpret_cast<const crr_vh_item*>(row0(5));
  S.n_act = n(0), S.n_timer = n(1), S.n_child = n(2), S.n_rc = n(3), S.n_sig = n(4), S.n_vh = n(5);
  S.rp = row0(6), S.n_rp = n(6), S.exec_slot = w;
  S.stride = 1;
  return S;
}

// 0x59 + MutableStateChecksumPayload.Encode up to the histories' list header (fields and order as verify_wf
// writes them); the caller writes the n_hist branches, then payload_tail
CRR_HD void payload_head(Crc& K, const StateView& S, const uint8_t* sticky, uint32_t sticky_len, int32_t current,
                         uint32_t n_hist) {
  const crr_exec_row& R = S.R;
  K.u8(0x59);                                                                   // preambleVersion0
  K.field(T_BOOL, 10); K.u8((R.flags & CRR_EXEC_CANCEL_REQUESTED) ? 1 : 0);     // CancelRequested
  K.field(T_I16, 15); K.be16((uint32_t)(uint16_t)(int16_t)R.state);             // State
  K.field(T_I64, 23); K.be64(R.last_first_event_id);
  K.field(T_I64, 24); K.be64(R.next_event_id);
  K.field(T_I64, 25); K.be64(R.last_processed_event);
  K.field(T_I64, 26); K.be64((int64_t)R.signal_count);
  K.field(T_I32, 35); K.be32((uint32_t)(int32_t)R.decision_attempt);
  K.field(T_I64, 36); K.be64(R.decision_version);
  K.field(T_I64, 37); K.be64(R.decision_schedule_id);
  K.field(T_I64, 38); K.be64(R.decision_started_id);
  auto ids = [&](uint32_t field_id, int t) {
    const uint32_t n = S.count(t);
    K.list_header(field_id, T_I64, n);
    for (uint32_t j = 0; j < n; ++j) K.be64(S.id(t, j));
  };
  ids(45, 1);   // PendingTimerStartedIDs
  ids(46, 0);   // PendingActivityScheduledIDs
  ids(47, 4);   // PendingSignalInitiatedIDs
  ids(48, 3);   // PendingReqCancelInitiatedIDs
  ids(49, 2);   // PendingChildInitiatedIDs
  K.field(T_STRING, 55); K.binary(sticky, sticky_len);                          // StickyTaskListName
  K.field(T_STRUCT, 56);                                                        // VersionHistories
  K.field(T_I32, 10); K.be32((uint32_t)current);                                //   CurrentVersionHistoryIndex
  K.list_header(20, T_STRUCT, n_hist);                                          //   Histories
}
// the three writers of a VersionHistory are templates on the sink: the CRC here, a byte sink for the blob to store
// (cadence_load_store_vh.h)
template <class Sink>
CRR_HD void payload_branch(Sink& K, const uint8_t* token, uint32_t token_len, uint32_t n_items) {
  K.field(T_STRING, 10); K.binary(token, token_len);                            //   VersionHistory.BranchToken
  K.list_header(20, T_STRUCT, n_items);                                         //   VersionHistory.Items
}
template <class Sink>
CRR_HD void payload_item(Sink& K, int64_t event_id, int64_t version) {
  K.field(T_I64, 10); K.be64(event_id);
  K.field(T_I64, 20); K.be64(version);
  K.u8(0);
}
template <class Sink>
CRR_HD void payload_branch_end(Sink& K) { K.u8(0); }
CRR_HD void payload_tail(Crc& K) {
  K.u8(0);   // VersionHistories stop
  K.u8(0);   // payload stop
}

// what a call reads beside the loader's context: the tasks with their decisions and the resident branch table
struct StoreIn {
  const crr_repl_task* tasks;
  const crr_last_event* last;
  const crr_ndc_result* results;
  const crr_ndc_route* routes;
  crr_load_branches br;
  uint64_t n_branches, n_items;   // the table's sizes: every index read from it is checked against them
  uint32_t n_tasks;
};

// the post-replay state of a workflow in the slot tables of the resumed batch (crr_outputs), addressed as
// load_place_kernel addresses them; have == false: no replay was run
struct ReplayAfter {
  const crr_workflow* wf;
  const uint32_t* position;
  crr_outputs out;
  uint32_t n_pos, stride, wave_begin;
  bool have;
  CRR_HD bool view(uint32_t w, StateView& S) const {
    if (!have) return false;
    const uint32_t p = position ? position[w] : w;
    if (p >= n_pos) return false;
    const crr_workflow& D = wf[p];
    if (!(D.flags & CRR_WF_FLAG_RESUME)) return false;
    S.R = out.exec[p];
    S.stride = p >= wave_begin ? 1 : stride;
    auto row0 = [&](const void* table, int64_t base, int t) {
      return static_cast<const uint8_t*>(table) + (uint64_t)base * kRowBytes[t];
    };
    S.act = row0(out.act, D.act_base, 0), S.timer = row0(out.timer, D.timer_base, 1), S.child = row0(out.child, D.child_base, 2);
    S.rc = row0(out.rc, D.rc_base, 3), S.sig = row0(out.sig, D.sig_base, 4);
    S.vh = reinterpret_cast<const crr_vh_item*>(row0(out.vh, D.vh_base, 5));
    // a garbage row cannot send the lane out of its tables: every count is bounded by the descriptor's capacity
    S.n_act = bounded_count(S.R.n_activity, D.act_cap, out.act), S.n_timer = bounded_count(S.R.n_timer, D.timer_cap, out.timer);
    S.n_child = bounded_count(S.R.n_child, D.child_cap, out.child), S.n_rc = bounded_count(S.R.n_rc, D.rc_cap, out.rc);
    S.n_sig = bounded_count(S.R.n_signal, D.sig_cap, out.sig), S.n_vh = bounded_count(S.R.n_vh_items, D.vh_cap, out.vh);
    S.rp = row0(out.rp, D.rp_base, 6), S.n_rp = bounded_count(S.R.n_reset_points, D.rp_cap, out.rp), S.exec_slot = p;
    return true;
  }
};

// the same from a dense image indexed by workflow (the host restatement); I == NULL: no replay was run
struct ImageAfter {
  const crr_load_image* I;
  uint32_t n_wf;
  CRR_HD bool view(uint32_t w, StateView& S) const {
    if (!I || !I->exec || !I->offsets || (I->status && I->status[w] != 0)) return false;
    S.R = I->exec[w];
    S.stride = 1;
    auto off = [&](int t) { return I->offsets[(uint64_t)t * ((uint64_t)n_wf + 1) + w]; };
    auto row0 = [&](int t) { return I->rows[t] ? static_cast<const uint8_t*>(I->rows[t]) + (uint64_t)off(t) * kRowBytes[t] : nullptr; };
    auto n = [&](int t, int32_t field) {
      const int64_t o = off(t), e = I->offsets[(uint64_t)t * ((uint64_t)n_wf + 1) + w + 1];
      return o < 0 ? 0u : bounded_count(field, e - o, I->rows[t]);
    };
    S.act = row0(0), S.timer = row0(1), S.child = row0(2), S.rc = row0(3), S.sig = row0(4);
    S.vh = reinterpret_cast<const crr_vh_item*>(row0(5));
    S.n_act = n(0, S.R.n_activity), S.n_timer = n(1, S.R.n_timer), S.n_child = n(2, S.R.n_child), S.n_rc = n(3, S.R.n_rc);
    S.n_sig = n(4, S.R.n_signal), S.n_vh = n(5, S.R.n_vh_items);
    S.rp = row0(6), S.n_rp = n(6, S.R.n_reset_points), S.exec_slot = w;
    return true;
  }
};

// What CloseTransactionAsMutation commits for task `idx` on its route (mutable_state_builder.go:3959-3996), decided
// once for everything that is generated from it -- the checksum (store_task) and the VersionHistories blob
// (cadence_load_store_vh.h): the outcome with cadence_load_store.h's precedence, its status, and for a generated
// task the view its scalars and current branch come from and what AddOrUpdateItem does to the target branch.
struct StoreDecision {
  int32_t outcome, status;
  bool apply;                 // the current route: the state as the resumed replay left it (S)
  int mode;                   // the target branch: 0 as it is, 1 the last item's event ID updated, 2 one item appended
  uint32_t w;
  int32_t current;
  int64_t b0, nb, target;     // the workflow's branches in the table, the task's among them
  uint64_t total;             // the batch's bytes
  uint64_t sticky_off;
  uint32_t sticky_len;
  crr_last_event e;
  StateView S;
  CRR_HD bool generated() const { return outcome == CRR_STORE_APPLIED || outcome == CRR_STORE_BACKFILLED; }
};

// a branch of the table, its ranges checked against the table's sizes and the batch's bytes
CRR_HD bool table_branch(const StoreIn& a, int64_t b, uint64_t total, crr_ndc_branch& br, crr_branch_token& tk) {
  br = a.br.branches[b];
  tk = a.br.tokens[b];
  return (uint64_t)br.item_begin + br.item_count <= a.n_items && tk.off <= total && tk.len <= total - tk.off;
}

// A table that is not this batch's (ranges outside the sizes given) reads as not loaded.
template <class After>
CRR_HD void store_decide(const Ctx& c, const StoreIn& a, const After& after, uint32_t idx, StoreDecision& D) {
  auto done = [&](int32_t outcome, int32_t status) {
    D.outcome = outcome;
    D.status = status;
  };
  const crr_repl_task t = a.tasks[idx];
  if (t.wf >= c.in.n_wf || c.status()[t.wf] != CRR_LOAD_OK) return done(CRR_STORE_NOT_LOADED, 0);
  const uint32_t w = t.wf;
  const ExecAux A = c.aux()[w];
  const uint64_t total = c.in.blob_off[c.in.n_blobs];
  const int64_t b0 = a.br.branch_begin[w], nb = a.br.branch_begin[w + 1] - b0;
  const int32_t current = a.br.current[w];
  if (b0 < 0 || nb <= 0 || (uint64_t)b0 + (uint64_t)nb > a.n_branches || nb != (int64_t)A.n_hist || current < 0 ||
      current >= nb || A.sticky_off > total || A.sticky_len > total - A.sticky_off)
    return done(CRR_STORE_NOT_LOADED, 0);
  D.w = w, D.current = current, D.b0 = b0, D.nb = nb, D.total = total;
  D.sticky_off = A.sticky_off, D.sticky_len = A.sticky_len;
  const crr_ndc_route rt = a.routes[idx];
  const crr_ndc_result r = a.results[idx];
  const bool apply = rt.route == CRR_ROUTE_APPLY_CURRENT;
  if ((!apply && rt.route != CRR_ROUTE_NON_CURRENT) || r.action == CRR_NDC_DUPLICATE) return done(CRR_STORE_NO_ROUTE, 0);
  if (apply) {
    if (!after.view(w, D.S)) return done(CRR_STORE_NOT_RESUMED, 0);
    if (D.S.R.status != CRR_OK) return done(CRR_STORE_REPLAY_FAILED, D.S.R.status);
  }
  if (r.action != CRR_NDC_APPEND) return done(CRR_STORE_NEW_BRANCH, 0);
  const crr_last_event e = a.last[idx];
  // NewVersionHistoryItem (versionHistory.go:37-43) comes before GetVersionHistory on the backfill's path
  if (!apply && (e.event_id < 0 || (e.version < 0 && e.version != CRR_EMPTY_VERSION)))
    return done(CRR_STORE_VH_ERROR, CRR_ERR_VH_INVALID_ITEM);
  if (r.branch_index < 0 || r.branch_index >= nb || (apply && r.branch_index != current))
    return done(CRR_STORE_VH_ERROR, CRR_ERR_NDC_BAD_INDEX);
  D.apply = apply, D.target = r.branch_index, D.e = e, D.mode = 0;
  if (!apply) {   // AddOrUpdateItem (versionHistory.go:193-226)
    crr_ndc_branch br;
    crr_branch_token tk;
    if (!table_branch(a, b0 + D.target, total, br, tk)) return done(CRR_STORE_NOT_LOADED, 0);
    D.mode = 2;
    if (br.item_count) {
      const crr_vh_item last = a.br.items[br.item_begin + br.item_count - 1];
      if (e.version < last.version) return done(CRR_STORE_VH_ERROR, CRR_ERR_VH_LOWER_VERSION);
      if (e.event_id <= last.event_id) return done(CRR_STORE_VH_ERROR, CRR_ERR_VH_EVENT_ID_NOT_INCREASING);
      D.mode = e.version > last.version ? 2 : 1;
    }
    D.S = scratch_view(c, w);
  }
  done(apply ? CRR_STORE_APPLIED : CRR_STORE_BACKFILLED, 0);
}

// branch h of a generated task as the commit writes it (the table of DESIGN.md §4, "The value to store"): the
// token always from the persisted bytes; on the current route the current branch's items the replay's vh rows,
// every other branch the table's, the backfill's target with AddOrUpdateItem(last event) applied
struct StoreBranch {
  crr_branch_token tk;
  const crr_vh_item* it;      // item 0 of the source
  uint64_t stride;            // rows between two items of the source
  uint32_t n_src;             // items the source holds
  uint32_t n;                 // items written: n_src, and one more when the last event is appended
  bool update_last;           // the last source item's event ID becomes the last event's
  CRR_HD crr_vh_item item(uint32_t j, const crr_last_event& e) const {
    if (j >= n_src) return crr_vh_item{e.event_id, e.version};
    crr_vh_item x = it[(uint64_t)j * stride];
    if (update_last && j + 1 == n_src) x.event_id = e.event_id;
    return x;
  }
};
CRR_HD bool store_branch(const StoreIn& a, const StoreDecision& D, int64_t h, StoreBranch& B) {
  crr_ndc_branch br;
  if (!table_branch(a, D.b0 + h, D.total, br, B.tk)) return false;
  if (D.apply && h == D.target) {   // the current branch as the replay left it
    B.it = D.S.vh, B.stride = D.S.stride, B.n_src = B.n = D.S.n_vh, B.update_last = false;
    return true;
  }
  const bool mine = !D.apply && h == D.target;
  B.it = a.br.items + br.item_begin, B.stride = 1, B.n_src = br.item_count;
  B.n = br.item_count + (mine && D.mode == 2 ? 1u : 0u);
  B.update_last = mine && D.mode == 1;
  return true;
}

// generateChecksum for task `idx` as CloseTransactionAsMutation reaches it on the task's route.  Nothing of the
// payload is stored.
template <class After>
CRR_HD void store_task(const Ctx& c, const StoreIn& a, const After& after, const uint32_t* tables, uint32_t idx,
                       crr_store_row* result) {
  crr_store_row o = {0, CRR_STORE_NOT_LOADED, 0, 0};
  StoreDecision D;
  store_decide(c, a, after, idx, D);
  o.outcome = D.outcome, o.status = D.status;
  if (!D.generated()) {
    result[idx] = o;
    return;
  }
  Crc K;
  K.init(tables);
  // ApplyEvents clears stickiness before its loop (state_builder.go:108); the backfill keeps the name as stored
  payload_head(K, D.S, c.in.bytes + (D.apply ? 0 : D.sticky_off), D.apply ? 0 : D.sticky_len, D.current, (uint32_t)D.nb);
  for (int64_t h = 0; h < D.nb; ++h) {
    StoreBranch B;
    if (!store_branch(a, D, h, B)) {
      o.outcome = CRR_STORE_NOT_LOADED;
      result[idx] = o;
      return;
    }
    payload_branch(K, c.in.bytes + B.tk.off, B.tk.len, B.n);
    for (uint32_t j = 0; j < B.n; ++j) {
      const crr_vh_item x = B.item(j, D.e);
      payload_item(K, x.event_id, x.version);
    }
    payload_branch_end(K);
  }
  payload_tail(K);
  o.payload_len = K.len;
  o.value = K.finish();
  result[idx] = o;
}

// ---- per task: the VersionHistories blob to store (cadence_load_store_vh.h) --------------------------------
// SerializeVersionHistories' thriftrw DataBlob (common/persistence/serializer.go:178-183): 0x59, then the struct
// payload_head .. payload_branch_end stream into the CRC inside field 56.  Go writes every field of the three
// structs, so every width is fixed: 16 bytes of head, per history 7 + token + 8 + 23 per item + 1, one stop byte.
constexpr uint64_t kVhHead = 16, kVhHistory = 16, kVhItem = 23;

// the blob's length for a generated task; false: a branch of the table is not this batch's (not loaded)
CRR_HD bool vh_blob_len(const StoreIn& a, const StoreDecision& D, uint64_t& len) {
  len = kVhHead + 1;
  for (int64_t h = 0; h < D.nb; ++h) {
    StoreBranch B;
    if (!store_branch(a, D, h, B)) return false;
    len += kVhHistory + B.tk.len + kVhItem * B.n;
  }
  return len <= 0xFFFFFFFFull;
}

// task idx's row and length: the decision of store_task, a branch that fails its check included
template <class After>
CRR_HD uint64_t vh_size_task(const Ctx& c, const StoreIn& a, const After& after, uint32_t idx, crr_vh_blob_row* rows) {
  StoreDecision D;
  store_decide(c, a, after, idx, D);
  crr_vh_blob_row o = {0, D.outcome, D.status, 0};
  uint64_t len = 0;
  if (D.generated()) {
    if (vh_blob_len(a, D, len)) o.len = (uint32_t)len;
    else o.outcome = CRR_STORE_NOT_LOADED, len = 0;
  }
  rows[idx] = o;
  return len;
}

// the plain sequential writer (the host restatement): bytes past `cap` are counted, not written
struct ByteSink {
  uint8_t* p;
  uint64_t cap, len;
  CRR_HD void u8(uint32_t b) {
    if (len < cap) p[len] = (uint8_t)b;
    ++len;
  }
  CRR_HD void be32(uint32_t v) {
    for (int i = 3; i >= 0; --i) u8(v >> (8 * i));
  }
  CRR_HD void be64(int64_t v) {
    for (int i = 7; i >= 0; --i) u8((uint32_t)((uint64_t)v >> (8 * i)));
  }
  CRR_HD void field(uint32_t type, uint32_t id) { u8(type), u8(id >> 8), u8(id); }
  CRR_HD void list_header(uint32_t id, uint32_t elem, uint32_t n) { field(T_LIST, id), u8(elem), be32(n); }
  CRR_HD void binary(const uint8_t* q, uint32_t n) {
    be32(n);
    for (uint32_t i = 0; i < n; ++i) u8(q[i]);
  }
};
template <class Sink>
CRR_HD bool vh_blob_write(Sink& K, const Ctx& c, const StoreIn& a, const StoreDecision& D) {
  K.u8(0x59);                                                                   // preambleVersion0
  K.field(T_I32, 10); K.be32((uint32_t)D.current);                              // CurrentVersionHistoryIndex
  K.list_header(20, T_STRUCT, (uint32_t)D.nb);                                  // Histories
  for (int64_t h = 0; h < D.nb; ++h) {
    StoreBranch B;
    if (!store_branch(a, D, h, B)) return false;
    payload_branch(K, c.in.bytes + B.tk.off, B.tk.len, B.n);
    for (uint32_t j = 0; j < B.n; ++j) {
      const crr_vh_item x = B.item(j, D.e);
      payload_item(K, x.event_id, x.version);
    }
    payload_branch_end(K);
  }
  K.u8(0);                                                                      // VersionHistories stop
  return true;
}

// The output-stationary form (load_store_vh_emit_kernel): bytes [16 * chunk, + 16) of the concatenated blobs as
// two little-endian words, whatever blobs they belong to.  The task that holds a byte is found by an upper-bound
// search over the plan's prefix (runs of zero-length tasks are stepped over), the history by walking the task's
// branches' lengths; inside a history the layout is closed-form.  A byte whose lookup fails -- a task the
// decision no longer generates, an offset past what its branches give now -- is zero; the lane reads blob_off
// within [0, n_tasks] only, and what it writes is the caller's 16 bytes.
CRR_HD uint32_t be_byte(uint64_t v, uint32_t width, uint32_t i) { return (uint32_t)(v >> (8 * (width - 1 - i))) & 0xffu; }

template <class After>
CRR_HD void vh_emit_chunk(const Ctx& c, const StoreIn& a, const After& after, const uint64_t* blob_off, uint64_t n_bytes,
                          uint64_t chunk, uint64_t& lo, uint64_t& hi) {
  lo = hi = 0;
  const uint64_t pos = chunk * 16;
  if (pos >= n_bytes || a.n_tasks == 0) return;
  uint32_t k = 0, r = a.n_tasks;   // the last task that starts at or before pos: blob_off[0] == 0
  while (k + 1 < r) {
    const uint32_t m = k + (r - k) / 2;
    if (blob_off[m] <= pos) k = m;
    else r = m;
  }
  uint64_t base = blob_off[k], end = blob_off[k + 1];
  StoreDecision D;
  StoreBranch B;
  bool fresh = true, gen = false;
  int64_t h = -1;
  uint64_t h_begin = 0, h_end = kVhHead;
  uint32_t j_have = 0xFFFFFFFFu;
  crr_vh_item x = {0, 0};
  for (uint32_t b = 0; b < 16; ++b) {
    const uint64_t g = pos + b;
    if (g >= n_bytes) return;
    while (g >= end) {   // the next task that holds bytes
      if (++k >= a.n_tasks) return;
      base = blob_off[k], end = blob_off[k + 1];
      fresh = true;
    }
    if (fresh) {
      store_decide(c, a, after, k, D);
      gen = D.generated() && g >= base;
      h = -1, h_begin = 0, h_end = kVhHead;
      fresh = false;
    }
    if (!gen) continue;
    const uint64_t p = g - base;
    uint32_t v = 0;
    if (p < kVhHead) {
      v = p == 0 ? 0x59u : p < 8 ? be_byte((0x08000aull << 32) | (uint32_t)D.current, 7, (uint32_t)p - 1)
                                 : be_byte((0x0f00140cull << 32) | (uint32_t)D.nb, 8, (uint32_t)p - 8);
    } else {
      while (p >= h_end && h < D.nb) {
        if (++h >= D.nb) break;
        if (!store_branch(a, D, h, B)) {
          gen = false;
          break;
        }
        h_begin = h_end;
        h_end = h_begin + kVhHistory + B.tk.len + kVhItem * B.n;
        j_have = 0xFFFFFFFFu;
      }
      if (!gen) continue;
      if (h < D.nb) {   // (past the last history: the struct's stop byte, zero like everything behind it)
        const uint64_t q = p - h_begin, items_at = 15ull + B.tk.len;
        if (q < 7) {
          v = be_byte((0x0b000aull << 32) | B.tk.len, 7, (uint32_t)q);
        } else if (q < 7ull + B.tk.len) {
          v = c.in.bytes[B.tk.off + (q - 7)];
        } else if (q < items_at) {
          v = be_byte((0x0f00140cull << 32) | B.n, 8, (uint32_t)(q - 7 - B.tk.len));
        } else if (q < items_at + kVhItem * B.n) {
          const uint64_t rem = q - items_at;
          const uint32_t j = (uint32_t)(rem / kVhItem), m = (uint32_t)(rem % kVhItem);
          if (j != j_have) {
            x = B.item(j, D.e);
            j_have = j;
          }
          v = m < 3 ? be_byte(0x0a000aull, 3, m) : m < 11 ? be_byte((uint64_t)x.event_id, 8, m - 3)
              : m < 14 ? be_byte(0x0a0014ull, 3, m - 11) : m < 22 ? be_byte((uint64_t)x.version, 8, m - 14) : 0u;
        }
      }
    }
    if (b < 8) lo |= (uint64_t)v << (8 * b);
    else hi |= (uint64_t)v << (8 * (b - 8));
  }
}

// ---- per task: the pending-entry mutation to store (cadence_load_mutation.h) ----------------------------------
// What CloseTransactionAsMutation writes beside ExecutionInfo (mutable_state_builder.go:4002-4011): per pending map
// the rows to upsert and the keys to delete, as the difference between the loader's dense image (before) and the
// state the resumed replay left (after), both behind the state view store_task reads.  The walk is written once
// and takes a visitor: the count pass counts, the emit pass writes the deleted keys and the directory.
static_assert(sizeof(crr_activity_row) == 112 && sizeof(crr_timer_row) == 40 && sizeof(crr_child_row) == 48 &&
                  sizeof(crr_initiated_row) == 32 && sizeof(crr_reset_point_row) == 16 && sizeof(crr_exec_row) == 208,
              "row images are compared and gathered as 8-byte words");
static_assert(__builtin_offsetof(crr_activity_row, last_hb_timeout_vis_s) == 56 && __builtin_offsetof(crr_activity_row, flags) == 96 &&
                  __builtin_offsetof(crr_child_row, flags) == 40 && __builtin_offsetof(crr_timer_row, key) == 28,
              "the masks of mut_mask and the timer's key");

constexpr uint64_t kMutNoSlot = ~0ull;   // a directory entry the emit pass did not write

CRR_HD uint64_t mut_word(const uint8_t* row, uint32_t k) {
  uint64_t v;
  memcpy(&v, row + 8u * k, sizeof v);
  return v;
}
// the persisted bits of word k of map t's row image: not the activity's last_hb_timeout_vis_s (word 7) and MAPPED
// flag (the low half of word 12), nor the child row's reserved word (the high half of word 5)
CRR_HD uint64_t mut_mask(int t, uint32_t k) {
  if (t == 0) return k == 7 ? 0ull : k == 12 ? ~(uint64_t)CRR_ROW_MAPPED : ~0ull;
  if (t == 2) return k == 5 ? 0xFFFFFFFFull : ~0ull;
  return ~0ull;
}
template <int T>
CRR_HD bool mut_same(const uint8_t* a, const uint8_t* b) {
  uint64_t diff = 0;
  for (uint32_t k = 0; k < kRowBytes[T] / 8; ++k) diff |= (mut_word(a, k) ^ mut_word(b, k)) & mut_mask(T, k);
  return diff == 0;
}
CRR_HD uint32_t mut_timer_key(const uint8_t* row) {
  uint32_t v;
  memcpy(&v, row + 28, sizeof v);
  return v;
}

// map T of one task: B the rows before, A the rows after, both ascending by their first field.  vis.upsert(row
// after) in slot order, vis.remove(key) in the order of the rows before.
template <int T, class Vis>
CRR_HD void mutation_walk(const StateView& B, const StateView& A, Vis& vis) {
  const uint8_t *pb = B.rows_of(T), *pa = A.rows_of(T);
  const uint64_t sb = B.stride * kRowBytes[T], sa = A.stride * kRowBytes[T];
  const uint32_t nb = B.count(T), na = A.count(T);
  auto gone = [&](const uint8_t* rb) {
    if (T != 1) return vis.remove((int64_t)mut_word(rb, 0));
    // a timer is the store's row of its TimerID: started again under it, the row is replaced, not deleted
    const uint32_t key = mut_timer_key(rb);
    for (uint32_t j = 0; j < na; ++j)
      if (mut_timer_key(pa + j * sa) == key) return;
    vis.remove((int64_t)key);
  };
  uint32_t i = 0, j = 0;
  while (i < nb || j < na) {
    const uint8_t *rb = pb + i * sb, *ra = pa + j * sa;
    if (j >= na) { gone(rb); ++i; continue; }
    if (i >= nb) { vis.upsert(ra); ++j; continue; }
    const int64_t ib = (int64_t)mut_word(rb, 0), ia = (int64_t)mut_word(ra, 0);
    if (ib < ia) { gone(rb); ++i; continue; }
    if (ia < ib) { vis.upsert(ra); ++j; continue; }
    if (T == 1 && mut_timer_key(rb) != mut_timer_key(ra)) {   // one started_id under two TimerIDs: two store rows
      gone(rb);
      vis.upsert(ra);
    } else if (!mut_same<T>(rb, ra)) {
      vis.upsert(ra);
    }
    ++i, ++j;
  }
}

CRR_HD bool mut_reset_points_differ(const StateView& B, const StateView& A) {
  if (B.n_rp != A.n_rp) return true;
  uint64_t diff = 0;
  for (uint32_t j = 0; j < A.n_rp; ++j) {
    const uint8_t *rb = B.rp + (uint64_t)j * B.stride * kRowBytes[6], *ra = A.rp + (uint64_t)j * A.stride * kRowBytes[6];
    diff |= (mut_word(rb, 0) ^ mut_word(ra, 0)) | (mut_word(rb, 1) ^ mut_word(ra, 1));
  }
  return diff != 0;
}

// the decision of store_task, its branch-table check included: true when the task has a pending-entry mutation
template <class After>
CRR_HD bool mutation_decide(const Ctx& c, const StoreIn& a, const After& after, uint32_t idx, StoreDecision& D,
                            int32_t& outcome, int32_t& status) {
  store_decide(c, a, after, idx, D);
  outcome = D.outcome, status = D.status;
  if (D.generated()) {
    for (int64_t h = 0; h < D.nb; ++h) {
      StoreBranch B;
      if (!store_branch(a, D, h, B)) {
        outcome = CRR_STORE_NOT_LOADED;
        break;
      }
    }
  }
  return outcome == CRR_STORE_APPLIED;
}

struct MutCount {
  uint32_t up, del;
  CRR_HD void upsert(const uint8_t*) { ++up; }
  CRR_HD void remove(int64_t) { ++del; }
};

// task idx's row with its counts (the begins zero: the offsets pass fills them); exec_index 0 marks an exec row
template <class After>
CRR_HD void mutation_count_task(const Ctx& c, const StoreIn& a, const After& after, uint32_t idx, crr_mutation_row& o) {
  memset(&o, 0, sizeof o);
  o.exec_index = 0xFFFFFFFFu;
  StoreDecision D;
  if (!mutation_decide(c, a, after, idx, D, o.outcome, o.status)) return;
  const StateView B = scratch_view(c, D.w);
  o.exec_index = 0;
  if (mut_reset_points_differ(B, D.S)) o.flags |= CRR_MUTATION_RESET_POINTS_CHANGED;
  MutCount k0 = {0, 0}, k1 = {0, 0}, k2 = {0, 0}, k3 = {0, 0}, k4 = {0, 0};
  mutation_walk<0>(B, D.S, k0);
  mutation_walk<1>(B, D.S, k1);
  mutation_walk<2>(B, D.S, k2);
  mutation_walk<3>(B, D.S, k3);
  mutation_walk<4>(B, D.S, k4);
  o.map[0].n_upsert = k0.up, o.map[0].n_delete = k0.del;
  o.map[1].n_upsert = k1.up, o.map[1].n_delete = k1.del;
  o.map[2].n_upsert = k2.up, o.map[2].n_delete = k2.del;
  o.map[3].n_upsert = k3.up, o.map[3].n_delete = k3.del;
  o.map[4].n_upsert = k4.up, o.map[4].n_delete = k4.del;
}

// The run call's directory and key buffers.  dir_exec[k]: the slot of exec row k in the after-state's exec table;
// dir[t][k]: the row index, in the after-state's table t, of upserted row k.  Both are preset to kMutNoSlot.
struct MutDst {
  uint64_t* dir_exec;
  uint64_t* dir[CRR_MUTATION_MAPS];
  int64_t* keys[CRR_MUTATION_MAPS];
  const uint8_t* base[CRR_MUTATION_MAPS];   // row 0 of the after-state's tables
  uint64_t n_exec, n_upsert[CRR_MUTATION_MAPS], n_delete[CRR_MUTATION_MAPS];   // the plan's totals
};

struct MutEmit {
  uint64_t* dir;
  int64_t* keys;
  const uint8_t* base;
  uint32_t row_bytes, up, del, n_up, n_del;
  CRR_HD void upsert(const uint8_t* ra) {
    if (up < n_up) dir[up] = (uint64_t)(ra - base) / row_bytes;
    ++up;
  }
  CRR_HD void remove(int64_t key) {
    if (del < n_del) keys[del] = key;
    ++del;
  }
};

// the walk again for planned row `o`: nothing is written outside the ranges the plan gave the task, and a range
// that does not lie within the plan's totals is not written at all; keys the walk no longer finds are zeros
template <int T>
CRR_HD void mutation_emit_map(const StateView& B, const StateView& A, const crr_mutation_map& m, const MutDst& d, bool walk) {
  const bool up_ok = (uint64_t)m.upsert_begin + m.n_upsert <= d.n_upsert[T];
  const bool del_ok = (uint64_t)m.delete_begin + m.n_delete <= d.n_delete[T];
  MutEmit e = {d.dir[T] + m.upsert_begin, d.keys[T] + m.delete_begin, d.base[T], kRowBytes[T], 0, 0,
               up_ok ? m.n_upsert : 0u, del_ok ? m.n_delete : 0u};
  if (walk) mutation_walk<T>(B, A, e);
  for (uint32_t k = e.del; k < e.n_del; ++k) e.keys[k] = 0;
}

template <class After>
CRR_HD void mutation_emit_task(const Ctx& c, const StoreIn& a, const After& after, uint32_t idx, const crr_mutation_row* rows,
                               const MutDst& d) {
  const crr_mutation_row o = rows[idx];
  StoreDecision D;
  int32_t outcome, status;
  const bool walk = mutation_decide(c, a, after, idx, D, outcome, status);
  if (!walk) {   // no longer a mutation: its keys are zeros, its directory entries stay unwritten (the views are not read)
    mutation_emit_map<0>(D.S, D.S, o.map[0], d, false);
    mutation_emit_map<1>(D.S, D.S, o.map[1], d, false);
    mutation_emit_map<2>(D.S, D.S, o.map[2], d, false);
    mutation_emit_map<3>(D.S, D.S, o.map[3], d, false);
    mutation_emit_map<4>(D.S, D.S, o.map[4], d, false);
    return;
  }
  const StateView B = scratch_view(c, D.w);
  if (o.exec_index < d.n_exec) d.dir_exec[o.exec_index] = D.S.exec_slot;
  mutation_emit_map<0>(B, D.S, o.map[0], d, walk);
  mutation_emit_map<1>(B, D.S, o.map[1], d, walk);
  mutation_emit_map<2>(B, D.S, o.map[2], d, walk);
  mutation_emit_map<3>(B, D.S, o.map[3], d, walk);
  mutation_emit_map<4>(B, D.S, o.map[4], d, walk);
}

// word g of a dense output of `words`-word rows, gathered through its directory from `table`
CRR_HD uint64_t mutation_gather_word(const uint64_t* table, const uint64_t* dir, uint32_t words, uint64_t g) {
  const uint64_t src = dir[g / words];
  return src == kMutNoSlot ? 0ull : table[src * words + g % words];
}

// ---- per task: the execution blob to store (cadence_load_store_exec.h) ------------------------------------------
// CloseTransactionAsMutation always writes ExecutionInfo (mutable_state_builder.go:3998-3999).  Every thrift scalar
// is fixed-width and thriftrw writes the set fields in ascending id, so the blob to store is the stored blob with a
// bounded number of edits: the decision (exec_plan_task) and the edit rules (exec_walk) are written once; the walk
// takes an emitter -- the edit script the device's emit kernel reads, or the sequential ByteSink of the host.
constexpr int kExecSegs = 48, kExecPatches = 24, kExecFields = 25;
constexpr uint32_t kSegStored = 0, kSegVh = 1, kSegTask = 2, kSegLit = 3;
constexpr uint32_t kSegLenMask = 0x3FFFFFFFu;

struct ExecSeg {
  uint32_t dst;        // offset in the new blob
  uint32_t len_kind;   // length in the low 30 bits, the source kind above
  uint64_t src;        // offset into the source's buffer; a literal: its (at most 8) bytes, the first one lowest
};
struct ExecPatch {
  uint32_t dst, width;   // `width` (1, 4 or 8) bytes at dst ...
  uint64_t value;        // ... are this value, big-endian
};
struct ExecScript {
  uint32_t n_seg, n_patch, len, reserved;
  ExecSeg seg[kExecSegs];       // ascending by dst, contiguous from 0 to len
  ExecPatch patch[kExecPatches];
};
static_assert(sizeof(ExecScript) == 16 + 16 * kExecSegs + 16 * kExecPatches, "scripts are packed, 16-byte aligned");

// the overridden fields in ascending id: slot <-> field id, and each slot's thrift type
CRR_HD int exec_slot_of(int id) {
  switch (id) {
    case 18: return 0;   case 34: return 1;   case 36: return 2;   case 48: return 3;   case 50: return 4;
    case 52: return 5;   case 56: return 6;   case 58: return 7;   case 60: return 8;   case 62: return 9;
    case 64: return 10;  case 66: return 11;  case 68: return 12;  case 69: return 13;  case 70: return 14;
    case 71: return 15;  case 74: return 16;  case 78: return 17;  case 80: return 18;  case 106: return 19;
    case 108: return 20; case 110: return 21; case 112: return 22; case 114: return 23; case 122: return 24;
    default: return -1;
  }
}
CRR_HD int exec_id_of(int slot) {
  switch (slot) {
    case 0: return 18;   case 1: return 34;   case 2: return 36;   case 3: return 48;   case 4: return 50;
    case 5: return 52;   case 6: return 56;   case 7: return 58;   case 8: return 60;   case 9: return 62;
    case 10: return 64;  case 11: return 66;  case 12: return 68;  case 13: return 69;  case 14: return 70;
    case 15: return 71;  case 16: return 74;  case 17: return 78;  case 18: return 80;  case 19: return 106;
    case 20: return 108; case 21: return 110; case 22: return 112; case 23: return 114; default: return 122;
  }
}
constexpr uint32_t kExecApplied = (1u << kExecFields) - 1u;
constexpr uint32_t kExecBackfill = (1u << 6) | (1u << 20) | (1u << 24);   // 56, 108, 122
constexpr uint32_t kExecStrings = (1u << 16) | (1u << 17) | (1u << 21) | (1u << 22) | (1u << 23) | (1u << 24);
constexpr int kExecSlot18 = 0, kExecSlot74 = 16, kExecSlot108 = 20, kExecSlot122 = 24;
CRR_HD uint8_t exec_type_of(int slot) {
  if ((kExecStrings >> slot) & 1u) return T_STRING;
  if (slot == 14) return T_BOOL;
  return (slot == 1 || slot == 2 || slot == 10) ? T_I32 : T_I64;
}
CRR_HD uint32_t exec_width_of(uint8_t t) { return t == T_BOOL ? 1u : t == T_I32 ? 4u : 8u; }
CRR_HD int64_t to_unix_nano(int64_t v) { return v == CRR_ZERO_TIME ? kGoZeroTimeNanos : v; }

// what a call reads beside StoreIn: the tasks' clocks, the VersionHistories plan of the same tasks, the tasks' event
// blobs (optional) and where the event types of this call are (the device: the replay's column; the host: a flag
// per workflow)
struct ExecIn {
  const crr_exec_blob_task* xt;
  const crr_vh_blob_row* vh_rows;
  const uint64_t* vh_off;
  uint64_t vh_total;
  const uint8_t* tb_bytes;
  const uint64_t* tb_off;
  const crr_blob_wf* tb_wf;
  uint32_t tb_n_blobs, tb_n_wf;
  const uint8_t* etype;
  const crr_workflow* ev_wf;
  uint32_t ev_n_wf, ev_stride, ev_wave_begin;
  const uint8_t* upserts;
};

// the tasks' event blobs into the tb_* fields of an ExecIn or a ResumeIn (host code only: the launchers and the host
// restatement).  It assigns the five fields and checks nothing: what a batch must hold differs from call to call
template <class In>
inline void pack_task_blobs(In& x, const crr_blob_batch& B) {
  x.tb_bytes = B.bytes;
  x.tb_off = B.blob_off;
  x.tb_wf = B.wf;
  x.tb_n_blobs = B.n_blobs;
  x.tb_n_wf = B.n_wf;
}

// what the decision leaves for the walk
struct ExecTask {
  uint32_t active, seen;   // the slots overridden; those of them the stored blob holds
  uint32_t exec_blob;      // the execution blob's index in the batch
  uint32_t vh_len, rq_len;
  int rq_mode;             // field 74: 0 "emptyUuid", 1 "", 2 the task's bytes at rq_off
  bool omit18;
  uint64_t vh_off, rq_off;
  int64_t now, hist;
};

CRR_HD int64_t exec_scalar(int slot, const crr_exec_row& R, const ExecTask& T) {
  switch (slot) {
    case 0: return R.completion_event_batch_id;
    case 1: return R.state;
    case 2: return R.close_status;
    case 3: return R.last_event_task_id;
    case 4: return R.last_first_event_id;
    case 5: return R.last_processed_event;
    case 6: return T.now;
    case 7: return R.decision_version;
    case 8: return R.decision_schedule_id;
    case 9: return R.decision_started_id;
    case 10: return R.decision_timeout;
    case 11: return R.decision_attempt;
    case 12: return to_unix_nano(R.decision_started_ts);
    case 13: return to_unix_nano(R.decision_scheduled_ts);
    case 14: return (R.flags & CRR_EXEC_CANCEL_REQUESTED) ? 1 : 0;
    case 15: return to_unix_nano(R.decision_orig_scheduled_ts);
    case 19: return R.signal_count;
    case 20: return T.hist;
    default: return 0;   // 80 StickyScheduleToStartTimeout
  }
}

// whether the events of this call at exec slot `slot` (the device position; the host: workflow w) hold an
// UpsertWorkflowSearchAttributes, the events addressed as the replay addresses them
CRR_HD bool exec_has_upsert(const ExecIn& x, uint64_t slot, uint32_t w) {
  if (x.upserts) return x.upserts[w] != 0;
  if (!x.etype || !x.ev_wf || slot >= x.ev_n_wf) return false;
  const crr_workflow& D = x.ev_wf[slot];
  const uint64_t st = slot >= x.ev_wave_begin ? 1 : x.ev_stride;
  for (int32_t s = 0; s < D.ev_count; ++s)
    if ((x.etype[(uint64_t)D.ev_begin + (uint64_t)s * st] & CRR_ETYPE_MASK) == CRR_EV_UPSERT_WORKFLOW_SEARCH_ATTRIBUTES) return true;
  return false;
}

// RequestId of event number `target` of the task at exec slot `slot`, counted across the workflow's blobs: 0x59,
// shared.History{10 list<HistoryEvent{30 eventType, 90 decisionTaskStartedEventAttributes{30 requestId}}>}.  false:
// no blobs, the event is not there, it is not a DecisionTaskStarted, or a blob is malformed.  The string lies within
// the batch's bytes.
CRR_HD bool exec_request_id(const ExecIn& x, uint64_t slot, int64_t target, uint64_t& off, uint32_t& len, Frame* stk) {
  off = 0, len = 0;
  if (!x.tb_bytes || !x.tb_off || !x.tb_wf || slot >= x.tb_n_wf || target < 0) return false;
  const crr_blob_wf W = x.tb_wf[slot];
  if ((uint64_t)W.blob_begin + W.blob_count > x.tb_n_blobs) return false;
  const uint64_t total = x.tb_off[x.tb_n_blobs];
  for (uint32_t b = W.blob_begin; b < W.blob_begin + W.blob_count; ++b) {
    Rd r = {x.tb_bytes, x.tb_off[b], x.tb_off[b + 1], false};
    if (r.end < r.pos || r.end > total) return false;
    if (r.end == r.pos) continue;   // an empty batch is an empty blob
    if (rd_u8(r) != 0x59) return false;
    uint8_t t, t2, t3;
    int16_t id, id2, id3;
    while (next_field(r, t, id)) {
      if (id != 10 || t != T_LIST) {
        skip(r, t, stk);
        continue;
      }
      const uint8_t et = rd_u8(r);
      const int32_t n = rd_i32(r);
      if (r.bad || et != T_STRUCT || n < 0 || (uint64_t)n > r.end - r.pos) return false;
      const int64_t before = target < n ? target : n;
      for (int64_t k = 0; k < before; ++k) skip(r, T_STRUCT, stk);
      if (r.bad) return false;
      target -= before;
      if (before == n) continue;
      int32_t etype = -1;
      bool attrs = false;
      while (next_field(r, t2, id2)) {
        if (id2 == 30 && t2 == T_I32) {
          etype = rd_i32(r);
        } else if (id2 == 90 && t2 == T_STRUCT) {
          attrs = true;
          while (next_field(r, t3, id3)) {
            if (id3 == 30 && t3 == T_STRING) rd_str(r, off, len);
            else skip(r, t3, stk);
          }
        } else {
          skip(r, t2, stk);
        }
      }
      return !r.bad && etype == CRR_EV_DECISION_TASK_STARTED && attrs;
    }
    if (r.bad) return false;
  }
  return false;
}

// the stored blob's top-level fields once: which overridden fields it holds, HistorySize as stored.  false: an
// overridden field of another thrift type or held twice (or bytes the loader did not validate)
CRR_HD bool exec_scan(const Ctx& c, uint32_t blob, uint32_t active, uint32_t& seen, int64_t& hist, Frame* stk) {
  Rd r = c.blob(blob);
  seen = 0, hist = 0;
  uint8_t t;
  int16_t id;
  while (next_field(r, t, id)) {
    const int s = exec_slot_of(id);
    if (s >= 0 && ((active >> s) & 1u)) {
      if (t != exec_type_of(s) || ((seen >> s) & 1u)) return false;
      seen |= 1u << s;
      if (s == kExecSlot108) {
        hist = rd_i64(r);
        continue;
      }
    }
    skip(r, t, stk);
  }
  return !r.bad;
}

// The decision for task idx: the row (outcome and status of store_task, the host flags, next_event_id; len is the
// caller's) and, when true is returned, what the walk needs.  vh_bad: the VersionHistories plan's row disagrees.
template <class After>
CRR_HD bool exec_plan_task(const Ctx& c, const StoreIn& a, const After& after, const ExecIn& x, uint32_t idx,
                           crr_exec_blob_row& row, StoreDecision& D, ExecTask& T, bool& vh_bad, Frame* stk) {
  int32_t outcome, status;
  mutation_decide(c, a, after, idx, D, outcome, status);
  row.outcome = outcome, row.status = status, row.flags = 0, row.len = 0, row.next_event_id = 0;
  const bool gen = outcome == CRR_STORE_APPLIED || outcome == CRR_STORE_BACKFILLED;
  const crr_vh_blob_row vr = x.vh_rows[idx];
  const uint64_t o0 = x.vh_off[idx], o1 = x.vh_off[idx + 1];
  vh_bad = vr.outcome != outcome || o1 < o0 || o1 > x.vh_total || o1 - o0 != vr.len || gen != (vr.len != 0);
  if (!gen || vh_bad) return false;
  const bool apply = outcome == CRR_STORE_APPLIED;
  const crr_exec_row& R = D.S.R;
  row.next_event_id = R.next_event_id;   // (the backfill's view is the loaded state: the stored column)
  const crr_state_wf W = c.in.wf[D.w];
  uint32_t flags = 0;
  T.active = apply ? kExecApplied : kExecBackfill;
  T.omit18 = false;
  T.rq_mode = 1, T.rq_off = 0, T.rq_len = 0;
  T.now = x.xt[idx].now_ns;
  T.vh_off = o0, T.vh_len = vr.len;
  T.exec_blob = W.blob_begin + (uint32_t)c.aux()[D.w].exec_idx;
  if (apply) {
    if (mut_reset_points_differ(scratch_view(c, D.w), D.S)) flags |= CRR_EXEC_BLOB_HOST_RESET_POINTS;
    if (exec_has_upsert(x, D.S.exec_slot, D.w)) flags |= CRR_EXEC_BLOB_HOST_SEARCH_ATTRIBUTES;
    T.omit18 = R.completion_event_batch_id == CRR_EMPTY_EVENT_ID;
    const int32_t src = R.decision_request_src;
    if (src == CRR_SRC_EMPTY_UUID) T.rq_mode = 0;
    else if (src == CRR_SRC_NONE) T.rq_mode = 1;
    else if (src >= 0 && (uint32_t)src < W.blob_count) T.active &= ~(1u << kExecSlot74);   // the load's: as stored
    else if (src >= 0 && exec_request_id(x, D.S.exec_slot, (int64_t)src - (int64_t)W.blob_count, T.rq_off, T.rq_len, stk)) T.rq_mode = 2;
    else flags |= CRR_EXEC_BLOB_HOST_REQUEST_ID;
  }
  int64_t stored_hist;
  if (!exec_scan(c, T.exec_blob, T.active, T.seen, stored_hist, stk)) flags |= CRR_EXEC_BLOB_HOST_STORED_SHAPE;
  T.hist = (int64_t)((uint64_t)stored_hist + (uint64_t)x.xt[idx].history_size_delta);
  row.flags = flags;
  return flags == 0;
}

// the emitter that records the edit script: neighbouring copies from one source merge, so a blob Go wrote takes a
// dozen segments; `overflow`: more edits than a script holds, or a blob past 2^30 bytes
struct ExecScriptEm {
  ExecScript* S;
  uint32_t n_seg, n_patch, dst;
  bool overflow;
  CRR_HD void seg(uint32_t kind, uint64_t src, uint32_t len) {
    if (len == 0 || overflow) return;
    if ((uint64_t)dst + len > kSegLenMask) {
      overflow = true;
      return;
    }
    if (kind != kSegLit && n_seg) {
      ExecSeg& L = S->seg[n_seg - 1];
      if ((L.len_kind >> 30) == kind && L.src + (L.len_kind & kSegLenMask) == src) {
        L.len_kind += len;
        dst += len;
        return;
      }
    }
    if (n_seg == (uint32_t)kExecSegs) {
      overflow = true;
      return;
    }
    const ExecSeg s = {dst, len | (kind << 30), src};
    S->seg[n_seg++] = s;
    dst += len;
  }
  CRR_HD void keep(uint64_t from, uint64_t to) { seg(kSegStored, from, (uint32_t)(to - from)); }
  CRR_HD void patch(uint64_t at, uint32_t width, int64_t value) {
    if (n_patch == (uint32_t)kExecPatches) overflow = true;
    if (overflow) return;
    const ExecPatch p = {dst, width, (uint64_t)value};
    S->patch[n_patch++] = p;
    seg(kSegStored, at, width);
  }
  CRR_HD void lit(uint64_t v, uint32_t n) { seg(kSegLit, v, n); }
  CRR_HD void src(uint32_t kind, uint64_t off, uint32_t len) { seg(kind, off, len); }
};

// the emitter of the host restatement: the bytes themselves, in order
struct ExecSinkEm {
  ByteSink K;
  const uint8_t *stored, *vh, *task;
  CRR_HD void keep(uint64_t from, uint64_t to) {
    for (uint64_t i = from; i < to; ++i) K.u8(stored[i]);
  }
  CRR_HD void patch(uint64_t, uint32_t width, int64_t value) {
    for (uint32_t i = 0; i < width; ++i) K.u8((uint32_t)((uint64_t)value >> (8 * (width - 1 - i))));
  }
  CRR_HD void lit(uint64_t v, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) K.u8((uint32_t)(v >> (8 * i)));
  }
  CRR_HD void src(uint32_t kind, uint64_t off, uint32_t len) {
    const uint8_t* p = kind == kSegVh ? vh : task;
    for (uint32_t i = 0; i < len; ++i) K.u8(p[off + i]);
  }
};

// The splice (cadence_load_store_exec.h) for a task exec_plan_task accepted.  false: the blob is not the one
// exec_scan walked.
template <class Em>
CRR_HD bool exec_walk(const Ctx& c, const crr_exec_row& R, const ExecTask& T, Em& em, Frame* stk) {
  Rd r = c.blob(T.exec_blob);
  uint64_t cs = r.pos;                    // stored bytes [cs, cursor) are kept but not yet emitted
  uint32_t todo = T.active & ~T.seen;     // overridden fields the stored blob lacks: to insert
  if (T.omit18) todo &= ~(1u << kExecSlot18);
  auto put = [&](int s) {                 // field s whole: header and new value
    const uint32_t id = (uint32_t)exec_id_of(s);
    const uint8_t t = exec_type_of(s);
    const uint64_t head = t | ((uint64_t)(id >> 8) << 8) | ((uint64_t)(id & 0xffu) << 16);
    if (t != T_STRING) {
      const uint32_t w = exec_width_of(t);
      const uint64_t v = (uint64_t)exec_scalar(s, R, T);
      em.lit(head, 3);
      em.lit(w == 8 ? __builtin_bswap64(v) : w == 4 ? (uint64_t)__builtin_bswap32((uint32_t)v) : (v & 0xffu), w);
      return;
    }
    const bool uuid = s == kExecSlot74 && T.rq_mode == 0;
    const uint32_t len = s == kExecSlot122 ? T.vh_len : s != kExecSlot74 ? 0u : uuid ? 9u : T.rq_mode == 2 ? T.rq_len : 0u;
    em.lit(head | ((uint64_t)__builtin_bswap32(len) << 24), 7);
    if (s == kExecSlot122) {
      em.src(kSegVh, T.vh_off, len);
    } else if (uuid) {
      em.lit(0x6975557974706d65ull, 8);   // "emptyUui"
      em.lit(0x64, 1);                    // "d"
    } else if (len) {
      em.src(kSegTask, T.rq_off, len);
    }
  };
  auto insert_below = [&](int limit) {
    for (int s = 0; s < kExecFields; ++s)
      if (((todo >> s) & 1u) && exec_id_of(s) < limit) {
        put(s);
        todo &= ~(1u << s);
      }
  };
  for (;;) {
    const uint64_t fstart = r.pos;
    uint8_t t;
    int16_t id;
    if (!next_field(r, t, id)) break;
    if (todo) {
      em.keep(cs, fstart);
      cs = fstart;
      insert_below(id);
    }
    const int s = exec_slot_of(id);
    if (s < 0 || !((T.active >> s) & 1u)) {
      skip(r, t, stk);
      continue;
    }
    if (t != exec_type_of(s)) return false;
    if (t == T_STRING) {
      uint64_t o;
      uint32_t l;
      if (!rd_str(r, o, l)) return false;
      em.keep(cs, fstart);
      put(s);
      cs = r.pos;
      continue;
    }
    const uint32_t w = exec_width_of(t);
    if (!need(r, w)) return false;
    if (s == kExecSlot18 && T.omit18) {
      em.keep(cs, fstart);
    } else {
      em.keep(cs, r.pos);
      em.patch(r.pos, w, exec_scalar(s, R, T));
    }
    r.pos += w;
    cs = r.pos;
  }
  if (r.bad) return false;
  const uint64_t stop = r.pos - 1;        // next_field consumed the stop byte
  em.keep(cs, stop);
  insert_below(0x10000);
  em.keep(stop, stop + 1);
  return true;
}

// task idx's row, script and length (0: nothing is generated on the device)
template <class After>
CRR_HD uint32_t exec_size_task(const Ctx& c, const StoreIn& a, const After& after, const ExecIn& x, uint32_t idx,
                               crr_exec_blob_row* rows, ExecScript* S, bool& vh_bad, Frame* stk) {
  crr_exec_blob_row row;
  StoreDecision D;
  ExecTask T;
  ExecScriptEm em = {S, 0, 0, 0, false};
  uint32_t len = 0;
  if (exec_plan_task(c, a, after, x, idx, row, D, T, vh_bad, stk)) {
    if (exec_walk(c, D.S.R, T, em, stk) && !em.overflow) len = em.dst;
    else row.flags |= CRR_EXEC_BLOB_HOST_STORED_SHAPE;
  }
  S->n_seg = len ? em.n_seg : 0;
  S->n_patch = len ? em.n_patch : 0;
  S->len = len;
  S->reserved = 0;
  row.len = len;
  rows[idx] = row;
  return len;
}

// The output-stationary form (load_store_exec_emit_kernel): bytes [16 * chunk, + 16) of the concatenated blobs as
// two little-endian words.  The task is found as vh_emit_chunk finds it, the segment by walking the task's script
// forward, then the source byte is read and a patch that covers it applied.  Counts and widths read from a script
// are clamped to what a script holds, every source offset is checked against its buffer's size, and a script
// whose length is not the one the offsets give is not read at all: such bytes are zero.
struct ExecSrc {
  const uint8_t *stored, *vh, *task;
  uint64_t n_stored, n_vh, n_task;
};
CRR_HD void exec_emit_chunk(const ExecScript* scripts, const ExecSrc& q, const uint64_t* blob_off, uint32_t n_tasks,
                            uint64_t n_bytes, uint64_t chunk, uint64_t& lo, uint64_t& hi) {
  lo = hi = 0;
  const uint64_t pos = chunk * 16;
  if (pos >= n_bytes || n_tasks == 0) return;
  uint32_t k = 0, r = n_tasks;   // the last task that starts at or before pos: blob_off[0] == 0
  while (k + 1 < r) {
    const uint32_t m = k + (r - k) / 2;
    if (blob_off[m] <= pos) k = m;
    else r = m;
  }
  uint64_t base = blob_off[k], end = blob_off[k + 1];
  bool fresh = true, ok = false;
  const ExecScript* S = scripts;
  uint32_t n_seg = 0, n_patch = 0, j = 0, pmask = 0;
  for (uint32_t b = 0; b < 16; ++b) {
    const uint64_t g = pos + b;
    if (g >= n_bytes) return;
    while (g >= end) {   // the next task that holds bytes
      if (++k >= n_tasks) return;
      base = blob_off[k], end = blob_off[k + 1];
      fresh = true;
    }
    if (g < base) continue;
    if (fresh) {
      S = scripts + k;
      n_seg = S->n_seg < (uint32_t)kExecSegs ? S->n_seg : (uint32_t)kExecSegs;
      n_patch = S->n_patch < (uint32_t)kExecPatches ? S->n_patch : (uint32_t)kExecPatches;
      ok = S->len == end - base;
      j = 0, pmask = 0;
      const uint64_t p0 = g - base;
      for (uint32_t i = 0; i < n_patch; ++i) {
        const uint64_t d = S->patch[i].dst;
        if (d < p0 + 16 && d + 8 > p0) pmask |= 1u << i;
      }
      fresh = false;
    }
    if (!ok) continue;
    const uint32_t p = (uint32_t)(g - base);
    while (j < n_seg && p - S->seg[j].dst >= (S->seg[j].len_kind & kSegLenMask)) ++j;
    uint32_t v = 0;
    if (j < n_seg) {
      const ExecSeg sg = S->seg[j];
      const uint64_t off = p - sg.dst;
      const uint32_t kind = sg.len_kind >> 30;
      if (kind == kSegLit) {
        v = off < 8 ? (uint32_t)(sg.src >> (8 * off)) & 0xffu : 0u;
      } else if (kind == kSegStored) {   // (a branch per source: the three buffers stay three scalars)
        if (q.stored && sg.src < q.n_stored && off < q.n_stored - sg.src) v = q.stored[sg.src + off];
      } else if (kind == kSegVh) {
        if (q.vh && sg.src < q.n_vh && off < q.n_vh - sg.src) v = q.vh[sg.src + off];
      } else {
        if (q.task && sg.src < q.n_task && off < q.n_task - sg.src) v = q.task[sg.src + off];
      }
    }
    for (uint32_t m = pmask; m; m &= m - 1) {
      const ExecPatch P = S->patch[__builtin_ctz(m)];
      const uint32_t w = P.width < 8 ? P.width : 8u;
      if (p - P.dst < w) v = (uint32_t)(P.value >> (8 * (w - 1 - (p - P.dst)))) & 0xffu;
    }
    if (b < 8) lo |= (uint64_t)v << (8 * b);
    else hi |= (uint64_t)v << (8 * (b - 8));
  }
}

// ---- cadence_load_resume.h: the resumed replay of routed tasks planned from the loaded states ----------------
// The columns counted per position and scanned: positions with a task, their blobs, those blobs' bytes, the
// applied states' dictionary entries, their string bytes, their tokens' bytes (each padded to 8).
constexpr int kResCols = 6;
enum { kResApplied = 0, kResBlobs, kResBlobBytes, kResKeys, kResKeyBytes, kResTokenBytes };
constexpr int kResCaps = 8;                      // the eight slot tables of a descriptor
constexpr uint32_t kResNoTask = 0xFFFFFFFFu;     // winner[p]: no task is applied at the position
constexpr uint32_t kResBlock = 128;              // positions per block sum

// the work buffer the three calls share: the winning task per position, the per-position counts scanned in place to
// offsets ([col][n_wf + 1]), the block sums ([col][n_blocks + 1], scanned in place) and totals of the plan and of
// the finalize (the capacities)
struct ResumeLayout {
  uint64_t winner, off, sums, totals, cap_sums, cap_totals, end;
  uint32_t n_blocks;
};
inline ResumeLayout carve_resume(uint32_t n_wf) {
  ResumeLayout L;
  L.n_blocks = (uint32_t)(((uint64_t)n_wf + kResBlock - 1) / kResBlock);
  uint64_t o = 0;
  L.winner = o;      o = align16(o + (uint64_t)n_wf * sizeof(uint32_t));
  L.off = o;         o = align16(o + (uint64_t)kResCols * ((uint64_t)n_wf + 1) * sizeof(uint64_t));
  L.sums = o;        o = align16(o + (uint64_t)kResCols * ((uint64_t)L.n_blocks + 1) * sizeof(int64_t));
  L.totals = o;      o = align16(o + kResCols * sizeof(uint64_t));
  L.cap_sums = o;    o = align16(o + (uint64_t)kResCaps * ((uint64_t)L.n_blocks + 1) * sizeof(int64_t));
  L.cap_totals = o;  o = align16(o + kResCaps * sizeof(uint64_t));
  L.end = o;
  return L;
}
struct ResumeWork {
  uint8_t* s;
  ResumeLayout L;
  uint32_t n_wf;
  CRR_HD uint32_t* winner() const { return reinterpret_cast<uint32_t*>(s + L.winner); }
  CRR_HD uint64_t* off(int col) const { return reinterpret_cast<uint64_t*>(s + L.off) + (uint64_t)col * ((uint64_t)n_wf + 1); }
  CRR_HD int64_t* sums() const { return reinterpret_cast<int64_t*>(s + L.sums); }
  CRR_HD uint64_t* totals() const { return reinterpret_cast<uint64_t*>(s + L.totals); }
  CRR_HD int64_t* cap_sums() const { return reinterpret_cast<int64_t*>(s + L.cap_sums); }
  CRR_HD uint64_t* cap_totals() const { return reinterpret_cast<uint64_t*>(s + L.cap_totals); }
};

// the tasks, their routes and their event blobs (workflow k of the blob batch is task k)
struct ResumeIn {
  const crr_repl_task* tasks;
  const crr_ndc_route* routes;
  uint32_t n_tasks;
  const uint8_t* tb_bytes;
  const uint64_t* tb_off;
  const crr_blob_wf* tb_wf;
  uint32_t tb_n_blobs, tb_n_wf;
};

// a task before the winner is known: NOT_ROUTED, NOT_LOADED, or APPLIED for one that may be applied
CRR_HD int32_t resume_candidate(const Ctx& c, const ResumeIn& r, uint32_t k) {
  if (r.routes[k].route != CRR_ROUTE_APPLY_CURRENT) return CRR_RESUME_NOT_ROUTED;
  const uint32_t w = r.tasks[k].wf;
  if (w >= c.in.n_wf || c.status()[w] != CRR_LOAD_OK) return CRR_RESUME_NOT_LOADED;
  return CRR_RESUME_APPLIED;
}

CRR_HD crr_load_resume_row resume_row(const Ctx& c, const ResumeIn& r, const uint32_t* winner, uint32_t k) {
  crr_load_resume_row o;
  o.outcome = resume_candidate(c, r, k);
  o.position = 0xFFFFFFFFu;
  if (o.outcome == CRR_RESUME_APPLIED) {
    o.position = r.tasks[k].wf;
    if (winner[o.position] != k) o.outcome = CRR_RESUME_SHADOWED;
  }
  return o;
}

// a task's blobs as they lie in the task batch: a range or offsets outside the batch read as no blobs
struct ResumeSrc {
  uint64_t blob0, n_blobs, byte0, n_bytes;
};
CRR_HD ResumeSrc resume_src(const ResumeIn& r, uint32_t k) {
  ResumeSrc s = {0, 0, 0, 0};
  if (k >= r.tb_n_wf || !r.tb_off || !r.tb_wf) return s;
  const uint64_t b0 = r.tb_wf[k].blob_begin, n = r.tb_wf[k].blob_count;
  if (b0 > r.tb_n_blobs || n > r.tb_n_blobs - b0) return s;
  const uint64_t o0 = r.tb_off[b0], o1 = r.tb_off[b0 + n], total = r.tb_off[r.tb_n_blobs];
  if (o1 < o0 || o1 > total) return s;
  s.blob0 = b0;
  s.n_blobs = n;
  s.byte0 = o0;
  s.n_bytes = o1 - o0;
  return s;
}

// position p's counts, task k applied there (kResNoTask: none, all zero)
CRR_HD void resume_counts(const Ctx& c, const ResumeIn& r, uint32_t k, uint32_t p, uint64_t v[kResCols]) {
  for (int col = 0; col < kResCols; ++col) v[col] = 0;
  if (k == kResNoTask) return;
  const ResumeSrc s = resume_src(r, k);
  v[kResApplied] = 1;
  v[kResBlobs] = s.n_blobs;
  v[kResBlobBytes] = s.n_bytes;
  v[kResKeys] = (uint64_t)(c.cnt(CRR_LOAD_T_KEYS)[p + 1] - c.cnt(CRR_LOAD_T_KEYS)[p]);
  v[kResKeyBytes] = (uint64_t)(c.cnt(CRR_LOAD_T_KEY_BYTES)[p + 1] - c.cnt(CRR_LOAD_T_KEY_BYTES)[p]);
  v[kResTokenBytes] = ((uint64_t)(c.cnt(CRR_LOAD_T_TOKEN)[p + 1] - c.cnt(CRR_LOAD_T_TOKEN)[p]) + 7u) & ~7ull;
}

// the largest p in [0, n) with off[p] <= x, for off[0] <= x < off[n] (an empty position is never found)
CRR_HD uint32_t resume_find(const uint64_t* off, uint32_t n, uint64_t x) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// the totals the gather addresses with: the plan's, as the host read them back
struct ResumeTotals {
  uint64_t n_blobs, blob_bytes, n_keys, key_bytes, n_bytes;
};

// bytes [16 i, 16 i + 16) of the gathered `bytes` as two little-endian words: the blobs, zeros to seed_base, the
// dictionary strings; a byte past n_bytes, or whose source is no longer where the plan found it, is zero
CRR_HD void resume_gather_chunk(const Ctx& c, const ResumeIn& r, const ResumeWork& k, const ResumeTotals& T, uint64_t i,
                                uint64_t& lo, uint64_t& hi) {
  lo = hi = 0;
  const uint64_t seed_base = align16(T.blob_bytes);
  const uint64_t* ob = k.off(kResBlobBytes);
  const uint64_t* ok = k.off(kResKeyBytes);
  uint32_t p = 0;
  int region = -1;                 // the region p was found in
  ResumeSrc src = {0, 0, 0, 0};
  for (uint32_t b = 0; b < 16; ++b) {
    const uint64_t o = 16 * i + b;
    uint32_t v = 0;
    if (o >= T.n_bytes) break;
    if (o < T.blob_bytes) {
      if (region != 0 || o >= ob[p + 1]) {
        p = resume_find(ob, k.n_wf, o);
        region = 0;
        const uint32_t task = k.winner()[p];
        src = task == kResNoTask ? ResumeSrc{0, 0, 0, 0} : resume_src(r, task);
      }
      const uint64_t d = o - ob[p];
      if (d < src.n_bytes) v = r.tb_bytes[src.byte0 + d];
    } else if (o >= seed_base) {
      const uint64_t q = o - seed_base;
      if (region != 1 || q >= ok[p + 1]) {
        p = resume_find(ok, k.n_wf, q);
        region = 1;
      }
      const uint64_t d = q - ok[p];
      const int64_t k0 = c.cnt(CRR_LOAD_T_KEY_BYTES)[p], k1 = c.cnt(CRR_LOAD_T_KEY_BYTES)[p + 1];
      if (k0 >= 0 && k1 >= k0 && d < (uint64_t)(k1 - k0)) v = c.key_bytes()[(uint64_t)k0 + d];
    }
    if (b < 8) lo |= (uint64_t)v << (8 * b);
    else hi |= (uint64_t)v << (8 * (b - 8));
  }
}

// entry j of the gathered blob_off (j == n_blobs: the end of the last blob)
CRR_HD uint64_t resume_blob_off(const ResumeIn& r, const ResumeWork& k, const ResumeTotals& T, uint64_t j) {
  if (j >= T.n_blobs) return T.blob_bytes;
  const uint64_t* ob = k.off(kResBlobBytes);
  const uint32_t p = resume_find(k.off(kResBlobs), k.n_wf, j);
  const uint64_t jl = j - k.off(kResBlobs)[p], room = ob[p + 1] - ob[p];
  const uint32_t task = k.winner()[p];
  uint64_t rel = room;
  if (task != kResNoTask) {
    const ResumeSrc s = resume_src(r, task);
    if (jl < s.n_blobs) {
      const uint64_t o = r.tb_off[s.blob0 + jl];
      rel = o < s.byte0 ? 0 : o - s.byte0;
    }
  }
  return ob[p] + (rel < room ? rel : room);
}

// entry e of the gathered seeds: the loader's dictionary entry, its offset into the gathered bytes
CRR_HD void resume_key(const Ctx& c, const ResumeWork& k, const ResumeTotals& T, uint64_t e, uint64_t& off, uint32_t& len) {
  const uint64_t seed_base = align16(T.blob_bytes);
  off = seed_base;
  len = 0;
  const uint32_t p = resume_find(k.off(kResKeys), k.n_wf, e);
  const uint64_t j = e - k.off(kResKeys)[p];
  const int64_t e0 = c.cnt(CRR_LOAD_T_KEYS)[p], e1 = c.cnt(CRR_LOAD_T_KEYS)[p + 1];
  const int64_t k0 = c.cnt(CRR_LOAD_T_KEY_BYTES)[p], k1 = c.cnt(CRR_LOAD_T_KEY_BYTES)[p + 1];
  if (e0 < 0 || e1 < e0 || j >= (uint64_t)(e1 - e0) || k0 < 0 || k1 < k0) return;
  const uint64_t so = c.key_off()[(uint64_t)e0 + j], sl = c.key_len()[(uint64_t)e0 + j];
  const uint64_t room = k.off(kResKeyBytes)[p + 1] - k.off(kResKeyBytes)[p];
  if (so < (uint64_t)k0 || so - (uint64_t)k0 + sl > (uint64_t)(k1 - k0) || so - (uint64_t)k0 + sl > room) return;
  off = seed_base + k.off(kResKeyBytes)[p] + (so - (uint64_t)k0);
  len = (uint32_t)sl;
}

// position p of the gathered batch: the winning task's crr_blob_wf with its blob range rewritten
CRR_HD crr_blob_wf resume_blob_wf(const ResumeIn& r, const ResumeWork& k, uint32_t p) {
  crr_blob_wf o;
  memset(&o, 0, sizeof o);
  const uint32_t task = k.winner()[p];
  if (task != kResNoTask && task < r.tb_n_wf && r.tb_wf) o = r.tb_wf[task];
  else o.final_token_len = 0xFFFFFFFFu;
  const int32_t nr = (task != kResNoTask && task < r.tb_n_wf && r.tb_wf) ? o.new_run_wf : -1;
  o.new_run_wf = -1;
  // (only a task that may be applied bids, so winning its workflow says it is applied)
  if (nr >= 0 && (uint32_t)nr < r.n_tasks && r.tasks[nr].wf < k.n_wf && k.winner()[r.tasks[nr].wf] == (uint32_t)nr)
    o.new_run_wf = (int32_t)r.tasks[nr].wf;
  o.blob_begin = (uint32_t)k.off(kResBlobs)[p];
  o.blob_count = (uint32_t)(k.off(kResBlobs)[p + 1] - k.off(kResBlobs)[p]);
  return o;
}

// position p's capacities: the loaded rows (applied positions) plus this call's inserts
CRR_HD void resume_caps(const Ctx& c, const ResumeWork& k, const int32_t* counts, uint64_t stride, uint32_t p,
                        uint64_t cap[kResCaps]) {
  const bool applied = k.winner()[p] != kResNoTask;
  for (int t = 0; t < kResCaps; ++t) {
    const int32_t ins = counts[(uint64_t)(2 + t) * stride + p];
    const int64_t loaded = applied && t < 7 ? c.cnt(t)[p + 1] - c.cnt(t)[p] : 0;
    const uint64_t v = (uint64_t)(loaded > 0 ? loaded : 0) + (uint64_t)(ins > 0 ? ins : 0);
    cap[t] = v < 0x7FFFFFFFull ? v : 0x7FFFFFFFull;
  }
}

// position p's descriptor from its capacities and their exclusive prefixes; the loaded token goes to the arena
CRR_HD crr_workflow resume_descriptor(const Ctx& c, const ResumeWork& k, const crr_blob_wf* gathered_wf, const int32_t* counts,
                                      uint64_t stride, uint32_t p, const uint64_t cap[kResCaps], const uint64_t base[kResCaps],
                                      uint8_t* arena, uint64_t arena_capacity) {
  crr_workflow d;
  memset(&d, 0, sizeof d);
  const bool applied = k.winner()[p] != kResNoTask;
  const crr_blob_wf s = gathered_wf[p];
  // (a position without blobs applies nothing, whatever the counts' source says of a workflow without batches)
  d.ev_count = s.blob_count ? counts[p] : 0;
  d.empty_batch_at = s.blob_count ? counts[stride + p] : -1;
  d.init_version = s.init_version;
  d.now_ns = s.now_ns;
  d.final_token_len = 0xFFFFFFFFu;
  d.act_base = (int64_t)base[0];   d.act_cap = (int32_t)cap[0];
  d.timer_base = (int64_t)base[1]; d.timer_cap = (int32_t)cap[1];
  d.child_base = (int64_t)base[2]; d.child_cap = (int32_t)cap[2];
  d.rc_base = (int64_t)base[3];    d.rc_cap = (int32_t)cap[3];
  d.sig_base = (int64_t)base[4];   d.sig_cap = (int32_t)cap[4];
  d.vh_base = (int64_t)base[5];    d.vh_cap = (int32_t)cap[5];
  d.rp_base = (int64_t)base[6];    d.rp_cap = (int32_t)cap[6];
  d.task_base = (int64_t)base[7];  d.task_cap = (int32_t)cap[7];
  d.flags = (s.flags & (CRR_WF_FLAG_NEW_RUN | CRR_WF_FLAG_REFRESH_TASKS)) | (applied ? CRR_WF_FLAG_RESUME : 0);
  d.retention_days = s.retention_days;
  const uint64_t at = k.off(kResTokenBytes)[p], room = k.off(kResTokenBytes)[p + 1] - at;
  d.start_token_off = (uint32_t)at;
  if (applied && room && at + room <= arena_capacity) {
    const int64_t t0 = c.cnt(CRR_LOAD_T_TOKEN)[p], t1 = c.cnt(CRR_LOAD_T_TOKEN)[p + 1];
    const uint64_t len = t0 >= 0 && t1 >= t0 && (uint64_t)(t1 - t0) <= room ? (uint64_t)(t1 - t0) : 0;
    const uint8_t* src = c.tokens() + (len ? (uint64_t)t0 : 0);
    for (uint64_t q = 0; q < room; ++q) arena[at + q] = q < len ? src[q] : (uint8_t)0;
    d.start_token_len = (uint32_t)len;
  }
  return d;
}

inline void fill_summary(crr_load_summary* S, const Ctx& c, const int64_t* totals /* [kCounters] */, uint64_t err_blob,
                         uint64_t failed, uint64_t needed) {
  memset(S, 0, sizeof *S);
  S->n_failed = (uint32_t)failed;
  S->err_blob = err_blob == ~0ull ? -1 : (int64_t)err_blob;
  for (int t = 0; t < CRR_LOAD_TABLES; ++t) S->totals[t] = (uint64_t)totals[t];
  S->staging[0] = (uint64_t)totals[kCand];
  S->staging[1] = (uint64_t)totals[kCandBytes];
  S->scratch_needed = needed;
  S->n_blobs = c.in.n_blobs;
  S->n_wf = c.in.n_wf;
}

// the layout read / place rebuild from a plan's summary
inline Layout layout_of(const crr_load_summary& S) {
  uint64_t tot[kCounters];
  for (int t = 0; t < CRR_LOAD_TABLES; ++t) tot[t] = S.totals[t];
  tot[kCand] = S.staging[0];
  tot[kCandBytes] = S.staging[1];
  return carve(S.n_blobs, S.n_wf, tot);
}

}  // namespace crr_load
#endif  // CADENCE_LOAD_DECODE_H_
