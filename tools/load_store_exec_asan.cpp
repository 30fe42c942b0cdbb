// load_store_exec_asan.cpp -- a stand-alone check of the host restatement of the execution blob generated for
// routed replication tasks (crr_load_store_exec_host, include/cadence_load_store_exec.h) under AddressSanitizer /
// UndefinedBehaviorSanitizer, in the style of load_store_vh_asan.cpp.  Hand-written states -- a Go-shaped blob with a
// sticky task list, client strings, a list and a map; one that holds field 18; a sparse one; one out of ascending
// order; one with an overridden field of another type; one whose stored blob is truncated (the loader refuses it) --
// hand-made decisions, and post-replay rows written by hand, a failed replay and counts no table holds among them.
// Each batch's bytes, the task blobs, every input array, every buffer of the post-replay image and every output (the
// rows, the offsets, and `out` at exactly n_bytes) lie in a heap block of exactly their size, so a read or a write
// past any of them is reported.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/load_store_exec_asan.cpp cadence_amd/csrc/load_states.cpp -o build/load_store_exec_asan -lpthread
//   build/load_store_exec_asan
//
// Exit status 0 and a line of counts when every row and every blob equals what the splicer written in this file
// gives and no sanitizer report ended the run.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "cadence_load_store_exec.h"

#include "load_asan_common.h"

namespace {

const int64_t kGoZero = -6795364578871345152LL;

// one top-level field: its thrift type and its value's bytes as they lie in the blob
struct Field {
  int16_t id;
  uint8_t type;
  std::string value;
};
Field f_i64(int16_t id, int64_t v) { Wr w; w.be((uint64_t)v, 8); return {id, 10, w.b}; }
Field f_i32(int16_t id, int32_t v) { Wr w; w.be((uint32_t)v, 4); return {id, 8, w.b}; }
Field f_bool(int16_t id, bool v) { return {id, 2, std::string(1, (char)(v ? 1 : 0))}; }
Field f_str(int16_t id, const std::string& s) { Wr w; w.be(s.size(), 4); return {id, 11, w.b + s}; }
Field f_list(int16_t id, const std::vector<std::string>& v) {
  Wr w;
  w.u8(11), w.be(v.size(), 4);
  for (auto& s : v) w.be(s.size(), 4), w.b += s;
  return {id, 15, w.b};
}
Field f_map(int16_t id, const std::map<std::string, std::string>& m) {
  Wr w;
  w.u8(11), w.u8(11), w.be(m.size(), 4);
  for (auto& kv : m) w.be(kv.first.size(), 4), w.b += kv.first, w.be(kv.second.size(), 4), w.b += kv.second;
  return {id, 13, w.b};
}
std::string encode(const std::vector<Field>& fs) {
  Wr w;
  for (auto& f : fs) w.field(f.type, f.id), w.b += f.value;
  w.u8(0);
  return w.b;
}

// ---- this file's own splicer: the header's rules over the field list ---------------------------------------------
struct Override {
  bool omit;
  Field f;
};
std::string splice(const std::vector<Field>& stored, const std::map<int16_t, Override>& over) {
  std::map<int16_t, bool> present;
  for (auto& f : stored) present[f.id] = true;
  std::map<int16_t, bool> inserted;
  std::vector<Field> out;
  auto insert_below = [&](int limit) {
    for (auto& kv : over)
      if (!kv.second.omit && !present.count(kv.first) && !inserted.count(kv.first) && kv.first < limit) {
        out.push_back(kv.second.f);
        inserted[kv.first] = true;
      }
  };
  for (auto& f : stored) {
    insert_below(f.id);
    auto it = over.find(f.id);
    if (it == over.end()) out.push_back(f);
    else if (!it->second.omit) out.push_back(it->second.f);
  }
  insert_below(0x10000);
  return encode(out);
}

std::string vh_blob(const std::string& token, const std::vector<std::pair<int64_t, int64_t>>& items) {
  Wr w;
  w.u8(0x59), w.i32(10, 0), w.field(15, 20), w.u8(12), w.be(1, 4);
  w.str(10, token), w.field(15, 20), w.u8(12), w.be(items.size(), 4);
  for (auto& it : items) w.i64(10, it.first), w.i64(20, it.second), w.u8(0);
  w.u8(0), w.u8(0);
  return w.b;
}

struct State {
  std::vector<Field> fields;
  bool truncated;
};

const std::vector<std::pair<int64_t, int64_t>> kItems = {{5, 1}, {19, 3}};

std::vector<Field> go_shaped(bool with18, const std::string& request) {
  std::vector<Field> f = {f_str(12, ""), f_i64(16, -23)};
  if (with18) f.push_back(f_i64(18, 17));
  std::vector<Field> rest = {
      f_str(22, ""), f_str(24, "task-list"), f_str(26, "workflow-type"), f_i32(28, 3600), f_i32(30, 10), f_str(32, "ctx"),
      f_i32(34, 1), f_i32(36, 0), f_i64(38, 0), f_i64(48, 777), f_i64(50, 18), f_i64(52, 15), f_i64(54, 1600000000000000000LL),
      f_i64(56, 1600000000500000000LL), f_i64(58, 3), f_i64(60, 18), f_i64(62, -23), f_i32(64, 10), f_i64(66, 0),
      f_i64(68, kGoZero), f_i64(69, 1600000000000000123LL), f_bool(70, false), f_i64(71, 1600000000000000123LL),
      f_str(72, "create-request"), f_str(74, request), f_str(76, ""), f_str(78, "sticky-task-list"), f_i64(80, 5), f_i64(82, 0),
      f_list(96, {"bad-input", "worse"}), f_bool(98, true), f_str(104, "branch-token"), f_i64(106, 2), f_i64(108, 4096),
      f_str(110, "1.7.0"), f_str(112, "1.7.0"), f_str(114, "uber-go"), f_str(116, "thriftrw"),
      f_map(118, {{"CustomKeywordField", "\"v\""}}), f_map(120, {{"note", "memo"}}), f_str(122, vh_blob("branch-token", kItems)),
      f_str(124, "thriftrw")};
  f.insert(f.end(), rest.begin(), rest.end());
  return f;
}

struct Task {
  uint32_t wf;
  int32_t route, action;
  int64_t id, version, now, delta;
  int32_t outcome, status;
  uint32_t flags;
};

std::map<int16_t, Override> overrides(const Task& t, const crr_exec_row& R, const std::vector<Field>& stored,
                                      const std::string& vh, int rq_mode, const std::string& rq) {
  std::map<int16_t, Override> o;
  int64_t hist = 0;
  for (auto& f : stored)
    if (f.id == 108) {
      uint64_t v = 0;
      for (char c : f.value) v = (v << 8) | (uint8_t)c;
      hist = (int64_t)v;
    }
  o[56] = {false, f_i64(56, t.now)};
  o[108] = {false, f_i64(108, (int64_t)((uint64_t)hist + (uint64_t)t.delta))};
  o[122] = {false, f_str(122, vh)};
  if (t.outcome != CRR_STORE_APPLIED) return o;
  auto nano = [](int64_t v) { return v == CRR_ZERO_TIME ? kGoZero : v; };
  o[18] = {R.completion_event_batch_id == CRR_EMPTY_EVENT_ID, f_i64(18, R.completion_event_batch_id)};
  o[34] = {false, f_i32(34, R.state)}, o[36] = {false, f_i32(36, R.close_status)};
  o[48] = {false, f_i64(48, R.last_event_task_id)}, o[50] = {false, f_i64(50, R.last_first_event_id)};
  o[52] = {false, f_i64(52, R.last_processed_event)}, o[58] = {false, f_i64(58, R.decision_version)};
  o[60] = {false, f_i64(60, R.decision_schedule_id)}, o[62] = {false, f_i64(62, R.decision_started_id)};
  o[64] = {false, f_i32(64, R.decision_timeout)}, o[66] = {false, f_i64(66, R.decision_attempt)};
  o[68] = {false, f_i64(68, nano(R.decision_started_ts))}, o[69] = {false, f_i64(69, nano(R.decision_scheduled_ts))};
  o[70] = {false, f_bool(70, (R.flags & CRR_EXEC_CANCEL_REQUESTED) != 0)};
  o[71] = {false, f_i64(71, nano(R.decision_orig_scheduled_ts))}, o[106] = {false, f_i64(106, R.signal_count)};
  o[78] = {false, f_str(78, "")}, o[80] = {false, f_i64(80, 0)};
  o[110] = {false, f_str(110, "")}, o[112] = {false, f_str(112, "")}, o[114] = {false, f_str(114, "")};
  if (rq_mode >= 0) o[74] = {false, f_str(74, rq)};
  return o;
}

int run(int threads, int* blobs_checked, uint64_t* bytes_checked, unsigned* flags_seen, unsigned* outcomes_seen) {
  // states: 0 Go-shaped, 1 Go-shaped with field 18 and a stored request id, 2 sparse, 3 out of order, 4 field 56 as an
  // i32, 5 truncated, 6 Go-shaped (the failed replay), 7 Go-shaped (the request id from the task)
  std::vector<State> states = {
      {go_shaped(false, "emptyUuid"), false},
      {go_shaped(true, "a-stored-request-id"), false},
      {{f_str(124, "thriftrw"), f_str(122, vh_blob("t", kItems)), f_i32(30, 10)}, false},
      {{f_str(24, "tl"), f_i64(108, 50), f_i64(56, 111), f_str(124, "thriftrw"), f_str(9, "x"), f_str(122, vh_blob("", kItems)), f_i64(48, 5)}, false},
      {{f_i32(56, 1), f_str(122, vh_blob("t", kItems)), f_str(124, "thriftrw")}, false},
      {go_shaped(false, "emptyUuid"), true},
      {go_shaped(false, "emptyUuid"), false},
      {go_shaped(false, "emptyUuid"), false},
  };
  const uint32_t n_wf = (uint32_t)states.size();
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off{0};
  std::vector<crr_state_blob> meta;
  std::vector<crr_state_wf> wf;
  for (auto& s : states) {
    std::string b = encode(s.fields);
    if (s.truncated) b.resize(b.size() - 9);
    wf.push_back({(uint32_t)meta.size(), 1, 20});
    bytes.insert(bytes.end(), b.begin(), b.end());
    off.push_back(bytes.size());
    meta.push_back({CRR_STATE_EXECUTION, 0, 0, 0, 0});
  }
  std::vector<uint8_t> strings = {'s'};
  const StateBatch batch(bytes, off, meta, wf, strings);
  const crr_state_batch& in = batch.in;

  // the after-image: exec rows by hand; the current branch's items per workflow; no pending rows at all, although
  // workflow 0's counts claim INT_MAX of everything (clamped to the tables' zero rows)
  std::vector<crr_exec_row> ex(n_wf);
  std::vector<int64_t> offsets((size_t)CRR_LOAD_TABLES * (n_wf + 1), 0);
  std::vector<int32_t> status(n_wf, 0);
  std::vector<crr_vh_item> vh;
  const std::vector<std::pair<int64_t, int64_t>> after_items = {{5, 1}, {26, 3}};
  for (uint32_t w = 0; w < n_wf; ++w) {
    crr_exec_row& R = ex[w];
    memset(&R, 0, sizeof R);
    R.state = 1, R.next_event_id = 27, R.last_first_event_id = 24, R.last_event_task_id = 900 + w, R.last_processed_event = 20;
    R.completion_event_batch_id = w == 1 ? 24 : CRR_EMPTY_EVENT_ID;
    R.decision_version = 4, R.decision_schedule_id = 23, R.decision_started_id = 24, R.decision_timeout = 12;
    R.decision_attempt = 1, R.decision_started_ts = 1600000000777000000LL, R.decision_scheduled_ts = 1600000000666000000LL;
    R.decision_orig_scheduled_ts = CRR_ZERO_TIME, R.signal_count = 3, R.flags = CRR_EXEC_CANCEL_REQUESTED | CRR_EXEC_RESET_POINTS_SET;
    R.decision_request_src = w == 1 ? 0 : w == 7 ? 1 + 1 : w == 2 ? CRR_SRC_NONE : CRR_SRC_EMPTY_UUID;
    R.src_next = 1;
    if (w == 6) R.status = 7;
    if (w == 0) R.n_activity = R.n_timer = R.n_child = R.n_rc = R.n_signal = R.n_reset_points = INT_MAX;
    offsets[5 * (n_wf + 1) + w] = (int64_t)vh.size();
    R.n_vh_items = w == 0 ? INT_MAX : (int32_t)after_items.size();
    for (auto& it : after_items) vh.push_back({it.first, it.second});
  }
  offsets[5 * (n_wf + 1) + n_wf] = (int64_t)vh.size();
  Image img;
  img.exec = exact(ex), img.offsets = exact(offsets), img.status = exact(status);
  img.rows[5] = exact(vh);
  for (int t = 0; t < 7; ++t)
    if (t != 5) img.rows[t] = malloc(0);

  // the task blobs: workflow 7 carries [ActivityTaskStarted, DecisionTaskStarted{request id}] behind an empty blob
  const std::string request = "the-task's-decision-request-id";
  Wr tb;
  tb.u8(0x59), tb.field(15, 10), tb.u8(12), tb.be(2, 4);
  tb.i64(10, 25), tb.i32(30, 11), tb.field(12, 150), tb.i64(10, 5), tb.str(30, "not-this-one"), tb.u8(0), tb.u8(0);
  tb.i64(10, 26), tb.i32(30, 5), tb.field(12, 90), tb.i64(10, 25), tb.str(20, "identity"), tb.str(30, request), tb.u8(0), tb.u8(0);
  tb.u8(0);
  std::vector<uint8_t> tbytes(tb.b.begin(), tb.b.end());
  std::vector<uint64_t> toff = {0, 0, tbytes.size()};
  std::vector<crr_blob_wf> twf(n_wf);
  memset(twf.data(), 0, twf.size() * sizeof(crr_blob_wf));
  for (uint32_t w = 0; w < n_wf; ++w) twf[w].blob_count = w == 7 ? 2 : 0;
  uint8_t* d_tbytes = exact(tbytes);
  uint64_t* d_toff = exact(toff);
  crr_blob_wf* d_twf = exact(twf);
  crr_blob_batch tbatch;
  memset(&tbatch, 0, sizeof tbatch);
  tbatch.bytes = d_tbytes, tbatch.blob_off = d_toff, tbatch.n_blobs = 2, tbatch.n_wf = n_wf, tbatch.wf = d_twf;
  std::vector<uint8_t> upserts(n_wf, 0);
  uint8_t* d_upserts = exact(upserts);

  const int32_t A = CRR_ROUTE_APPLY_CURRENT, N = CRR_ROUTE_NON_CURRENT, APP = CRR_NDC_APPEND;
  const int32_t GA = CRR_STORE_APPLIED, GB = CRR_STORE_BACKFILLED;
  std::vector<Task> tasks = {
      {0, A, APP, 26, 3, 1700000000000000001LL, 100, GA, 0, 0},              // garbage counts, clamped
      {1, A, APP, 26, 3, kGoZero, -96, GA, 0, 0},                            // field 18 patched, 74 as stored
      {2, A, APP, 26, 3, 1700000000000000003LL, 7, GA, 0, 0},                // nearly everything inserted
      {3, N, APP, 25, 3, 1700000000000000004LL, 7, GB, 0, 0},                // out of order, patched in place
      {4, N, APP, 25, 3, 1700000000000000005LL, 7, GB, 0, CRR_EXEC_BLOB_HOST_STORED_SHAPE},
      {5, N, APP, 25, 3, 1700000000000000006LL, 7, CRR_STORE_NOT_LOADED, 0, 0},   // the truncated blob
      {6, A, APP, 26, 3, 1700000000000000007LL, 7, CRR_STORE_REPLAY_FAILED, 7, 0},
      {7, A, APP, 26, 3, 1700000000000000008LL, 7, GA, 0, 0},                // the request id from the task's blob
      {0, CRR_ROUTE_REBUILD, APP, 26, 3, 1, 1, CRR_STORE_NO_ROUTE, 0, 0},
      {0, N, CRR_NDC_NEW_BRANCH, 26, 3, 1, 1, CRR_STORE_NEW_BRANCH, 0, 0},
      {0, N, APP, 4, 3, 1, 1, CRR_STORE_VH_ERROR, CRR_ERR_VH_EVENT_ID_NOT_INCREASING, 0},
      {2, N, APP, 25, 7, 1700000000000000009LL, -4000, GB, 0, 0},            // a generated task last
  };
  const uint32_t n = (uint32_t)tasks.size();
  int bad = 0;
  for (int with_blobs = 1; with_blobs >= 0 && !bad; --with_blobs) {
    std::vector<std::string> want(n);
    std::vector<Task> exp = tasks;
    for (uint32_t k = 0; k < n; ++k) {
      Task& t = exp[k];
      if (t.outcome != GA && t.outcome != GB) continue;
      if (t.flags) continue;
      const State& s = states[t.wf];
      std::string token;
      for (auto& f : s.fields)
        if (f.id == 122) {   // the token of the one stored branch: the first string of the blob's history
          const std::string& v = f.value;
          const size_t at = 4 + 1 + 7 + 8 + 3;
          const size_t len = ((uint8_t)v[at] << 24) | ((uint8_t)v[at + 1] << 16) | ((uint8_t)v[at + 2] << 8) | (uint8_t)v[at + 3];
          token = v.substr(at + 4, len);
        }
      auto items = kItems;
      if (t.outcome == GA) items = after_items;
      else if (t.version > items.back().second) items.push_back({t.id, t.version});
      else items.back().first = t.id;
      int rq_mode = -1;
      std::string rq;
      const int32_t src = ex[t.wf].decision_request_src;
      if (t.outcome == GA) {
        if (src == CRR_SRC_EMPTY_UUID) rq_mode = 0, rq = "emptyUuid";
        else if (src == CRR_SRC_NONE) rq_mode = 1;
        else if (src >= 1) {
          if (with_blobs) rq_mode = 2, rq = request;
          else {
            t.flags = CRR_EXEC_BLOB_HOST_REQUEST_ID;
            continue;
          }
        }
      }
      want[k] = splice(s.fields, overrides(t, ex[t.wf], s.fields, vh_blob(token, items), rq_mode, rq));
    }
    std::vector<crr_repl_task> rt(n);
    std::vector<crr_last_event> le(n);
    std::vector<crr_ndc_result> res(n);
    std::vector<crr_ndc_route> routes(n);
    std::vector<crr_exec_blob_task> xt(n);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n; ++k) {
      memset(&rt[k], 0, sizeof rt[k]), memset(&res[k], 0, sizeof res[k]), memset(&routes[k], 0, sizeof routes[k]);
      rt[k].wf = tasks[k].wf;
      le[k] = {tasks[k].id, tasks[k].version};
      res[k].action = tasks[k].action, res[k].branch_index = 0;
      routes[k].route = tasks[k].route;
      xt[k] = {tasks[k].now, tasks[k].delta};
      total += want[k].size();
    }
    crr_repl_task* d_rt = exact(rt);
    crr_last_event* d_le = exact(le);
    crr_ndc_result* d_res = exact(res);
    crr_ndc_route* d_routes = exact(routes);
    crr_exec_blob_task* d_xt = exact(xt);
    const crr_blob_batch* blobs = with_blobs ? &tbatch : nullptr;
    crr_exec_blob_sizes P;
    int rc = crr_load_store_exec_host(&in, d_rt, d_le, n, d_res, d_routes, &img, d_xt, blobs, d_upserts, nullptr, nullptr, nullptr, 0, &P, 1);
    bad = rc != 0 || P.n_bytes != total || P.n_tasks != n;
    if (bad) fprintf(stderr, "sizing call: rc %d, %llu bytes for %llu expected\n", rc, (unsigned long long)P.n_bytes, (unsigned long long)total);
    crr_exec_blob_row* rows = static_cast<crr_exec_blob_row*>(malloc(n * sizeof(crr_exec_blob_row)));
    uint64_t* blob_off = static_cast<uint64_t*>(malloc(((size_t)n + 1) * sizeof(uint64_t)));
    uint8_t* out = static_cast<uint8_t*>(malloc((size_t)total));
    if (!bad) {   // one byte short: refused, nothing touched
      memset(out, 0xA5, (size_t)total);
      rc = crr_load_store_exec_host(&in, d_rt, d_le, n, d_res, d_routes, &img, d_xt, blobs, d_upserts, rows, blob_off, out, (size_t)total - 1, &P, 1);
      for (size_t i = 0; i < total; ++i) bad |= out[i] != 0xA5;
      if (rc != -1 || bad) fprintf(stderr, "a capacity one byte short: rc %d, buffer %s\n", rc, bad ? "written" : "intact"), bad = 1;
    }
    if (!bad) {
      rc = crr_load_store_exec_host(&in, d_rt, d_le, n, d_res, d_routes, &img, d_xt, blobs, d_upserts, rows, blob_off, out, (size_t)total, &P, threads);
      bad = rc != 0;
      if (bad) fprintf(stderr, "crr_load_store_exec_host: %d\n", rc);
    }
    uint64_t at = 0;
    for (uint32_t k = 0; k < n && !bad; ++k) {
      const crr_exec_blob_row& g = rows[k];
      const Task& e = exp[k];
      const bool gen = e.outcome == GA || e.outcome == GB;
      const int64_t nei = !gen ? 0 : e.outcome == GA ? 27 : 20;
      if (g.len != want[k].size() || g.outcome != e.outcome || g.status != e.status || g.flags != e.flags || g.next_event_id != nei ||
          blob_off[k] != at || (g.len && memcmp(out + at, want[k].data(), g.len) != 0)) {
        fprintf(stderr, "task %u (wf %u, blobs %d): got len %u outcome %d status %d flags %u nei %lld at %llu, expected %zu/%d/%d/%u/%lld at %llu (or other bytes)\n",
                k, e.wf, with_blobs, g.len, g.outcome, g.status, g.flags, (long long)g.next_event_id, (unsigned long long)blob_off[k],
                want[k].size(), e.outcome, e.status, e.flags, (long long)nei, (unsigned long long)at);
        bad = 1;
      }
      at += want[k].size();
      *blobs_checked += g.len != 0;
      *flags_seen |= g.flags;
      *outcomes_seen |= 1u << g.outcome;
    }
    if (!bad && blob_off[n] != total) bad = 1;
    *bytes_checked += total;
    free(rows), free(blob_off), free(out);
    free(d_rt), free(d_le), free(d_res), free(d_routes), free(d_xt);
  }
  // no tasks at all
  if (!bad) {
    crr_exec_blob_sizes P;
    uint64_t one_off = 7;
    bad = crr_load_store_exec_host(&in, nullptr, nullptr, 0, nullptr, nullptr, &img, nullptr, nullptr, nullptr, nullptr, &one_off, nullptr, 0, &P, 1) != 0 ||
          P.n_bytes != 0 || one_off != 0;
  }
  free(d_tbytes), free(d_toff), free(d_twf), free(d_upserts);
  return bad;
}

}  // namespace

int main() {
  int blobs = 0;
  uint64_t bytes = 0;
  unsigned flags = 0, outcomes = 0;
  for (int threads : {1, 3})
    if (run(threads, &blobs, &bytes, &flags, &outcomes)) return 1;
  const unsigned want_flags = CRR_EXEC_BLOB_HOST_STORED_SHAPE | CRR_EXEC_BLOB_HOST_REQUEST_ID;
  const unsigned want_outcomes = (1u << CRR_STORE_APPLIED) | (1u << CRR_STORE_BACKFILLED) | (1u << CRR_STORE_NOT_LOADED) |
                                 (1u << CRR_STORE_NO_ROUTE) | (1u << CRR_STORE_NEW_BRANCH) | (1u << CRR_STORE_VH_ERROR) |
                                 (1u << CRR_STORE_REPLAY_FAILED);
  if ((flags & want_flags) != want_flags || (outcomes & want_outcomes) != want_outcomes) {
    fprintf(stderr, "flags reached: %x, outcomes reached: %x\n", flags, outcomes);
    return 1;
  }
  printf("load_store_exec_asan: %d blobs as this file's splicer gives them, %llu bytes, a failed replay, garbage counts and a "
         "truncated stored blob among the inputs, no sanitizer report\n", blobs, (unsigned long long)bytes);
  return 0;
}
