// load_mutation_asan.cpp -- a stand-alone check of the host restatement of the pending-entry mutation of committed
// replication tasks (crr_load_mutation_host, include/cadence_load_mutation.h) under AddressSanitizer /
// UndefinedBehaviorSanitizer.  Hand-written states with zero to several entries in every pending map are loaded by
// crr_load_states_host; the states after are made from that image by a rule of this file (keep, change a persisted
// field, change a derived field only, delete, add, restart a TimerID), and the result is compared with a classifier
// of this file's own, which matches the rows by key through std::map and compares them field by field.  Every
// input array, every buffer of the after-image and every output buffer lies in a heap block of exactly its size, so
// a read or a write past any of them is reported.  Some exec rows of the after-image carry a failed status or counts
// no table holds: the counts are clamped to what the image holds for the workflow.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/load_mutation_asan.cpp cadence_amd/csrc/load_states.cpp -o build/load_mutation_asan -lpthread
//   build/load_mutation_asan
//
// Exit status 0 and a line of counts when every row, gathered row and key equals this file's and no sanitizer report
// ended the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "cadence_load_mutation.h"

#include "load_asan_common.h"

namespace {

std::string execution_blob(int n_points) {
  Wr vh;
  vh.u8(0x59), vh.i32(10, 0), vh.list(20, 12, 1);
  vh.str(10, "token"), vh.list(20, 12, 1), vh.i64(10, 19), vh.i64(20, 3), vh.stop(), vh.stop(), vh.stop();
  Wr rp;
  rp.u8(0x59), rp.list(10, 12, (size_t)n_points);
  for (int i = 0; i < n_points; ++i) rp.str(10, "bin-" + std::to_string(i)), rp.stop();
  rp.stop();
  Wr w;
  w.i32(34, 1), w.i64(50, 18), w.i64(52, 15), w.i64(58, 3), w.i64(60, 18), w.i64(62, -23), w.i64(106, 2);
  w.str(115, rp.b), w.str(116, "thriftrw"), w.str(122, vh.b), w.str(124, "thriftrw");
  w.stop();
  return w.b;
}

// ---- this file's own comparison of the persisted fields, by name ------------------------------------------------
bool same(const crr_activity_row& a, const crr_activity_row& b) {
  return a.schedule_id == b.schedule_id && a.version == b.version && a.scheduled_batch_id == b.scheduled_batch_id &&
         a.scheduled_time == b.scheduled_time && a.started_id == b.started_id && a.started_time == b.started_time &&
         a.cancel_request_id == b.cancel_request_id && a.sched_src == b.sched_src && a.started_src == b.started_src &&
         a.schedule_to_start == b.schedule_to_start && a.schedule_to_close == b.schedule_to_close &&
         a.start_to_close == b.start_to_close && a.heartbeat == b.heartbeat && a.timer_task_status == b.timer_task_status &&
         a.key == b.key && (a.flags & ~CRR_ROW_MAPPED) == (b.flags & ~CRR_ROW_MAPPED) && a.attempt == b.attempt &&
         a.last_heartbeat_time == b.last_heartbeat_time;
}
bool same(const crr_timer_row& a, const crr_timer_row& b) {
  return a.started_id == b.started_id && a.version == b.version && a.expiry_time == b.expiry_time && a.task_status == b.task_status &&
         a.key == b.key && a.src == b.src && a.flags == b.flags;
}
bool same(const crr_child_row& a, const crr_child_row& b) {
  return a.initiated_id == b.initiated_id && a.version == b.version && a.initiated_batch_id == b.initiated_batch_id &&
         a.started_id == b.started_id && a.src == b.src && a.started_src == b.started_src && a.flags == b.flags;
}
bool same(const crr_initiated_row& a, const crr_initiated_row& b) {
  return a.initiated_id == b.initiated_id && a.version == b.version && a.initiated_batch_id == b.initiated_batch_id &&
         a.src == b.src && a.flags == b.flags;
}
int64_t key_of(const crr_activity_row& r) { return r.schedule_id; }
int64_t key_of(const crr_timer_row& r) { return (int64_t)r.key; }
int64_t key_of(const crr_child_row& r) { return r.initiated_id; }
int64_t key_of(const crr_initiated_row& r) { return r.initiated_id; }

template <class Row>
void classify(const std::vector<Row>& before, const std::vector<Row>& after, std::vector<Row>& ups, std::vector<int64_t>& dels) {
  std::map<int64_t, const Row*> old, now;
  for (auto& r : before) old[key_of(r)] = &r;
  for (auto& r : after) now[key_of(r)] = &r;
  for (auto& r : after) {
    auto it = old.find(key_of(r));
    if (it == old.end() || !same(*it->second, r)) ups.push_back(r);
  }
  for (auto& r : before)
    if (!now.count(key_of(r))) dels.push_back(key_of(r));
}

// the state after from the state before, by position: 0 kept, 1 a persisted field changed, 2 a derived field only,
// 3 deleted; then `add` new rows above every ID; timers: a deleted row of position 3 mod 8 is started again
void derive(std::vector<crr_activity_row>& v, int64_t top, int add, uint32_t next_key, int salt) {
  std::vector<crr_activity_row> out;
  for (size_t i = 0; i < v.size(); ++i) {
    crr_activity_row r = v[i];
    const int rule = (int)((i + salt) % 4);
    if (rule == 3) continue;
    if (rule == 1) r.started_id = top + 100 + (int64_t)i, r.started_src = 40;
    if (rule == 2) r.flags ^= CRR_ROW_MAPPED, r.last_hb_timeout_vis_s = 9;
    out.push_back(r);
  }
  for (int k = 0; k < add; ++k) {
    crr_activity_row r;
    memset(&r, 0, sizeof r);
    r.schedule_id = top + 1 + k, r.version = 3, r.key = next_key + (uint32_t)k, r.flags = CRR_ROW_LIVE, r.sched_src = 41 + k, r.started_src = -1;
    out.push_back(r);
  }
  v = out;
}
void derive(std::vector<crr_timer_row>& v, int64_t top, int add, uint32_t next_key, int salt) {
  std::vector<crr_timer_row> out, again;
  for (size_t i = 0; i < v.size(); ++i) {
    crr_timer_row r = v[i];
    const int rule = (int)((i + salt) % 4);
    if (rule == 3) {
      if ((i + salt) % 8 == 3) r.started_id = top + 50 + (int64_t)i, r.src = 42, again.push_back(r);   // the same TimerID
      continue;
    }
    if (rule == 1) r.task_status ^= 1;
    out.push_back(r);
  }
  for (int k = 0; k < add; ++k) {
    crr_timer_row r;
    memset(&r, 0, sizeof r);
    r.started_id = top + 1 + k, r.version = 3, r.key = next_key + 16 + (uint32_t)k, r.flags = CRR_ROW_LIVE, r.src = 43 + k;
    out.push_back(r);
  }
  out.insert(out.end(), again.begin(), again.end());   // (top + 50 + i: above the added rows, ascending in i)
  v = out;
}
void derive(std::vector<crr_child_row>& v, int64_t top, int add, uint32_t, int salt) {
  std::vector<crr_child_row> out;
  for (size_t i = 0; i < v.size(); ++i) {
    crr_child_row r = v[i];
    const int rule = (int)((i + salt) % 4);
    if (rule == 3) continue;
    if (rule == 1) r.started_id = top + 100 + (int64_t)i, r.started_src = 44;
    if (rule == 2) r.reserved = 7;
    out.push_back(r);
  }
  for (int k = 0; k < add; ++k) {
    crr_child_row r;
    memset(&r, 0, sizeof r);
    r.initiated_id = top + 1 + k, r.version = 3, r.started_id = -23, r.flags = CRR_ROW_LIVE, r.src = 45 + k, r.started_src = -1;
    out.push_back(r);
  }
  v = out;
}
void derive(std::vector<crr_initiated_row>& v, int64_t top, int add, uint32_t, int salt) {
  std::vector<crr_initiated_row> out;
  for (size_t i = 0; i < v.size(); ++i) {
    crr_initiated_row r = v[i];
    const int rule = (int)((i + salt) % 4);
    if (rule == 3) continue;
    if (rule == 1) r.version += 1;
    out.push_back(r);
  }
  for (int k = 0; k < add; ++k) {
    crr_initiated_row r;
    memset(&r, 0, sizeof r);
    r.initiated_id = top + 1 + k, r.version = 3, r.flags = CRR_ROW_LIVE, r.src = 46 + k;
    out.push_back(r);
  }
  v = out;
}

struct Expect {
  std::vector<crr_exec_row> exec;
  std::vector<crr_activity_row> act;
  std::vector<crr_timer_row> timer;
  std::vector<crr_child_row> child;
  std::vector<crr_initiated_row> rc, sig;
  std::vector<int64_t> del[CRR_MUTATION_MAPS];
};

template <class Row>
std::vector<Row> slice(const void* rows, const int64_t* off, uint32_t w) {
  const Row* p = static_cast<const Row*>(rows);
  return std::vector<Row>(p + off[w], p + off[w + 1]);
}

int fail(const char* what, long a = 0, long b = 0) {
  fprintf(stderr, "load_mutation_asan: %s (%ld, %ld)\n", what, a, b);
  return 1;
}

// one batch of n_wf states, workflow w with (w + shape) % 5 entries per pending map
int check(uint32_t n_wf, int shape, int* n_rows) {
  std::vector<uint8_t> bytes, strings;
  std::vector<uint64_t> off{0};
  std::vector<crr_state_blob> meta;
  std::vector<crr_state_wf> wf;
  auto add = [&](uint32_t kind, int64_t id, const std::string& name, const std::string& b) {
    bytes.insert(bytes.end(), b.begin(), b.end());
    off.push_back(bytes.size());
    meta.push_back({kind, kind == CRR_STATE_TIMER ? (uint32_t)name.size() : 0u, id, 0, strings.size()});
    if (kind == CRR_STATE_TIMER) strings.insert(strings.end(), name.begin(), name.end());
  };
  for (uint32_t w = 0; w < n_wf; ++w) {
    const int n = (int)((w + shape) % 5);
    const uint32_t first = (uint32_t)meta.size();
    for (int i = n - 1; i >= 0; --i) {   // out of ID order
      Wr a, t, c, r;
      a.i64(10, 3), a.i64(20, -23), a.str(28, "act-" + std::to_string(i)), a.stop();
      add(CRR_STATE_ACTIVITY, 5 + 10 * i, "", a.b);
      t.i64(10, 3), t.i64(12, 6 + 10 * i), t.i64(16, 1), t.stop();
      add(CRR_STATE_TIMER, 0, "timer-" + std::to_string(i), t.b);
      c.i64(10, 3), c.i64(12, 6 + 10 * i), c.i64(14, -23), c.stop();
      add(CRR_STATE_CHILD, 7 + 10 * i, "", c.b);
      r.i64(10, 3), r.i64(11, 7 + 10 * i), r.stop();
      add(CRR_STATE_REQUEST_CANCEL, 8 + 10 * i, "", r.b);
      add(CRR_STATE_SIGNAL, 9 + 10 * i, "", r.b);
    }
    add(CRR_STATE_EXECUTION, 0, "", execution_blob((int)(w % 3)));
    wf.push_back({first, (uint32_t)meta.size() - first, 60});
  }
  bytes.resize(bytes.size() + 32, 0);   // readable CRR_INGEST_PAD bytes past the last blob, as the interface asks
  const StateBatch batch(bytes, off, meta, wf, strings);
  const crr_state_batch& in = batch.in;

  // the image before, by the loader
  crr_load_summary S;
  if (crr_load_states_host(&in, nullptr, &S, 1) != 0) return fail("sizing the load");
  Image B;
  const size_t row_bytes[7] = {sizeof(crr_activity_row), sizeof(crr_timer_row), sizeof(crr_child_row), sizeof(crr_initiated_row),
                               sizeof(crr_initiated_row), sizeof(crr_vh_item), sizeof(crr_reset_point_row)};
  B.exec = static_cast<crr_exec_row*>(malloc(n_wf * sizeof(crr_exec_row)));
  for (int t = 0; t < 7; ++t) B.rows[t] = malloc((size_t)S.totals[t] * row_bytes[t]);
  B.offsets = static_cast<int64_t*>(malloc((size_t)CRR_LOAD_TABLES * (n_wf + 1) * sizeof(int64_t)));
  B.status = static_cast<int32_t*>(malloc(n_wf * sizeof(int32_t)));
  if (crr_load_states_host(&in, &B, &S, 1) != 0 || S.n_failed != 0) return fail("the load", S.n_failed);
  auto offs = [&](int t) { return B.offsets + (size_t)t * (n_wf + 1); };

  // the image after, and what this file expects of it: one task per workflow in reverse order, then three others
  std::vector<crr_exec_row> ex(B.exec, B.exec + n_wf);
  std::vector<crr_activity_row> act;
  std::vector<crr_timer_row> timer;
  std::vector<crr_child_row> child;
  std::vector<crr_initiated_row> rc, sig;
  std::vector<crr_vh_item> vh;
  std::vector<crr_reset_point_row> rp;
  std::vector<int64_t> o2((size_t)CRR_LOAD_TABLES * (n_wf + 1), 0);
  struct Per {
    Expect e;
    uint32_t flags;
    int32_t outcome, status;
  };
  std::vector<Per> per(n_wf);
  for (uint32_t w = 0; w < n_wf; ++w) {
    auto a = slice<crr_activity_row>(B.rows[0], offs(0), w);
    auto t = slice<crr_timer_row>(B.rows[1], offs(1), w);
    auto c = slice<crr_child_row>(B.rows[2], offs(2), w);
    auto r = slice<crr_initiated_row>(B.rows[3], offs(3), w);
    auto s = slice<crr_initiated_row>(B.rows[4], offs(4), w);
    auto v = slice<crr_vh_item>(B.rows[5], offs(5), w);
    auto p = slice<crr_reset_point_row>(B.rows[6], offs(6), w);
    const auto a0 = a;
    const auto t0 = t;
    const auto c0 = c;
    const auto r0 = r, s0 = s;
    const auto p0 = p;
    const int salt = (int)(w % 7), more = (int)(w % 3);
    const uint32_t next_key = 1000;
    derive(a, 60, more, next_key, salt), derive(t, 60, more, next_key, salt + 1), derive(c, 60, more, next_key, salt + 2);
    derive(r, 60, more, next_key, salt + 3), derive(s, 60, (more + 1) % 3, next_key, salt);
    v.push_back({61, 3});
    if (w % 4 == 1) p.push_back(p.empty() ? crr_reset_point_row{1, 0, 1, 0} : p[0]);
    if (w % 4 == 2 && !p.empty()) p[0].flags ^= CRR_ROW_RESETTABLE;
    const int64_t at[7] = {(int64_t)act.size(), (int64_t)timer.size(), (int64_t)child.size(), (int64_t)rc.size(),
                           (int64_t)sig.size(), (int64_t)vh.size(), (int64_t)rp.size()};
    for (int k = 0; k < 7; ++k) o2[(size_t)k * (n_wf + 1) + w] = at[k];
    act.insert(act.end(), a.begin(), a.end()), timer.insert(timer.end(), t.begin(), t.end());
    child.insert(child.end(), c.begin(), c.end()), rc.insert(rc.end(), r.begin(), r.end()), sig.insert(sig.end(), s.begin(), s.end());
    vh.insert(vh.end(), v.begin(), v.end()), rp.insert(rp.end(), p.begin(), p.end());
    crr_exec_row& X = ex[w];
    X.next_event_id = 62, X.n_activity = (int32_t)a.size(), X.n_timer = (int32_t)t.size(), X.n_child = (int32_t)c.size();
    X.n_rc = (int32_t)r.size(), X.n_signal = (int32_t)s.size(), X.n_vh_items = (int32_t)v.size(), X.n_reset_points = (int32_t)p.size();
    Per& P = per[w];
    P.outcome = CRR_STORE_APPLIED, P.status = 0, P.flags = 0;
    if (w % 6 == 4) {          // a failed replay with counts no table holds
      X.status = 9, X.n_activity = X.n_timer = X.n_child = X.n_rc = X.n_signal = X.n_reset_points = 1 << 30;
      P.outcome = CRR_STORE_REPLAY_FAILED, P.status = 9;
      continue;
    }
    if (w % 6 == 5)            // counts no table holds: clamped to the rows the image has for the workflow
      X.n_activity = X.n_timer = X.n_child = X.n_rc = X.n_signal = X.n_reset_points = 0x7FFFFFFF, X.n_vh_items = -5;
    P.e.exec.push_back(X);
    classify(a0, a, P.e.act, P.e.del[0]), classify(t0, t, P.e.timer, P.e.del[1]), classify(c0, c, P.e.child, P.e.del[2]);
    classify(r0, r, P.e.rc, P.e.del[3]), classify(s0, s, P.e.sig, P.e.del[4]);
    bool differ = p0.size() != p.size();
    for (size_t i = 0; !differ && i < p.size(); ++i) differ = memcmp(&p0[i], &p[i], sizeof p[i]) != 0;
    if (differ) P.flags = CRR_MUTATION_RESET_POINTS_CHANGED;
  }
  const int64_t totals[7] = {(int64_t)act.size(), (int64_t)timer.size(), (int64_t)child.size(), (int64_t)rc.size(),
                             (int64_t)sig.size(), (int64_t)vh.size(), (int64_t)rp.size()};
  for (int k = 0; k < 7; ++k) o2[(size_t)k * (n_wf + 1) + n_wf] = totals[k];
  Image A;
  A.exec = exact(ex), A.offsets = exact(o2);
  A.rows[0] = exact(act), A.rows[1] = exact(timer), A.rows[2] = exact(child), A.rows[3] = exact(rc), A.rows[4] = exact(sig);
  A.rows[5] = exact(vh), A.rows[6] = exact(rp);

  const uint32_t n = n_wf + 3;
  std::vector<crr_repl_task> rt(n);
  std::vector<crr_last_event> le(n);
  std::vector<crr_ndc_result> res(n);
  std::vector<crr_ndc_route> routes(n);
  std::vector<crr_mutation_row> want(n);
  Expect all;
  for (uint32_t k = 0; k < n; ++k) {
    memset(&rt[k], 0, sizeof rt[k]), memset(&res[k], 0, sizeof res[k]), memset(&routes[k], 0, sizeof routes[k]);
    memset(&want[k], 0, sizeof want[k]);
    le[k] = {70, 3};
    res[k].action = CRR_NDC_APPEND, routes[k].route = CRR_ROUTE_APPLY_CURRENT;
    crr_mutation_row& W = want[k];
    W.exec_index = 0xFFFFFFFFu;
    W.map[0].upsert_begin = (uint32_t)all.act.size(), W.map[1].upsert_begin = (uint32_t)all.timer.size();
    W.map[2].upsert_begin = (uint32_t)all.child.size(), W.map[3].upsert_begin = (uint32_t)all.rc.size();
    W.map[4].upsert_begin = (uint32_t)all.sig.size();
    for (int t = 0; t < CRR_MUTATION_MAPS; ++t) W.map[t].delete_begin = (uint32_t)all.del[t].size();
    if (k >= n_wf) {
      rt[k].wf = k == n_wf ? n_wf + 7 : 0;                        // past the batch: not loaded
      if (k == n_wf + 1) routes[k].route = CRR_ROUTE_REBUILD;     // no route
      if (k == n_wf + 2) routes[k].route = CRR_ROUTE_NON_CURRENT; // a backfill: reported, nothing pending
      W.outcome = k == n_wf ? CRR_STORE_NOT_LOADED : k == n_wf + 1 ? CRR_STORE_NO_ROUTE : CRR_STORE_BACKFILLED;
      continue;
    }
    const uint32_t w = n_wf - 1 - k;
    rt[k].wf = w;
    const Per& P = per[w];
    W.outcome = P.outcome, W.status = P.status, W.flags = P.flags;
    if (P.outcome != CRR_STORE_APPLIED) continue;
    W.exec_index = (uint32_t)all.exec.size();
    all.exec.push_back(P.e.exec[0]);
    W.map[0].n_upsert = (uint32_t)P.e.act.size(), W.map[1].n_upsert = (uint32_t)P.e.timer.size();
    W.map[2].n_upsert = (uint32_t)P.e.child.size(), W.map[3].n_upsert = (uint32_t)P.e.rc.size(), W.map[4].n_upsert = (uint32_t)P.e.sig.size();
    all.act.insert(all.act.end(), P.e.act.begin(), P.e.act.end()), all.timer.insert(all.timer.end(), P.e.timer.begin(), P.e.timer.end());
    all.child.insert(all.child.end(), P.e.child.begin(), P.e.child.end()), all.rc.insert(all.rc.end(), P.e.rc.begin(), P.e.rc.end());
    all.sig.insert(all.sig.end(), P.e.sig.begin(), P.e.sig.end());
    for (int t = 0; t < CRR_MUTATION_MAPS; ++t) {
      W.map[t].n_delete = (uint32_t)P.e.del[t].size();
      all.del[t].insert(all.del[t].end(), P.e.del[t].begin(), P.e.del[t].end());
    }
  }
  crr_repl_task* d_rt = exact(rt);
  crr_last_event* d_le = exact(le);
  crr_ndc_result* d_res = exact(res);
  crr_ndc_route* d_routes = exact(routes);

  crr_mutation_sizes P;
  if (crr_load_mutation_host(&in, d_rt, d_le, n, d_res, d_routes, &A, nullptr, nullptr, &P, 1) != 0) return fail("sizing");
  const uint64_t want_up[5] = {all.act.size(), all.timer.size(), all.child.size(), all.rc.size(), all.sig.size()};
  if (P.n_exec != all.exec.size()) return fail("exec rows", (long)P.n_exec, (long)all.exec.size());
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) {
    if (P.n_upsert[t] != want_up[t]) return fail("upserted rows of map", t, (long)P.n_upsert[t]);
    if (P.n_delete[t] != all.del[t].size()) return fail("deleted keys of map", t, (long)P.n_delete[t]);
  }
  // exact-size outputs; then each of them one row short: refused, nothing written
  int bad = 0;
  for (int shorter = -1; shorter < 11 && !bad; ++shorter) {
    uint64_t cap[11];
    cap[0] = P.n_exec;
    for (int t = 0; t < 5; ++t) cap[1 + t] = P.n_upsert[t], cap[6 + t] = P.n_delete[t];
    if (shorter >= 0) {
      if (cap[shorter] == 0) continue;
      cap[shorter] -= 1;
    }
    crr_mutation_out o;
    memset(&o, 0, sizeof o);
    o.exec = static_cast<crr_exec_row*>(malloc((size_t)cap[0] * sizeof(crr_exec_row))), o.exec_capacity = cap[0];
    for (int t = 0; t < 5; ++t) {
      o.upsert[t] = malloc((size_t)cap[1 + t] * row_bytes[t]), o.upsert_capacity[t] = cap[1 + t];
      o.deleted[t] = static_cast<int64_t*>(malloc((size_t)cap[6 + t] * sizeof(int64_t))), o.delete_capacity[t] = cap[6 + t];
    }
    crr_mutation_row* rows = static_cast<crr_mutation_row*>(calloc(n, sizeof(crr_mutation_row)));
    const int rc2 = crr_load_mutation_host(&in, d_rt, d_le, n, d_res, d_routes, &A, rows, &o, &P, shorter < 0 ? 1 : 2);
    if (shorter >= 0) {
      if (rc2 != -1) bad = fail("a short capacity was not refused", shorter, rc2);
    } else if (rc2 != 0) {
      bad = fail("the run", rc2);
    } else {
      for (uint32_t k = 0; k < n && !bad; ++k)
        if (memcmp(&rows[k], &want[k], sizeof rows[k]) != 0) bad = fail("row of task", k, rows[k].outcome);
      const void* exp[5] = {all.act.data(), all.timer.data(), all.child.data(), all.rc.data(), all.sig.data()};
      if (!bad && P.n_exec && memcmp(o.exec, all.exec.data(), (size_t)P.n_exec * sizeof(crr_exec_row)) != 0) bad = fail("exec rows differ");
      for (int t = 0; t < 5 && !bad; ++t) {
        if (P.n_upsert[t] && memcmp(o.upsert[t], exp[t], (size_t)P.n_upsert[t] * row_bytes[t]) != 0) bad = fail("upserted rows differ, map", t);
        if (P.n_delete[t] && memcmp(o.deleted[t], all.del[t].data(), (size_t)P.n_delete[t] * 8) != 0) bad = fail("deleted keys differ, map", t);
        *n_rows += (int)(P.n_upsert[t] + P.n_delete[t]);
      }
    }
    free(rows), free(o.exec);
    for (int t = 0; t < 5; ++t) free(o.upsert[t]), free(o.deleted[t]);
  }
  free(d_rt), free(d_le), free(d_res), free(d_routes);
  return bad;
}

}  // namespace

int main() {
  int batches = 0, rows = 0;
  for (uint32_t n_wf : {1u, 6u, 13u, 40u})
    for (int shape = 0; shape < 5; ++shape) {
      if (check(n_wf, shape, &rows)) {
        fprintf(stderr, "n_wf %u, shape %d\n", n_wf, shape);
        return 1;
      }
      ++batches;
    }
  if (rows < 500) {
    fprintf(stderr, "only %d rows and keys compared\n", rows);
    return 1;
  }
  printf("load_mutation_asan: %d batches as this file's classifier gives them, %d upserted rows and deleted keys, no sanitizer report\n",
         batches, rows);
  return 0;
}
