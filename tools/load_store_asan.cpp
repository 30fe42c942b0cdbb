// load_store_asan.cpp -- a stand-alone check of the host restatement of the checksum generated for routed
// replication tasks (crr_load_store_checksums_host, include/cadence_load_store.h) under AddressSanitizer /
// UndefinedBehaviorSanitizer: hand-written states with one to three branches, tokens and sticky names of several
// lengths (absent, empty, 300 bytes), absent Items fields, and hand-made decisions that reach every outcome.
// Each batch's bytes, every input array and every buffer of the post-replay image lie in a heap block of exactly
// their size, so a read past any of them is reported.  The last workflow's execution blob ends with its sticky
// name (only the struct's stop byte behind it) or with its version histories (the last branch's token followed by
// stop bytes alone), so the eight-bytes-at-a-time reader runs up to the block's end.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/load_store_asan.cpp cadence_amd/csrc/load_states.cpp -o build/load_store_asan -lpthread
//   build/load_store_asan
//
// Exit status 0 and a line of counts when every row equals the value of the encoder written in this file and no
// sanitizer report ended the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "cadence_load_store.h"

#include "load_asan_common.h"

namespace {

typedef std::vector<std::pair<int64_t, int64_t>> Items;

struct Branch {
  bool has_token, has_items;
  std::string token;
  Items items;
};

struct State {
  bool loads;
  int64_t nei;
  std::string sticky;
  int32_t current;
  std::vector<Branch> hs;
  bool sticky_last;   // the sticky name is the execution blob's last field (else the version histories are)
};

std::string version_histories(int32_t current, const std::vector<Branch>& hs) {
  Wr w;
  w.u8(0x59), w.i32(10, current), w.list(20, 12, hs.size());
  for (auto& h : hs) {
    if (h.has_items) {   // the items first: a token without items behind it ends its struct
      w.list(20, 12, h.items.size());
      for (auto& it : h.items) w.i64(10, it.first), w.i64(20, it.second), w.stop();
    }
    if (h.has_token) w.str(10, h.token);
    w.stop();
  }
  w.stop();
  return w.b;
}

// the scalars every state of this file is written with
const int64_t kLastFirst = 18, kLastProcessed = 15, kDecisionVersion = 3, kDecisionSchedule = 18, kDecisionStarted = -23;
const int64_t kTimerStartedID = 7;

std::string execution_blob(const State& s) {
  Wr w;
  w.i32(34, 1), w.i64(50, kLastFirst), w.i64(52, kLastProcessed), w.i64(58, kDecisionVersion), w.i64(60, kDecisionSchedule);
  w.i64(62, kDecisionStarted), w.i64(66, 1), w.boolean(70, true), w.i64(106, 2), w.str(124, "thriftrw");
  if (s.sticky_last) w.str(122, version_histories(s.current, s.hs)), w.str(78, s.sticky);
  else w.str(78, s.sticky), w.str(122, version_histories(s.current, s.hs));
  w.stop();
  return w.b;
}

// ---- this file's own encoder of 0x59 + MutableStateChecksumPayload and CRC32-IEEE ----------------------------------
struct Scalars {
  bool cancel;
  int16_t state;
  int64_t last_first, next_event, last_processed, signal_count;
  int32_t attempt;
  int64_t decision_version, schedule_id, started_id;
  std::vector<int64_t> timers, acts, sigs, rcs, children;
};

std::string payload(const Scalars& x, const std::string& sticky, int32_t current, const std::vector<Branch>& hs) {
  Wr w;
  w.u8(0x59);
  w.boolean(10, x.cancel), w.i16(15, x.state), w.i64(23, x.last_first), w.i64(24, x.next_event), w.i64(25, x.last_processed);
  w.i64(26, x.signal_count), w.i32(35, x.attempt), w.i64(36, x.decision_version), w.i64(37, x.schedule_id), w.i64(38, x.started_id);
  auto ids = [&](int16_t id, const std::vector<int64_t>& v) {
    w.list(id, 10, v.size());
    for (int64_t x : v) w.be((uint64_t)x, 8);
  };
  ids(45, x.timers), ids(46, x.acts), ids(47, x.sigs), ids(48, x.rcs), ids(49, x.children);
  w.str(55, sticky);
  w.field(12, 56);
  w.i32(10, current), w.list(20, 12, hs.size());
  for (auto& h : hs) {
    w.str(10, h.has_token ? h.token : std::string());
    w.list(20, 12, h.has_items ? h.items.size() : 0);
    if (h.has_items)
      for (auto& it : h.items) w.i64(10, it.first), w.i64(20, it.second), w.stop();
    w.stop();
  }
  w.stop(), w.stop();
  return w.b;
}

uint32_t crc32(const std::string& s) {
  uint32_t c = 0xFFFFFFFFu;
  for (unsigned char ch : s) {
    c ^= ch;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

Scalars stored_scalars(const State& s) {
  return {true, 1, kLastFirst, s.nei, kLastProcessed, 2, 1, kDecisionVersion, kDecisionSchedule, kDecisionStarted,
          {kTimerStartedID}, {}, {}, {}, {}};
}

// NewVersionHistoryItem + AddOrUpdateItem: 0 and the branch updated, or the status
int add_or_update(Branch& b, int64_t id, int64_t version) {
  if (id < 0 || (version < 0 && version != -24)) return CRR_ERR_VH_INVALID_ITEM;
  if (!b.has_items || b.items.empty()) {
    b.has_items = true;
    b.items = {{id, version}};
    return 0;
  }
  if (version < b.items.back().second) return CRR_ERR_VH_LOWER_VERSION;
  if (id <= b.items.back().first) return CRR_ERR_VH_EVENT_ID_NOT_INCREASING;
  if (version > b.items.back().second) b.items.push_back({id, version});
  else b.items.back().first = id;
  return 0;
}

struct Task {
  uint32_t wf;
  int32_t route, action, branch;
  int64_t id, version;
  crr_store_row want;
};

// the post-replay state of a resumed workflow, written by hand
struct After {
  bool resumed;
  int32_t status;
  std::vector<int64_t> acts, children;
  Items vh;
};

// runs one batch; `tasks` comes back with the expected rows this file computed
int check(const std::vector<State>& states, const std::vector<After>& after, std::vector<Task>& tasks, bool with_after, int* generated) {
  // the batch: per workflow a timer blob, then its execution blob (a state that does not load: two of them)
  Wr timer;
  timer.i64(10, 3), timer.i64(12, kTimerStartedID), timer.stop();
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off{0};
  std::vector<crr_state_blob> meta;
  std::vector<crr_state_wf> wf;
  auto add = [&](uint32_t kind, const std::string& b) {
    bytes.insert(bytes.end(), b.begin(), b.end());
    off.push_back(bytes.size());
    meta.push_back({kind, kind == CRR_STATE_TIMER ? 5u : 0u, 0, 0, 0});
  };
  for (auto& s : states) {
    wf.push_back({(uint32_t)meta.size(), 2, s.nei});
    add(s.loads ? (uint32_t)CRR_STATE_TIMER : (uint32_t)CRR_STATE_EXECUTION, s.loads ? timer.b : execution_blob(s));
    add(CRR_STATE_EXECUTION, execution_blob(s));
  }
  const uint32_t n_wf = (uint32_t)states.size(), n = (uint32_t)tasks.size();
  std::vector<uint8_t> strings = {'t', 'i', 'm', 'e', 'r'};
  const StateBatch batch(bytes, off, meta, wf, strings);
  const crr_state_batch& in = batch.in;

  // the after-image: dense rows in workflow order, exact blocks
  std::vector<crr_exec_row> ex(n_wf);
  std::vector<int64_t> offsets((size_t)CRR_LOAD_TABLES * (n_wf + 1), 0);
  std::vector<int32_t> status(n_wf, 0);
  std::vector<crr_activity_row> act;
  std::vector<crr_child_row> child;
  std::vector<crr_vh_item> vh;
  for (uint32_t w = 0; w < n_wf; ++w) {
    memset(&ex[w], 0, sizeof ex[w]);
    const After& A = after[w];
    status[w] = A.resumed ? 0 : 1;
    offsets[0 * (n_wf + 1) + w] = (int64_t)act.size(), offsets[2 * (n_wf + 1) + w] = (int64_t)child.size();
    offsets[5 * (n_wf + 1) + w] = (int64_t)vh.size();
    if (!A.resumed) continue;
    ex[w].status = A.status, ex[w].state = 2, ex[w].next_event_id = 40 + w, ex[w].last_first_event_id = 37, ex[w].last_processed_event = 30;
    ex[w].signal_count = 4, ex[w].decision_attempt = 0, ex[w].decision_version = -24, ex[w].decision_schedule_id = -23, ex[w].decision_started_id = -23;
    ex[w].n_activity = (int32_t)A.acts.size(), ex[w].n_child = (int32_t)A.children.size(), ex[w].n_vh_items = (int32_t)A.vh.size();
    for (int64_t id : A.acts) {
      crr_activity_row r;
      memset(&r, 0, sizeof r);
      r.schedule_id = id;
      act.push_back(r);
    }
    for (int64_t id : A.children) {
      crr_child_row r;
      memset(&r, 0, sizeof r);
      r.initiated_id = id;
      child.push_back(r);
    }
    for (auto& it : A.vh) vh.push_back({it.first, it.second});
  }
  for (int t = 0; t < CRR_LOAD_TABLES; ++t) {
    const int64_t total = t == 0 ? (int64_t)act.size() : t == 2 ? (int64_t)child.size() : t == 5 ? (int64_t)vh.size() : 0;
    offsets[(size_t)t * (n_wf + 1) + n_wf] = total;
  }
  Image img;
  img.exec = exact(ex), img.offsets = exact(offsets), img.status = exact(status);
  img.rows[0] = exact(act), img.rows[2] = exact(child), img.rows[5] = exact(vh);
  // the tables without rows: exact blocks of no bytes
  img.rows[1] = malloc(0), img.rows[3] = malloc(0), img.rows[4] = malloc(0);

  // expected rows, from this file's encoder
  for (auto& t : tasks) {
    if (t.want.outcome != CRR_STORE_APPLIED && t.want.outcome != CRR_STORE_BACKFILLED) continue;
    const State& s = states[t.wf];
    std::vector<Branch> hs = s.hs;
    std::string p;
    if (t.want.outcome == CRR_STORE_BACKFILLED) {
      const int st = add_or_update(hs[t.branch], t.id, t.version);
      if (st != 0) {
        t.want = {0, CRR_STORE_VH_ERROR, 0, st};
        continue;
      }
      p = payload(stored_scalars(s), s.sticky, s.current, hs);
    } else if (!with_after) {
      continue;
    } else {
      const After& A = after[t.wf];
      hs[s.current].has_items = true, hs[s.current].items = A.vh;
      const Scalars x = {false, 2, 37, 40 + (int64_t)t.wf, 30, 4, 0, -24, -23, -23, {}, A.acts, {}, {}, A.children};
      p = payload(x, "", s.current, hs);
    }
    t.want = {crc32(p), t.want.outcome, (uint32_t)p.size(), 0};
    ++*generated;
  }
  if (!with_after)   // no post-replay state: every task on the current route of a loaded state is not resumed
    for (auto& t : tasks)
      if (t.route == CRR_ROUTE_APPLY_CURRENT && t.wf < n_wf && states[t.wf].loads) t.want = {0, CRR_STORE_NOT_RESUMED, 0, 0};

  std::vector<crr_repl_task> rt(n);
  std::vector<crr_last_event> le(n);
  std::vector<crr_ndc_result> res(n);
  std::vector<crr_ndc_route> routes(n);
  for (uint32_t k = 0; k < n; ++k) {
    memset(&rt[k], 0, sizeof rt[k]), memset(&res[k], 0, sizeof res[k]), memset(&routes[k], 0, sizeof routes[k]);
    rt[k].wf = tasks[k].wf;
    le[k] = {tasks[k].id, tasks[k].version};
    res[k].action = tasks[k].action, res[k].branch_index = tasks[k].branch;
    routes[k].route = tasks[k].route;
  }
  crr_repl_task* d_rt = exact(rt);
  crr_last_event* d_le = exact(le);
  crr_ndc_result* d_res = exact(res);
  crr_ndc_route* d_routes = exact(routes);
  crr_store_row* out = static_cast<crr_store_row*>(malloc(n * sizeof(crr_store_row)));
  const int rc = crr_load_store_checksums_host(&in, d_rt, d_le, n, d_res, d_routes, with_after ? &img : nullptr, out, 1);
  int bad = rc != 0;
  for (uint32_t k = 0; k < n && !bad; ++k) {
    const crr_store_row& g = out[k];
    const crr_store_row& e = tasks[k].want;
    if (g.value != e.value || g.outcome != e.outcome || g.payload_len != e.payload_len || g.status != e.status) {
      fprintf(stderr, "task %u (wf %u route %d action %d branch %d): got %08x/%d/%u/%d, expected %08x/%d/%u/%d\n", k, tasks[k].wf,
              tasks[k].route, tasks[k].action, tasks[k].branch, g.value, g.outcome, g.payload_len, g.status, e.value, e.outcome,
              e.payload_len, e.status);
      bad = 1;
    }
  }
  if (rc != 0) fprintf(stderr, "crr_load_store_checksums_host: %d\n", rc);
  free(out), free(d_rt), free(d_le), free(d_res), free(d_routes);
  return bad;
}

}  // namespace

int main() {
  const Items items = {{5, 1}, {19, 3}}, longer = {{5, 1}, {9, 2}, {30, 3}, {31, 8}};
  const int32_t A = CRR_ROUTE_APPLY_CURRENT, N = CRR_ROUTE_NON_CURRENT, APP = CRR_NDC_APPEND, NEW = CRR_NDC_NEW_BRANCH;
  int batches = 0, generated = 0;
  unsigned seen = 0;
  for (size_t tok_len : {0u, 1u, 7u, 8u, 9u, 300u})
    for (size_t sticky_len : {0u, 1u, 9u, 300u})
      for (int last = 0; last < 2; ++last) {
        const std::string tok = bytes_of(tok_len, 11), name = bytes_of(sticky_len, 40);
        const std::vector<State> states = {
            {true, 20, name, 0, {{true, true, tok, items}}, true},
            {true, 21, "s", 1, {{false, true, "", items}, {true, true, tok, longer}}, false},
            {false, 22, "", 0, {{true, true, tok, items}}, true},
            {true, 23, "sticky-tl", 2, {{true, false, tok, {}}, {true, true, "", {}}, {tok_len != 0, true, tok, items}}, true},
            // the block's last bytes: the sticky name, or the last branch's token
            {true, 24, name, 0, {{true, true, "cur", longer}, {true, last == 1, tok, items}}, last == 0},
        };
        const std::vector<After> after = {{true, 0, {5, 8}, {}, {{10, 1}, {22, 3}}}, {true, 0, {}, {9}, {{5, 1}, {9, 2}, {30, 3}, {44, 8}}},
                                          {false, 0, {}, {}, {}}, {true, 7, {}, {}, {{1, 1}}}, {false, 0, {}, {}, {}}};
        const crr_store_row gen_a = {0, CRR_STORE_APPLIED, 0, 0}, gen_b = {0, CRR_STORE_BACKFILLED, 0, 0};
        std::vector<Task> tasks = {
            {1, N, APP, 0, 25, 7, gen_b},          // a higher version appends
            {1, N, APP, 0, 30, 3, gen_b},          // an equal version updates the last item's event ID
            {3, N, APP, 0, 4, 2, gen_b},           // Items absent: the empty branch takes the item
            {3, N, APP, 1, 4, -24, gen_b},         // Items empty; EmptyVersion is a valid version
            {4, N, APP, 1, 40, 9, gen_b},          // the state at the block's end
            {4, N, APP, 0, 31, 9, gen_b},
            {0, N, APP, 0, 40, 2, gen_b},          // a lower version (the expected row is set from add_or_update)
            {0, N, APP, 0, 19, 3, gen_b},          // the event ID does not increase
            {0, N, APP, 0, 10, 5, gen_b},
            {0, N, APP, 0, -1, 3, gen_b},          // NewVersionHistoryItem panics
            {0, N, APP, 0, 5, -2, gen_b},
            {0, N, APP, 7, -1, 3, {0, CRR_STORE_VH_ERROR, 0, CRR_ERR_VH_INVALID_ITEM}},
            {0, N, APP, 1, 25, 7, {0, CRR_STORE_VH_ERROR, 0, CRR_ERR_NDC_BAD_INDEX}},
            {1, N, APP, -1, 25, 7, {0, CRR_STORE_VH_ERROR, 0, CRR_ERR_NDC_BAD_INDEX}},
            {1, A, APP, 0, 25, 7, {0, CRR_STORE_VH_ERROR, 0, CRR_ERR_NDC_BAD_INDEX}},   // the current route, not the current branch
            {0, CRR_ROUTE_NONE, CRR_NDC_DUPLICATE, 0, 25, 7, {0, CRR_STORE_NO_ROUTE, 0, 0}},
            {0, CRR_ROUTE_REBUILD, APP, 0, 25, 7, {0, CRR_STORE_NO_ROUTE, 0, 0}},
            {1, CRR_ROUTE_BAD_REQUEST, APP, 0, 25, 7, {0, CRR_STORE_NO_ROUTE, 0, 0}},
            {0, N, NEW, 1, 25, 7, {0, CRR_STORE_NEW_BRANCH, 0, 0}},
            {0, A, NEW, 1, 25, 7, {0, CRR_STORE_NEW_BRANCH, 0, 0}},
            {2, N, APP, 0, 25, 7, {0, CRR_STORE_NOT_LOADED, 0, 0}},
            {2, A, APP, 0, 25, 7, {0, CRR_STORE_NOT_LOADED, 0, 0}},
            {5, N, APP, 0, 25, 7, {0, CRR_STORE_NOT_LOADED, 0, 0}},
            {0xFFFFFFFFu, A, APP, 0, 25, 7, {0, CRR_STORE_NOT_LOADED, 0, 0}},
            {0, A, APP, 0, 0, 0, gen_a},
            {1, A, APP, 1, 0, 0, gen_a},
            {3, A, APP, 2, 0, 0, {0, CRR_STORE_REPLAY_FAILED, 0, 7}},
            {3, A, NEW, 3, 0, 0, {0, CRR_STORE_REPLAY_FAILED, 0, 7}},
            {4, A, APP, 0, 0, 0, {0, CRR_STORE_NOT_RESUMED, 0, 0}},
        };
        for (int with_after = 0; with_after < 2; ++with_after) {
          std::vector<Task> done = tasks;
          if (check(states, after, done, with_after != 0, &generated)) {
            fprintf(stderr, "token %zu, sticky %zu, last %d, after %d\n", tok_len, sticky_len, last, with_after);
            return 1;
          }
          for (auto& t : done) seen |= 1u << t.want.outcome;
          ++batches;
        }
      }
  if (seen != 0xFFu) {
    fprintf(stderr, "outcomes reached: %02x\n", seen);
    return 1;
  }
  printf("load_store_asan: %d batches as this file's encoder gives them, %d generated values, every outcome, no sanitizer report\n",
         batches, generated);
  return 0;
}
