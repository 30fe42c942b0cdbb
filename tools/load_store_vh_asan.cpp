// load_store_vh_asan.cpp -- a stand-alone check of the host restatement of the VersionHistories blob generated for
// routed replication tasks (crr_load_store_vh_host, include/cadence_load_store_vh.h) under AddressSanitizer /
// UndefinedBehaviorSanitizer, in the style of load_store_asan.cpp: hand-written states with one to three branches,
// tokens of several lengths (absent, empty, 300 bytes), absent Items fields, and hand-made decisions that reach
// every outcome.  Each batch's bytes, every input array, every buffer of the post-replay image and every output
// (the rows, the offsets, and `out` at exactly round_up(n_bytes, 16) bytes) lie in a heap block of exactly their
// size, so a read or a write past any of them is reported.  The last workflow's execution blob ends with its
// version histories (the last branch's token followed by stop bytes alone) or with its sticky name.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/load_store_vh_asan.cpp cadence_amd/csrc/load_states.cpp -o build/load_store_vh_asan -lpthread
//   build/load_store_vh_asan
//
// Exit status 0 and a line of counts when every row and every blob equals what the encoder written in this file
// gives and no sanitizer report ended the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "cadence_load_store_vh.h"

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

// the stored form: a history's absent field is left out; the items first, so that a token can end its struct
std::string stored_histories(int32_t current, const std::vector<Branch>& hs) {
  Wr w;
  w.u8(0x59), w.i32(10, current), w.list(20, 12, hs.size());
  for (auto& h : hs) {
    if (h.has_items) {
      w.list(20, 12, h.items.size());
      for (auto& it : h.items) w.i64(10, it.first), w.i64(20, it.second), w.stop();
    }
    if (h.has_token) w.str(10, h.token);
    w.stop();
  }
  w.stop();
  return w.b;
}

// ---- this file's own encoder of the blob Go stores: every field of every struct, token before items ---------------
std::string go_histories(int32_t current, const std::vector<Branch>& hs) {
  Wr w;
  w.u8(0x59), w.i32(10, current), w.list(20, 12, hs.size());
  for (auto& h : hs) {
    w.str(10, h.has_token ? h.token : std::string());
    w.list(20, 12, h.has_items ? h.items.size() : 0);
    if (h.has_items)
      for (auto& it : h.items) w.i64(10, it.first), w.i64(20, it.second), w.stop();
    w.stop();
  }
  w.stop();
  return w.b;
}

std::string execution_blob(const State& s) {
  Wr w;
  w.i32(34, 1), w.i64(50, 18), w.i64(52, 15), w.i64(58, 3), w.i64(60, 18);
  w.i64(62, -23), w.i64(66, 1), w.boolean(70, true), w.i64(106, 2), w.str(124, "thriftrw");
  if (s.sticky_last) w.str(122, stored_histories(s.current, s.hs)), w.str(78, s.sticky);
  else w.str(78, s.sticky), w.str(122, stored_histories(s.current, s.hs));
  w.stop();
  return w.b;
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
  int32_t outcome, status;   // expected; a generated one may become a VH error from add_or_update
  std::string blob;          // expected bytes
};

// the post-replay state of a resumed workflow, written by hand
struct After {
  bool resumed;
  int32_t status;
  Items vh;
};

int check(const std::vector<State>& states, const std::vector<After>& after, std::vector<Task>& tasks, bool with_after,
          int* generated, uint64_t* bytes_checked) {
  Wr timer;
  timer.i64(10, 3), timer.i64(12, 7), timer.stop();
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

  // the after-image: exec rows and vh rows in workflow order, exact blocks; the other tables hold no rows
  std::vector<crr_exec_row> ex(n_wf);
  std::vector<int64_t> offsets((size_t)CRR_LOAD_TABLES * (n_wf + 1), 0);
  std::vector<int32_t> status(n_wf, 0);
  std::vector<crr_vh_item> vh;
  for (uint32_t w = 0; w < n_wf; ++w) {
    memset(&ex[w], 0, sizeof ex[w]);
    const After& A = after[w];
    status[w] = A.resumed ? 0 : 1;
    offsets[5 * (n_wf + 1) + w] = (int64_t)vh.size();
    if (!A.resumed) continue;
    ex[w].status = A.status, ex[w].state = 2, ex[w].next_event_id = 40 + w;
    ex[w].n_vh_items = (int32_t)A.vh.size();
    for (auto& it : A.vh) vh.push_back({it.first, it.second});
  }
  offsets[5 * (n_wf + 1) + n_wf] = (int64_t)vh.size();
  Image img;
  img.exec = exact(ex), img.offsets = exact(offsets), img.status = exact(status);
  img.rows[5] = exact(vh);
  for (int t = 0; t < 5; ++t) img.rows[t] = malloc(0);

  // expected rows and blobs, from this file's encoder
  for (auto& t : tasks) {
    t.blob.clear();
    if (t.outcome != CRR_STORE_APPLIED && t.outcome != CRR_STORE_BACKFILLED) continue;
    const State& s = states[t.wf];
    std::vector<Branch> hs = s.hs;
    if (t.outcome == CRR_STORE_BACKFILLED) {
      const int st = add_or_update(hs[t.branch], t.id, t.version);
      if (st != 0) {
        t.outcome = CRR_STORE_VH_ERROR, t.status = st;
        continue;
      }
    } else if (!with_after) {
      continue;
    } else {
      hs[s.current].has_items = true, hs[s.current].items = after[t.wf].vh;
    }
    t.blob = go_histories(s.current, hs);
    ++*generated;
  }
  if (!with_after)   // no post-replay state: every task on the current route of a loaded state is not resumed
    for (auto& t : tasks)
      if (t.route == CRR_ROUTE_APPLY_CURRENT && t.wf < n_wf && states[t.wf].loads) t.outcome = CRR_STORE_NOT_RESUMED, t.status = 0, t.blob.clear();

  std::vector<crr_repl_task> rt(n);
  std::vector<crr_last_event> le(n);
  std::vector<crr_ndc_result> res(n);
  std::vector<crr_ndc_route> routes(n);
  uint64_t total = 0;
  for (uint32_t k = 0; k < n; ++k) {
    memset(&rt[k], 0, sizeof rt[k]), memset(&res[k], 0, sizeof res[k]), memset(&routes[k], 0, sizeof routes[k]);
    rt[k].wf = tasks[k].wf;
    le[k] = {tasks[k].id, tasks[k].version};
    res[k].action = tasks[k].action, res[k].branch_index = tasks[k].branch;
    routes[k].route = tasks[k].route;
    total += tasks[k].blob.size();
  }
  crr_repl_task* d_rt = exact(rt);
  crr_last_event* d_le = exact(le);
  crr_ndc_result* d_res = exact(res);
  crr_ndc_route* d_routes = exact(routes);
  const crr_load_image* image = with_after ? &img : nullptr;

  // the sizing call, then exact blocks for the outputs
  crr_vh_blob_sizes P;
  int rc = crr_load_store_vh_host(&in, d_rt, d_le, n, d_res, d_routes, image, nullptr, nullptr, nullptr, 0, &P, 1);
  int bad = rc != 0 || P.n_bytes != total || P.n_tasks != n;
  if (bad) fprintf(stderr, "sizing call: rc %d, %llu bytes for %llu expected\n", rc, (unsigned long long)P.n_bytes, (unsigned long long)total);
  const size_t padded = (size_t)((total + 15) / 16 * 16);
  crr_vh_blob_row* rows = static_cast<crr_vh_blob_row*>(malloc(n * sizeof(crr_vh_blob_row)));
  uint64_t* blob_off = static_cast<uint64_t*>(malloc(((size_t)n + 1) * sizeof(uint64_t)));
  uint8_t* out = static_cast<uint8_t*>(malloc(padded));
  if (!bad && padded) {   // one byte short: refused, nothing touched
    memset(out, 0xA5, padded);
    rc = crr_load_store_vh_host(&in, d_rt, d_le, n, d_res, d_routes, image, rows, blob_off, out, padded - 1, &P, 1);
    for (size_t i = 0; i < padded; ++i) bad |= out[i] != 0xA5;
    if (rc != -1 || bad) fprintf(stderr, "a capacity one byte short: rc %d, buffer %s\n", rc, bad ? "written" : "intact"), bad = 1;
  }
  if (!bad) {
    rc = crr_load_store_vh_host(&in, d_rt, d_le, n, d_res, d_routes, image, rows, blob_off, out, padded, &P, 2);
    bad = rc != 0;
    if (bad) fprintf(stderr, "crr_load_store_vh_host: %d\n", rc);
  }
  uint64_t run = 0;
  for (uint32_t k = 0; k < n && !bad; ++k) {
    const crr_vh_blob_row& g = rows[k];
    const Task& e = tasks[k];
    if (g.len != e.blob.size() || g.outcome != e.outcome || g.status != e.status || g.reserved != 0 || blob_off[k] != run ||
        (g.len && memcmp(out + run, e.blob.data(), g.len) != 0)) {
      fprintf(stderr, "task %u (wf %u route %d action %d branch %d): got %u/%d/%d at %llu, expected %zu/%d/%d at %llu (or other bytes)\n",
              k, e.wf, e.route, e.action, e.branch, g.len, g.outcome, g.status, (unsigned long long)blob_off[k], e.blob.size(),
              e.outcome, e.status, (unsigned long long)run);
      bad = 1;
    }
    run += e.blob.size();
  }
  if (!bad && blob_off[n] != total) bad = 1;
  for (size_t i = (size_t)total; i < padded && !bad; ++i) bad = out[i] != 0;   // the tail is zeros
  *bytes_checked += total;
  free(rows), free(blob_off), free(out);
  free(d_rt), free(d_le), free(d_res), free(d_routes);
  return bad;
}

}  // namespace

int main() {
  const Items items = {{5, 1}, {19, 3}}, longer = {{5, 1}, {9, 2}, {30, 3}, {31, 8}};
  const int32_t A = CRR_ROUTE_APPLY_CURRENT, N = CRR_ROUTE_NON_CURRENT, APP = CRR_NDC_APPEND, NEW = CRR_NDC_NEW_BRANCH;
  const int32_t GA = CRR_STORE_APPLIED, GB = CRR_STORE_BACKFILLED, VE = CRR_STORE_VH_ERROR;
  int batches = 0, generated = 0;
  uint64_t bytes_checked = 0;
  unsigned seen = 0;
  for (size_t tok_len : {0u, 1u, 7u, 8u, 9u, 300u})
    for (int last = 0; last < 2; ++last) {
      const std::string tok = bytes_of(tok_len, 11);
      const std::vector<State> states = {
          {true, 20, "", 0, {{true, true, tok, items}}, true},
          {true, 21, "s", 1, {{false, true, "", items}, {true, true, tok, longer}}, false},
          {false, 22, "", 0, {{true, true, tok, items}}, true},
          {true, 23, "sticky-tl", 2, {{true, false, tok, {}}, {true, true, "", {}}, {tok_len != 0, true, tok, items}}, true},
          // the block's last bytes: the sticky name, or the last branch's token
          {true, 24, "name", 0, {{true, true, "cur", longer}, {true, last == 1, tok, items}}, last == 0},
      };
      const std::vector<After> after = {{true, 0, {{10, 1}, {22, 3}}}, {true, 0, {{5, 1}, {9, 2}, {30, 3}, {44, 8}}}, {false, 0, {}},
                                        {true, 7, {{1, 1}}}, {false, 0, {}}};
      std::vector<Task> tasks = {
          {1, N, APP, 0, 25, 7, GB, 0, ""},          // a higher version appends
          {1, N, APP, 0, 30, 3, GB, 0, ""},          // an equal version updates the last item's event ID
          {3, N, APP, 0, 4, 2, GB, 0, ""},           // Items absent: the empty branch takes the item
          {3, N, APP, 1, 4, -24, GB, 0, ""},         // Items empty; EmptyVersion is a valid version
          {4, N, APP, 1, 40, 9, GB, 0, ""},          // the state at the block's end
          {4, N, APP, 0, 31, 9, GB, 0, ""},
          {0, N, APP, 0, 40, 2, GB, 0, ""},          // a lower version (the expected row is set from add_or_update)
          {0, N, APP, 0, 19, 3, GB, 0, ""},          // the event ID does not increase
          {0, N, APP, 0, -1, 3, GB, 0, ""},          // NewVersionHistoryItem panics
          {0, N, APP, 7, -1, 3, VE, CRR_ERR_VH_INVALID_ITEM, ""},
          {0, N, APP, 1, 25, 7, VE, CRR_ERR_NDC_BAD_INDEX, ""},
          {1, A, APP, 0, 25, 7, VE, CRR_ERR_NDC_BAD_INDEX, ""},   // the current route, not the current branch
          {0, CRR_ROUTE_NONE, CRR_NDC_DUPLICATE, 0, 25, 7, CRR_STORE_NO_ROUTE, 0, ""},
          {0, CRR_ROUTE_REBUILD, APP, 0, 25, 7, CRR_STORE_NO_ROUTE, 0, ""},
          {0, N, NEW, 1, 25, 7, CRR_STORE_NEW_BRANCH, 0, ""},
          {0, A, NEW, 1, 25, 7, CRR_STORE_NEW_BRANCH, 0, ""},
          {2, N, APP, 0, 25, 7, CRR_STORE_NOT_LOADED, 0, ""},
          {5, N, APP, 0, 25, 7, CRR_STORE_NOT_LOADED, 0, ""},
          {0xFFFFFFFFu, A, APP, 0, 25, 7, CRR_STORE_NOT_LOADED, 0, ""},
          {0, A, APP, 0, 0, 0, GA, 0, ""},
          {1, A, APP, 1, 0, 0, GA, 0, ""},
          {3, A, APP, 2, 0, 0, CRR_STORE_REPLAY_FAILED, 7, ""},
          {4, A, APP, 0, 0, 0, CRR_STORE_NOT_RESUMED, 0, ""},
          {4, N, APP, 1, 41, 9, GB, 0, ""},          // a generated task last: its blob ends the output
      };
      for (int with_after = 0; with_after < 2; ++with_after)
        for (int drop_last = 0; drop_last < 2; ++drop_last) {   // ... or a task that generates nothing does
          std::vector<Task> done = tasks;
          if (drop_last) done.pop_back();
          if (check(states, after, done, with_after != 0, &generated, &bytes_checked)) {
            fprintf(stderr, "token %zu, last %d, after %d, drop %d\n", tok_len, last, with_after, drop_last);
            return 1;
          }
          for (auto& t : done) seen |= 1u << t.outcome;
          ++batches;
        }
    }
  // no tasks at all, and no states
  {
    std::vector<Task> none;
    std::vector<State> no_states;
    std::vector<After> no_after;
    if (check(no_states, no_after, none, false, &generated, &bytes_checked)) return 1;
    ++batches;
  }
  if (seen != 0xFFu) {
    fprintf(stderr, "outcomes reached: %02x\n", seen);
    return 1;
  }
  printf("load_store_vh_asan: %d batches as this file's encoder gives them, %d generated blobs, %llu bytes, every outcome, "
         "no sanitizer report\n", batches, generated, (unsigned long long)bytes_checked);
  return 0;
}
