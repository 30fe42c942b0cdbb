// load_states.cpp -- crr_load_states_host: the host restatement of the persisted mutable-state loader
// (include/cadence_load.h).  The decoder itself is load_decode.h, the same text the gfx950 kernels of
// load_kernel.hip compile; this file runs its phases as loops (optionally over threads), with serial
// prefix scans between them, over a scratch laid out exactly like the device's.
// crr_load_states_verify_host (include/cadence_load_verify.h) runs the same load, then load_decode.h's verify_wf;
// crr_load_branches_host (include/cadence_load_ndc.h) the same load, then its branch walk;
// crr_load_store_checksums_host (include/cadence_load_store.h) both, then load_decode.h's store_task per task;
// crr_load_store_vh_host (include/cadence_load_store_vh.h) the same, then its sizes and its sequential blob writer;
// crr_load_mutation_host (include/cadence_load_mutation.h) the same, then its count and emit passes and the gather;
// crr_load_store_exec_host (include/cadence_load_store_exec.h) the same, then its decision and its splice per task;
// crr_load_resume_host (include/cadence_load_resume.h) the load, then its decisions, serial prefixes and the gather.
//
// What the calls share is written once: Owned frees a scratch or work buffer, zeroed() gives every other temporary
// an owner (so no exit path frees by hand, and out of memory is a NULL to test, never an exception), StoreHost is
// the load, the branch walk and the branch table the four store-family calls start from, exclusive_scan every
// serial prefix, write_vh_blobs the VersionHistories writer, load_decode.h's pack_task_blobs the tasks' event blobs.
#include <stdlib.h>

#include <memory>
#include <thread>
#include <vector>

#include "load_decode.h"

namespace {

using namespace crr_load;

template <class Fn>
void parallel_for(uint32_t n, int threads, Fn fn) {
  if (threads <= 1 || n < 1024) {
    Frame stk[kMaxDepth];
    for (uint32_t i = 0; i < n; ++i) fn(i, stk);
    return;
  }
  std::vector<std::thread> pool;
  const uint32_t per = (n + threads - 1) / threads;
  for (int t = 0; t < threads; ++t) {
    const uint32_t lo = (uint32_t)t * per, hi = lo + per < n ? lo + per : n;
    if (lo >= hi) break;
    pool.emplace_back([=] {
      Frame stk[kMaxDepth];
      for (uint32_t i = lo; i < hi; ++i) fn(i, stk);
    });
  }
  for (auto& th : pool) th.join();
}

// p[0..n) to its exclusive prefix sums in place, p[n] = the total, which is returned
template <class T>
T exclusive_scan(T* p, uint32_t n) {
  T run = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const T x = p[i];
    p[i] = run;
    run += x;
  }
  p[n] = run;
  return run;
}

// a Ctx, NdcWork or ResumeWork whose buffer (.s) is this call's own
template <class T>
struct Owned : T {
  Owned() { this->s = nullptr; }
  ~Owned() { free(this->s); }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
};

struct Free {
  void operator()(void* p) const { free(p); }
};
template <class T>
using Buf = std::unique_ptr<T[], Free>;

// n zeroed elements, or NULL when out of memory
template <class T>
Buf<T> zeroed(uint64_t n) {
  return Buf<T>(static_cast<T*>(calloc((size_t)n, sizeof(T))));
}

// every phase of the load over a scratch this allocates (c owns it): 0, -1 invalid argument, -2 out of memory
int run_load(const crr_state_batch* in, int threads, Owned<Ctx>& c) {
  if (in->n_blobs && (!in->bytes || !in->blob_off || !in->blob)) return -1;
  if (in->n_wf && !in->wf) return -1;
  const uint32_t n_wf = in->n_wf;
  uint64_t blobs = 0;
  for (uint32_t w = 0; w < n_wf; ++w) {   // consecutive ranges covering the blobs
    if (in->wf[w].blob_begin != blobs) return -1;
    blobs += in->wf[w].blob_count;
  }
  if (blobs != in->n_blobs) return -1;
  c.in = *in;
  c.L = carve(in->n_blobs, n_wf, nullptr);
  c.s = static_cast<uint8_t*>(calloc(c.L.end + 16, 1));
  if (!c.s) return -2;
  c.err()[0] = ~0ull;
  parallel_for(in->n_blobs, threads, [&](uint32_t b, Frame* stk) { parse_blob(c, b, stk); });
  parallel_for(n_wf, threads, [&](uint32_t w, Frame* stk) { count_wf(c, w, stk); });
  for (int t = 0; t < kCounters; ++t)
    if (t != CRR_LOAD_T_KEYS && t != CRR_LOAD_T_KEY_BYTES) exclusive_scan(c.cnt(t), n_wf);
  uint64_t tot[kCounters];
  for (int t = 0; t < kCounters; ++t) tot[t] = (uint64_t)c.cnt(t)[n_wf];
  const Layout full = carve(in->n_blobs, n_wf, tot);
  uint8_t* s = static_cast<uint8_t*>(realloc(c.s, full.end + 16));
  if (!s) return -2;
  memset(s + c.L.end, 0, full.end + 16 - c.L.end);
  c.s = s;
  c.L = full;
  parallel_for(n_wf, threads, [&](uint32_t w, Frame* stk) { emit_wf(c, w, stk); });
  exclusive_scan(c.cnt(CRR_LOAD_T_KEYS), n_wf);
  exclusive_scan(c.cnt(CRR_LOAD_T_KEY_BYTES), n_wf);
  parallel_for(n_wf, threads, [&](uint32_t w, Frame*) { dict_wf(c, w); });
  return 0;
}

constexpr CrcTab kCrcTab = make_crc_tab();

// the branch walk's count phase and its serial scans over a work buffer this allocates (k owns it):
// 0, -2 out of memory
int count_branches(const Ctx& c, int threads, Owned<NdcWork>& k) {
  const uint32_t n_wf = c.in.n_wf;
  k.L = carve_ndc(n_wf, 0);
  k.n_wf = n_wf;
  k.n_tasks = 0;
  k.s = static_cast<uint8_t*>(calloc(k.L.end + 16, 1));
  if (!k.s) return -2;
  parallel_for(n_wf, threads, [&](uint32_t w, Frame* stk) { branches_count_wf(c, k, w, stk); });
  for (int t = 0; t < 2; ++t) exclusive_scan(k.cnt(t), n_wf);
  return 0;
}

// what the four store-family calls start from: the load, the branch walk into a table of this call, and the tasks
// with their decisions over it (a) beside the dense after-image (img).  rc: 0, -1 invalid argument, -2 out of memory
struct StoreHost {
  Owned<Ctx> c;
  Owned<NdcWork> k;
  StoreIn a;
  ImageAfter img;
  Buf<crr_ndc_branch> branches;
  Buf<crr_vh_item> items;
  Buf<crr_branch_token> tokens;
  Buf<int64_t> branch_begin;
  Buf<int32_t> current;
  int rc;

  StoreHost(const crr_state_batch* in, const crr_repl_task* tasks, const crr_last_event* last_events, uint32_t n_tasks,
            const crr_ndc_result* results, const crr_ndc_route* routes, const crr_load_image* after, int threads)
      : img{after, in->n_wf} {
    rc = run_load(in, threads, c);
    if (rc != 0) return;
    rc = -2;
    if (count_branches(c, threads, k) != 0) return;
    const uint32_t n_wf = in->n_wf;
    a.tasks = tasks;
    a.last = last_events;
    a.results = results;
    a.routes = routes;
    a.n_branches = (uint64_t)k.cnt(kBrHist)[n_wf];
    a.n_items = (uint64_t)k.cnt(kBrItems)[n_wf];
    a.n_tasks = n_tasks;
    // (calloc(0) may be NULL: at least one element each)
    a.br.branches = (branches = zeroed<crr_ndc_branch>(a.n_branches + 1)).get();
    a.br.items = (items = zeroed<crr_vh_item>(a.n_items + 1)).get();
    a.br.tokens = (tokens = zeroed<crr_branch_token>(a.n_branches + 1)).get();
    a.br.branch_begin = (branch_begin = zeroed<int64_t>((uint64_t)n_wf + 1)).get();
    a.br.current = (current = zeroed<int32_t>((uint64_t)n_wf + 1)).get();
    if (!branches || !items || !tokens || !branch_begin || !current) return;
    parallel_for(n_wf, threads, [&](uint32_t w, Frame* stk) { branches_emit_wf(c, k, w, a.br, stk); });
    rc = 0;
  }
};

// the VersionHistories blob of every generated task at dst + off[i], by load_decode.h's sequential writer; a task
// whose blob does not come out at its planned length is left as zeros
void write_vh_blobs(const Ctx& c, const StoreIn& a, const ImageAfter& img, const uint64_t* off, uint8_t* dst,
                    uint32_t n_tasks, int threads) {
  parallel_for(n_tasks, threads, [&](uint32_t i, Frame*) {
    const uint64_t len = off[i + 1] - off[i];
    if (len == 0) return;
    StoreDecision D;
    store_decide(c, a, img, i, D);
    ByteSink K = {dst + off[i], len, 0};
    if (!D.generated() || !vh_blob_write(K, c, a, D) || K.len != len) memset(dst + off[i], 0, (size_t)len);
  });
}

}  // namespace

extern "C" int crr_load_states_host(const crr_state_batch* in, const crr_load_image* dst, crr_load_summary* summary,
                                    int threads) {
  if (!in || !summary) return -1;
  Owned<Ctx> c;
  const int rc = run_load(in, threads, c);
  if (rc != 0) return rc;
  const uint32_t n_wf = in->n_wf;
  int64_t totals[kCounters];
  for (int t = 0; t < kCounters; ++t) totals[t] = c.cnt(t)[n_wf];
  fill_summary(summary, c, totals, c.err()[0], c.err()[1], c.L.end);
  if (dst) {
    const size_t n = n_wf;
    if (dst->exec) memcpy(dst->exec, c.exec(), n * sizeof(crr_exec_row));
    for (int t = 0; t < 7; ++t)
      if (dst->rows[t]) memcpy(dst->rows[t], c.rows(t), (size_t)totals[t] * kRowBytes[t]);
    if (dst->offsets) memcpy(dst->offsets, c.cnt(0), (size_t)CRR_LOAD_TABLES * (n + 1) * sizeof(int64_t));
    if (dst->tokens) memcpy(dst->tokens, c.tokens(), (size_t)totals[CRR_LOAD_T_TOKEN]);
    if (dst->key_off) memcpy(dst->key_off, c.key_off(), (size_t)totals[CRR_LOAD_T_KEYS] * sizeof(uint64_t));
    if (dst->key_len) memcpy(dst->key_len, c.key_len(), (size_t)totals[CRR_LOAD_T_KEYS] * sizeof(uint32_t));
    if (dst->key_bytes) memcpy(dst->key_bytes, c.key_bytes(), (size_t)totals[CRR_LOAD_T_KEY_BYTES]);
    if (dst->status) memcpy(dst->status, c.status(), n * sizeof(int32_t));
    if (dst->flags) memcpy(dst->flags, c.flags(), n * sizeof(uint32_t));
  }
  return 0;
}

// the branch table of every loaded state (include/cadence_load_ndc.h): load_decode.h's count and emit phases as
// host loops over a work buffer laid out like the device's, a serial scan between them
extern "C" int crr_load_branches_host(const crr_state_batch* in, const crr_load_branches* dst, crr_load_ndc_sizes* plan,
                                      int threads) {
  if (!in || !plan) return -1;
  Owned<Ctx> c;
  const int rc = run_load(in, threads, c);
  if (rc != 0) return rc;
  const uint32_t n_wf = in->n_wf;
  Owned<NdcWork> k;
  if (count_branches(c, threads, k) != 0) return -2;
  memset(plan, 0, sizeof *plan);
  plan->n_wf = n_wf;
  plan->n_branches = (uint64_t)k.cnt(kBrHist)[n_wf];
  plan->n_items = (uint64_t)k.cnt(kBrItems)[n_wf];
  plan->work_needed = k.L.end;
  if (dst) {
    parallel_for(n_wf, threads, [&](uint32_t w, Frame* stk) { branches_emit_wf(c, k, w, *dst, stk); });
    if (n_wf == 0 && dst->branch_begin) dst->branch_begin[0] = 0;
  }
  return 0;
}

// the checksum to store for routed tasks (include/cadence_load_store.h): the load and the branch walk as above into
// a table of this call, then load_decode.h's store_task per task over the dense after-image
extern "C" int crr_load_store_checksums_host(const crr_state_batch* in, const crr_repl_task* tasks,
                                             const crr_last_event* last_events, uint32_t n_tasks,
                                             const crr_ndc_result* results, const crr_ndc_route* routes,
                                             const crr_load_image* after, crr_store_row* result, int threads) {
  if (!in || (n_tasks && (!tasks || !last_events || !results || !routes || !result))) return -1;
  if (after && in->n_wf && (!after->exec || !after->offsets)) return -1;
  StoreHost h(in, tasks, last_events, n_tasks, results, routes, after, threads);
  if (h.rc != 0) return h.rc;
  parallel_for(n_tasks, threads, [&](uint32_t i, Frame*) { store_task(h.c, h.a, h.img, kCrcTab.v, i, result); });
  return 0;
}

// the VersionHistories blob to store for routed tasks (include/cadence_load_store_vh.h): the same load, branch walk
// and decision, the lengths scanned serially, then load_decode.h's sequential writer per generated task
extern "C" int crr_load_store_vh_host(const crr_state_batch* in, const crr_repl_task* tasks,
                                      const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                                      const crr_ndc_route* routes, const crr_load_image* after, crr_vh_blob_row* rows,
                                      uint64_t* blob_off, uint8_t* out, size_t out_capacity, crr_vh_blob_sizes* plan,
                                      int threads) {
  if (!in || !plan || (n_tasks && (!tasks || !last_events || !results || !routes))) return -1;
  if (after && in->n_wf && (!after->exec || !after->offsets)) return -1;
  StoreHost h(in, tasks, last_events, n_tasks, results, routes, after, threads);
  if (h.rc != 0) return h.rc;
  const Buf<crr_vh_blob_row> row_buf = zeroed<crr_vh_blob_row>((uint64_t)n_tasks + 1);
  const Buf<uint64_t> off_buf = zeroed<uint64_t>((uint64_t)n_tasks + 1);
  if (!row_buf || !off_buf) return -2;
  crr_vh_blob_row* my_rows = row_buf.get();
  uint64_t* my_off = off_buf.get();
  parallel_for(n_tasks, threads, [&](uint32_t i, Frame*) { my_off[i] = vh_size_task(h.c, h.a, h.img, i, my_rows); });
  uint64_t generated = 0;
  for (uint32_t i = 0; i < n_tasks; ++i) generated += my_off[i] != 0;
  const uint64_t run = exclusive_scan(my_off, n_tasks);
  memset(plan, 0, sizeof *plan);
  plan->n_tasks = n_tasks;
  plan->n_generated = generated;
  plan->n_bytes = run;
  const uint64_t padded = align16(run);
  if (out && (uint64_t)out_capacity < padded) return -1;   // nothing written
  if (rows && n_tasks) memcpy(rows, my_rows, (size_t)n_tasks * sizeof(crr_vh_blob_row));
  if (blob_off) memcpy(blob_off, my_off, ((size_t)n_tasks + 1) * sizeof(uint64_t));
  if (out) {
    write_vh_blobs(h.c, h.a, h.img, my_off, out, n_tasks, threads);
    if (padded > run) memset(out + run, 0, (size_t)(padded - run));
  }
  return 0;
}

// the pending-entry mutation to store for routed tasks (include/cadence_load_mutation.h): the same load, branch walk
// and decision, load_decode.h's count pass per task, serial prefixes, then its emit pass into a directory of this
// call and the rows copied through it
extern "C" int crr_load_mutation_host(const crr_state_batch* in, const crr_repl_task* tasks,
                                      const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                                      const crr_ndc_route* routes, const crr_load_image* after, crr_mutation_row* rows,
                                      const crr_mutation_out* out, crr_mutation_sizes* plan, int threads) {
  if (!in || !plan || (n_tasks && (!tasks || !last_events || !results || !routes))) return -1;
  if (after && in->n_wf && (!after->exec || !after->offsets)) return -1;
  StoreHost h(in, tasks, last_events, n_tasks, results, routes, after, threads);
  if (h.rc != 0) return h.rc;
  const Buf<crr_mutation_row> row_buf = zeroed<crr_mutation_row>((uint64_t)n_tasks + 1);
  if (!row_buf) return -2;
  crr_mutation_row* my_rows = row_buf.get();
  parallel_for(n_tasks, threads, [&](uint32_t i, Frame*) { mutation_count_task(h.c, h.a, h.img, i, my_rows[i]); });
  memset(plan, 0, sizeof *plan);
  plan->n_tasks = n_tasks;
  for (uint32_t i = 0; i < n_tasks; ++i) {
    crr_mutation_row& o = my_rows[i];
    if (o.exec_index != 0xFFFFFFFFu) o.exec_index = (uint32_t)plan->n_exec++;
    for (int t = 0; t < CRR_MUTATION_MAPS; ++t) {
      o.map[t].upsert_begin = (uint32_t)plan->n_upsert[t];
      o.map[t].delete_begin = (uint32_t)plan->n_delete[t];
      plan->n_upsert[t] += o.map[t].n_upsert;
      plan->n_delete[t] += o.map[t].n_delete;
    }
  }
  bool ok = true;
  uint64_t dir_bytes = align16(plan->n_exec * sizeof(uint64_t));
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) {
    dir_bytes += align16(plan->n_upsert[t] * sizeof(uint64_t));
    if (plan->n_upsert[t] > 0xFFFFFFFFull || plan->n_delete[t] > 0xFFFFFFFFull) ok = false;
  }
  plan->run_work_needed = dir_bytes;
  if (out && ok) {
    auto usable = [](const void* p, uint64_t capacity, uint64_t total) { return capacity >= total && (total == 0 || p); };
    ok = usable(out->exec, out->exec_capacity, plan->n_exec);
    for (int t = 0; t < CRR_MUTATION_MAPS; ++t)
      ok = ok && usable(out->upsert[t], out->upsert_capacity[t], plan->n_upsert[t]) &&
           usable(out->deleted[t], out->delete_capacity[t], plan->n_delete[t]);
  }
  if (!ok) return -1;   // nothing written
  if (rows && n_tasks) memcpy(rows, my_rows, (size_t)n_tasks * sizeof(crr_mutation_row));
  if (!out || !plan->n_exec) return 0;
  MutDst d;
  memset(&d, 0, sizeof d);
  d.n_exec = plan->n_exec;
  const Buf<uint64_t> dir_exec = zeroed<uint64_t>(plan->n_exec);
  Buf<uint64_t> dir[CRR_MUTATION_MAPS];
  ok = dir_exec != nullptr;
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) {
    dir[t] = zeroed<uint64_t>(plan->n_upsert[t] + 1);
    ok = ok && dir[t];
    d.dir[t] = dir[t].get();
    d.keys[t] = out->deleted[t];
    d.base[t] = static_cast<const uint8_t*>(after->rows[t]);
    d.n_upsert[t] = plan->n_upsert[t];
    d.n_delete[t] = plan->n_delete[t];
  }
  d.dir_exec = dir_exec.get();
  if (!ok) return -2;
  memset(d.dir_exec, 0xFF, (size_t)plan->n_exec * sizeof(uint64_t));
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) memset(d.dir[t], 0xFF, (size_t)plan->n_upsert[t] * sizeof(uint64_t));
  parallel_for(n_tasks, threads, [&](uint32_t i, Frame*) { mutation_emit_task(h.c, h.a, h.img, i, my_rows, d); });
  auto gather = [&](const void* table, const uint64_t* dr, uint32_t row_bytes, uint64_t n_rows, void* dst) {
    const uint32_t words = row_bytes / 8;
    uint64_t* q = static_cast<uint64_t*>(dst);
    for (uint64_t g = 0; g < n_rows * words; ++g) q[g] = mutation_gather_word(static_cast<const uint64_t*>(table), dr, words, g);
  };
  gather(after->exec, d.dir_exec, sizeof(crr_exec_row), plan->n_exec, out->exec);
  for (int t = 0; t < CRR_MUTATION_MAPS; ++t) gather(after->rows[t], d.dir[t], kRowBytes[t], plan->n_upsert[t], out->upsert[t]);
  return 0;
}

// the execution blob to store for routed tasks (include/cadence_load_store_exec.h): the same load, branch walk and
// decision; the VersionHistories blobs of the same tasks written first into a buffer of this call (as
// crr_load_store_vh_host writes them); then load_decode.h's decision and splice per task -- sized through the edit
// script the device records (so both builds flag the same blobs), written by the sequential ByteSink emitter
extern "C" int crr_load_store_exec_host(const crr_state_batch* in, const crr_repl_task* tasks,
                                        const crr_last_event* last_events, uint32_t n_tasks, const crr_ndc_result* results,
                                        const crr_ndc_route* routes, const crr_load_image* after,
                                        const crr_exec_blob_task* exec_tasks, const crr_blob_batch* task_blobs,
                                        const uint8_t* upserts, crr_exec_blob_row* rows, uint64_t* blob_off, uint8_t* out,
                                        size_t out_capacity, crr_exec_blob_sizes* plan, int threads) {
  if (!in || !plan || (n_tasks && (!tasks || !last_events || !results || !routes || !exec_tasks))) return -1;
  if (after && in->n_wf && (!after->exec || !after->offsets)) return -1;
  if (task_blobs && ((task_blobs->n_wf && !task_blobs->wf) || (task_blobs->n_blobs && (!task_blobs->bytes || !task_blobs->blob_off))))
    return -1;
  StoreHost h(in, tasks, last_events, n_tasks, results, routes, after, threads);
  if (h.rc != 0) return h.rc;
  const Buf<crr_vh_blob_row> vh_row_buf = zeroed<crr_vh_blob_row>((uint64_t)n_tasks + 1);
  const Buf<uint64_t> vh_off_buf = zeroed<uint64_t>((uint64_t)n_tasks + 1);
  const Buf<crr_exec_blob_row> row_buf = zeroed<crr_exec_blob_row>((uint64_t)n_tasks + 1);
  const Buf<uint64_t> off_buf = zeroed<uint64_t>((uint64_t)n_tasks + 1);
  if (!vh_row_buf || !vh_off_buf || !row_buf || !off_buf) return -2;
  crr_vh_blob_row* vh_rows = vh_row_buf.get();
  uint64_t* vh_off = vh_off_buf.get();
  crr_exec_blob_row* my_rows = row_buf.get();
  uint64_t* my_off = off_buf.get();
  parallel_for(n_tasks, threads, [&](uint32_t i, Frame*) { vh_off[i] = vh_size_task(h.c, h.a, h.img, i, vh_rows); });
  const Buf<uint8_t> vh_buf = zeroed<uint8_t>(exclusive_scan(vh_off, n_tasks) + 1);
  if (!vh_buf) return -2;
  uint8_t* vh_bytes = vh_buf.get();
  write_vh_blobs(h.c, h.a, h.img, vh_off, vh_bytes, n_tasks, threads);
  ExecIn x;
  memset(&x, 0, sizeof x);
  x.xt = exec_tasks;
  x.vh_rows = vh_rows;
  x.vh_off = vh_off;
  x.vh_total = vh_off[n_tasks];
  if (task_blobs && task_blobs->n_wf && task_blobs->blob_off) pack_task_blobs(x, *task_blobs);
  x.upserts = upserts;
  parallel_for(n_tasks, threads, [&](uint32_t i, Frame* stk) {
    ExecScript S;
    bool vh_bad;
    my_off[i] = exec_size_task(h.c, h.a, h.img, x, i, my_rows, &S, vh_bad, stk);
  });
  memset(plan, 0, sizeof *plan);
  plan->n_tasks = n_tasks;
  for (uint32_t i = 0; i < n_tasks; ++i) {
    plan->n_blobs += my_off[i] != 0;
    plan->n_host += my_off[i] == 0 && my_rows[i].flags != 0;
  }
  const uint64_t run = exclusive_scan(my_off, n_tasks);
  plan->n_bytes = run;
  if (out && (uint64_t)out_capacity < run) return -1;   // nothing written
  if (rows && n_tasks) memcpy(rows, my_rows, (size_t)n_tasks * sizeof(crr_exec_blob_row));
  if (blob_off) memcpy(blob_off, my_off, ((size_t)n_tasks + 1) * sizeof(uint64_t));
  if (out) {
    parallel_for(n_tasks, threads, [&](uint32_t i, Frame* stk) {
      const uint64_t len = my_off[i + 1] - my_off[i];
      if (len == 0) return;
      crr_exec_blob_row row;
      StoreDecision D;
      ExecTask T;
      bool vh_bad;
      ExecSinkEm em = {{out + my_off[i], len, 0}, in->bytes, vh_bytes, x.tb_bytes};
      if (!exec_plan_task(h.c, h.a, h.img, x, i, row, D, T, vh_bad, stk) || !exec_walk(h.c, D.S.R, T, em, stk) || em.K.len != len)
        memset(out + my_off[i], 0, (size_t)len);
    });
  }
  return 0;
}

// the resumed replay of routed tasks planned from the loaded states (include/cadence_load_resume.h): the same load,
// then load_decode.h's decisions over a work buffer laid out like the device's -- the bids as a loop that keeps the
// lowest index, the prefixes as serial scans, the byte gather chunk by chunk through the device's own function
extern "C" int crr_load_resume_host(const crr_state_batch* in, const crr_repl_task* tasks, const crr_ndc_route* routes,
                                    uint32_t n_tasks, const crr_blob_batch* task_blobs, const int32_t* counts,
                                    crr_load_resume_row* rows, const crr_load_resume_out* out, crr_workflow* wf,
                                    uint8_t* arena, size_t arena_capacity, crr_load_resume_sizes* plan,
                                    crr_load_resume_totals* totals, int threads) {
  if (!in || !plan || (n_tasks && (!tasks || !routes || !task_blobs))) return -1;
  if (task_blobs && ((task_blobs->n_wf && !task_blobs->wf) || !task_blobs->blob_off || (task_blobs->n_blobs && !task_blobs->bytes)))
    return -1;
  Owned<Ctx> c;
  const int rc = run_load(in, threads, c);
  if (rc != 0) return rc;
  const uint32_t n_wf = in->n_wf;
  ResumeIn r;
  memset(&r, 0, sizeof r);
  r.tasks = tasks;
  r.routes = routes;
  r.n_tasks = n_tasks;
  if (task_blobs) pack_task_blobs(r, *task_blobs);
  Owned<ResumeWork> k;
  k.L = carve_resume(n_wf);
  k.n_wf = n_wf;
  k.s = static_cast<uint8_t*>(calloc(k.L.end + 16, 1));
  if (!k.s) return -2;
  int ret = 0;
  memset(k.winner(), 0xFF, (size_t)n_wf * sizeof(uint32_t));
  for (uint32_t i = n_tasks; i-- > 0;)   // descending: the lowest index is written last
    if (resume_candidate(c, r, i) == CRR_RESUME_APPLIED) k.winner()[tasks[i].wf] = i;
  uint64_t run[kResCols] = {0, 0, 0, 0, 0, 0};
  for (uint32_t p = 0; p < n_wf; ++p) {
    uint64_t v[kResCols];
    resume_counts(c, r, k.winner()[p], p, v);
    for (int col = 0; col < kResCols; ++col) {
      k.off(col)[p] = run[col];
      run[col] += v[col];
    }
  }
  for (int col = 0; col < kResCols; ++col) k.off(col)[n_wf] = run[col];
  memset(plan, 0, sizeof *plan);
  plan->n_tasks = n_tasks;
  plan->n_wf = n_wf;
  plan->n_applied = run[kResApplied];
  plan->n_blobs = run[kResBlobs];
  plan->blob_bytes = run[kResBlobBytes];
  plan->n_keys = run[kResKeys];
  plan->key_bytes = run[kResKeyBytes];
  plan->token_bytes = run[kResTokenBytes];
  plan->n_bytes = align16(run[kResBlobBytes]) + run[kResKeyBytes];
  plan->work_needed = k.L.end;
  if (run[kResBlobs] >= 0xFFFFFFFFull || run[kResKeys] > 0xFFFFFFFFull || run[kResTokenBytes] > 0xFFFFFFFFull) ret = -1;
  if (totals) {
    memset(totals, 0, sizeof *totals);
    totals->arena_bytes = plan->token_bytes;
  }
  if (ret == 0 && out) {
    bool ok = out->bytes_capacity >= plan->n_bytes && (plan->n_bytes == 0 || out->bytes) && out->blob_off &&
              out->blob_capacity >= plan->n_blobs && out->key_capacity >= plan->n_keys &&
              (plan->n_keys == 0 || (out->key_off && out->key_len));
    if (n_wf && (!out->wf || !out->key_begin || !out->key_count || !out->task_of)) ok = false;
    if (!ok) ret = -1;   // nothing written
  }
  if (ret == 0 && (wf || arena) && (uint64_t)arena_capacity < plan->token_bytes) ret = -1;
  if (ret != 0) return ret;
  if (rows)
    for (uint32_t i = 0; i < n_tasks; ++i) rows[i] = resume_row(c, r, k.winner(), i);
  const ResumeTotals T = {plan->n_blobs, plan->blob_bytes, plan->n_keys, plan->key_bytes, plan->n_bytes};
  if (out) {
    for (uint32_t p = 0; p < n_wf; ++p) {
      out->wf[p] = resume_blob_wf(r, k, p);
      out->key_begin[p] = (uint32_t)k.off(kResKeys)[p];
      out->key_count[p] = (uint32_t)(k.off(kResKeys)[p + 1] - k.off(kResKeys)[p]);
      const uint32_t task = k.winner()[p];
      out->task_of[p] = task == kResNoTask ? -1 : (int32_t)task;
    }
    for (uint64_t j = 0; j <= T.n_blobs; ++j) out->blob_off[j] = n_wf ? resume_blob_off(r, k, T, j) : 0;
    for (uint64_t e = 0; e < T.n_keys; ++e) resume_key(c, k, T, e, out->key_off[e], out->key_len[e]);
    const uint64_t n_chunks = (T.n_bytes + 15) / 16;
    for (uint64_t i = 0; i < n_chunks; ++i) {
      uint64_t lo, hi;
      resume_gather_chunk(c, r, k, T, i, lo, hi);
      const uint64_t n = T.n_bytes - 16 * i < 16 ? T.n_bytes - 16 * i : 16;
      for (uint64_t b = 0; b < n; ++b) out->bytes[16 * i + b] = (uint8_t)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xffu);
    }
  }
  if (counts && wf && out && n_wf) {
    if (plan->token_bytes && !arena) return -1;
    uint64_t base[kResCaps] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t p = 0; p < n_wf; ++p) {
      uint64_t cap[kResCaps];
      resume_caps(c, k, counts, n_wf, p, cap);
      wf[p] = resume_descriptor(c, k, out->wf, counts, n_wf, p, cap, base, arena, arena_capacity);
      for (int t = 0; t < kResCaps; ++t) base[t] += cap[t];
    }
    if (totals)
      for (int t = 0; t < kResCaps; ++t) totals->table_rows[t] = base[t];
  }
  return 0;
}

extern "C" int crr_load_states_verify_host(const crr_state_batch* in, const crr_stored_checksum* stored,
                                           int64_t invalidate_before_ns, crr_verify_row* result, int threads) {
  if (!in || (in->n_wf && !result)) return -1;
  Owned<Ctx> c;
  const int rc = run_load(in, threads, c);
  if (rc != 0) return rc;
  parallel_for(in->n_wf, threads, [&](uint32_t w, Frame* stk) {
    verify_wf(c, w, kCrcTab.v, stored, invalidate_before_ns, result, stk);
  });
  return 0;
}
