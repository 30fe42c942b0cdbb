// load_resume_asan.cpp -- a stand-alone check of the host restatement of the resumed-replay planner
// (crr_load_resume_host, include/cadence_load_resume.h) under AddressSanitizer / UndefinedBehaviorSanitizer.
// Hand-written states -- zero to several keyed entries, with and without reset points, with and without a branch
// token, some that do not load -- are loaded by crr_load_states_host; tasks name them in shuffled order with garbage
// routes, workflow indices past the batch, several tasks for one workflow and blob ranges outside the task batch.  The
// result is compared with this file's own: the winner through a std::map, the gathered bytes, offsets and seeds built
// by appending strings, the descriptors by running sums.  Every input array and every output buffer lies in a heap
// block of exactly its size (the task blobs' bytes too: the restatement decodes none of them), so a read or a write
// past any of them is reported.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/load_resume_asan.cpp cadence_amd/csrc/load_states.cpp -o build/load_resume_asan -lpthread
//   build/load_resume_asan
//
// Exit status 0 and a line of counts when everything equals this file's and no sanitizer report ended the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "cadence_load_resume.h"

#include "load_asan_common.h"

namespace {

std::string execution_blob(int n_points, const std::string& token) {
  Wr vh;
  vh.u8(0x59), vh.i32(10, 0), vh.list(20, 12, 1);
  if (!token.empty()) vh.str(10, token);
  vh.list(20, 12, 1), vh.i64(10, 19), vh.i64(20, 3), vh.stop(), vh.stop(), vh.stop();
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

int fail(const char* what, long a = 0, long b = 0) {
  fprintf(stderr, "load_resume_asan: %s (%ld, %ld)\n", what, a, b);
  return 1;
}

struct Tally {
  long applied = 0, shadowed = 0, not_routed = 0, not_loaded = 0, keys = 0, bytes = 0, empty_dict = 0, no_token = 0;
};

// one batch of n_wf states; workflow w has (w + shape) % 4 activities and timers, w % 3 reset points, a token unless
// w % 5 == 2, and two execution blobs (it does not load) when w % 7 == 6
int check(uint32_t n_wf, int shape, Tally& tally) {
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
    const int n = (int)((w + shape) % 4);
    const uint32_t first = (uint32_t)meta.size();
    for (int i = n - 1; i >= 0; --i) {
      Wr a, t;
      a.i64(10, 3), a.i64(20, -23), a.str(28, "activity-" + std::to_string(w) + "-" + std::string((size_t)(3 * i), 'x')), a.stop();
      add(CRR_STATE_ACTIVITY, 5 + 10 * i, "", a.b);
      t.i64(10, 3), t.i64(12, 6 + 10 * i), t.i64(16, 1), t.stop();
      add(CRR_STATE_TIMER, 0, "timer-" + std::to_string(i), t.b);
    }
    const std::string token = w % 5 == 2 ? "" : "token-of-" + std::to_string(w);
    add(CRR_STATE_EXECUTION, 0, "", execution_blob((int)(w % 3), token));
    if (w % 7 == 6) add(CRR_STATE_EXECUTION, 0, "", execution_blob(0, token));
    wf.push_back({first, (uint32_t)meta.size() - first, 60});
  }
  bytes.resize(bytes.size() + 32, 0);   // readable CRR_INGEST_PAD bytes past the last blob, as the loader's interface asks
  const StateBatch batch(bytes, off, meta, wf, strings);
  const crr_state_batch& in = batch.in;

  // the loaded image, by the loader
  crr_load_summary S;
  if (crr_load_states_host(&in, nullptr, &S, 1) != 0) return fail("sizing the load");
  Image B;
  B.offsets = static_cast<int64_t*>(malloc((size_t)CRR_LOAD_TABLES * (n_wf + 1) * sizeof(int64_t)));
  B.status = static_cast<int32_t*>(malloc(n_wf * sizeof(int32_t)));
  B.tokens = static_cast<uint8_t*>(malloc((size_t)S.totals[CRR_LOAD_T_TOKEN]));
  B.key_off = static_cast<uint64_t*>(malloc((size_t)S.totals[CRR_LOAD_T_KEYS] * sizeof(uint64_t)));
  B.key_len = static_cast<uint32_t*>(malloc((size_t)S.totals[CRR_LOAD_T_KEYS] * sizeof(uint32_t)));
  B.key_bytes = static_cast<uint8_t*>(malloc((size_t)S.totals[CRR_LOAD_T_KEY_BYTES]));
  if (crr_load_states_host(&in, &B, &S, 1) != 0) return fail("the load");
  auto offs = [&](int t) { return B.offsets + (size_t)t * (n_wf + 1); };

  // the tasks: two per workflow in a shuffled order and six others; the blobs are bytes of this file's
  const uint32_t n = 2 * n_wf + 6;
  std::vector<crr_repl_task> rt(n);
  std::vector<crr_ndc_route> routes(n);
  std::vector<crr_blob_wf> tw(n);
  std::vector<uint8_t> tbytes;
  std::vector<uint64_t> toff{0};
  std::vector<std::vector<std::string>> blobs_of(n);
  for (uint32_t k = 0; k < n; ++k) {
    memset(&rt[k], 0, sizeof rt[k]), memset(&routes[k], 0, sizeof routes[k]), memset(&tw[k], 0, sizeof tw[k]);
    routes[k].route = CRR_ROUTE_APPLY_CURRENT;
    rt[k].wf = k < 2 * n_wf ? (uint32_t)(((uint64_t)k * 7 + 3) % n_wf) : 0;
    if (k % 5 == 3) routes[k].route = CRR_ROUTE_NON_CURRENT;
    if (k % 11 == 7) routes[k].route = 77;
    if (k % 13 == 9) routes[k].route = -1;
    if (k == 2 * n_wf) rt[k].wf = n_wf;                  // past the batch
    if (k == 2 * n_wf + 1) rt[k].wf = 0xFFFFFFFFu;
    if (k == 2 * n_wf + 2) rt[k].wf = n_wf + 1000, routes[k].route = CRR_ROUTE_REBUILD;
    const uint32_t nb = k % 3;                           // 0 .. 2 blobs, some of them empty
    tw[k].blob_begin = (uint32_t)(toff.size() - 1), tw[k].blob_count = nb;
    tw[k].init_version = 100 + k, tw[k].now_ns = 1000000 + k, tw[k].retention_days = (int32_t)(k % 4);
    tw[k].flags = (int32_t)(k % 2 ? CRR_WF_FLAG_REFRESH_TASKS : 0) | 64;   // (an unknown bit: not carried over)
    tw[k].new_run_wf = k % 4 == 0 ? (int32_t)((k + 1) % n) : (k % 4 == 1 ? 1 << 30 : -1);
    tw[k].final_token_len = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < nb; ++j) {
      const std::string b = j == 1 && k % 2 ? std::string() : "blob-" + std::to_string(k) + "-" + std::string((size_t)(k % 9 + j), 'y');
      blobs_of[k].push_back(b);
      tbytes.insert(tbytes.end(), b.begin(), b.end());
      toff.push_back(tbytes.size());
    }
  }
  const uint32_t n_tblobs = (uint32_t)(toff.size() - 1);
  // blob ranges outside the task batch: applied with no blobs
  tw[2 * n_wf + 3].blob_begin = n_tblobs + 5, tw[2 * n_wf + 3].blob_count = 1, blobs_of[2 * n_wf + 3].clear();
  tw[2 * n_wf + 4].blob_begin = 1, tw[2 * n_wf + 4].blob_count = 0xFFFFFFFFu, blobs_of[2 * n_wf + 4].clear();
  rt[2 * n_wf + 3].wf = n_wf - 1, rt[2 * n_wf + 4].wf = n_wf / 2;

  // this file's expectation
  std::map<uint32_t, uint32_t> winner;
  std::vector<crr_load_resume_row> want_rows(n);
  for (uint32_t k = 0; k < n; ++k) {
    crr_load_resume_row& R = want_rows[k];
    R.position = 0xFFFFFFFFu;
    if (routes[k].route != CRR_ROUTE_APPLY_CURRENT) {
      R.outcome = CRR_RESUME_NOT_ROUTED, ++tally.not_routed;
    } else if (rt[k].wf >= n_wf || B.status[rt[k].wf] != CRR_LOAD_OK) {
      R.outcome = CRR_RESUME_NOT_LOADED, ++tally.not_loaded;
    } else {
      R.position = rt[k].wf;
      if (winner.count(rt[k].wf)) R.outcome = CRR_RESUME_SHADOWED, ++tally.shadowed;
      else R.outcome = CRR_RESUME_APPLIED, winner[rt[k].wf] = k, ++tally.applied;
    }
  }
  std::string all_blobs, all_keys, want_arena;
  std::vector<uint64_t> want_off{0}, want_key_off;
  std::vector<uint32_t> want_key_len, want_kb(n_wf), want_kc(n_wf);
  std::vector<crr_blob_wf> want_wf(n_wf);
  std::vector<int32_t> want_task(n_wf);
  std::vector<crr_workflow> want_desc(n_wf);
  std::vector<int32_t> counts((size_t)CRR_RESUME_COUNT_ROWS * n_wf);
  for (size_t i = 0; i < counts.size(); ++i) counts[i] = (int32_t)((i * 2654435761u) % 7) - 1;   // -1 .. 5
  uint64_t base[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t p = 0; p < n_wf; ++p) {
    crr_blob_wf& W = want_wf[p];
    memset(&W, 0, sizeof W);
    crr_workflow& D = want_desc[p];
    memset(&D, 0, sizeof D);
    want_kb[p] = (uint32_t)want_key_len.size();
    W.blob_begin = (uint32_t)(want_off.size() - 1);
    const bool applied = winner.count(p) != 0;
    want_task[p] = applied ? (int32_t)winner[p] : -1;
    if (applied) {
      const uint32_t k = winner[p];
      W = tw[k];
      W.blob_begin = (uint32_t)(want_off.size() - 1), W.blob_count = (uint32_t)blobs_of[k].size();
      const int32_t nr = tw[k].new_run_wf;
      W.new_run_wf = -1;
      if (nr >= 0 && (uint32_t)nr < n && want_rows[nr].outcome == CRR_RESUME_APPLIED) W.new_run_wf = (int32_t)rt[nr].wf;
      for (auto& b : blobs_of[k]) all_blobs += b, want_off.push_back(all_blobs.size());
      for (int64_t e = offs(CRR_LOAD_T_KEYS)[p]; e < offs(CRR_LOAD_T_KEYS)[p + 1]; ++e) {
        want_key_off.push_back(all_keys.size());   // + seed_base, below
        want_key_len.push_back(B.key_len[e]);
        all_keys.append(reinterpret_cast<const char*>(B.key_bytes) + B.key_off[e], B.key_len[e]);
      }
      if (offs(CRR_LOAD_T_KEYS)[p] == offs(CRR_LOAD_T_KEYS)[p + 1]) ++tally.empty_dict;
      const int64_t t0 = offs(CRR_LOAD_T_TOKEN)[p], t1 = offs(CRR_LOAD_T_TOKEN)[p + 1];
      D.start_token_off = (uint32_t)want_arena.size(), D.start_token_len = (uint32_t)(t1 - t0);
      want_arena.append(reinterpret_cast<const char*>(B.tokens) + t0, (size_t)(t1 - t0));
      want_arena.resize((want_arena.size() + 7) & ~(size_t)7, '\0');
      if (t0 == t1) ++tally.no_token;
      D.flags = CRR_WF_FLAG_RESUME;
    } else {
      W.final_token_len = 0xFFFFFFFFu, W.new_run_wf = -1;
      D.start_token_off = (uint32_t)want_arena.size();
    }
    want_kc[p] = (uint32_t)want_key_len.size() - want_kb[p];
    D.ev_count = W.blob_count ? counts[p] : 0;
    D.empty_batch_at = W.blob_count ? counts[n_wf + p] : -1;
    D.init_version = W.init_version, D.now_ns = W.now_ns, D.retention_days = W.retention_days;
    D.flags |= W.flags & (CRR_WF_FLAG_NEW_RUN | CRR_WF_FLAG_REFRESH_TASKS);
    D.final_token_len = 0xFFFFFFFFu;
    int64_t* bases[8] = {&D.act_base, &D.timer_base, &D.child_base, &D.rc_base, &D.sig_base, &D.vh_base, &D.rp_base, &D.task_base};
    int32_t* caps[8] = {&D.act_cap, &D.timer_cap, &D.child_cap, &D.rc_cap, &D.sig_cap, &D.vh_cap, &D.rp_cap, &D.task_cap};
    for (int t = 0; t < 8; ++t) {
      const int32_t ins = counts[(size_t)(2 + t) * n_wf + p];
      const int64_t loaded = applied && t < 7 ? offs(t)[p + 1] - offs(t)[p] : 0;
      *caps[t] = (int32_t)(loaded + (ins > 0 ? ins : 0));
      *bases[t] = (int64_t)base[t];
      base[t] += (uint64_t)*caps[t];
    }
  }
  const uint64_t seed_base = (all_blobs.size() + 15) / 16 * 16;
  for (auto& o : want_key_off) o += seed_base;
  std::string want_bytes = all_blobs;
  want_bytes.resize((size_t)seed_base, '\0');
  want_bytes += all_keys;
  tally.keys += (long)want_key_len.size(), tally.bytes += (long)want_bytes.size();

  uint8_t* d_tbytes = exact(tbytes);
  uint64_t* d_toff = exact(toff);
  crr_blob_wf* d_tw = exact(tw);
  crr_blob_batch tb;
  memset(&tb, 0, sizeof tb);
  tb.bytes = d_tbytes, tb.blob_off = d_toff, tb.n_blobs = n_tblobs, tb.n_wf = n, tb.wf = d_tw;
  crr_repl_task* d_rt = exact(rt);
  crr_ndc_route* d_routes = exact(routes);
  int32_t* d_counts = exact(counts);

  crr_load_resume_sizes P;
  crr_load_resume_totals Q;
  if (crr_load_resume_host(&in, d_rt, d_routes, n, &tb, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &P, &Q, 1) != 0) return fail("sizing");
  if (P.n_applied != winner.size() || P.n_blobs != want_off.size() - 1 || P.blob_bytes != all_blobs.size() ||
      P.n_keys != want_key_len.size() || P.key_bytes != all_keys.size() || P.token_bytes != want_arena.size() ||
      P.n_bytes != want_bytes.size() || P.n_wf != n_wf || P.n_tasks != n)
    return fail("the plan's totals", (long)P.n_applied, (long)P.n_bytes);
  // exact-size outputs; then the bytes, the blobs, the keys and the arena one short each: refused, nothing written
  int bad = 0;
  for (int shorter = -1; shorter < 4 && !bad; ++shorter) {
    uint64_t cap[4] = {P.n_bytes, P.n_blobs, P.n_keys, P.token_bytes};
    if (shorter >= 0) {
      if (cap[shorter] == 0) continue;
      cap[shorter] -= 1;
    }
    crr_load_resume_out o;
    memset(&o, 0, sizeof o);
    o.bytes = static_cast<uint8_t*>(malloc((size_t)cap[0])), o.bytes_capacity = cap[0];
    o.blob_off = static_cast<uint64_t*>(malloc((size_t)(cap[1] + 1) * sizeof(uint64_t))), o.blob_capacity = cap[1];
    o.wf = static_cast<crr_blob_wf*>(malloc(n_wf * sizeof(crr_blob_wf)));
    o.key_begin = static_cast<uint32_t*>(malloc(n_wf * sizeof(uint32_t)));
    o.key_count = static_cast<uint32_t*>(malloc(n_wf * sizeof(uint32_t)));
    o.key_off = static_cast<uint64_t*>(malloc((size_t)cap[2] * sizeof(uint64_t)));
    o.key_len = static_cast<uint32_t*>(malloc((size_t)cap[2] * sizeof(uint32_t))), o.key_capacity = cap[2];
    o.task_of = static_cast<int32_t*>(malloc(n_wf * sizeof(int32_t)));
    crr_load_resume_row* rows = static_cast<crr_load_resume_row*>(malloc(n * sizeof(crr_load_resume_row)));
    crr_workflow* desc = static_cast<crr_workflow*>(malloc(n_wf * sizeof(crr_workflow)));
    uint8_t* arena = static_cast<uint8_t*>(malloc((size_t)cap[3]));
    const int rc = crr_load_resume_host(&in, d_rt, d_routes, n, &tb, d_counts, rows, &o, desc, arena, (size_t)cap[3], &P, &Q,
                                        shorter < 0 ? 1 : 2);
    if (shorter >= 0) {
      if (rc != -1) bad = fail("a short capacity was not refused", shorter, rc);
    } else if (rc != 0) {
      bad = fail("the run", rc);
    } else {
      if (memcmp(rows, want_rows.data(), n * sizeof rows[0]) != 0) bad = fail("rows differ");
      if (!bad && P.n_bytes && memcmp(o.bytes, want_bytes.data(), (size_t)P.n_bytes) != 0) bad = fail("bytes differ");
      if (!bad && memcmp(o.blob_off, want_off.data(), want_off.size() * 8) != 0) bad = fail("blob offsets differ");
      if (!bad && memcmp(o.wf, want_wf.data(), n_wf * sizeof(crr_blob_wf)) != 0) bad = fail("blob workflows differ");
      if (!bad && (memcmp(o.key_begin, want_kb.data(), n_wf * 4) != 0 || memcmp(o.key_count, want_kc.data(), n_wf * 4) != 0)) bad = fail("seed ranges differ");
      if (!bad && P.n_keys && (memcmp(o.key_off, want_key_off.data(), (size_t)P.n_keys * 8) != 0 || memcmp(o.key_len, want_key_len.data(), (size_t)P.n_keys * 4) != 0))
        bad = fail("seeds differ");
      if (!bad && memcmp(o.task_of, want_task.data(), n_wf * 4) != 0) bad = fail("task_of differs");
      for (uint32_t p = 0; p < n_wf && !bad; ++p)
        if (memcmp(&desc[p], &want_desc[p], sizeof desc[p]) != 0) bad = fail("descriptor of position", p, desc[p].act_cap);
      if (!bad && P.token_bytes && memcmp(arena, want_arena.data(), (size_t)P.token_bytes) != 0) bad = fail("arena differs");
      for (int t = 0; t < 8 && !bad; ++t)
        if (Q.table_rows[t] != base[t]) bad = fail("table rows", t, (long)Q.table_rows[t]);
      if (!bad && Q.arena_bytes != want_arena.size()) bad = fail("arena bytes");
    }
    free(o.bytes), free(o.blob_off), free(o.wf), free(o.key_begin), free(o.key_count), free(o.key_off), free(o.key_len), free(o.task_of);
    free(rows), free(desc), free(arena);
  }
  free(d_tbytes), free(d_toff), free(d_tw), free(d_rt), free(d_routes), free(d_counts);
  return bad;
}

}  // namespace

int main() {
  int batches = 0;
  Tally t;
  for (uint32_t n_wf : {1u, 2u, 6u, 13u, 40u, 150u})
    for (int shape = 0; shape < 4; ++shape) {
      if (check(n_wf, shape, t)) {
        fprintf(stderr, "n_wf %u, shape %d\n", n_wf, shape);
        return 1;
      }
      ++batches;
    }
  if (t.applied < 300 || t.shadowed < 50 || t.not_routed < 100 || t.not_loaded < 50 || t.keys < 500 || t.empty_dict < 5 || t.no_token < 20) {
    fprintf(stderr, "too little exercised: %ld applied, %ld shadowed, %ld not routed, %ld not loaded, %ld keys, %ld empty dictionaries, %ld without token\n",
            t.applied, t.shadowed, t.not_routed, t.not_loaded, t.keys, t.empty_dict, t.no_token);
    return 1;
  }
  printf("load_resume_asan: %d batches as this file builds them: %ld applied, %ld shadowed, %ld not routed, %ld not loaded, %ld seeds, "
         "%ld gathered bytes, %ld empty dictionaries, %ld states without a token, no sanitizer report\n",
         batches, t.applied, t.shadowed, t.not_routed, t.not_loaded, t.keys, t.bytes, t.empty_dict, t.no_token);
  return 0;
}
