// load_branches_asan.cpp -- a stand-alone check of the host branch extraction (crr_load_branches_host,
// include/cadence_load_ndc.h) under AddressSanitizer / UndefinedBehaviorSanitizer: execution blobs whose
// VersionHistories hold one to four branches, tokens of several lengths, absent tokens and absent Items fields,
// each batch's bytes and every output buffer in a heap block of exactly its size, so a read past a blob's end or
// a write past the counted table is reported; and every truncation length of one such blob, which must come back
// without branches.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/load_branches_asan.cpp cadence_amd/csrc/load_states.cpp -o build/load_branches_asan -lpthread
//   build/load_branches_asan
//
// Exit status 0 and a line of counts when every state's table equals the branches this file wrote, every
// truncation has none, and no sanitizer report ended the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "cadence_load_ndc.h"

#include "load_asan_common.h"

namespace {

struct Branch {
  bool has_token, has_items;
  std::string token;
  std::vector<std::pair<int64_t, int64_t>> items;
};

std::string version_histories(int32_t current, const std::vector<Branch>& hs) {
  Wr w;
  w.u8(0x59), w.i32(10, current), w.list(20, 12, hs.size());
  for (auto& h : hs) {
    if (h.has_token) w.str(10, h.token);
    if (h.has_items) {
      w.list(20, 12, h.items.size());
      for (auto& it : h.items) w.i64(10, it.first), w.i64(20, it.second), w.stop();
    }
    w.stop();
  }
  w.stop();
  return w.b;
}

// the version histories last: the last branch's bytes lie at the end of the block
std::string execution_blob(int32_t current, const std::vector<Branch>& hs) {
  Wr w;
  w.i32(34, 1), w.i64(50, 18), w.i64(52, 15), w.str(124, "thriftrw"), w.str(122, version_histories(current, hs)), w.stop();
  return w.b;
}

struct Table {
  int rc;
  crr_load_ndc_sizes sizes;
  std::vector<crr_ndc_branch> branches;
  std::vector<crr_vh_item> items;
  std::vector<crr_branch_token> tokens;
  std::vector<int64_t> begin;
  int32_t current;
  std::string bytes;
};

// one workflow: a timer blob in front, the execution blob last (its end is the block's end)
Table extract(const std::string& exec) {
  Wr timer;
  timer.i64(10, 3), timer.i64(12, 7), timer.stop();
  Packed blobs;   // exactly the blobs: no pad to hide an over-read
  blobs.add(timer.b), blobs.add(exec);
  const StateBatch batch(blobs.bytes, blobs.off, {{CRR_STATE_TIMER, 5, 0, 0, 0}, {CRR_STATE_EXECUTION, 0, 0, 0, 0}}, {{0, 2, 20}},
                         {'t', 'i', 'm', 'e', 'r'});
  const crr_state_batch& in = batch.in;
  Table T;
  T.current = -7;
  T.rc = crr_load_branches_host(&in, nullptr, &T.sizes, 1);
  if (T.rc == 0) {
    // exact-size heap blocks (malloc(0) is a valid block no byte of which may be touched)
    crr_load_branches d;
    d.branches = static_cast<crr_ndc_branch*>(malloc(T.sizes.n_branches * sizeof(crr_ndc_branch)));
    d.items = static_cast<crr_vh_item*>(malloc(T.sizes.n_items * sizeof(crr_vh_item)));
    d.tokens = static_cast<crr_branch_token*>(malloc(T.sizes.n_branches * sizeof(crr_branch_token)));
    d.branch_begin = static_cast<int64_t*>(malloc(2 * sizeof(int64_t)));
    d.current = static_cast<int32_t*>(malloc(sizeof(int32_t)));
    crr_load_ndc_sizes again;
    T.rc = crr_load_branches_host(&in, &d, &again, 1);
    if (again.n_branches != T.sizes.n_branches || again.n_items != T.sizes.n_items) T.rc = -99;
    T.branches.assign(d.branches, d.branches + T.sizes.n_branches);
    T.items.assign(d.items, d.items + T.sizes.n_items);
    T.tokens.assign(d.tokens, d.tokens + T.sizes.n_branches);
    T.begin.assign(d.branch_begin, d.branch_begin + 2);
    T.current = *d.current;
    free(d.branches), free(d.items), free(d.tokens), free(d.branch_begin), free(d.current);
  }
  T.bytes.assign(blobs.bytes.begin(), blobs.bytes.end());
  return T;
}

bool same(const Table& T, int32_t current, const std::vector<Branch>& hs) {
  if (T.rc != 0 || T.sizes.n_wf != 1 || T.branches.size() != hs.size() || T.current != current) return false;
  if (T.begin[0] != 0 || T.begin[1] != (int64_t)hs.size()) return false;
  size_t at = 0;
  for (size_t h = 0; h < hs.size(); ++h) {
    const Branch& B = hs[h];
    const size_t n = B.has_items ? B.items.size() : 0;
    if (T.branches[h].item_begin != at || T.branches[h].item_count != n) return false;
    for (size_t i = 0; i < n; ++i)
      if (T.items[at + i].event_id != B.items[i].first || T.items[at + i].version != B.items[i].second) return false;
    at += n;
    const std::string tok = B.has_token ? B.token : std::string();
    if (T.tokens[h].wf != 0 || T.tokens[h].len != tok.size()) return false;
    if (T.tokens[h].off + tok.size() > T.bytes.size() || T.bytes.compare(T.tokens[h].off, tok.size(), tok) != 0) return false;
  }
  return at == T.items.size();
}

}  // namespace

int main() {
  const std::vector<std::pair<int64_t, int64_t>> items = {{5, 1}, {19, 3}}, longer = {{5, 1}, {9, 2}, {30, 3}, {31, 8}};
  int full = 0, cuts = 0;
  std::string longest;
  for (size_t tok_len : {0u, 1u, 7u, 8u, 9u, 95u, 96u, 97u})
    for (int shape = 0; shape < 6; ++shape) {
      const std::string tok = bytes_of(tok_len, 11);
      std::vector<Branch> hs;
      int32_t current = 0;
      if (shape == 0) hs = {{true, true, tok, items}};
      if (shape == 1) hs = {{true, true, "decoy", {{1, 0}}}, {true, true, tok, items}}, current = 1;
      if (shape == 2) hs = {{true, true, tok, {}}, {false, true, "", items}, {true, true, tok, longer}}, current = 2;
      if (shape == 3) hs = {{false, true, "", longer}, {true, false, tok, {}}}, current = 0;
      if (shape == 4) hs = {{false, false, "", {}}, {true, true, tok, items}, {true, true, tok, longer}, {true, false, tok, {}}}, current = 3;
      if (shape == 5) hs = {{false, false, "", {}}};
      const std::string exec = execution_blob(current, hs);
      const Table T = extract(exec);
      if (!same(T, current, hs)) {
        fprintf(stderr, "token %zu shape %d: rc %d, %zu branches, %zu items, current %d\n", tok_len, shape, T.rc, T.branches.size(),
                T.items.size(), T.current);
        return 1;
      }
      ++full;
      if (tok_len == 9 && shape == 4) longest = exec;
    }
  for (size_t n = 0; n < longest.size(); ++n, ++cuts) {
    const Table T = extract(longest.substr(0, n));
    if (T.rc != 0 || T.sizes.n_branches != 0 || T.sizes.n_items != 0 || T.current != 0 || T.begin[0] != 0 || T.begin[1] != 0) {
      fprintf(stderr, "cut at %zu of %zu: rc %d, %llu branches\n", n, longest.size(), T.rc, (unsigned long long)T.sizes.n_branches);
      return 1;
    }
  }
  printf("load_branches_asan: %d states' tables as written, %d truncations without branches, no sanitizer report\n", full, cuts);
  return 0;
}
