// load_states_asan.cpp -- a stand-alone check of the host state decoder (crr_load_states_host) under
// AddressSanitizer / UndefinedBehaviorSanitizer: every truncation length of one blob of each kind, each
// batch's bytes in a heap block of exactly its size, so a read past a truncated blob's end is reported.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/load_states_asan.cpp cadence_amd/csrc/load_states.cpp -o build/load_states_asan -lpthread
//   build/load_states_asan
//
// Exit status 0 and a line of counts when every truncation reported CRR_LOAD_MALFORMED, the full blobs loaded
// OK, and no sanitizer report ended the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cadence_load.h"

#include "load_asan_common.h"

namespace {

void list_str(Wr& w, int16_t id, const std::vector<std::string>& v) {
  w.list(id, 11, v.size());
  for (auto& s : v) w.be(s.size(), 4), w.b += s;
}
void map_str(Wr& w, int16_t id, const std::vector<std::string>& kv) {
  w.field(13, id), w.u8(11), w.u8(11), w.be(kv.size() / 2, 4);
  for (auto& s : kv) w.be(s.size(), 4), w.b += s;
}

std::string version_histories() {
  Wr w;
  w.u8(0x59), w.i32(10, 1), w.field(15, 20), w.u8(12), w.be(2, 4);
  for (int h = 0; h < 2; ++h) {
    w.str(10, h ? "current-token" : "other-token"), w.field(15, 20), w.u8(12), w.be(2, 4);
    for (int k = 0; k < 2; ++k) w.i64(10, 5 + 7 * k), w.i64(20, 1 + k), w.stop();
    w.stop();
  }
  w.stop();
  return w.b;
}

std::string reset_points() {
  Wr w;
  w.u8(0x59), w.field(15, 10), w.u8(12), w.be(2, 4);
  for (int k = 0; k < 2; ++k)
    w.str(10, k ? "bin-b" : "bin-a"), w.str(20, "run"), w.i64(30, 4), w.i64(40, 99), w.boolean(60, k == 0), w.stop();
  w.stop();
  return w.b;
}

std::string execution_blob() {
  Wr w;
  w.str(12, "parent"), w.i64(16, -23), w.str(24, "task-list"), w.i32(30, 10), w.i32(34, 1), w.i32(36, 0);
  w.i64(48, 777), w.i64(50, 18), w.i64(52, 15), w.i64(58, 3), w.i64(60, 18), w.i64(62, -23), w.i32(64, 10), w.i64(66, 0);
  w.i64(68, -6795364578871345152LL), w.i64(69, 1600000000000000000LL), w.boolean(70, true), w.i64(71, 1600000000000000000LL);
  w.str(74, "emptyUuid"), w.str(78, "sticky"), w.dbl(92), w.i64(94, 0), list_str(w, 96, {"a", "bb"}), w.boolean(98, false);
  w.i64(106, 2), w.str(115, reset_points()), w.str(116, "thriftrw"), map_str(w, 118, {"k", "v", "k2", ""});
  w.str(122, version_histories()), w.str(124, "thriftrw"), w.stop();
  return w.b;
}

std::string pending_blob(uint32_t kind) {
  Wr w;
  w.i64(10, 3);
  if (kind == CRR_STATE_ACTIVITY) {
    w.i64(12, 4), w.str(14, "event"), w.i64(18, 1600000000000000005LL), w.i64(20, 6), w.i64(26, 1600000001000000000LL);
    w.str(28, "activity-five"), w.str(30, "request"), w.i32(32, 5), w.i32(34, 30), w.i32(36, 20), w.i32(38, 3), w.boolean(40, true);
    w.i64(42, 9), w.i32(44, 1), w.i32(46, 2), w.str(48, "tl"), w.boolean(52, true), w.dbl(62), list_str(w, 64, {"x"});
  } else if (kind == CRR_STATE_TIMER) {
    w.i64(12, 7), w.i64(14, 1600000100000000000LL), w.i64(16, 1);
  } else if (kind == CRR_STATE_CHILD) {
    w.i64(12, 8), w.i64(14, 10), w.str(16, "event"), w.str(20, "child-wf"), w.str(28, "request"), w.i32(35, 0);
  } else {
    w.i64(11, 10), w.str(12, "request");
    if (kind == CRR_STATE_SIGNAL) w.str(14, "sig"), w.str(16, "input");
  }
  w.stop();
  return w.b;
}

// one workflow: [a full execution blob unless the cut one is the execution blob,] the cut blob last
int load_one(uint32_t kind, const std::string& full_exec, const std::string& cut, int32_t* status) {
  Packed blobs;   // exactly the blobs: no pad to hide an over-read
  std::vector<crr_state_blob> meta;
  if (kind != CRR_STATE_EXECUTION) {
    blobs.add(full_exec);
    meta.push_back({CRR_STATE_EXECUTION, 0, 0, 0, 0});
  }
  blobs.add(cut);
  meta.push_back({kind, kind == CRR_STATE_TIMER ? 5u : 0u, 5, 0, 0});
  const StateBatch batch(blobs.bytes, blobs.off, meta, {{0, (uint32_t)meta.size(), 20}}, {'t', 'i', 'm', 'e', 'r'});
  const crr_state_batch& in = batch.in;
  crr_load_summary S;
  int rc = crr_load_states_host(&in, nullptr, &S, 1);   // sizes
  if (rc == 0) {
    std::vector<crr_exec_row> exec(1);
    std::vector<uint8_t> rows[7], tokens(S.totals[CRR_LOAD_T_TOKEN] + 1), kb(S.totals[CRR_LOAD_T_KEY_BYTES] + 1);
    const size_t row_bytes[7] = {sizeof(crr_activity_row), sizeof(crr_timer_row), sizeof(crr_child_row), sizeof(crr_initiated_row),
                                 sizeof(crr_initiated_row), sizeof(crr_vh_item), sizeof(crr_reset_point_row)};
    std::vector<int64_t> offsets(CRR_LOAD_TABLES * 2);
    std::vector<uint64_t> key_off(S.totals[CRR_LOAD_T_KEYS] + 1);
    std::vector<uint32_t> key_len(S.totals[CRR_LOAD_T_KEYS] + 1);
    uint32_t flags = 0;
    crr_load_image img;
    memset(&img, 0, sizeof img);
    img.exec = exec.data();
    for (int t = 0; t < 7; ++t) {
      rows[t].resize(S.totals[t] * row_bytes[t] + 8);
      img.rows[t] = rows[t].data();
    }
    img.offsets = offsets.data(), img.tokens = tokens.data(), img.key_off = key_off.data(), img.key_len = key_len.data();
    img.key_bytes = kb.data(), img.status = status, img.flags = &flags;
    rc = crr_load_states_host(&in, &img, &S, 1);
  }
  return rc;
}

}  // namespace

int main() {
  const std::string full_exec = execution_blob();
  int cuts = 0;
  for (uint32_t kind = CRR_STATE_EXECUTION; kind <= CRR_STATE_SIGNAL; ++kind) {
    const std::string full = kind == CRR_STATE_EXECUTION ? full_exec : pending_blob(kind);
    int32_t st = -1;
    if (load_one(kind, full_exec, full, &st) != 0 || st != CRR_LOAD_OK) {
      fprintf(stderr, "kind %u: the full blob gave status %d\n", kind, st);
      return 1;
    }
    for (size_t n = 0; n < full.size(); ++n, ++cuts) {
      st = -1;
      if (load_one(kind, full_exec, full.substr(0, n), &st) != 0 || st != CRR_LOAD_MALFORMED) {
        fprintf(stderr, "kind %u cut at %zu of %zu: status %d, expected CRR_LOAD_MALFORMED\n", kind, n, full.size(), st);
        return 1;
      }
    }
  }
  printf("load_states_asan: 6 full blobs OK, %d truncations malformed, no sanitizer report\n", cuts);
  return 0;
}
