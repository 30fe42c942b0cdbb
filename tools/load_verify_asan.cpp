// load_verify_asan.cpp -- a stand-alone check of the host checksum verification (crr_load_states_verify_host,
// include/cadence_load_verify.h) under AddressSanitizer / UndefinedBehaviorSanitizer: execution blobs with
// sticky names and branch tokens of several lengths (absent and empty ones included), each batch's bytes in a
// heap block of exactly its size, so a read past a blob's end while the payload is generated is reported; and
// every truncation length of one such blob, which must come back CRR_VERIFY_NOT_LOADED with zeros.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/load_verify_asan.cpp cadence_amd/csrc/load_states.cpp -o build/load_verify_asan -lpthread
//   build/load_verify_asan
//
// Exit status 0 and a line of counts when every full blob's CRC equals the one this file computes bit by bit
// over a payload it writes itself, every truncation is not loaded, and no sanitizer report ended the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "cadence_load_verify.h"

#include "load_asan_common.h"

namespace {

struct Branch {
  bool has_token;
  std::string token;
  std::vector<std::pair<int64_t, int64_t>> items;
};

std::string version_histories(int32_t current, const std::vector<Branch>& hs) {
  Wr w;
  w.u8(0x59), w.i32(10, current), w.list(20, 12, hs.size());
  for (auto& h : hs) {
    if (h.has_token) w.str(10, h.token);
    w.list(20, 12, h.items.size());
    for (auto& it : h.items) w.i64(10, it.first), w.i64(20, it.second), w.stop();
    w.stop();
  }
  w.stop();
  return w.b;
}

// the version histories last, the sticky name's and the last token's bytes close to the end of the block
std::string execution_blob(const std::string& sticky, int32_t current, const std::vector<Branch>& hs) {
  Wr w;
  w.i32(34, 1), w.i64(50, 18), w.i64(52, 15), w.i64(56, 1600000000500000000LL), w.i64(58, 3), w.i64(60, 18), w.i64(62, -23);
  w.i64(66, 4), w.boolean(70, true), w.str(78, sticky), w.i64(106, 2), w.str(122, version_histories(current, hs));
  w.str(124, "thriftrw"), w.stop();
  return w.b;
}

// what Load generates for that state with one timer (StartedID 7) and two signals (12, 9: the list is sorted)
std::string payload(const std::string& sticky, int32_t current, const std::vector<Branch>& hs) {
  Wr w;
  w.u8(0x59), w.boolean(10, true), w.i16(15, 1), w.i64(23, 18), w.i64(24, 20), w.i64(25, 15), w.i64(26, 2), w.i32(35, 4);
  w.i64(36, 3), w.i64(37, 18), w.i64(38, -23);
  w.list(45, 10, 1), w.be(7, 8), w.list(46, 10, 0), w.list(47, 10, 2), w.be(9, 8), w.be(12, 8), w.list(48, 10, 0), w.list(49, 10, 0);
  w.str(55, sticky), w.field(12, 56), w.i32(10, current), w.list(20, 12, hs.size());
  for (auto& h : hs) {
    w.str(10, h.token), w.list(20, 12, h.items.size());
    for (auto& it : h.items) w.i64(10, it.first), w.i64(20, it.second), w.stop();
    w.stop();
  }
  w.stop(), w.stop();
  return w.b;
}

uint32_t crc32_bitwise(const std::string& s) {
  uint32_t c = 0xFFFFFFFFu;
  for (unsigned char ch : s) {
    c ^= ch;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

std::string small_blob(int64_t version, int64_t started_id) {
  Wr w;
  w.i64(10, version);
  if (started_id) w.i64(12, started_id);
  w.stop();
  return w.b;
}

// one workflow: a timer and two signals, then the execution blob last (its end is the block's end)
crr_verify_row verify_one(const std::string& exec, const crr_stored_checksum* stored, int64_t cut_off, int* rc) {
  Packed blobs;   // exactly the blobs: no pad to hide an over-read
  for (auto& b : {small_blob(3, 7), small_blob(3, 0), small_blob(3, 0), exec}) blobs.add(b);
  const StateBatch batch(blobs.bytes, blobs.off,
                         {{CRR_STATE_TIMER, 5, 0, 0, 0}, {CRR_STATE_SIGNAL, 0, 12, 0, 0}, {CRR_STATE_SIGNAL, 0, 9, 0, 0},
                          {CRR_STATE_EXECUTION, 0, 0, 0, 0}},
                         {{0, 4, 20}}, {'t', 'i', 'm', 'e', 'r'});
  crr_verify_row* out = static_cast<crr_verify_row*>(malloc(sizeof(crr_verify_row)));   // exactly one row
  memset(out, 0xEE, sizeof *out);
  *rc = crr_load_states_verify_host(&batch.in, stored, cut_off, out, 1);
  const crr_verify_row r = *out;
  free(out);
  return r;
}

}  // namespace

int main() {
  const std::vector<std::pair<int64_t, int64_t>> items = {{5, 1}, {19, 3}};
  int full = 0, cuts = 0;
  std::string longest;
  for (size_t sticky_len : {0u, 1u, 9u, 300u})
    for (size_t tok_len : {0u, 1u, 7u, 8u, 9u, 95u, 96u, 97u})
      for (int shape = 0; shape < 4; ++shape) {
        const std::string sticky = bytes_of(sticky_len, 3), tok = bytes_of(tok_len, 11);
        std::vector<Branch> hs;
        int32_t current = 0;
        if (shape == 0) hs = {{true, tok, items}};
        if (shape == 1) hs = {{true, "decoy", {{1, 0}}}, {true, tok, items}}, current = 1;
        if (shape == 2) hs = {{true, tok, {}}, {false, "", items}, {true, tok, items}}, current = 2;
        if (shape == 3) hs = {{false, "", items}, {true, tok, {}}}, current = 0;
        const std::string exec = execution_blob(sticky, current, hs), pay = payload(sticky, current, hs);
        const uint32_t want = crc32_bitwise(pay);
        const crr_stored_checksum good = {CRR_CHECKSUM_PAYLOAD_V1, CRR_CHECKSUM_FLAVOR_CRC32, want, 4};
        int rc = -9;
        crr_verify_row r = verify_one(exec, &good, 1600000000500000000LL, &rc);
        if (rc != 0 || r.outcome != CRR_VERIFY_MATCH || r.computed != want || r.payload_len != pay.size() || r.reserved != 0) {
          fprintf(stderr, "sticky %zu token %zu shape %d: rc %d outcome %d crc %08x (want %08x) len %u (want %zu)\n", sticky_len,
                  tok_len, shape, rc, r.outcome, r.computed, want, r.payload_len, pay.size());
          return 1;
        }
        r = verify_one(exec, nullptr, 0, &rc);
        if (rc != 0 || r.outcome != CRR_VERIFY_NONE || r.computed != want) return fprintf(stderr, "compute only\n"), 1;
        r = verify_one(exec, &good, 1600000000500000001LL, &rc);
        if (rc != 0 || r.outcome != CRR_VERIFY_INVALIDATED || r.computed != want) return fprintf(stderr, "cut-off\n"), 1;
        ++full;
        if (sticky_len == 9 && tok_len == 9 && shape == 2) longest = exec;
      }
  for (size_t n = 0; n < longest.size(); ++n, ++cuts) {
    int rc = -9;
    const crr_stored_checksum any = {CRR_CHECKSUM_PAYLOAD_V1, CRR_CHECKSUM_FLAVOR_CRC32, 1, 4};
    const crr_verify_row r = verify_one(longest.substr(0, n), &any, 0, &rc);
    if (rc != 0 || r.outcome != CRR_VERIFY_NOT_LOADED || r.computed || r.payload_len || r.reserved) {
      fprintf(stderr, "cut at %zu of %zu: rc %d outcome %d\n", n, longest.size(), rc, r.outcome);
      return 1;
    }
  }
  printf("load_verify_asan: %d full states match, %d truncations not loaded, no sanitizer report\n", full, cuts);
  return 0;
}
