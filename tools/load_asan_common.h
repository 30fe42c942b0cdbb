// load_asan_common.h -- what the stand-alone sanitizer programs of the host restatement (tools/load_*_asan.cpp)
// share: a thriftrw writer, exact-size heap blocks, and owners of a crr_state_batch and a crr_load_image made of
// such blocks.  Each program keeps its own blobs, its own cases and its own encoder of the values it expects.
#ifndef CADENCE_LOAD_ASAN_COMMON_H_
#define CADENCE_LOAD_ASAN_COMMON_H_

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cadence_load.h"

namespace {

// thrift binary, field by field
struct Wr {
  std::string b;
  void u8(uint8_t v) { b.push_back((char)v); }
  void be(uint64_t v, int n) {
    for (int i = n - 1; i >= 0; --i) u8((uint8_t)(v >> (8 * i)));
  }
  void field(uint8_t t, int16_t id) {
    u8(t);
    be((uint16_t)id, 2);
  }
  void boolean(int16_t id, bool v) { field(2, id), u8(v ? 1 : 0); }
  void dbl(int16_t id) { field(4, id), be(0x4000000000000000ull, 8); }
  void i16(int16_t id, int16_t v) { field(6, id), be((uint16_t)v, 2); }
  void i32(int16_t id, int32_t v) { field(8, id), be((uint32_t)v, 4); }
  void i64(int16_t id, int64_t v) { field(10, id), be((uint64_t)v, 8); }
  void str(int16_t id, const std::string& s) { field(11, id), be(s.size(), 4), b += s; }
  void list(int16_t id, uint8_t elem, size_t n) { field(15, id), u8(elem), be(n, 4); }
  void stop() { u8(0); }
};

inline std::string bytes_of(size_t n, int seed) {
  std::string s;
  for (size_t i = 0; i < n; ++i) s.push_back((char)(uint8_t)(seed + 7 * i));
  return s;
}

template <class T>
T* exact(const std::vector<T>& v) {   // a heap block of exactly the vector's bytes (malloc(0): no byte may be touched)
  T* p = static_cast<T*>(malloc(v.size() * sizeof(T)));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

// blobs end to end, no pad behind the last: bytes and off ready for a StateBatch
struct Packed {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off{0};
  void add(const std::string& blob) {
    bytes.insert(bytes.end(), blob.begin(), blob.end());
    off.push_back(bytes.size());
  }
};

// a crr_state_batch over exact-size copies of its five arrays, freed with it
struct StateBatch {
  crr_state_batch in;
  StateBatch(const std::vector<uint8_t>& bytes, const std::vector<uint64_t>& off, const std::vector<crr_state_blob>& meta,
             const std::vector<crr_state_wf>& wf, const std::vector<uint8_t>& strings)
      : in{exact(bytes), exact(off), exact(meta), exact(wf), exact(strings), (uint32_t)meta.size(), (uint32_t)wf.size()} {}
  ~StateBatch() {
    for (const void* p : {(const void*)in.bytes, (const void*)in.blob_off, (const void*)in.blob, (const void*)in.wf, (const void*)in.strings})
      free(const_cast<void*>(p));
  }
  StateBatch(const StateBatch&) = delete;
  StateBatch& operator=(const StateBatch&) = delete;
};

// a crr_load_image, all NULL at first, that frees whatever heap blocks its pointers are given
struct Image : crr_load_image {
  Image() { memset(static_cast<crr_load_image*>(this), 0, sizeof(crr_load_image)); }
  ~Image() {
    free(exec), free(offsets), free(tokens), free(key_off), free(key_len), free(key_bytes), free(status), free(flags);
    for (void* p : rows) free(p);
  }
  Image(const Image&) = delete;
  Image& operator=(const Image&) = delete;
};

}  // namespace

#endif  // CADENCE_LOAD_ASAN_COMMON_H_
