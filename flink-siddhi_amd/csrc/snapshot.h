// Snapshot codec: a host-side image of everything a snapshot carries, and the
// byte format.  Pure host code (no HIP): cep_snapshot pulls device state into
// a SnapImage and encodes it; cep_restore decodes into a SnapImage, so nothing
// on the device has changed when the bytes are refused, and then commits.
//
// Snapshot format (little endian), versions 2 - 7:
//   "CEPS" u32 version, u64 plan_hash, i64 events_in, u32 n_patterns,
//   per pattern: i64 key_capacity, u32 S, u32 slot_words, u32 n_live,
//                n_live x { u32 key, u64 header, u32 n, n * slot_words u64 }
//                (n = pending partials, inline slots then the overflow run;
//                versions 2 / 3 have no n: n = header & 0xff)
//   (version >= 3) the event-time reorder buffer ("queuedRecordsState",
//   AbstractSiddhiOperator.java:98): i32 input (-1: empty), u8 has_stream,
//   i64 n, i64 released_max, then n rows: every column of the input's
//   definition (type width each), n x i64 ts, n x u8 stream if has_stream;
//   (version >= 4) per pattern: u8 sparse keys, if set u32 count, u32 id of
//   the value -1 (0xffffffff: none), count x i64 partition value per dense slot.
//   (version >= 5) u32 n_groups, per multi-query group: i64 key_capacity,
//   u32 words per key, u32 n_live, n_live x { u32 key, words x u64 }.
//   (version >= 6, written only by apps that hold a join; others still write 5)
//   u32 n_joins, per join: u32 entry words, per side: u64 rows kept so far,
//   u64 tail entries, tail x entry words u64 (the side's live rows, oldest first).
//   (version 7, written only by apps that hold a table) u32 n_tables, per
//   table with an operation: i64 key_capacity, u32 words per row, u32 n_live,
//   n_live x { u32 key, words x u64 }; then u64 inserts dropped so far.
// Keys are dense keys, ascending in the bucket-major key index.  Versions 2
// (no reorder section), 3 and 4 are still restored (apps without multi-query
// groups).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "frontend.h"

namespace cep {

uint64_t plan_hash(const CompiledApp& app);

// Bucket-major key index (bucket = the key's low lg bits, kpb keys per bucket)
// <-> dense key.
inline int64_t key_index(uint32_t key, int64_t kpb, int lg) {
  return (int64_t)(key & ((1u << lg) - 1)) * kpb + (key >> lg);
}
inline uint32_t dense_key(int64_t i, int64_t kpb, int lg) { return (uint32_t)(((i % kpb) << lg) | (i / kpb)); }

// What a snapshot must agree with to be restored into a runtime.
struct SnapGeometry {
  uint64_t plan_hash = 0;
  uint32_t hdr_ovf = 0;          // kernels.h kHdrOvf (never set in a stored header)
  uint64_t join_tail_cap = 0;    // kernels.h kJoinTailCap
  struct Pattern {
    int64_t key_capacity, kstride, pool_cap;
    int lg;
    uint32_t S, slot_words;
    bool has_kext, sparse;
    uint64_t table_cap;
  };
  struct Group {
    int64_t key_capacity, kstride;
    int lg, kpb;
    uint32_t words;
  };
  struct Join {
    uint32_t ew;
    int win_kind[2];
    int64_t win_param[2];
  };
  struct Table {
    int64_t key_capacity, kstride;
    int lg;
    uint32_t nwords;
  };
  std::vector<Pattern> pats;
  std::vector<Group> groups;
  std::vector<Join> joins;
  std::vector<Table> tabs;
  std::vector<std::vector<int>> inputs;   // per input stream: its columns' widths in bytes
};

// Host image of a snapshot, in the device's layouts.
struct SnapImage {
  SnapGeometry geo;
  uint32_t version = 0;          // decode: the version read
  int64_t events_in = 0;
  struct Pattern {
    std::vector<uint32_t> hdr;           // [kstride]
    std::vector<uint64_t> slots;         // [S * slot_words][kstride]
    std::vector<uint64_t> ext, pool;     // [kstride] count | run offset << 32; [slots][slot_words]
    int64_t ts_max = INT64_MIN;          // decode: largest partial ts (the closed form's high-water mark)
    uint32_t kcount[2] = {0, 0xffffffffu};   // sparse keys: count, id of the value -1
    std::vector<uint64_t> krev;          // dense slot -> value
    std::vector<uint64_t> tkey;          // decode: the map rebuilt as the device's hash table
    std::vector<uint32_t> tval;
  };
  std::vector<Pattern> pats;
  struct Reorder {
    int32_t input = -1;
    bool has_stream = false;
    int64_t n = 0, released_max = INT64_MIN;
    std::vector<uint8_t> rows;           // every column, then ts, then stream: n values each
  } ro;
  std::vector<std::vector<uint64_t>> groups;   // per group: state [bucket][word][key of bucket]
  struct Join {
    uint64_t kept[2] = {0, 0}, tail[2] = {0, 0};
    std::vector<uint64_t> rows[2];
  };
  std::vector<Join> joins;
  struct Table {
    std::vector<uint32_t> hdr;           // [kstride], bit 0: present
    std::vector<uint64_t> words;         // [nwords][kstride]
  };
  std::vector<Table> tabs;
  uint64_t tab_dropped = 0;
};

std::vector<uint8_t> snapshot_encode(const SnapImage& img);
// CEP_OK, or the status to return with *why (the image is then unspecified).
int snapshot_decode(const SnapGeometry& geo, const uint8_t* buf, size_t len, SnapImage* img, std::string* why);

}  // namespace cep
