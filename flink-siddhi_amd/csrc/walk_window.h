// LDS windows over one key bucket's records of a chunk, shared by the walks
// that run one lane per key over k_partition's output (k_winwalk in
// win_kernels.hip, k_tabwalk in tab_kernels.hip).
//
// k_partition leaves a chunk's records tile by tile, each tile's records
// grouped by bucket (tile_off: per tile P + 1 exclusive offsets).  A bucket's
// workgroup walks them in LDS windows: runs of whole tiles (a tile's segment
// is in rank order, not arrival order, so it cannot be split) of at most
// kWinWindow records, grouped by key with a counting sort, each key's run
// then sorted on the arrival number.  Args is the walk's argument block
// (pat, recs, tile_off, ntiles, tile_rows, err as in WinArgs).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "dev_common.h"

namespace cep {
namespace {

// Records per LDS window.  One tile holds at most kPartThreads * kPartItems
// records of a bucket: an unkeyed query's single bucket gets all of them.
constexpr int kWinWindow = kPartThreads * kPartItems;

struct WinLds {
  uint32_t wrec[kWinWindow];         // global record index per window slot
  uint16_t wkey[kWinWindow];         // key within the bucket
  uint16_t sorted[kWinWindow];       // window slots grouped by key, arrival order
  uint32_t wseq[kWinWindow];         // chunk-relative arrival number
  uint32_t kstart[kWalkMaxKeys + 1];
  uint32_t khdr[kWalkMaxKeys];       // per-key state headers of this bucket
  uint32_t kcur[kWalkMaxKeys];       // counting-sort cursors
  uint32_t scratch[16];
  unsigned long long base;
  uint32_t t1;
};

// Event ts of a record (w1 = chunk-relative arrival number | chunk-relative ts << 32).
__device__ __forceinline__ int64_t rec_ts_rel(const uint64_t* rec, int64_t ts_base) {
  return ts_base + (int64_t)(int32_t)(rec[1] >> 32);
}

// Segment starts and sizes of `bucket` in every tile -> exclusive prefix over
// the tiles (Lseg[0..ntiles], Llo[t] = the segment's start inside tile t).
// Every thread of the block takes part; ends with a barrier.
template <class Args>
__device__ __forceinline__ void win_segments(const Args& a, int bucket, int P, WinLds& L, uint32_t* Lseg,
                                             uint16_t* Llo) {
  const int tid = threadIdx.x;
  const int ntiles = a.ntiles;   // <= kWalkMaxTiles (host-checked)
  constexpr int MAXPER = kWalkMaxTiles / kWalkThreads;
  const int per = (ntiles + kWalkThreads - 1) / kWalkThreads;   // <= MAXPER
  uint32_t cnt[MAXPER];
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < MAXPER; ++i) {
    const int t = tid * per + i;
    cnt[i] = 0;
    if (i < per && t < ntiles) {
      const uint16_t* o = a.tile_off + (int64_t)t * (P + 1) + bucket;
      const uint32_t lo = o[0], hi = o[1];
      Llo[t] = (uint16_t)lo;
      cnt[i] = hi - lo;
    }
    sum += cnt[i];
  }
  uint32_t total;
  uint32_t off = block_excl_scan(sum, L.scratch, &total);
#pragma unroll
  for (int i = 0; i < MAXPER; ++i) {
    const int t = tid * per + i;
    if (i < per && t < ntiles) {
      Lseg[t] = off;
      off += cnt[i];
    }
  }
  if (tid == 0) Lseg[ntiles] = total;
  lds_barrier();
}

// The LDS window that starts at tile t0: tiles [t0, t1), its records in
// L.wrec / wkey / wseq, grouped by key in L.sorted (key k's run is
// [L.kstart[k], L.kstart[k + 1]), in arrival order).  Returns t1; *nw = the
// window's records.  Every thread of the block takes part; ends with a barrier.
template <class Args>
__device__ __forceinline__ int win_build(const Args& a, int kpb, int t0, WinLds& L, const uint32_t* Lseg,
                                         const uint16_t* Llo, uint32_t* nw_out) {
  const int tid = threadIdx.x;
  const PatternArgs& p = a.pat;
  const int ntiles = a.ntiles;
  const int rw = p.rec_words;
  if (tid == 0) {
    // largest t1 with seg[t1] - seg[t0] <= window
    int lo = t0 + 1, hi = ntiles;
    const uint32_t lim = Lseg[t0] + kWinWindow;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (Lseg[mid] <= lim) lo = mid;
      else hi = mid - 1;
    }
    L.t1 = (uint32_t)lo;
  }
  for (int k = tid; k <= kpb; k += kWalkThreads) L.kstart[k] = 0;
  lds_barrier();
  const int t1 = (int)L.t1;
  const uint32_t wbase = Lseg[t0];
  const uint32_t nrec = Lseg[t1] - wbase;
  if (nrec > (uint32_t)kWinWindow) set_err(a.err, ERR_WINDOW);   // (a tile larger than the partition pass makes)
  const uint32_t nw = nrec < (uint32_t)kWinWindow ? nrec : (uint32_t)kWinWindow;
  for (uint32_t w = tid; w < nw; w += kWalkThreads) {
    const uint32_t flat = wbase + w;
    // the tile whose segment holds record `flat`: last t in [t0, t1) with Lseg[t] <= flat
    int lo = t0, hi = t1 - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (Lseg[mid] <= flat) lo = mid;
      else hi = mid - 1;
    }
    const uint32_t g = (uint32_t)lo * (uint32_t)a.tile_rows + Llo[lo] + (flat - Lseg[lo]);
    const uint64_t* rec = a.recs + (int64_t)g * rw;
    const uint64_t h = rec[0], w1 = rec[1];
    uint32_t kin = (uint32_t)h >> p.buckets_log2;
    if (kin >= (uint32_t)kpb) {   // (k_partition keeps keys below key_capacity)
      set_err(a.err, ERR_WINDOW);
      kin = 0;
    }
    L.wrec[w] = g;
    L.wkey[w] = (uint16_t)kin;
    L.wseq[w] = (uint32_t)w1;
    atomicAdd(&L.kstart[kin + 1], 1u);
  }
  lds_barrier();
  // exclusive scan of key counts (kstart[1..kpb] -> kstart[0..kpb]); kpb <= kWalkThreads
  {
    const uint32_t c = (tid < kpb) ? L.kstart[tid + 1] : 0u;
    uint32_t tot;
    const uint32_t off = block_excl_scan(c, L.scratch, &tot);
    if (tid < kpb) {
      L.kstart[tid] = off;
      L.kcur[tid] = off;
    }
    if (tid == 0) L.kstart[kpb] = tot;
  }
  lds_barrier();
  for (uint32_t w = tid; w < nw; w += kWalkThreads) {
    const uint32_t slot = atomicAdd(&L.kcur[L.wkey[w]], 1u);
    L.sorted[slot] = (uint16_t)w;
  }
  lds_barrier();
  // restore arrival order inside each key run (insertion / shell sort on seq)
  for (int k = tid; k < kpb; k += kWalkThreads) {
    const uint32_t r0 = L.kstart[k], r1 = L.kstart[k + 1];
    const uint32_t len = r1 - r0;
    if (len < 2) continue;
    for (uint32_t gap = len > 64 ? len / 3 : 1;; gap = gap / 3 ? gap / 3 : 1) {
      for (uint32_t i = r0 + gap; i < r1; ++i) {
        const uint16_t v = L.sorted[i];
        const uint32_t sv = L.wseq[v];
        uint32_t j = i;
        while (j >= r0 + gap && L.wseq[L.sorted[j - gap]] > sv) {
          L.sorted[j] = L.sorted[j - gap];
          j -= gap;
        }
        L.sorted[j] = v;
      }
      if (gap == 1) break;
    }
  }
  lds_barrier();
  *nw_out = nw;
  return t1;
}

}  // namespace
}  // namespace cep
