// Sliding-window aggregates for gfx950: `#window.length(N)` / `#window.time(T)`
// in front of a group-by query (kernels.h WinArgs).
//
// k_winwalk consumes the generic partition pass's output (k_partition: recs,
// tile_off, chunk_base) like k_walk does: one workgroup per key bucket builds
// LDS windows of the bucket's records, groups them by key in arrival order,
// and one lane per key walks its run.
//
// Semantics (upstream Siddhi 4.x, [U] in DESIGN.md): for every kept row e of
// a window instance, in arrival order,
//   1. expire   length(N): the window holds N rows -> pop the oldest;
//               time(T): pop from the front while front.ts + T <= e.ts, stop at
//               the first row that stays (positional: a later row with a small
//               ts sits behind a front row that blocks it);
//   2. remove   every popped row leaves its group's aggregates, oldest first:
//               long sums subtract (wrapping), fp64 sums do acc -= (double)v,
//               min / max become the exact extreme of the rows left;
//   3. add e, evaluate having, emit one row with e's ts and arrival number.
// fp64 results are exactly this sequence of += and -= (one lane per key, in
// order), not a fresh sum over the window.
//
// The walk never writes the ring while it runs.  A key's window is a queue of
// logical entries: the n0 entries its ring held at the start of the LDS
// window, then the key's records of the LDS window in arrival order.  The
// front index f only moves forward, values of entry i come from the ring
// (i < n0, HBM) or from the record itself (i >= n0).  So the count pass and
// the emit pass of a `having` query replay the same read-only state, and the
// commit stores only the entries that are still live at the end: at most
// `ring` of them, each at ring position (head0 + i) % ring, which is either a
// free position or one whose entry was popped (live entries with i < n0 stay
// where they are).  A length window's steady state stores N entries per key
// per LDS window however many records the key had.
//
// A time window that needs more than `ring` live rows sets ERR_PENDING (the
// next flush fails: raise pending_slots) and drops its oldest row, so ring
// positions stay below `ring` whatever the input.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "vm.h"
#include "dev_common.h"
#include "walk_window.h"

namespace cep {

namespace {

__device__ __forceinline__ double win_as_double(uint64_t v, int t) {
  switch (t) {
    case T_INT: return (double)(int32_t)v;
    case T_LONG: return (double)(int64_t)v;
    case T_FLOAT: return (double)as_f32(v);
    default: return as_f64(v);
  }
}

__device__ __forceinline__ bool win_less(uint64_t a, uint64_t b, int t) {
  switch (t) {
    case T_LONG: return (int64_t)a < (int64_t)b;
    case T_FLOAT: return as_f32(a) < as_f32(b);
    case T_DOUBLE: return as_f64(a) < as_f64(b);
    default: return (int32_t)a < (int32_t)b;
  }
}

// VM / emission environment: the current record and the window's aggregates.
struct WinEnv {
  const PatternArgs* p;
  const uint64_t* rec;     // current record (carried words at rec[2..])
  int64_t ev_ts;
  uint64_t cnt;            // rows in the window (the current one included)
  uint64_t acc[kMaxAggs];
  __device__ uint64_t col(int c, int) const { return rec[2 + c]; }
  __device__ uint64_t cap(int) const { return 0; }
  __device__ uint64_t outv(int, bool* n) const { *n = true; return 0; }
  __device__ uint64_t agg(int i, bool* isnull) const {
    // masked pick (a select chain on i would become a scratch array access)
    uint64_t x = 0;
#pragma unroll
    for (int j = 0; j < kMaxAggs; ++j) x |= acc[j] & (0ull - (uint64_t)(i == j));
    *isnull = false;   // the window holds at least the current row
    const int fn = p->agg_fn[i];
    if (fn == AGG_COUNT) return cnt;
    if (fn == AGG_AVG) return from_f64(as_f64(x) / (double)(int64_t)cnt);
    return x;
  }
  __device__ int64_t ts() const { return ev_ts; }
};

template <bool kVm>
__device__ __forceinline__ void win_emit(const WinArgs& a, uint64_t* R, const WinEnv& env, int64_t key,
                                         int64_t seq, unsigned long long pos) {
  if ((int64_t)pos >= a.out.cap) {
    set_err(a.err, ERR_OUT_CAP);
    return;
  }
  for (int c = 0; c < a.out.ncols; ++c) {
    const int src = a.out.src[c];
    uint64_t v;
    bool isnull = false;
    if (src == SRC_KEY) {
      v = (uint64_t)key;
    } else if (src >= SRC_AGG && src < SRC_AGG + kMaxAggs) {
      v = env.agg(src - SRC_AGG, &isnull);
    } else if (!kVm || (src >= SRC_REC && src < SRC_TS)) {
      v = env.col(src - SRC_REC, 0);
    } else {
      v = vm_eval(a.vm.code, a.vm.konst, a.out.prog[c], R, threadIdx.x, kWalkThreads, env, &isnull);
      if (isnull) v = 0;
    }
    store_col(a.out.col[c], a.out.type[c], (int64_t)pos, v);
  }
  a.out.ts[pos] = env.ev_ts;
  if (a.out.write_seq) a.out.seq[pos] = seq;
}

// One key's records of the LDS window, in arrival order.  kEmit = false: the
// count pass of a `having` query (rows that pass; nothing is stored).
template <bool kEmit, bool kVm>
__device__ __forceinline__ uint32_t win_key(const WinArgs& a, WinLds& L, uint64_t* R, int k, int bucket,
                                            int kpb, int64_t ts_base, int64_t seq_base,
                                            unsigned long long out_pos) {
  const PatternArgs& p = a.pat;
  const int64_t idx = (int64_t)bucket * kpb + k;
  const int64_t kl = ((int64_t)k << p.buckets_log2) | bucket;
  const int64_t ks = a.kstride;
  const int rw = p.rec_words;
  const int nagg = p.nagg;
  const int ring = a.ring, ew = a.entry_words;
  const bool timed = a.kind == WIN_TIME;
  uint64_t* sl = a.kslot + idx;   // state word w of this key: sl[w * ks]
  const uint32_t hdr = L.khdr[k];
  const bool live = (hdr & 1u) != 0;
  // (a header that does not fit this ring — no kernel writes one — must not index past it)
  const int head0 = live ? (int)((hdr >> 16) & 0xffu) % ring : 0;
  int n0 = live ? (int)(hdr >> 24) : 0;
  if (n0 > ring) n0 = ring;
  const uint32_t r0 = L.kstart[k], r1 = L.kstart[k + 1];

  WinEnv env;
  env.p = &p;
#pragma unroll
  for (int j = 0; j < kMaxAggs; ++j) env.acc[j] = (live && j < nagg) ? sl[(int64_t)j * ks] : 0;

  // logical queue entry i: ring entry (i < n0) or the key's record r0 + i - n0
  auto qrec = [&](int i) { return a.recs + (int64_t)L.wrec[L.sorted[r0 + (uint32_t)(i - n0)]] * rw; };
  auto qval = [&](int i, int v) -> uint64_t {
    if (i < n0) {
      int e = head0 + i;
      if (e >= ring) e -= ring;
      return sl[(int64_t)(nagg + e * ew + v) * ks];
    }
    return qrec(i)[2 + a.val_word[v]];
  };
  auto qts = [&](int i) -> int64_t {
    if (i < n0) {
      int e = head0 + i;
      if (e >= ring) e -= ring;
      return (int64_t)sl[(int64_t)(nagg + e * ew + ew - 1) * ks];
    }
    return rec_ts_rel(qrec(i), ts_base);
  };

  int f = 0, end = n0;
  uint32_t emitted = 0;
  for (uint32_t q = r0; q < r1; ++q) {
    const uint64_t* rec = a.recs + (int64_t)L.wrec[L.sorted[q]] * rw;
    const int64_t ts = rec_ts_rel(rec, ts_base);
    // 1. expire, 2. remove (oldest first)
    uint32_t redo = 0;   // bit j: min / max j lost a row that may have been its extreme
    while (f < end) {
      bool pop;
      if (end - f >= ring) {
        // length: the window is full.  time: more live rows than the ring holds
        if (timed && !(qts(f) + a.param <= ts)) set_err(a.err, ERR_PENDING);
        pop = true;
      } else {
        pop = timed && qts(f) + a.param <= ts;
      }
      if (!pop) break;
#pragma unroll
      for (int j = 0; j < kMaxAggs; ++j) {
        if (j >= nagg) break;
        const int fn = p.agg_fn[j], at = p.agg_arg_type[j];
        if (fn == AGG_COUNT) continue;
        const uint64_t v = qval(f, a.agg_val[j]);
        if (fn == AGG_SUM && p.agg_out_type[j] == T_LONG) env.acc[j] -= v;
        else if (fn == AGG_SUM || fn == AGG_AVG) env.acc[j] = from_f64(as_f64(env.acc[j]) - win_as_double(v, at));
        else if (fn == AGG_MIN) redo |= win_less(env.acc[j], v, at) ? 0u : 1u << j;
        else redo |= win_less(v, env.acc[j], at) ? 0u : 1u << j;
      }
      ++f;
    }
    // min / max: the exact extreme of the rows left (ring <= 255 entries)
    if (redo) {
#pragma unroll
      for (int j = 0; j < kMaxAggs; ++j) {
        if (j >= nagg) break;
        if (!((redo >> j) & 1u)) continue;
        const int at = p.agg_arg_type[j];
        const bool mn = p.agg_fn[j] == AGG_MIN;
        uint64_t x = 0;
        for (int i = f; i < end; ++i) {
          const uint64_t v = qval(i, a.agg_val[j]);
          if (i == f || (mn ? win_less(v, x, at) : win_less(x, v, at))) x = v;
        }
        env.acc[j] = x;
      }
    }
    // 3. add the row
    const bool first = end == f;
#pragma unroll
    for (int j = 0; j < kMaxAggs; ++j) {
      if (j >= nagg) break;
      const int fn = p.agg_fn[j], at = p.agg_arg_type[j];
      if (fn == AGG_COUNT) continue;
      const uint64_t v = rec[2 + p.agg_word[j]];
      if (fn == AGG_SUM && p.agg_out_type[j] == T_LONG) env.acc[j] += v;
      else if (fn == AGG_SUM || fn == AGG_AVG) env.acc[j] = from_f64(as_f64(env.acc[j]) + win_as_double(v, at));
      else if (fn == AGG_MIN) { if (first || win_less(v, env.acc[j], at)) env.acc[j] = v; }
      else if (first || win_less(env.acc[j], v, at)) env.acc[j] = v;
    }
    ++end;
    env.rec = rec;
    env.ev_ts = ts;
    env.cnt = (uint64_t)(end - f);
    bool pass = true;
    if (kVm && p.having_prog >= 0) {
      bool isnull = false;
      const uint64_t v = vm_eval(a.vm.code, a.vm.konst, p.having_prog, R, threadIdx.x, kWalkThreads, env, &isnull);
      pass = !isnull && (v & 1u);
    }
    if (!pass) continue;
    if (kEmit) win_emit<kVm>(a, R, env, kl * p.key_stride + p.key_offset, seq_base + (int64_t)(uint32_t)rec[1],
                             out_pos + emitted);
    ++emitted;
  }
  if (kEmit) {
    // commit: the live entries that came from records (end - f <= ring of them)
    const int c0 = f > n0 ? f : n0;
    int e = (head0 + c0) % ring;
    for (int i = c0; i < end; ++i) {
      const uint64_t* rec = qrec(i);
      uint64_t* dst = sl + (int64_t)(nagg + e * ew) * ks;
      for (int v = 0; v < a.nval; ++v) dst[(int64_t)v * ks] = rec[2 + a.val_word[v]];
      if (timed) dst[(int64_t)(ew - 1) * ks] = (uint64_t)rec_ts_rel(rec, ts_base);
      if (++e == ring) e = 0;
    }
#pragma unroll
    for (int j = 0; j < kMaxAggs; ++j) {
      if (j >= nagg) break;
      sl[(int64_t)j * ks] = env.acc[j];
    }
    const uint32_t nh = 1u | ((uint32_t)((head0 + f) % ring) << 16) | ((uint32_t)(end - f) << 24);
    L.khdr[k] = nh;
    a.khdr[idx] = nh;
  }
  return emitted;
}

}  // namespace

// kVm = false: no having, every select item is the key, an aggregate or a
// carried word (no interpreter, no LDS register file).
template <bool kVm>
__global__ __launch_bounds__(kWalkThreads) void k_winwalk(WinArgs a) {
  __shared__ WinLds L;
  __shared__ uint64_t R[kVm ? kMaxRegs * kWalkThreads : 1];   // VM registers, [reg][lane]
  __shared__ uint32_t Lseg[kWalkMaxTiles + 1];                 // exclusive prefix of segment sizes
  __shared__ uint16_t Llo[kWalkMaxTiles];                      // segment start inside each tile
  const int tid = threadIdx.x;
  const PatternArgs& p = a.pat;
  const int P = 1 << p.buckets_log2;
  const int bucket = xcd_bucket(blockIdx.x, P);
  const int kpb = (int)((p.key_capacity + P - 1) >> p.buckets_log2);   // <= kWalkMaxKeys (host-checked)
  const int ntiles = a.ntiles;                                         // <= kWalkMaxTiles (host-checked)
  const int64_t ts_base = a.chunk_base[0];
  const int64_t seq_base = a.chunk_base[1];
  // this bucket's per-key headers: kpb consecutive words (bucket-major index)
  for (int k = tid; k < kpb; k += kWalkThreads) L.khdr[k] = a.khdr[(int64_t)bucket * kpb + k];

  // segment starts and sizes -> exclusive prefix over tiles
  win_segments(a, bucket, P, L, Lseg, Llo);

  // LDS windows: runs of whole tiles [t0, t1) with at most kWinWindow records
  int t0 = 0;
  while (t0 < ntiles) {
    uint32_t nw;
    const int t1 = win_build(a, kpb, t0, L, Lseg, Llo, &nw);

    // one lane per key (kpb <= kWalkThreads: key k is lane k in every window,
    // so a lane re-reads only state it wrote itself)
    const bool mine_has = tid < kpb && L.kstart[tid + 1] > L.kstart[tid];
    if (kVm && p.having_prog >= 0) {
      // count pass, output positions, emit pass
      uint32_t mine = 0;
      if (mine_has) mine = win_key<false, kVm>(a, L, R, tid, bucket, kpb, ts_base, seq_base, 0);
      uint32_t tot;
      const uint32_t off = block_excl_scan(mine, L.scratch, &tot);
      if (tid == 0) L.base = tot ? atomicAdd(a.out.count, (unsigned long long)tot) : 0ull;
      lds_barrier();
      if (mine_has) win_key<true, kVm>(a, L, R, tid, bucket, kpb, ts_base, seq_base, L.base + off);
    } else {
      // every record emits one row: a key's rows start at its run's offset
      if (tid == 0) L.base = atomicAdd(a.out.count, (unsigned long long)nw);
      lds_barrier();
      if (mine_has) win_key<true, kVm>(a, L, R, tid, bucket, kpb, ts_base, seq_base, L.base + L.kstart[tid]);
    }
    // the next window reuses the LDS arrays and re-reads state this one wrote
    if (t1 < ntiles) __syncthreads();
    t0 = t1;
  }
}

void launch_winwalk(const WinArgs& a, int nbuckets, bool vm, hipStream_t s) {
  if (vm) hipLaunchKernelGGL(k_winwalk<true>, dim3((unsigned)nbuckets), dim3(kWalkThreads), 0, s, a);
  else hipLaunchKernelGGL(k_winwalk<false>, dim3((unsigned)nbuckets), dim3(kWalkThreads), 0, s, a);
}

}  // namespace cep
