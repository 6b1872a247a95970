// Tumbling-window aggregates for gfx950: `#window.lengthBatch(N)` /
// `#window.externalTimeBatch(c, T)` in front of a group-by query inside a
// partition (kernels.h BatchArgs).
//
// k_batchwalk consumes the generic partition pass's output like k_winwalk:
// one workgroup per key bucket builds LDS windows of the bucket's records
// (walk_window.h), grouped by key in arrival order, and one lane per key walks
// its run.
//
// Semantics (upstream Siddhi 4.x, [U] in DESIGN.md): per kept row e of a
// window instance, in arrival order,
//   lengthBatch(N)            e joins the batch; at N rows the batch closes
//                             (trigger e);
//   externalTimeBatch(c, T)   x = e.c.  First row: start = x, end = x + T.
//                             Else if x >= end: the batch closes (trigger e,
//                             which is not a member) and end = x + (T - ((x -
//                             start) mod T)).  Then e joins the batch.
// A closing batch folds its rows oldest first into fresh aggregates,
// evaluating `having` after each row; it emits the last row for which having
// held, with the aggregates as of that row, the row's own ts and the
// trigger's arrival number.
//
// The fold runs as rows arrive: the state is the open batch's accumulators
// and row count plus the candidate, the last row so far that passed having.
// Without having the candidate is the batch's last row and its aggregates are
// the batch's; lengthBatch without having emits the trigger itself and keeps
// no candidate at all.  The candidate may be a row of an earlier LDS window or
// chunk: its ts and carried words then come from the state, otherwise from
// its record (the walk only remembers its position in the run).
//
// A key's rows per LDS window depend on the data, so a count pass (nothing is
// stored) precedes the emit pass; both replay the same read-only state, which
// the emit pass commits once at its end.  lengthBatch without having skips
// the count pass: (rows in the open batch + records) / N.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "vm.h"
#include "dev_common.h"
#include "walk_window.h"

namespace cep {

namespace {

__device__ __forceinline__ double bat_as_double(uint64_t v, int t) {
  switch (t) {
    case T_INT: return (double)(int32_t)v;
    case T_LONG: return (double)(int64_t)v;
    case T_FLOAT: return (double)as_f32(v);
    default: return as_f64(v);
  }
}

__device__ __forceinline__ bool bat_less(uint64_t a, uint64_t b, int t) {
  switch (t) {
    case T_LONG: return (int64_t)a < (int64_t)b;
    case T_FLOAT: return as_f32(a) < as_f32(b);
    case T_DOUBLE: return as_f64(a) < as_f64(b);
    default: return (int32_t)a < (int32_t)b;
  }
}

// VM / emission environment: a row (its record, or the candidate block of the
// key's state when the row arrived in an earlier LDS window) and aggregates.
struct BatchEnv {
  const PatternArgs* p;
  const uint64_t* row;     // carried word c of the row at row[c * stride]: its record's
  int64_t stride;          // words (stride 1) or the candidate block of the state (kstride)
  int64_t ev_ts;
  uint64_t cnt;            // rows folded so far
  uint64_t acc[kMaxAggs];
  __device__ uint64_t col(int c, int) const { return row[(int64_t)c * stride]; }
  __device__ uint64_t cap(int) const { return 0; }
  __device__ uint64_t outv(int, bool* n) const { *n = true; return 0; }
  __device__ uint64_t agg(int i, bool* isnull) const {
    // masked pick (a select chain on i would become a scratch array access)
    uint64_t x = 0;
#pragma unroll
    for (int j = 0; j < kMaxAggs; ++j) x |= acc[j] & (0ull - (uint64_t)(i == j));
    *isnull = false;   // at least one row is folded
    const int fn = p->agg_fn[i];
    if (fn == AGG_COUNT) return cnt;
    if (fn == AGG_AVG) return from_f64(as_f64(x) / (double)(int64_t)cnt);
    return x;
  }
  __device__ int64_t ts() const { return ev_ts; }
};

template <bool kVm>
__device__ __forceinline__ void bat_emit(const BatchArgs& a, uint64_t* R, const BatchEnv& env, int64_t key,
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
// count pass (closed batches with a candidate; nothing is stored).
template <bool kEmit, bool kVm>
__device__ __forceinline__ uint32_t bat_key(const BatchArgs& a, WinLds& L, uint64_t* R, int k, int bucket, int kpb,
                                            int64_t ts_base, int64_t seq_base, unsigned long long out_pos) {
  const PatternArgs& p = a.pat;
  const int64_t idx = (int64_t)bucket * kpb + k;
  const int64_t kl = ((int64_t)k << p.buckets_log2) | bucket;
  const int64_t key = kl * p.key_stride + p.key_offset;
  const int64_t ks = a.kstride;
  const int rw = p.rec_words;
  const int nagg = p.nagg;
  const bool timed = a.kind == WIN_TIME_BATCH;
  const bool hav = kVm && p.having_prog >= 0;
  const bool keep = a.cand_w >= 0;          // the candidate outlives the row that made it
  uint64_t* sl = a.kslot + idx;             // state word w of this key: sl[w * ks]
  const bool live = (L.khdr[k] & 1u) != 0;
  const uint32_t r0 = L.kstart[k], r1 = L.kstart[k + 1];

  BatchEnv env;   // the open batch: running aggregates, the current row
  env.p = &p;
  env.stride = 1;
#pragma unroll
  for (int j = 0; j < kMaxAggs; ++j) env.acc[j] = (live && j < nagg) ? sl[(int64_t)j * ks] : 0;
  const uint64_t w0 = live ? sl[(int64_t)nagg * ks] : 0;
  uint32_t cnt = (uint32_t)w0;
  bool has = keep && ((w0 >> 32) & 1u);     // a candidate exists
  int64_t start = 0, end = 0;
  if (timed && live) {
    start = (int64_t)sl[(int64_t)a.time_w * ks];
    end = (int64_t)sl[(int64_t)(a.time_w + 1) * ks];
  }
  bool started = live;
  // the candidate: record cq of this run, or (cq < 0) the state's candidate block
  int64_t cq = -1;
  uint64_t cacc[kMaxAggs];                  // its aggregates (having only)
  uint64_t ccnt = 0;
  if (kVm) {
#pragma unroll
    for (int j = 0; j < kMaxAggs; ++j) cacc[j] = (hav && has && j < nagg) ? sl[(int64_t)(a.cand_acc_w + j) * ks] : 0;
    if (hav && has) ccnt = sl[(int64_t)(a.cand_acc_w + nagg) * ks];
  }

  auto rec_at = [&](uint32_t q) { return a.recs + (int64_t)L.wrec[L.sorted[q]] * rw; };
  uint32_t emitted = 0;
  for (uint32_t q = r0; q < r1; ++q) {
    const uint64_t* rec = rec_at(q);
    const int64_t seq = seq_base + (int64_t)(uint32_t)rec[1];
    // externalTimeBatch closes the batch before the row joins it, lengthBatch
    // after: the loop body visits the one close site on either side of the
    // join (a second copy of it costs the <false> build its scratch-free frame)
    int64_t x = 0;
    bool fire = false;
    if (timed) {
      x = (int64_t)rec[2 + a.time_word];
      if (!started) {
        start = x;
        end = x + a.param;
        started = true;
      } else {
        fire = x >= end;
      }
    }
    for (bool joined = false;; joined = true) {
      if (fire) {
        // the open batch closes at this row: its candidate leaves
        if (has) {
          if (kEmit) {
            BatchEnv ce;
            ce.p = &p;
            if (cq >= 0) {
              const uint64_t* crec = rec_at((uint32_t)cq);
              ce.row = crec + 2;
              ce.stride = 1;
              ce.ev_ts = rec_ts_rel(crec, ts_base);
            } else {
              ce.row = sl + (int64_t)(a.cand_w + 1) * ks;
              ce.stride = ks;
              ce.ev_ts = (int64_t)sl[(int64_t)a.cand_w * ks];
            }
            ce.cnt = (kVm && hav) ? ccnt : (uint64_t)cnt;
#pragma unroll
            for (int j = 0; j < kMaxAggs; ++j) ce.acc[j] = (kVm && hav) ? cacc[j] : env.acc[j];
            bat_emit<kVm>(a, R, ce, key, seq, out_pos + emitted);
          }
          ++emitted;
        }
        has = false;
        cq = -1;
        cnt = 0;
#pragma unroll
        for (int j = 0; j < kMaxAggs; ++j) env.acc[j] = 0;
        if (timed) end = x + (a.param - ((x - start) % a.param));
      }
      if (joined) break;
      // the row joins the batch
      const bool first = cnt == 0;
#pragma unroll
      for (int j = 0; j < kMaxAggs; ++j) {
        if (j >= nagg) break;
        const int fn = p.agg_fn[j], at = p.agg_arg_type[j];
        if (fn == AGG_COUNT) continue;
        const uint64_t v = rec[2 + p.agg_word[j]];
        if (fn == AGG_SUM && p.agg_out_type[j] == T_LONG) env.acc[j] = first ? v : env.acc[j] + v;
        else if (fn == AGG_SUM || fn == AGG_AVG) env.acc[j] = from_f64((first ? 0.0 : as_f64(env.acc[j])) + bat_as_double(v, at));
        else if (fn == AGG_MIN) { if (first || bat_less(v, env.acc[j], at)) env.acc[j] = v; }
        else if (first || bat_less(env.acc[j], v, at)) env.acc[j] = v;
      }
      ++cnt;
      bool pass = true;
      if (kVm && hav) {
        env.row = rec + 2;
        env.ev_ts = rec_ts_rel(rec, ts_base);
        env.cnt = (uint64_t)cnt;
        bool isnull = false;
        const uint64_t v = vm_eval(a.vm.code, a.vm.konst, p.having_prog, R, threadIdx.x, kWalkThreads, env, &isnull);
        pass = !isnull && (v & 1u);
      }
      if (pass) {
        has = true;
        cq = (int64_t)q;
        if (kVm && hav) {
          ccnt = (uint64_t)cnt;
#pragma unroll
          for (int j = 0; j < kMaxAggs; ++j) cacc[j] = env.acc[j];
        }
      }
      fire = !timed && cnt == (uint32_t)a.param;
      if (!fire) break;
    }
  }
  if (kEmit) {
    // commit: the open batch, and the candidate when it is a record of this run
#pragma unroll
    for (int j = 0; j < kMaxAggs; ++j) {
      if (j >= nagg) break;
      sl[(int64_t)j * ks] = env.acc[j];
    }
    sl[(int64_t)nagg * ks] = (uint64_t)cnt | ((uint64_t)((keep && has) ? 1u : 0u) << 32);
    if (timed) {
      sl[(int64_t)a.time_w * ks] = (uint64_t)start;
      sl[(int64_t)(a.time_w + 1) * ks] = (uint64_t)end;
    }
    if (keep && has && cq >= 0) {
      const uint64_t* rec = rec_at((uint32_t)cq);
      sl[(int64_t)a.cand_w * ks] = (uint64_t)rec_ts_rel(rec, ts_base);
      for (int c = 0; c < p.nrec_a; ++c) sl[(int64_t)(a.cand_w + 1 + c) * ks] = rec[2 + c];
      if (kVm && hav) {
#pragma unroll
        for (int j = 0; j < kMaxAggs; ++j) {
          if (j >= nagg) break;
          sl[(int64_t)(a.cand_acc_w + j) * ks] = cacc[j];
        }
        sl[(int64_t)(a.cand_acc_w + nagg) * ks] = ccnt;
      }
    }
    if (!live) {
      L.khdr[k] = 1u;
      a.khdr[idx] = 1u;
    }
  }
  return emitted;
}

}  // namespace

// kVm = false: no having, every select item is the key, an aggregate or a
// carried word (no interpreter, no LDS register file).
template <bool kVm>
__global__ __launch_bounds__(kWalkThreads) void k_batchwalk(BatchArgs a) {
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
  for (int k = tid; k < kpb; k += kWalkThreads) L.khdr[k] = a.khdr[(int64_t)bucket * kpb + k];

  win_segments(a, bucket, P, L, Lseg, Llo);

  // closed-form row count: lengthBatch whose candidate is always the trigger
  const bool counted = a.kind == WIN_LENGTH_BATCH && a.cand_w < 0;
  int t0 = 0;
  while (t0 < ntiles) {
    uint32_t nw;
    const int t1 = win_build(a, kpb, t0, L, Lseg, Llo, &nw);

    // one lane per key (kpb <= kWalkThreads: key k is lane k in every window,
    // so a lane re-reads only state it wrote itself)
    const bool mine_has = tid < kpb && L.kstart[tid + 1] > L.kstart[tid];
    uint32_t mine = 0;
    if (mine_has) {
      if (counted) {
        const uint64_t c0 = (L.khdr[tid] & 1u)
                                ? (uint32_t)a.kslot[(int64_t)p.nagg * a.kstride + (int64_t)bucket * kpb + tid]
                                : 0u;
        mine = (uint32_t)((c0 + (L.kstart[tid + 1] - L.kstart[tid])) / (uint64_t)a.param);
      } else {
        mine = bat_key<false, kVm>(a, L, R, tid, bucket, kpb, ts_base, seq_base, 0);
      }
    }
    uint32_t tot;
    const uint32_t off = block_excl_scan(mine, L.scratch, &tot);
    if (tid == 0) L.base = tot ? atomicAdd(a.out.count, (unsigned long long)tot) : 0ull;
    lds_barrier();
    if (mine_has) bat_key<true, kVm>(a, L, R, tid, bucket, kpb, ts_base, seq_base, L.base + off);
    // the next window reuses the LDS arrays and re-reads state this one wrote
    if (t1 < ntiles) __syncthreads();
    t0 = t1;
  }
}

void launch_batchwalk(const BatchArgs& a, int nbuckets, bool vm, hipStream_t s) {
  if (vm) hipLaunchKernelGGL(k_batchwalk<true>, dim3((unsigned)nbuckets), dim3(kWalkThreads), 0, s, a);
  else hipLaunchKernelGGL(k_batchwalk<false>, dim3((unsigned)nbuckets), dim3(kWalkThreads), 0, s, a);
}

}  // namespace cep
