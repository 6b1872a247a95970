// Event tables for gfx950: `@PrimaryKey('k') define table T (...)` with its
// writers and readers (kernels.h TabArgs).
//
// k_tabwalk consumes the generic partition pass's output (k_partition in its
// N-state record form: role bit j = the row passed operation j's filter) like
// k_winwalk does: one workgroup per key bucket builds LDS windows of the
// bucket's records (walk_window.h), groups them by key in arrival order, and
// one lane per key walks its run.
//
// Semantics (upstream Siddhi 4.x, [U] in DESIGN.md): rows are processed in
// arrival order, and for one row the operations that read its stream run in
// plan order; so a reader sees exactly the writes of earlier arrivals plus
// those of earlier operations on the same row.  Per operation, on key k:
//   insert            absent: the row is stored; present: the row is dropped
//                     (the first row stays) and counted in *dropped;
//   update or insert  present: the `set` attributes (without `set`: all) are
//                     overwritten; absent: the select row is stored;
//   update            overwrites only when present;
//   delete            removes only when present;
//   lookup join       present and C holds: one output row with the stream
//                     row's ts and arrival number (a write never emits);
//   in / not in       the filter conjunct is true iff the key is present
//                     (absent): then one output row.
//
// The lane loads its key's row once per LDS window into registers (a present
// flag and up to 8 words).  Readers make the output data-dependent, so the
// walk follows the window walk's two-pass discipline: a count pass and an emit
// pass replay the same run from the same loaded row, neither writes anything
// the other reads, and the row is committed to global memory once, after the
// emit pass, and only when a writer changed it.  A key whose run spans several
// LDS windows hands its row over through that committed state (key k is lane
// k in every window: a lane re-reads only what it wrote itself).  A table
// without readers has no count pass.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "vm.h"
#include "dev_common.h"
#include "walk_window.h"

namespace cep {

namespace {

// Word i of a lane's row.  i is a plan constant, not a compile-time one: a
// masked pick (an indexed register array would become a scratch array).
__device__ __forceinline__ uint64_t tab_pick(const uint64_t (&v)[kMaxCaps], int i) {
  uint64_t x = 0;
#pragma unroll
  for (int w = 0; w < kMaxCaps; ++w) x |= v[w] & (0ull - (uint64_t)(i == w));
  return x;
}

// VM / emission environment: the stream row's record and the table row.
struct TabEnv {
  const uint64_t* rec;     // current record (carried words at rec[2..])
  int64_t ev_ts;
  uint64_t row[kMaxCaps];  // the key's row
  __device__ uint64_t col(int c, int) const { return rec[2 + c]; }
  __device__ uint64_t cap(int i) const { return tab_pick(row, i); }
  __device__ uint64_t outv(int, bool* n) const { *n = true; return 0; }
  __device__ uint64_t agg(int, bool* n) const { *n = true; return 0; }
  __device__ int64_t ts() const { return ev_ts; }
};

template <bool kVm>
__device__ __forceinline__ void tab_emit(const TabArgs& a, const OutArgs& o, uint64_t* R, const TabEnv& env,
                                         int64_t seq, unsigned long long pos) {
  if ((int64_t)pos >= o.cap) {
    set_err(a.err, ERR_OUT_CAP);
    return;
  }
  for (int c = 0; c < o.ncols; ++c) {
    const int src = o.src[c];
    uint64_t v = 0;
    if (src >= SRC_CAP && src < SRC_CAP + kMaxCaps) {
      v = env.cap(src - SRC_CAP);
    } else if (src >= SRC_REC && src < SRC_REC + kMaxCaps) {
      v = env.col(src - SRC_REC, 0);
    } else if (kVm) {
      bool isnull = false;
      v = vm_eval(a.vm.code, a.vm.konst, o.prog[c], R, threadIdx.x, kWalkThreads, env, &isnull);
      if (isnull) v = 0;
    }
    store_col(o.col[c], o.type[c], (int64_t)pos, v);
  }
  o.ts[pos] = env.ev_ts;
  if (o.write_seq) o.seq[pos] = seq;
}

// Per-lane reader counters (LDS: indexed by the operation, which is a loop
// variable; registers indexed that way would live in scratch).
struct TabLds {
  uint32_t n[kTabMaxOps][kWalkThreads];     // rows operation j emitted so far in this pass
  uint32_t off[kTabMaxOps][kWalkThreads];   // the lane's first row of operation j, from base[j]
  unsigned long long base[kTabMaxOps];      // first output row of operation j in this window
};

// One key's records of the LDS window in arrival order, applied to the row
// (present, env.row).  kEmit = false: the count pass (T.n[j][lane] = rows
// operation j emits; nothing is stored).  kEmit = true: operation j's rows
// go to T.base[j] + T.off[j][lane] + 0, 1, ...; drops counts the inserts
// dropped.
template <bool kEmit, bool kVm>
__device__ __forceinline__ void tab_key(const TabArgs& a, const WinLds& L, TabLds& T, uint64_t* R, int k,
                                        int64_t ts_base, int64_t seq_base, bool& present, TabEnv& env, bool& dirty,
                                        uint32_t& drops) {
  const int rw = a.pat.rec_words;
  const int nops = a.nops;
  const uint32_t r0 = L.kstart[k], r1 = L.kstart[k + 1];
  for (uint32_t q = r0; q < r1; ++q) {
    const uint64_t* rec = a.recs + (int64_t)L.wrec[L.sorted[q]] * rw;
    const uint32_t role = (uint32_t)(rec[0] >> 32) & 0xffu;
    env.rec = rec;
    env.ev_ts = rec_ts_rel(rec, ts_base);
    for (int j = 0; j < nops; ++j) {
      if (!((role >> j) & 1u)) continue;
      const TabOp& op = a.op[j];
      const int kind = op.kind;
      if (kind == TOP_JOIN || kind == TOP_IN) {
        bool pass = kind == TOP_JOIN ? present : (present != (op.negate != 0));
        if (kVm && pass && kind == TOP_JOIN && op.on_prog >= 0) {
          bool isnull = false;
          const uint64_t v = vm_eval(a.vm.code, a.vm.konst, op.on_prog, R, threadIdx.x, kWalkThreads, env, &isnull);
          pass = !isnull && (v & 1u);
        }
        if (!pass) continue;
        const uint32_t m = T.n[j][k];
        if (kEmit)
          tab_emit<kVm>(a, a.out[j], R, env, seq_base + (int64_t)(uint32_t)rec[1], T.base[j] + T.off[j][k] + m);
        T.n[j][k] = m + 1;
      } else if (kind == TOP_DELETE) {
        dirty |= present;
        present = false;
      } else if (present) {
        if (kind == TOP_INSERT) {
          ++drops;   // the first row stays
        } else {     // update, update or insert
#pragma unroll
          for (int w = 0; w < kMaxCaps; ++w) {
            const int s = op.set[w];
            if (s >= 0) env.row[w] = rec[2 + s];
          }
          dirty = true;
        }
      } else if (kind != TOP_UPDATE) {   // insert, update or insert: the select row
#pragma unroll
        for (int w = 0; w < kMaxCaps; ++w) {
          const int s = op.ins[w];
          env.row[w] = s >= 0 ? rec[2 + s] : 0ull;
        }
        present = true;
        dirty = true;
      }
    }
  }
}

}  // namespace

// kVm = false: no `on` conjunct beside the key equality, every select item a
// plain attribute of either row (no interpreter, no LDS register file).
template <bool kVm>
__global__ __launch_bounds__(kWalkThreads) void k_tabwalk(TabArgs a) {
  __shared__ WinLds L;
  __shared__ TabLds T;
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
  const int64_t ks = a.kstride;
  const int64_t idx = (int64_t)bucket * kpb + tid;   // this lane's key (tid < kpb)
  uint32_t drops = 0;

  win_segments(a, bucket, P, L, Lseg, Llo);

  // LDS windows: runs of whole tiles [t0, t1) with at most kWinWindow records
  int t0 = 0;
  while (t0 < ntiles) {
    uint32_t nw;
    const int t1 = win_build(a, kpb, t0, L, Lseg, Llo, &nw);

    // the key's row as the window finds it (only when the key has records)
    const bool mine = tid < kpb && L.kstart[tid + 1] > L.kstart[tid];
    bool present0 = false;
    uint64_t row0[kMaxCaps];
#pragma unroll
    for (int w = 0; w < kMaxCaps; ++w) row0[w] = 0;
    if (mine) {
      present0 = (a.thdr[idx] & 1u) != 0;
      if (present0) {
#pragma unroll
        for (int w = 0; w < kMaxCaps; ++w)
          if (w < a.nwords) row0[w] = a.tword[(int64_t)w * ks + idx];
      }
    }
    TabEnv env;
    bool present = present0, dirty = false;
    for (int j = 0; j < a.nops; ++j) {
      T.n[j][tid] = 0;
      T.off[j][tid] = 0;
    }
    if (a.nreaders > 0) {
      // count pass, output positions per reader, emit pass from the same row
      uint32_t nodrops = 0;
      if (mine) {
#pragma unroll
        for (int w = 0; w < kMaxCaps; ++w) env.row[w] = row0[w];
        tab_key<false, kVm>(a, L, T, R, tid, ts_base, seq_base, present, env, dirty, nodrops);
      }
      for (int j = 0; j < a.nops; ++j) {
        if (!a.op[j].reader) continue;   // (uniform: every lane takes the same barriers)
        uint32_t tot;
        const uint32_t off = block_excl_scan(T.n[j][tid], L.scratch, &tot);
        if (tid == 0) T.base[j] = tot ? atomicAdd(a.out[j].count, (unsigned long long)tot) : 0ull;
        T.off[j][tid] = off;
        T.n[j][tid] = 0;
      }
      lds_barrier();
      present = present0;
      dirty = false;
    }
    if (mine) {
#pragma unroll
      for (int w = 0; w < kMaxCaps; ++w) env.row[w] = row0[w];
      tab_key<true, kVm>(a, L, T, R, tid, ts_base, seq_base, present, env, dirty, drops);
      // commit: once, and only a row some writer changed
      if (dirty) {
        if (present) {
#pragma unroll
          for (int w = 0; w < kMaxCaps; ++w)
            if (w < a.nwords) a.tword[(int64_t)w * ks + idx] = env.row[w];
        }
        a.thdr[idx] = present ? 1u : 0u;
      }
    }
    // the next window reuses the LDS arrays and re-reads state this one wrote
    if (t1 < ntiles) __syncthreads();
    t0 = t1;
  }
  // inserts dropped on an existing key: one atomic per workgroup
  {
    uint32_t tot;
    block_excl_scan(drops, L.scratch, &tot);
    if (tid == 0 && tot) atomicAdd(a.dropped, (unsigned long long)tot);
  }
}

void launch_tabwalk(const TabArgs& a, int nbuckets, bool vm, hipStream_t s) {
  if (vm) hipLaunchKernelGGL(k_tabwalk<true>, dim3((unsigned)nbuckets), dim3(kWalkThreads), 0, s, a);
  else hipLaunchKernelGGL(k_tabwalk<false>, dim3((unsigned)nbuckets), dim3(kWalkThreads), 0, s, a);
}

}  // namespace cep
