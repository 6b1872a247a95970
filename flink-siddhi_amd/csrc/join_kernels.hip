// Windowed stream joins for gfx950: `from A[f]#window.wa as a join
// B[g]#window.wb as b on C select ... insert into O` (kernels.h JoinArgs,
// DESIGN.md §10).
//
// Semantics (upstream Siddhi 4.x, [U] in DESIGN.md): per kept row e of side X,
// in arrival order over both streams,
//   1. the other side Y's window as it stands when e arrives: of Y's kept
//      rows that arrived before e, the last N (length(N)) or those with
//      r.ts + T > e.ts (time(T));
//   2. for each such r, oldest first, evaluate `on` (a.* = the A-side row,
//      b.* = the B-side row, whichever of the two is e);
//   3. where it holds, emit the select list with e's ts and arrival number;
//   4. e enters X's own window (it never joins rows of its own side).
//
// Per chunk, on one stream:
//   k_joinmark     each row's side and filter -> a flag byte; kept rows per
//                  block and side
//   k_joinscan     one workgroup: exclusive prefix of the block counts, list
//                  sizes, probe count
//   k_joinappend   kept rows appended behind each side's tail (arrival order),
//                  one probe entry per kept row in the merged probe list
//   k_joinprobe    count pass: one lane per probe, matches in [lo, hi)
//   k_joinscan2    one workgroup: output offsets per probe block, the chunk's
//                  row total, the output rows reserved
//   k_joinprobe    emit pass: replays the same read-only lists, rows at off + j
//   k_jointail     the rows that can still join later rows move to the front
//                  of the side's other buffer (never in place)
// Nothing a pass reads is written by that pass, so the count and emit passes
// see the same state (the two-pass discipline of k_winwalk).
//
// A workgroup's probes are consecutive arrivals, so their ranges in the other
// list overlap.  The direct `on` form (JoinTerm) stages the compared words of
// that span through LDS in tiles of kJoinTile entries, one array per term
// ([term][entry], 8-byte words): lanes that test consecutive entries read
// consecutive banks, lanes that test the same entry broadcast.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "vm.h"
#include "dev_common.h"

namespace cep {

namespace {

struct JoinRowEnv {          // a side's filter over the batch row
  const RowsArgs* r;
  int64_t row;
  __device__ uint64_t col(int c, int type) const { return load_col(r->cols.p[c], type, row); }
  __device__ uint64_t cap(int) const { return 0; }
  __device__ uint64_t outv(int, bool* n) const { *n = true; return 0; }
  __device__ uint64_t agg(int, bool* n) const { *n = true; return 0; }
  __device__ int64_t ts() const { return r->ts[row]; }
};

struct JoinEnv {             // `on` and select items over a pair of list entries
  const uint64_t* ar;        // A-side entry
  const uint64_t* br;        // B-side entry
  int64_t ev_ts;             // the triggering row's ts
  __device__ uint64_t col(int c, int) const { return ar[2 + c]; }
  __device__ uint64_t cap(int i) const { return br[2 + i]; }
  __device__ uint64_t outv(int, bool* n) const { *n = true; return 0; }
  __device__ uint64_t agg(int, bool* n) const { *n = true; return 0; }
  __device__ int64_t ts() const { return ev_ts; }
};

// A term-list predicate over one batch row (plan.h TermList: promotion
// applied at compile time, a null arithmetic result compares false).
__device__ __forceinline__ bool join_terms_row(const TermList& tl, const ColSet& cols, int64_t row) {
  bool acc = tl.any == 0;
#pragma unroll
  for (int i = 0; i < kMaxTerms; ++i) {
    if (i >= tl.n) break;
    const Term& t = tl.t[i];
    uint64_t v = load_col(cols.p[t.col], cols.t[t.col], row);
    int ty = (t.coltype == T_BOOL || t.coltype == T_STRING) ? T_INT : t.coltype;
    bool ok = true;
    if (t.aop) {
      uint64_t r = 0;
      ok = vm_arith(t.aop, t.atype, vm_convert(v, ty, t.atype), t.aconst, &r);
      v = r;
      ty = t.atype;
    }
    ok = ok && vm_compare(t.cop, t.ctype, vm_convert(v, ty, t.ctype), t.cconst);
    acc = tl.any ? (acc || ok) : (acc && ok);
  }
  return acc;
}

// Rows [lo, hi) of a ts-ordered list: the first whose ts + T > ts.
__device__ __forceinline__ uint64_t join_time_lo(const uint64_t* list, int ew, uint64_t hi, int64_t T, int64_t ts) {
  uint64_t l = 0, h = hi;
  while (l < h) {
    const uint64_t m = (l + h) >> 1;
    if ((int64_t)list[m * (uint64_t)ew] + T > ts) h = m;
    else l = m + 1;
  }
  return l;
}

template <bool kVmSel>
__device__ __forceinline__ void join_emit(const JoinArgs& a, uint64_t* R, const JoinEnv& env, const uint64_t* own,
                                          uint64_t pos) {
  if ((int64_t)pos >= a.out.cap) {
    set_err(a.err, ERR_OUT_CAP);
    return;
  }
  for (int c = 0; c < a.out.ncols; ++c) {
    const int src = a.out.src[c];
    uint64_t v = 0;
    if (src >= SRC_REC && src < SRC_REC + kMaxCaps) {
      v = env.ar[2 + src - SRC_REC];
    } else if (src >= SRC_CAP && src < SRC_CAP + kMaxCaps) {
      v = env.br[2 + src - SRC_CAP];
    } else if (kVmSel) {
      bool isnull = false;
      v = vm_eval(a.vm.code, a.vm.konst, a.out.prog[c], R, threadIdx.x, kJoinThreads, env, &isnull);
      if (isnull) v = 0;
    }
    store_col(a.out.col[c], a.out.type[c], (int64_t)pos, v);
  }
  a.out.ts[pos] = (int64_t)own[0];
  if (a.out.write_seq) a.out.seq[pos] = (int64_t)own[1];
}

}  // namespace

// One pass over the chunk's columns: side, filter, flag byte, ts descent check.
template <bool kVm>
__global__ __launch_bounds__(kJoinThreads) void k_joinmark(JoinArgs a) {
  __shared__ uint64_t R[kVm ? kMaxRegs * kJoinThreads : 1];   // VM registers, [reg][lane]
  __shared__ uint32_t tot[2];
  const int tid = threadIdx.x;
  if (tid < 2) tot[tid] = 0;
  __syncthreads();
  const RowsArgs& r = a.rows;
  const int64_t i0 = (int64_t)blockIdx.x * kJoinBlockRows + (int64_t)tid * kJoinItems;
  uint32_t c0 = 0, c1 = 0;
  for (int e = 0; e < kJoinItems; ++e) {
    const int64_t i = i0 + e;
    if (i >= r.n) break;
    const int64_t row = r.row0 + i;
    const int sh = r.stream ? (int)r.stream[row] : (int)r.input;
    uint32_t f = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (sh != a.stream[s]) continue;
      bool keep = true;
      if (a.filter_prog[s] >= 0) {
        if (a.filter_terms[s].n >= 0) {
          keep = join_terms_row(a.filter_terms[s], r.cols, row);
        } else if (kVm) {
          JoinRowEnv env{&r, row};
          bool isnull = false;
          const uint64_t v = vm_eval(a.vm.code, a.vm.konst, a.filter_prog[s], R, tid, kJoinThreads, env, &isnull);
          keep = !isnull && (v & 1u);
        }
      }
      if (keep) f = (uint32_t)s + 1u;
    }
    if (a.check_order) {
      const int64_t prev = row > 0 ? r.ts[row - 1] : batch_prev_ts(r);
      if (r.ts[row] < prev) report_descent(r, a.err);
    }
    a.flag[i] = (uint8_t)f;
    c0 += f == 1u;
    c1 += f == 2u;
  }
  if (c0) atomicAdd(&tot[0], c0);
  if (c1) atomicAdd(&tot[1], c1);
  __syncthreads();
  if (tid < 2) a.bsum[(int64_t)blockIdx.x * 2 + tid] = tot[tid];
}

// One workgroup: exclusive prefix of the per-block kept counts of each side.
__global__ __launch_bounds__(kJoinThreads) void k_joinscan(JoinArgs a, int nblk) {
  __shared__ uint32_t scratch[16];
  const int tid = threadIdx.x;
  uint32_t run0 = 0, run1 = 0;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    uint32_t run = 0;
    for (int base = 0; base < nblk; base += kJoinThreads) {
      const int b = base + tid;
      const uint32_t v = b < nblk ? a.bsum[(int64_t)b * 2 + s] : 0u;
      uint32_t t;
      const uint32_t off = block_excl_scan(v, scratch, &t);
      if (b < nblk) a.boff[(int64_t)b * 2 + s] = run + off;
      run += t;
    }
    if (s == 0) run0 = run;
    else run1 = run;
  }
  if (tid == 0) {
    JoinState* st = a.st;
    st->n[0] = st->tail[0] + run0;
    st->n[1] = st->tail[1] + run1;
    st->kept[0] += run0;
    st->kept[1] += run1;
    st->nprobe = (uint64_t)run0 + run1;
  }
}

// Kept rows behind each side's tail, in arrival order; one probe per kept row.
__global__ __launch_bounds__(kJoinThreads) void k_joinappend(JoinArgs a) {
  __shared__ uint32_t scratch[16];
  const int tid = threadIdx.x;
  const RowsArgs& r = a.rows;
  const int64_t i0 = (int64_t)blockIdx.x * kJoinBlockRows + (int64_t)tid * kJoinItems;
  uint32_t f[kJoinItems];
  uint32_t c0 = 0, c1 = 0;
#pragma unroll
  for (int e = 0; e < kJoinItems; ++e) {
    f[e] = i0 + e < r.n ? (uint32_t)a.flag[i0 + e] : 0u;
    c0 += f[e] == 1u;
    c1 += f[e] == 2u;
  }
  uint32_t t0, t1;
  const uint32_t off0 = block_excl_scan(c0, scratch, &t0);
  const uint32_t off1 = block_excl_scan(c1, scratch, &t1);
  const uint32_t b0 = a.boff[(int64_t)blockIdx.x * 2], b1 = a.boff[(int64_t)blockIdx.x * 2 + 1];
  uint64_t pos0 = a.st->tail[0] + b0 + off0;     // A-side entries before this lane's rows
  uint64_t pos1 = a.st->tail[1] + b1 + off1;
  uint64_t pp = (uint64_t)b0 + b1 + off0 + off1;   // probes before them
  const int ew = a.ew;
#pragma unroll
  for (int e = 0; e < kJoinItems; ++e) {
    if (!f[e]) continue;
    const int64_t row = r.row0 + i0 + e;
    const bool sb = f[e] == 2u;
    const uint64_t own = sb ? pos1 : pos0, hi = sb ? pos0 : pos1;
    uint64_t* list = sb ? a.list[1] : a.list[0];
    const int64_t cap = sb ? a.list_cap[1] : a.list_cap[0];
    if ((int64_t)own < cap) {
      uint64_t* dst = list + own * (uint64_t)ew;
      dst[0] = (uint64_t)r.ts[row];
      dst[1] = (uint64_t)row_seq(r, row);
      for (int w = 0; w < a.nw; ++w) dst[2 + w] = load_col(r.cols.p[a.rec[w]], r.cols.t[a.rec[w]], row);
    } else {
      set_err(a.err, ERR_WINDOW);   // (the arenas hold tail cap + chunk entries: host-sized)
    }
    a.probe[pp] = own | (hi << 31) | ((uint64_t)(sb ? 1u : 0u) << 62);
    ++pp;
    if (sb) ++pos1;
    else ++pos0;
  }
}

// One lane per probe, in arrival order.  kEmit = false: the count pass.
// kVmOn = false: `on` is JoinArgs::terms (LDS-staged window words);
// kVmOn = true: the interpreter, A-side entry through col(), B-side through cap().
template <bool kVmOn, bool kVmSel, bool kEmit>
__global__ __launch_bounds__(kJoinThreads) void k_joinprobe(JoinArgs a) {
  constexpr bool kRegs = kVmOn || (kEmit && kVmSel);
  __shared__ uint64_t R[kRegs ? kMaxRegs * kJoinThreads : 1];          // VM registers, [reg][lane]
  __shared__ uint64_t tile[kVmOn ? 1 : kMaxTerms * kJoinTile];        // [term][entry]
  __shared__ uint32_t span[2];
  __shared__ uint32_t scratch[16];
  const int tid = threadIdx.x;
  const uint64_t np = a.st->nprobe;
  if ((uint64_t)blockIdx.x * kJoinThreads >= np) {   // (uniform: before any barrier)
    if (!kEmit && tid == 0) a.pbsum[blockIdx.x] = 0;
    return;
  }
  const uint64_t gi = (uint64_t)blockIdx.x * kJoinThreads + tid;
  bool valid = gi < np;
  const int ew = a.ew;
  const uint64_t pe = valid ? a.probe[gi] : 0ull;
  const bool sb = (pe >> 62) & 1u;                   // the probe row's side
  const uint64_t own = pe & 0x7fffffffull;
  uint64_t hi = (pe >> 31) & 0x7fffffffull;
  // (entries the arenas cannot hold: no kernel writes such a probe)
  if (valid && ((int64_t)own >= (sb ? a.list_cap[1] : a.list_cap[0]) ||
                (int64_t)hi > (sb ? a.list_cap[0] : a.list_cap[1]))) {
    set_err(a.err, ERR_WINDOW);
    valid = false;
  }
  if (!valid) hi = 0;
  const uint64_t* ownp = (sb ? a.list[1] : a.list[0]) + own * (uint64_t)ew;
  const uint64_t* olist = sb ? a.list[0] : a.list[1];
  const int64_t ets = valid ? (int64_t)ownp[0] : 0;
  uint64_t lo = 0;
  if (valid) {
    const int okind = sb ? a.win_kind[0] : a.win_kind[1];      // the other side's window
    const int64_t oparam = sb ? a.win_param[0] : a.win_param[1];
    if (okind == WIN_LENGTH) lo = hi > (uint64_t)oparam ? hi - (uint64_t)oparam : 0;
    else lo = join_time_lo(olist, ew, hi, oparam, ets);
  }
  uint64_t pos = 0;
  if (kEmit) {
    uint32_t t;
    const uint32_t off = block_excl_scan(valid ? a.pcnt[gi] : 0u, scratch, &t);
    pos = a.st->out_base + a.pboff[blockIdx.x] + off;
  }
  uint32_t cnt = 0;
  JoinEnv env;
  env.ev_ts = ets;
  if (kVmOn) {
    for (uint64_t j = lo; j < hi; ++j) {
      const uint64_t* win = olist + j * (uint64_t)ew;
      env.ar = sb ? win : ownp;
      env.br = sb ? ownp : win;
      bool ok = true;
      if (a.on_prog >= 0) {
        bool isnull = false;
        const uint64_t v = vm_eval(a.vm.code, a.vm.konst, a.on_prog, R, tid, kJoinThreads, env, &isnull);
        ok = !isnull && (v & 1u);
      }
      if (!ok) continue;
      if (kEmit) join_emit<kVmSel>(a, R, env, ownp, pos + cnt);
      ++cnt;
    }
  } else {
    // the probe row's compared words (fixed term indices: no register array is indexed at run time)
    uint64_t pv[kMaxTerms];
#pragma unroll
    for (int i = 0; i < kMaxTerms; ++i)
      pv[i] = (valid && i < a.nterms) ? ownp[2 + (sb ? a.terms[i].wb : a.terms[i].wa)] : 0ull;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      // probes of side p read the other side's list: one span per side and workgroup
      if (tid == 0) {
        span[0] = 0xffffffffu;
        span[1] = 0;
      }
      lds_barrier();
      const bool active = valid && (int)sb == p && lo < hi;
      if (active) {
        atomicMin(&span[0], (uint32_t)lo);
        atomicMax(&span[1], (uint32_t)hi);
      }
      lds_barrier();
      const uint32_t s0 = span[0], s1 = span[1];
      const uint64_t* wl = p ? a.list[0] : a.list[1];
      for (uint32_t t0 = s0; t0 < s1; t0 += kJoinTile) {
        const uint32_t n = s1 - t0 < (uint32_t)kJoinTile ? s1 - t0 : (uint32_t)kJoinTile;
#pragma unroll
        for (int i = 0; i < kMaxTerms; ++i) {
          if (i >= a.nterms) break;
          const int wi = p ? a.terms[i].wa : a.terms[i].wb;   // the window row's word of term i
          if ((uint32_t)tid < n) tile[i * kJoinTile + tid] = wl[(uint64_t)(t0 + tid) * ew + 2 + wi];
        }
        lds_barrier();
        if (active) {
          const uint32_t j0 = (uint32_t)lo > t0 ? (uint32_t)lo : t0;
          const uint32_t j1 = (uint32_t)hi < t0 + n ? (uint32_t)hi : t0 + n;
          for (uint32_t j = j0; j < j1; ++j) {
            bool ok = true;
#pragma unroll
            for (int i = 0; i < kMaxTerms; ++i) {
              if (i >= a.nterms) break;
              const uint64_t wv = tile[i * kJoinTile + (j - t0)];
              const uint64_t av = p ? wv : pv[i], bv = p ? pv[i] : wv;
              ok = ok && vm_compare(a.terms[i].op, a.terms[i].type, av, bv);
            }
            if (!ok) continue;
            if (kEmit) {
              const uint64_t* win = wl + (uint64_t)j * ew;
              env.ar = p ? win : ownp;
              env.br = p ? ownp : win;
              join_emit<kVmSel>(a, R, env, ownp, pos + cnt);
            }
            ++cnt;
          }
        }
        lds_barrier();   // the next tile (and the next side's span) reuse the LDS words
      }
      lds_barrier();
    }
  }
  if (!kEmit) {
    if (valid) a.pcnt[gi] = cnt;
    uint32_t t;
    block_excl_scan(cnt, scratch, &t);
    if (tid == 0) a.pbsum[blockIdx.x] = t;
  }
}

// One workgroup: output offsets per probe block, the chunk's row total, and
// the output rows it takes (the host grows the output to hold them before the
// emit pass runs).
__global__ __launch_bounds__(kJoinThreads) void k_joinscan2(JoinArgs a, int npb) {
  __shared__ uint32_t scratch[16];
  const int tid = threadIdx.x;
  uint64_t run = 0;
  for (int base = 0; base < npb; base += kJoinThreads) {
    const int b = base + tid;
    const uint32_t v = b < npb ? a.pbsum[b] : 0u;
    uint32_t t;
    const uint32_t off = block_excl_scan(v, scratch, &t);
    // (a chunk of <= 2^18 probes over lists of < 2^31 entries: block offsets fit 32 bits only
    // below 2^32 rows per chunk; beyond, the capacity check of the emit pass refuses the rows)
    if (b < npb) a.pboff[b] = (uint32_t)(run + off);
    run += t;
  }
  if (tid == 0) {
    if (run > 0xffffffffull) set_err(a.err, ERR_OUT_CAP);
    a.st->total = run;
    a.st->out_base = run ? atomicAdd(a.out.count, (unsigned long long)run) : 0ull;
  }
}

// The rows later arrivals can still join: the last N of a length side, the
// rows with ts + T > the chunk's last ts of a time side, moved to the front
// of the side's other buffer.
__global__ __launch_bounds__(kJoinThreads) void k_jointail(JoinArgs a) {
  __shared__ uint64_t sh_start;
  const int tid = threadIdx.x;
  const int s = blockIdx.y;
  const int ew = a.ew;
  const uint64_t* src = s ? a.list[1] : a.list[0];
  uint64_t* dst = s ? a.next[1] : a.next[0];
  const int64_t cap = s ? a.list_cap[1] : a.list_cap[0];
  uint64_t n = a.st->n[s];
  if (n > (uint64_t)cap) n = (uint64_t)cap;
  if (tid == 0) {
    const int kind = s ? a.win_kind[1] : a.win_kind[0];
    const int64_t param = s ? a.win_param[1] : a.win_param[0];
    uint64_t start;
    if (kind == WIN_LENGTH) {
      start = n > (uint64_t)param ? n - (uint64_t)param : 0;
    } else {
      const int64_t last = a.rows.ts[a.rows.row0 + a.rows.n - 1];
      start = join_time_lo(src, ew, n, param, last);
      if (n - start > (uint64_t)kJoinTailCap) {
        if (blockIdx.x == 0) set_err(a.err, ERR_JOIN_TAIL);
        start = n - (uint64_t)kJoinTailCap;
      }
    }
    sh_start = start;
  }
  __syncthreads();
  const uint64_t start = sh_start;
  const uint64_t words = (n - start) * (uint64_t)ew;
  const uint64_t* from = src + start * (uint64_t)ew;
  for (uint64_t i = (uint64_t)blockIdx.x * kJoinThreads + tid; i < words; i += (uint64_t)gridDim.x * kJoinThreads)
    dst[i] = from[i];
  if (blockIdx.x == 0 && tid == 0) a.st->tail[s] = n - start;
}

void launch_join_mark(const JoinArgs& a, bool vm, hipStream_t s) {
  const int nblk = (int)((a.rows.n + kJoinBlockRows - 1) / kJoinBlockRows);
  if (vm) hipLaunchKernelGGL(k_joinmark<true>, dim3((unsigned)nblk), dim3(kJoinThreads), 0, s, a);
  else hipLaunchKernelGGL(k_joinmark<false>, dim3((unsigned)nblk), dim3(kJoinThreads), 0, s, a);
  hipLaunchKernelGGL(k_joinscan, dim3(1), dim3(kJoinThreads), 0, s, a, nblk);
  hipLaunchKernelGGL(k_joinappend, dim3((unsigned)nblk), dim3(kJoinThreads), 0, s, a);
}

void launch_join_count(const JoinArgs& a, bool vm, hipStream_t s) {
  const int npb = (int)((a.rows.n + kJoinThreads - 1) / kJoinThreads);
  if (vm) hipLaunchKernelGGL((k_joinprobe<true, false, false>), dim3((unsigned)npb), dim3(kJoinThreads), 0, s, a);
  else hipLaunchKernelGGL((k_joinprobe<false, false, false>), dim3((unsigned)npb), dim3(kJoinThreads), 0, s, a);
  hipLaunchKernelGGL(k_joinscan2, dim3(1), dim3(kJoinThreads), 0, s, a, npb);
}

void launch_join_emit(const JoinArgs& a, bool vm_on, bool vm_sel, hipStream_t s) {
  const dim3 g((unsigned)((a.rows.n + kJoinThreads - 1) / kJoinThreads)), b(kJoinThreads);
  if (vm_on && vm_sel) hipLaunchKernelGGL((k_joinprobe<true, true, true>), g, b, 0, s, a);
  else if (vm_on) hipLaunchKernelGGL((k_joinprobe<true, false, true>), g, b, 0, s, a);
  else if (vm_sel) hipLaunchKernelGGL((k_joinprobe<false, true, true>), g, b, 0, s, a);
  else hipLaunchKernelGGL((k_joinprobe<false, false, true>), g, b, 0, s, a);
}

void launch_join_tail(const JoinArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_jointail, dim3(64, 2), dim3(kJoinThreads), 0, s, a);
}

}  // namespace cep
