// Query chaining: k_derive builds one stage of a view (kernels.h DeriveArgs).
//
// A query that reads a derived stream M (`from S[p] select ... insert into
// M`) does not read M's compacted output: it reads the batch itself through a
// view in which the rows of S that pass p carry M's handle and M's computed
// attributes stand in dense columns indexed like the batch.  ts, arrival
// numbers and row positions are the batch's, so every kernel downstream runs
// unchanged and sees M's events interleaved with the other streams' exactly
// as synchronous delivery would.
//
// One streaming pass: each lane owns kDeriveRows consecutive rows, loads the
// handle bytes and every column it needs with 16-byte (8-byte types) or
// 8-byte vector loads, all issued before the first use, evaluates up to
// kDeriveProds producers' filters, and stores the handles (8 rows per store)
// and the materialised columns.  No LDS, no look-back, no atomics except the
// error flag.  k_derive_vec<NQ, false>: term-list filters and plain-copy items
// over NQ prefetched columns (no interpreter register file, no scratch);
// k_derive_vec<NQ, true>: the same loads, then the interpreter (vm.h) reading
// the prefetched registers, for computed select items and filters no term list
// expresses.  k_derive<kVm> goes row by row with per-use loads: a slice not
// aligned for the vector accesses (an odd first row or odd pointers), or a
// stage that reads more than kDerivePref distinct columns.  A ragged tail goes
// row by row too.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "vm.h"
#include "dev_common.h"

namespace cep {

namespace {

constexpr int E = kDeriveRows;
static_assert(kDerivePref == 6, "launch_derive instantiates k_derive_vec<1..6>");

typedef unsigned int g4u32 __attribute__((ext_vector_type(4)));
typedef unsigned int g2u32 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint2 gload2(const void* p) {
  const g2u32 x = *(const __attribute__((address_space(1))) g2u32*)p;
  return make_uint2(x.x, x.y);
}
__device__ __forceinline__ void gstore4(void* p, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
  g4u32 v;
  v.x = x;
  v.y = y;
  v.z = z;
  v.w = w;
  *(__attribute__((address_space(1))) g4u32*)p = v;
}
__device__ __forceinline__ void gstore2(void* p, uint32_t x, uint32_t y) {
  g2u32 v;
  v.x = x;
  v.y = y;
  *(__attribute__((address_space(1))) g2u32*)p = v;
}

struct DeriveEnv {
  const RowsArgs* r;
  int64_t row;
  __device__ uint64_t col(int c, int type) const { return load_col(r->cols.p[c], type, row); }
  __device__ uint64_t cap(int) const { return 0; }
  __device__ uint64_t outv(int, bool* n) const { *n = true; return 0; }
  __device__ uint64_t agg(int, bool* n) const { *n = true; return 0; }
  __device__ int64_t ts() const { return r->ts[row]; }
};

// The interpreter's view of row `e` of a lane's prefetched rows: LDCOL reads
// the registers (masked OR over static indices: no dynamically indexed array,
// no scratch), never memory.
template <int NQ>
struct RegEnv {
  const uint64_t (&pv)[NQ][kDeriveRows];
  const int32_t* col_slot;
  const int64_t* ts_row;   // the lane's first row's ts
  int e;
  __device__ uint64_t col(int c, int) const {
    const int slot = col_slot[c];
    uint64_t x = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int j = 0; j < kDeriveRows; ++j) x |= pv[q][j] & (0ull - (uint64_t)(slot == q && e == j));
    return x;
  }
  __device__ uint64_t cap(int) const { return 0; }
  __device__ uint64_t outv(int, bool* n) const { *n = true; return 0; }
  __device__ uint64_t agg(int, bool* n) const { *n = true; return 0; }
  __device__ int64_t ts() const { return ts_row[e]; }
};

// Term-list predicate of one row (the stages of eval_terms_regs, N = 1).
__device__ __forceinline__ bool terms_row(const TermList& tl, const RowsArgs& rows, int64_t row) {
  bool acc = !tl.any;
  for (int i = 0; i < tl.n; ++i) {
    const Term& t = tl.t[i];
    uint64_t v[1] = {load_col(rows.cols.p[t.col], t.coltype, row)};
    int ty = (t.coltype == T_BOOL || t.coltype == T_STRING) ? T_INT : t.coltype;
    uint32_t nullm = 0;
    if (t.aop) {
      convert_run<1>(v, ty, t.atype);
      arith_run<1>(v, t.aop, t.atype, t.aconst, &nullm);
      ty = t.atype;
    }
    convert_run<1>(v, ty, t.ctype);
    const bool bit = (compare_run<1>(v, t.cop, t.ctype, t.cconst) & ~nullm & 1u) != 0;
    acc = tl.any ? (acc || bit) : (acc && bit);
  }
  return acc;
}

// One row: its handle in the view; materialised columns stored.
template <bool kVm>
__device__ __forceinline__ uint32_t derive_row(const DeriveArgs& a, uint64_t* R, int64_t row) {
  const uint32_t h = a.rows.stream ? (uint32_t)a.rows.stream[row] : (uint32_t)a.rows.input;
  const DeriveEnv env{&a.rows, row};
  int hit = -1;
  bool twice = false;
  for (int p = 0; p < a.nprod; ++p) {
    const DeriveProd& d = a.prod[p];
    if ((uint32_t)d.src != h) continue;
    bool ok = true;
    if (d.filter_prog >= 0) {
      if (!kVm || d.terms.n >= 0) {
        ok = terms_row(d.terms, a.rows, row);
      } else {
        bool isnull = false;
        const uint64_t v = vm_eval(a.vm.code, a.vm.konst, d.filter_prog, R, threadIdx.x, blockDim.x, env, &isnull);
        ok = !isnull && (v & 1u);
      }
    }
    if (ok) {
      twice = twice || hit >= 0;
      if (hit < 0) hit = p;
    }
  }
  if (twice) set_err(a.err, ERR_DERIVE);
  for (int c = 0; c < a.ncols; ++c) {
    if (!a.col_out[c]) continue;
    uint64_t v = 0;
    if (hit >= 0) {
      const int src = a.prod[hit].item_src[c];
      if (src >= SRC_REC && src < SRC_TS) {
        v = load_col(a.rows.cols.p[src - SRC_REC], a.rows.cols.t[src - SRC_REC], row);
      } else if (kVm) {
        bool isnull = false;
        v = vm_eval(a.vm.code, a.vm.konst, a.prod[hit].item_prog[c], R, threadIdx.x, blockDim.x, env, &isnull);
        if (isnull) v = 0;
      }
    } else if (a.own_col[c] >= 0) {
      v = load_col(a.rows.cols.p[a.own_col[c]], a.out_type[c], row);
    }
    store_col(a.col_out[c], a.out_type[c], row, v);
  }
  return hit >= 0 ? (uint32_t)a.prod[hit].dst : h;
}

// E VM words -> a column's E elements at `row`, vector stores.
__device__ __forceinline__ void store_run(void* p, int type, int64_t row, const uint64_t (&v)[E]) {
  const int w = type_width(type);
  char* b = (char*)p + row * w;
  if (w == 8) {
#pragma unroll
    for (int i = 0; i < E / 2; ++i)
      gstore4(b + 16 * i, (uint32_t)v[2 * i], (uint32_t)(v[2 * i] >> 32), (uint32_t)v[2 * i + 1],
              (uint32_t)(v[2 * i + 1] >> 32));
  } else if (w == 4) {
#pragma unroll
    for (int i = 0; i < E / 4; ++i)
      gstore4(b + 16 * i, (uint32_t)v[4 * i], (uint32_t)v[4 * i + 1], (uint32_t)v[4 * i + 2], (uint32_t)v[4 * i + 3]);
  } else {
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo |= (uint32_t)(v[e] & 1u) << (8 * e);
      hi |= (uint32_t)(v[4 + e] & 1u) << (8 * e);
    }
    gstore2(b, lo, hi);
  }
}

}  // namespace

// Row by row: the interpreter instance, and slices not aligned for the vector
// accesses.
template <bool kVm>
__device__ __forceinline__ void derive_rows(const DeriveArgs& a, uint64_t* R, int64_t row, int nvalid) {
  uint32_t lo = 0, hi = 0;
  for (int e = 0; e < nvalid; ++e) {
    const uint32_t h = derive_row<kVm>(a, R, row + e);
    if (e < 4) lo |= h << (8 * e);
    else hi |= h << (8 * (e - 4));
  }
  if (a.vec && nvalid == E) {
    gstore2(a.stream_out + row, lo, hi);
  } else {
    for (int e = 0; e < nvalid; ++e)
      a.stream_out[row + e] = (uint8_t)((e < 4 ? lo >> (8 * e) : hi >> (8 * (e - 4))) & 0xffu);
  }
}

template <bool kVm>
__global__ __launch_bounds__(kDeriveThreads) void k_derive(DeriveArgs a) {
  __shared__ uint64_t R[kVm ? kMaxRegs * kDeriveThreads : 1];
  const int64_t i0 = ((int64_t)blockIdx.x * kDeriveThreads + threadIdx.x) * E;   // lane's first row of the slice
  if (i0 >= a.rows.n) return;
  const int64_t left = a.rows.n - i0;
  derive_rows<kVm>(a, R, a.rows.row0 + i0, left < E ? (int)left : E);
}

// The term-list instance over NQ loaded columns (a.vec: everything aligned).
// The loads have one shape whatever the column types: four 16-byte loads per
// column, the surplus ones of a narrower type repeating its last address (the
// same cache line), and no branch between them.  A branch on the type, even a
// uniform one that holds loads only, ends in a join that merges registers of
// loads in flight with their alternative: an s_waitcnt before the next
// column's loads, i.e. one dependent HBM round trip per column.
// A 1-byte column loads the aligned 16-byte granule that holds the lane's 8
// bytes (it cannot cross a page) and picks its half afterwards.
template <int NQ, bool kVm>
__global__ __launch_bounds__(kDeriveThreads) void k_derive_vec(DeriveArgs a) {
  __shared__ uint64_t R[kVm ? kMaxRegs * kDeriveThreads : 1];
  const int64_t i0 = ((int64_t)blockIdx.x * kDeriveThreads + threadIdx.x) * E;
  if (i0 >= a.rows.n) return;
  const int64_t row = a.rows.row0 + i0;
  const int64_t left = a.rows.n - i0;
  if (left < E) {   // the ragged tail
    derive_rows<kVm>(a, R, row, (int)left);
    return;
  }
  // ---- every load of the lane's E rows, before any use ------------------------
  // (no handle column: the same 8 bytes from the lane's ts rows, in bounds,
  // and the handle selected afterwards)
  const void* sp = a.rows.stream ? (const void*)(a.rows.stream + row) : (const void*)(a.rows.ts + row);
  const uint2 hraw = gload2(sp);
  uint4 raw[NQ][E / 2];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int w = type_width(a.rows.cols.t[a.pcol[q]]);
    const char* b = (const char*)a.rows.cols.p[a.pcol[q]] + row * w;
    const char* b0 = w == 1 ? b - ((uintptr_t)b & 15u) : b;
    const int last = w == 8 ? 48 : (w == 4 ? 16 : 0);   // surplus loads repeat the last address
#pragma unroll
    for (int i = 0; i < E / 2; ++i) raw[q][i] = gload4(b0 + (16 * i < last ? 16 * i : last));
  }
  // ---- decode --------------------------------------------------------------------
  uint32_t hb[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t x = e < 4 ? hraw.x >> (8 * e) : hraw.y >> (8 * (e - 4));
    hb[e] = a.rows.stream ? (x & 0xffu) : (uint32_t)a.rows.input;
  }
  uint64_t pv[NQ][E];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int ty = a.rows.cols.t[a.pcol[q]];
    if (type_width(ty) == 1) {   // the lane's 8 bytes: the low or the high half of the granule
      const bool up = (((uintptr_t)a.rows.cols.p[a.pcol[q]] + (uintptr_t)row) & 8u) != 0;
      raw[q][0] = make_uint4(up ? raw[q][0].z : raw[q][0].x, up ? raw[q][0].w : raw[q][0].y, 0, 0);
    }
    decode<E>(raw[q], ty, pv[q]);
  }

  if constexpr (!kVm) {
    // ---- producers' filters --------------------------------------------------------
    uint32_t pass[kDeriveProds];
    uint32_t any = 0, twice = 0;
  #pragma unroll
    for (int p = 0; p < kDeriveProds; ++p) {
      pass[p] = 0;
      if (p < a.nprod) {
        const DeriveProd& d = a.prod[p];
        uint32_t on = 0;
  #pragma unroll
        for (int e = 0; e < E; ++e) on |= (hb[e] == (uint32_t)d.src ? 1u : 0u) << e;
        if (on && d.filter_prog >= 0) on &= eval_terms_regs<E, NQ>(d.terms, d.fslot, a.rows.cols, pv);
        twice |= any & on;
        pass[p] = on & ~any;   // the first producer a row passes names it
        any |= on;
      }
    }
    if (twice) set_err(a.err, ERR_DERIVE);
  #pragma unroll
    for (int p = 0; p < kDeriveProds; ++p) {
      if (p < a.nprod) {
        const uint32_t dst = (uint32_t)a.prod[p].dst;
  #pragma unroll
        for (int e = 0; e < E; ++e) hb[e] = ((pass[p] >> e) & 1u) ? dst : hb[e];
      }
    }
    gstore2(a.stream_out + row, hb[0] | hb[1] << 8 | hb[2] << 16 | hb[3] << 24,
            hb[4] | hb[5] << 8 | hb[6] << 16 | hb[7] << 24);

    // ---- materialised columns: the producer's item on its rows, the slice's own
    // column on the others
    for (int c = 0; c < a.ncols; ++c) {
      if (!a.col_out[c]) continue;
      uint64_t v[E];
      take_slot<E, NQ>(pv, a.own_slot[c], v);
  #pragma unroll
      for (int p = 0; p < kDeriveProds; ++p) {
        if (p < a.nprod && pass[p]) {
          uint64_t s[E];
          take_slot<E, NQ>(pv, a.prod[p].item_slot[c], s);
  #pragma unroll
          for (int e = 0; e < E; ++e) v[e] = ((pass[p] >> e) & 1u) ? s[e] : v[e];
        }
      }
      store_run(a.col_out[c], a.out_type[c], row, v);
    }
  } else {
    // ---- the interpreter over the prefetched rows (computed select items, filters
    // no term list expresses); runtime loops keep it to two inlined interpreters
    RegEnv<NQ> env{pv, a.col_slot, a.rows.ts + row, 0};
    uint32_t passb = 0, any = 0, twice = 0;   // passb: 8 row bits per producer
    for (int p = 0; p < a.nprod; ++p) {
      const DeriveProd& d = a.prod[p];
      uint32_t on = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) on |= (hb[e] == (uint32_t)d.src ? 1u : 0u) << e;
      if (on && d.filter_prog >= 0) {
        if (d.terms.n >= 0) {
          on &= eval_terms_regs<E, NQ>(d.terms, d.fslot, a.rows.cols, pv);
        } else {
          uint32_t ok = 0;
          for (int e = 0; e < E; ++e) {
            if (!((on >> e) & 1u)) continue;
            env.e = e;
            bool isnull = false;
            const uint64_t v = vm_eval(a.vm.code, a.vm.konst, d.filter_prog, R, threadIdx.x, blockDim.x, env, &isnull);
            if (!isnull && (v & 1u)) ok |= 1u << e;
          }
          on = ok;
        }
      }
      twice |= any & on;
      passb |= (on & ~any) << (8 * p);   // the first producer a row passes names it
      any |= on;
    }
    if (twice) set_err(a.err, ERR_DERIVE);
    for (int p = 0; p < a.nprod; ++p) {
      const uint32_t dst = (uint32_t)a.prod[p].dst, m = (passb >> (8 * p)) & 0xffu;
#pragma unroll
      for (int e = 0; e < E; ++e) hb[e] = ((m >> e) & 1u) ? dst : hb[e];
    }
    gstore2(a.stream_out + row, hb[0] | hb[1] << 8 | hb[2] << 16 | hb[3] << 24,
            hb[4] | hb[5] << 8 | hb[6] << 16 | hb[7] << 24);
    for (int c = 0; c < a.ncols; ++c) {
      if (!a.col_out[c]) continue;
      uint64_t v[E];
      take_slot<E, NQ>(pv, a.own_slot[c], v);
      for (int p = 0; p < a.nprod; ++p) {
        const uint32_t m = (passb >> (8 * p)) & 0xffu;
        if (!m) continue;
        const int src = a.prod[p].item_src[c];
        if (src >= SRC_REC && src < SRC_TS) {
          uint64_t s[E];
          take_slot<E, NQ>(pv, a.prod[p].item_slot[c], s);
#pragma unroll
          for (int e = 0; e < E; ++e) v[e] = ((m >> e) & 1u) ? s[e] : v[e];
        } else {
          for (int e = 0; e < E; ++e) {
            if (!((m >> e) & 1u)) continue;
            env.e = e;
            bool isnull = false;
            uint64_t x = vm_eval(a.vm.code, a.vm.konst, a.prod[p].item_prog[c], R, threadIdx.x, blockDim.x, env, &isnull);
            if (isnull) x = 0;
#pragma unroll
            for (int j = 0; j < E; ++j) v[j] = j == e ? x : v[j];
          }
        }
      }
      store_run(a.col_out[c], a.out_type[c], row, v);
    }
  }
}

template <bool kVm>
static void launch_vec(const DeriveArgs& a, dim3 g, dim3 b, hipStream_t s) {
  switch (a.npref) {   // no column at all: one (unused) slot
    case 0:
    case 1: hipLaunchKernelGGL((k_derive_vec<1, kVm>), g, b, 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_derive_vec<2, kVm>), g, b, 0, s, a); break;
    case 3: hipLaunchKernelGGL((k_derive_vec<3, kVm>), g, b, 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_derive_vec<4, kVm>), g, b, 0, s, a); break;
    case 5: hipLaunchKernelGGL((k_derive_vec<5, kVm>), g, b, 0, s, a); break;
    default: hipLaunchKernelGGL((k_derive_vec<6, kVm>), g, b, 0, s, a); break;
  }
}

void launch_derive(const DeriveArgs& a, bool vm, bool rowwise, hipStream_t s) {
  constexpr int64_t kTile = (int64_t)kDeriveThreads * kDeriveRows;
  const int64_t nb = (a.rows.n + kTile - 1) / kTile;
  if (nb <= 0) return;
  const dim3 g((unsigned)nb), b(kDeriveThreads);
  if (rowwise || !a.vec) {
    if (vm) hipLaunchKernelGGL(k_derive<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_derive<false>, g, b, 0, s, a);
  } else if (vm) {
    launch_vec<true>(a, g, b, s);
  } else {
    launch_vec<false>(a, g, b, s);
  }
}

}  // namespace cep
