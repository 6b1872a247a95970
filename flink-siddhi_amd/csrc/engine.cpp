// libcep runtime: the C ABI of include/cep.h over the gfx950 kernels.
//
// One cep_app = one Siddhi app runtime (AbstractSiddhiOperator.java:114-176
// QueryRuntimeHandler).  Device layout (HBM, sized for 288 GB/GPU):
//   * plan: VM instruction array + constant pool (tiny, read-only),
//   * per output stream: typed columns + ts + seq + a device row cursor,
//     capacity = the host-known bound on rows since the last flush (no
//     device->host sync is ever needed to size a launch),
//   * per keyed pattern: dense per-key state [key][S][2+ncap] words plus a
//     pending count and `started` byte per key, and a chunk-sized record
//     arena [tiles][2048 rows][rec_words] + tile offset table.
// All work for a batch is enqueued on the app's HIP stream; cep_flush
// synchronises, checks the device error word and delivers rows to callbacks.
#include <cstdio>
#include <cstring>
#include <numeric>

#include "rt.h"
#include "snapshot.h"

using namespace cep;

namespace {

void set_err(char* err, size_t errlen, const std::string& m) {
  if (err && errlen) {
    std::snprintf(err, errlen, "%s", m.c_str());
  }
}

bool is_pinned(const void* p) {
  hipPointerAttribute_t at;
  if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();   // pageable memory: clear the sticky lookup error
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

}  // namespace

namespace cep {

void harvest_timers(cep_app* a) {
  for (auto& t : a->timed) {
    float ms = 0;
    hipEventElapsedTime(&ms, t.a, t.b);
    a->kernel_ms[t.kind] += ms;
    a->kernel_timed[t.kind]++;
    a->event_pool.push_back(std::move(t.a));
    a->event_pool.push_back(std::move(t.b));
  }
  a->timed.clear();
}

hipStream_t ChunkPipe::open(cep_app* a) {
  hipEventRecord(a->in_ready, a->stream);
  hipStreamWaitEvent(a->side, a->in_ready, 0);
  static const bool no_overlap = std::getenv("CEP_NO_OVERLAP") != nullptr;
  events = true;
  return no_overlap ? a->stream.h : a->side.h;
}

hipStream_t ChunkPipe::open_cf(cep_app* a) {
  // Both passes on the main stream by default: k_cfpart and k_cfwalk cannot
  // share a CU (each fills its register file), so the side stream only
  // time-slices them (measured: no throughput gain, inflated kernel times).
  // CEP_OVERLAP=1 puts the partition on the side stream.  Serial mode issues
  // no cross-stream events: every event between two kernels of one stream
  // costs a gap (rocprofv3 trace: ~15 us between k_cfpart and k_cfwalk).
  static const bool overlap = std::getenv("CEP_OVERLAP") != nullptr;
  events = overlap;
  if (!overlap) return a->stream;
  hipEventRecord(a->in_ready, a->stream);
  hipStreamWaitEvent(a->side, a->in_ready, 0);
  return a->side;
}

int ensure_out_cap(cep_app* a, OutStream& o, int64_t need) {
  if (need <= o.cap) return CEP_OK;
  int64_t nc = std::max<int64_t>(need, std::max<int64_t>(o.cap * 2, 1 << 16));
  for (size_t c = 0; c < o.cols.size(); ++c)
    if (!dev_ensure(&o.cols[c], (size_t)nc * type_width(o.types[c]), a->stream, true))
      return fail(a, CEP_E_DEVICE, "out of device memory (output columns)");
  if (!dev_ensure(&o.ts, (size_t)nc * 8, a->stream, true) ||
      !dev_ensure(&o.seq, (size_t)nc * 8, a->stream, true))
    return fail(a, CEP_E_DEVICE, "out of device memory (output ts/seq)");
  o.cap = nc;
  // diagnostics: an output whose arrival numbers nobody reads (write_seq 0)
  // keeps its seq column at a known pattern; cep_flush fails if any kernel
  // stored into it (tests/test_gpu_seq_poison.py)
  if (a->seq_poison && !o.write_seq) hipMemsetAsync(o.seq.p, 0xa5, (size_t)nc * 8, a->stream);
  return CEP_OK;
}

OutArgs out_args(OutStream& o, const Query& q) {
  OutArgs oa{};
  oa.ncols = (int32_t)o.cols.size();
  for (int c = 0; c < oa.ncols; ++c) {
    oa.col[c] = o.cols[c].p;
    oa.type[c] = o.types[c];
    oa.prog[c] = q.select[c].prog.off;
    oa.src[c] = q.select[c].src;
  }
  oa.ts = (int64_t*)o.ts.p;
  oa.seq = (int64_t*)o.seq.p;
  oa.count = o.count;
  oa.cap = o.cap;
  oa.write_seq = o.write_seq ? 1 : 0;
  return oa;
}


int create_runtime(cep_app* a) {
  const CompiledApp& app = a->app;
  if (hipSetDevice(a->opt.device) != hipSuccess)
    return fail(a, CEP_E_DEVICE, "no HIP device " + std::to_string(a->opt.device));
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, a->opt.device) != hipSuccess)
    return fail(a, CEP_E_DEVICE, "hipGetDeviceProperties failed");
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return fail(a, CEP_E_DEVICE, std::string("libcep is built for gfx950, device is ") +
                                     prop.gcnArchName);
  if (!a->stream.create() || !a->side.create() || !a->in_ready.create() || !a->ext_ready.create() ||
      !a->out_ready.create() || !a->copy.create() || !a->rstream.create() || !a->r_ready.create() ||
      !a->r_host.create())
    return fail(a, CEP_E_DEVICE, "hipStreamCreate failed");
  size_t cb = std::max<size_t>(app.code.size(), 1) * sizeof(Ins);
  size_t kb = std::max<size_t>(app.konst.size(), 1) * 8;
  if (!dev_ensure(&a->code, cb, a->stream, false) || !dev_ensure(&a->konst, kb, a->stream, false) ||
      !dev_ensure(&a->err, 64, a->stream, false) || !dev_ensure(&a->rerr, 64, a->stream, false) ||
      !dev_ensure(&a->ticket, 64, a->stream, false))
    return fail(a, CEP_E_DEVICE, "out of device memory (plan)");
  if (!app.code.empty())
    hipMemcpy(a->code.p, app.code.data(), app.code.size() * sizeof(Ins), hipMemcpyHostToDevice);
  if (!app.konst.empty())
    hipMemcpy(a->konst.p, app.konst.data(), app.konst.size() * 8, hipMemcpyHostToDevice);
  hipMemset(a->err.p, 0, 64);
  hipMemset(a->rerr.p, 0, 64);
  // every output's row cursor in one device array: the flush reads them with
  // one copy and resets them with one memset (64 outputs at config 5)
  if (!dev_ensure(&a->out_counts, std::max<size_t>(app.outputs.size(), 1) * 8, a->stream, false))
    return fail(a, CEP_E_DEVICE, "out of device memory");
  hipMemset(a->out_counts.p, 0, std::max<size_t>(app.outputs.size(), 1) * 8);
  for (auto& sd : app.outputs) {
    OutStream o;
    o.id = sd.id;
    for (auto& at : sd.attrs) o.types.push_back(at.type);
    o.cols.resize(sd.attrs.size());
    o.count = (unsigned long long*)a->out_counts.p + a->outs.size();
    // arrival numbers: read by the ordered flush and by consumers that asked
    // for them (cep_output_device returns seq = NULL otherwise)
    o.write_seq = !(a->opt.omit_seq && !a->opt.ordered_output);
    a->outs.push_back(std::move(o));
    if (const char* e = std::getenv("CEP_SEQ_POISON")) a->seq_poison = std::atoi(e) != 0;
  }
  if (const char* e = std::getenv("CEP_CF_PART")) a->cf_one_wg = std::atoi(e) == 1;
  {
    const int rc = build_mq_groups(a);
    if (rc) return rc;
  }
  for (size_t qi = 0; qi < app.queries.size(); ++qi) {
    const Query& q = app.queries[qi];
    if (q.kind != Q_PATTERN && q.kind != Q_AGG) continue;
    if (a->in_mq[qi]) continue;   // served by a multi-query group
    const bool agg = q.kind == Q_AGG;
    const bool batch = agg && win_is_batch(q.win_kind);
    const bool win = agg && q.win_kind != WIN_NONE && !batch;
    // group-by state: one slot of (accumulator, count) pairs per group (a
    // window query: one slot of accumulators + the ring, kernels.h WinArgs)
    const int S = agg ? 1 : a->opt.pending_slots;
    PatternRT rt;
    rt.q = (int)qi;
    PatternArgs& p = rt.pa;
    if (win) {
      // Case (c), `group by k` + #window.time outside a partition: Siddhi's
      // window spans every group, the engine keeps one per key.  With
      // non-decreasing ts the global window's front pops are monotone in ts:
      // when row e arrives, the rows popped so far are exactly those with
      // ts + T <= e.ts (every row before a blocked front has a ts >= the
      // front's, so none of them is due either).  A group's accumulator may
      // take its removes lazily, at the group's next own row e: nothing reads
      // it in between, and the rows of the group removed before add(e) are
      // then exactly the group's rows with ts + T <= e.ts, oldest first — what
      // the per-key window pops at e.  With ts in any order a front row of
      // another group can block (or release) this group's rows, so the two
      // differ.
      if (q.win_global && a->opt.ts_order != 1)
        return fail(a, CEP_E_UNSUPPORTED,
                    "group by with #window.time outside a partition is not supported with ts_order = 0: Siddhi's "
                    "window spans every group, and one window per group equals it only for non-decreasing "
                    "timestamps (set ts_order = 1, or partition the query)");
      if (q.win_kind == WIN_LENGTH && q.win_param > kWinMaxRing)
        return fail(a, CEP_E_CAPACITY, "#window.length(" + std::to_string(q.win_param) + ") exceeds the capacity of " +
                                           std::to_string(kWinMaxRing) + " window rows per key");
      WinArgs& w = rt.win;
      w.kind = q.win_kind;
      w.param = q.win_param;
      w.ring = q.win_kind == WIN_LENGTH ? (int)q.win_param : a->opt.pending_slots;
      w.nval = 0;
      for (size_t i = 0; i < q.aggs.size(); ++i) {
        w.agg_val[i] = -1;
        if (q.aggs[i].word < 0) continue;
        for (int v = 0; v < w.nval; ++v)
          if (w.val_word[v] == q.aggs[i].word) w.agg_val[i] = v;
        if (w.agg_val[i] < 0) {
          w.val_word[w.nval] = q.aggs[i].word;
          w.agg_val[i] = w.nval++;
        }
      }
      w.entry_words = w.nval + (q.win_kind == WIN_TIME ? 1 : 0);
      rt.win_vm = q.having.valid();
      for (auto& it : q.select) rt.win_vm |= it.src == SRC_VM;
    }
    p.a_stream = q.a_stream;
    p.b_stream = q.b_stream;
    p.f_prog = q.f.off;
    p.g_raw_prog = q.g_raw.off;
    p.g_walk_prog = q.g_walk.off;
    p.f_terms = q.f_terms;
    p.g_terms = q.g_terms;
    p.every = q.every ? 1 : 0;
    p.within = q.within;
    p.key_col_a = q.key_col_a;
    p.key_col_b = q.key_col_b;
    p.nrec_a = (int)q.rec_cols_a.size();
    p.nrec_b = (int)q.rec_cols_b.size();
    for (int i = 0; i < p.nrec_a; ++i) p.rec_a[i] = q.rec_cols_a[i];
    for (int i = 0; i < p.nrec_b; ++i) p.rec_b[i] = q.rec_cols_b[i];
    p.ncap = (int)q.cap_from_rec.size();
    for (int i = 0; i < p.ncap; ++i) p.cap_from_rec[i] = q.cap_from_rec[i];
    p.rec_words = 2 + std::max(p.nrec_a, p.nrec_b);
    p.slot_words = agg ? 2 * (int)q.aggs.size() : 2 + p.ncap;
    if (win) p.slot_words = (int)q.aggs.size() + rt.win.ring * rt.win.entry_words;
    if (batch) {
      // one slot per key: the open batch, then the candidate (kernels.h BatchArgs)
      BatchArgs& b = rt.bat;
      const int nagg = (int)q.aggs.size();
      const bool timed = q.win_kind == WIN_TIME_BATCH;
      const bool hav = q.having.valid();
      b.kind = q.win_kind;
      b.param = q.win_param;
      b.time_word = q.win_word;
      int w = nagg + 1;
      b.time_w = timed ? w : -1;
      if (timed) w += 2;
      b.cand_acc_w = hav ? w : -1;
      if (hav) w += nagg + 1;
      // the emitted row is the trigger itself only for lengthBatch without having
      b.cand_w = (timed || hav) ? w : -1;
      if (b.cand_w >= 0) w += 1 + p.nrec_a;
      p.slot_words = w;
      rt.win_vm = hav;
      for (auto& it : q.select) rt.win_vm |= it.src == SRC_VM;
    }
    p.key_words = 1 + S * p.slot_words;
    p.pending_slots = S;
    // case (c) relies on event-time order: the partition pass checks it
    if (win && q.win_global) p.within = q.win_param;
    // closed form keeps each record's carried words in LDS (kWalkCapLds)
    p.closed_form = (!agg && q.every && !q.g_in_walk && p.rec_words <= 2 + kWalkCapLds) ? 1 : 0;
    p.agg_mode = agg ? 1 : 0;
    p.nagg = agg ? (int)q.aggs.size() : 0;
    for (int i = 0; i < p.nagg; ++i) {
      p.agg_fn[i] = q.aggs[i].fn;
      p.agg_arg_type[i] = q.aggs[i].arg_type;
      p.agg_out_type[i] = q.aggs[i].out_type;
      p.agg_word[i] = q.aggs[i].word;
    }
    p.having_prog = agg ? q.having.off : -1;
    if (q.nfa) {
      if (app.inputs.size() > 8)
        return fail(a, CEP_E_UNSUPPORTED, "patterns / sequences over apps with more than 8 input streams");
      p.nfa_mode = 1;
      p.nfa_seq = q.sequence ? 1 : 0;
      p.nstates = (int)q.nstates.size();
      p.closed_form = 0;
      p.ncap = (int)q.ncaps.size();
      p.slot_words = 2 + p.ncap;
      p.key_words = 1 + S * p.slot_words;
      p.stream_mask = 0;
      p.st_logic = 0;
      for (int j = 0; j < p.nstates; ++j) {
        const auto& st = q.nstates[j];
        p.st_stream[j] = st.stream;
        p.st_min[j] = st.min_count;
        p.st_max[j] = st.max_count;
        p.st_raw[j] = st.raw.off;
        p.st_walk[j] = st.walk.off;
        p.st_logic |= st.logic << (2 * j);
        p.stream_mask |= 1 << st.stream;
        // a pattern with a count state: the walk's third instance
        if (!q.sequence && (st.min_count != 1 || st.max_count != 1)) p.nfa_mode = kNfaModeCount;
      }
      for (int j = 0; j < p.nstates; ++j) {
        bool opt = true;
        for (int k = j + 1; k < p.nstates; ++k) opt = opt && q.nstates[k].min_count == 0;
        p.st_tail_opt[j] = opt ? 1 : 0;
      }
      for (int i = 0; i < 8; ++i) p.key_col_s[i] = i < (int)q.key_col_s.size() ? q.key_col_s[i] : -1;
      for (int i = 0; i < p.ncap; ++i) {
        p.cap_state[i] = q.ncaps[i].state;
        p.cap_index[i] = q.ncaps[i].index;
        p.cap_word[i] = q.ncaps[i].word;
        // Siddhi reads an unmatched (optional) state's attribute as null: for
        // a STRING the engine writes dictionary id -1, which no string has
        const int st = q.nstates[q.ncaps[i].state].stream;
        const int col = q.ncaps[i].word < (int)q.rec_cols_a.size() ? q.rec_cols_a[q.ncaps[i].word] : -1;
        const bool str = st >= 0 && st < (int)app.inputs.size() && col >= 0 &&
                         col < (int)app.inputs[st].attrs.size() && app.inputs[st].attrs[col].type == T_STRING;
        p.cap_null[i] = str ? ~0ull : 0ull;
      }
    }
    // NFA patterns stage advanced partials in a second bank of S slots (so do
    // the order-tolerant runs of a 2-state pattern with `within`: nfa_pair)
    const int bank = (q.nfa || (q.within >= 0 && !agg)) ? 2 : 1;
    const bool keyed = q.key_col_a >= 0;
    int64_t kcap = keyed ? a->opt.key_capacity : 1;
    p.key_capacity = kcap;
    p.key_stride = keyed ? std::max(1, a->opt.key_stride) : 1;
    p.key_offset = keyed ? a->opt.key_offset : 0;
    if (!keyed && (a->opt.key_stride > 1))
      return fail(a, CEP_E_UNSUPPORTED, "an unpartitioned query cannot be sharded");
    int lg = std::max(0, std::min(12, a->opt.buckets_log2));
    while ((kcap >> lg) > kWalkMaxKeys && lg < 12) ++lg;
    if ((kcap + (1 << lg) - 1) >> lg > kWalkMaxKeys)
      return fail(a, CEP_E_CAPACITY, "key_capacity exceeds 1024 * 4096 keys");
    if (!keyed) lg = 0;
    p.buckets_log2 = lg;
    const int64_t kc = kcap;
    const int64_t kpb = (kc + (1 << lg) - 1) >> lg;
    rt.kstride = kpb << lg;
    if (win) {
      // the rings are the one state here that grows with a plan constant
      const double bytes = (double)rt.kstride * p.slot_words * 8;
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > (double)free_b)
        return fail(a, CEP_E_CAPACITY, "window state of " + std::to_string((unsigned long long)bytes) + " bytes (" +
                                           std::to_string(rt.kstride) + " keys x " + std::to_string(p.slot_words) +
                                           " words) exceeds the GPU's memory capacity: lower key_capacity" +
                                           (q.win_kind == WIN_TIME ? " or pending_slots" : ""));
    }
    if (!dev_ensure(&rt.khdr, (size_t)rt.kstride * 4, a->stream, false) ||
        !dev_ensure(&rt.kslot, (size_t)rt.kstride * bank * S * p.slot_words * 8, a->stream, false))
      return fail(a, CEP_E_DEVICE, "out of device memory (pattern state)");
    hipMemset(rt.khdr.p, 0, (size_t)rt.kstride * 4);
    // snapshots store a live key's whole slots: a window's free ring entries,
    // and slot word 1, which the closed form never writes, read as zero
    // instead of whatever the memory held before
    hipMemset(rt.kslot.p, 0, (size_t)rt.kstride * bank * S * p.slot_words * 8);
    // the walk build decides the chunk cap (its LDS segment tables)
    bool walk_vm = q.g_in_walk || agg || q.nfa;
    for (auto& it : q.select) walk_vm |= it.src == SRC_VM;
    int64_t chunk = a->opt.chunk_events;
    chunk = std::max<int64_t>(chunk, kPartThreads * kPartItems);
    chunk = std::min<int64_t>(chunk, (int64_t)(walk_vm ? kWalkMaxTiles : kWalkMaxTiles / 4) *
                                         kPartThreads * kPartItems);
    chunk = (chunk / (kPartThreads * kPartItems)) * (kPartThreads * kPartItems);
    rt.pipe.chunk = chunk;
    // the order-tolerant form of a `within` pattern (ts_order 0, released
    // late rows) runs on the VM walk, whose segment tables hold 4x the tiles:
    // its chunks may be that long, so per-key state is loaded and committed
    // a quarter as often
    int64_t chunk_tol = chunk;
    if (!walk_vm && q.within >= 0) {
      chunk_tol = std::max<int64_t>(a->opt.chunk_events, kPartThreads * kPartItems);
      chunk_tol = std::min<int64_t>(chunk_tol, (int64_t)kWalkMaxTiles * kPartThreads * kPartItems);
      chunk_tol = (chunk_tol / (kPartThreads * kPartItems)) * (kPartThreads * kPartItems);
    }
    rt.chunk_tol = chunk_tol;
    const int64_t ntiles = std::max(chunk, chunk_tol) / (kPartThreads * kPartItems);
    if (!rt.pipe.alloc((size_t)std::max(chunk, chunk_tol) * p.rec_words * 8 + 16,
                       (size_t)ntiles * ((1 << lg) + 1) * 2, a->stream))
      return fail(a, CEP_E_DEVICE, "out of device memory (record arena)");
    rt.extra_bound = (int64_t)S * kc;
    rt.part_vm = (q.f.off >= 0 && q.f_terms.n < 0) || (q.g_raw.off >= 0 && q.g_terms.n < 0) || q.nfa;
    // fast partition path: all columns the pass reads fit kPref registers
    if (!rt.part_vm && q.key_col_a == q.key_col_b && p.nrec_a <= kPfRec && p.nrec_b <= kPfRec) {
      PrefPlan& pf = rt.pref;
      std::vector<int> cols;
      auto slot = [&](int c) {
        for (size_t i = 0; i < cols.size(); ++i)
          if (cols[i] == c) return (int)i;
        cols.push_back(c);
        return (int)cols.size() - 1;
      };
      pf.key_slot = q.key_col_a >= 0 ? slot(q.key_col_a) : -1;   // slot 0: k_cfpart reads it there
      if (q.f.off >= 0)
        for (int i = 0; i < q.f_terms.n; ++i) pf.f_slot[i] = slot(q.f_terms.t[i].col);
      if (q.g_raw.off >= 0)
        for (int i = 0; i < q.g_terms.n; ++i) pf.g_slot[i] = slot(q.g_terms.t[i].col);
      for (int i = 0; i < p.nrec_a; ++i) pf.reca_slot[i] = slot(p.rec_a[i]);
      for (int i = 0; i < p.nrec_b; ++i) pf.recb_slot[i] = slot(p.rec_b[i]);
      if (!cols.empty() && (int)cols.size() <= kPref) {
        pf.n = (int)cols.size();
        for (int i = 0; i < kPref; ++i) pf.col[i] = i < pf.n ? cols[i] : cols[0];
      } else {
        pf.n = -1;
      }
    }
    // group-by and N-state / sequence walks live in the VM build of k_walk
    rt.walk_vm = walk_vm;
    // N-state patterns / sequences: partial lists longer than pending_slots
    // continue in the pending pool (nfa_key), as on the closed-form path; so
    // do the order-tolerant runs of any 2-state pattern with `within`
    // (nfa_pair: ts_order 0 or released late rows), which never prune at A
    // arrivals
    if (q.nfa || (q.within >= 0 && !agg)) {
      const int plg = a->opt.pending_pool_log2 > 0 ? std::min(a->opt.pending_pool_log2, 30) : 20;
      rt.pool_cap = (int64_t)1 << plg;
      const bool ok = dev_ensure(&rt.kext, (size_t)rt.kstride * 8, a->stream, false) &&
                      dev_ensure(&rt.pool[0], (size_t)rt.pool_cap * p.slot_words * 8, a->stream, false) &&
                      dev_ensure(&rt.pool[1], (size_t)rt.pool_cap * p.slot_words * 8, a->stream, false) &&
                      dev_ensure(&rt.pool_cur, 64, a->stream, false);
      if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (pending pool)");
      hipMemset(rt.kext.p, 0, (size_t)rt.kstride * 8);
      for (auto& pl : rt.pool) hipMemset(pl.p, 0, (size_t)rt.pool_cap * p.slot_words * 8);   // (as kslot)
      rt.extra_bound += rt.pool_cap;   // pool partials may complete too
    }
    // closed-form fast path: `every A -> B` with f / g as term lists on the
    // events' own columns, plain-copy select items, <= 2 captures, <= 512
    // keys per bucket (CEP_NO_CF=1 forces the general path)
    {
      bool ok = p.closed_form && !q.nfa && !agg && !rt.part_vm && !rt.walk_vm && rt.pref.n >= 0 &&
                p.ncap <= kCfMaxCaps && p.nrec_a <= kPfRec && p.nrec_b <= kPfRec &&
                kpb <= kCfMaxKeys && (1 << lg) <= kCfMaxBuckets && !std::getenv("CEP_NO_CF") && S >= 2 &&
                (double)rt.kstride * S * p.slot_words * 8 < 4294967296.0;   // 32-bit slot offsets
      ok = ok && (int)q.select.size() <= kCfMaxOut;
      for (auto& it : q.select)
        ok = ok && (it.src == SRC_KEY || (it.src >= SRC_CAP && it.src < SRC_CAP + kCfMaxCaps) ||
                    (it.src >= SRC_REC && it.src < SRC_REC + kPfRec));
      if (ok) {
        int64_t cc = std::max<int64_t>(a->opt.chunk_events, kCfTile);
        cc = std::min<int64_t>(cc, (int64_t)kCfMaxTiles * kCfTile);
        cc = (cc / kCfTile) * kCfTile;
        const int64_t nt = cc / kCfTile;
        const int rw = 1 + std::max(p.nrec_a, p.nrec_b);
        // offset rows: P key buckets, then kCfHotMax hot buckets or (the
        // adaptive ts_order-0 build) P expiry-entry twins
        const int64_t trows = std::max<int64_t>((1 << lg) + kCfHotMax, 2 << lg) + 1;
        for (int b = 0; b < 2 && ok; ++b)
          ok = dev_ensure(&rt.cf_recs[b], (size_t)cc * rw * 8 + 16, a->stream, false) &&
               dev_ensure(&rt.cf_toff[b], (size_t)nt * trows * 2 + 16, a->stream, false);
        if (ok && q.within >= 0) {
          ok = dev_ensure(&rt.atol_gate, 64, a->stream, false) && dev_ensure(&rt.hwm, 128 * 8, a->stream, false);
          if (ok) {
            hipMemset(rt.atol_gate.p, 0, 64);
            hipMemset(rt.hwm.p, 0, 128 * 8);   // 0 = INT64_MIN (order-preserving u64)
          }
        }
        if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (record arena)");
        const int plg = a->opt.pending_pool_log2 > 0 ? std::min(a->opt.pending_pool_log2, 30) : 20;
        const bool pool_counted = rt.pool_cap > 0;   // (allocated above for a `within` pattern)
        rt.pool_cap = (int64_t)1 << plg;
        ok = dev_ensure(&rt.kext, (size_t)rt.kstride * 8, a->stream, false) &&
             dev_ensure(&rt.pool[0], (size_t)rt.pool_cap * p.slot_words * 8, a->stream, false) &&
             dev_ensure(&rt.pool[1], (size_t)rt.pool_cap * p.slot_words * 8, a->stream, false) &&
             dev_ensure(&rt.pool_cur, 64, a->stream, false);
        if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (pending pool)");
        hipMemset(rt.kext.p, 0, (size_t)rt.kstride * 8);
        for (auto& pl : rt.pool) hipMemset(pl.p, 0, (size_t)rt.pool_cap * p.slot_words * 8);   // (as kslot)
        if (!pool_counted) rt.extra_bound += rt.pool_cap;   // pool partials may complete too
        rt.cf = true;
        rt.cf_chunk = cc;
        // hot keys: candidate lists now, the match arenas when first needed
        if ((1 << lg) + kCfHotMax <= kCfMaxBuckets && !std::getenv("CEP_NO_HOT")) {
          rt.hot_thresh = (uint32_t)std::max<int64_t>(256, cc >> 16);
          if (const char* e = std::getenv("CEP_HOT_THRESH")) rt.hot_thresh = (uint32_t)std::max(16, std::atoi(e));
          ok = dev_ensure(&rt.hot_id, (size_t)kc * 2 + 16, a->stream, false) &&
               dev_ensure(&rt.hot_key, kCfHotMax * 4, a->stream, false) &&
               dev_ensure(&rt.hot_m, kCfHotMax * 4, a->stream, false) &&
               dev_ensure(&rt.cand, kCfHotMax * 4 * 8, a->stream, false) &&
               dev_ensure(&rt.ncand, 64, a->stream, false) && dev_ensure(&rt.hot_active, 64, a->stream, false) &&
               host_ensure(&rt.hot_active_host, 64);
          ok = ok && rt.hot_fork.create() && rt.hot_join.create();
          if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (hot keys)");
          hipMemset(rt.hot_id.p, 0xff, (size_t)kc * 2 + 16);
          hipMemset(rt.hot_key.p, 0xff, kCfHotMax * 4);
          hipMemset(rt.hot_m.p, 0, kCfHotMax * 4);
          hipMemset(rt.ncand.p, 0, 64);
          hipMemset(rt.hot_active.p, 0, 64);
          std::memset(rt.hot_active_host.p, 0, 64);
          rt.hot = true;
        }
      }
    }
    if (a->opt.sparse_keys && keyed) {
      // the map feeds the closed-form path's key column: the key may appear
      // in the plan only as the partition key (and `select s1.k`)
      const PrefPlan& pf = rt.pref;
      bool ok = rt.cf && a->opt.key_stride <= 1 && pf.key_slot == 0;
      for (int i = 0; ok && i < q.f_terms.n; ++i) ok = pf.f_slot[i] != 0;
      for (int i = 0; ok && i < q.g_terms.n; ++i) ok = pf.g_slot[i] != 0;
      for (int i = 0; ok && i < p.nrec_a; ++i) ok = pf.reca_slot[i] != 0;
      for (int i = 0; ok && i < p.nrec_b; ++i) ok = pf.recb_slot[i] != 0;
      const int kt = app.inputs[q.a_stream].attrs[q.key_col_a].type;
      ok = ok && (kt == T_INT || kt == T_LONG);
      if (!ok)
        return fail(a, CEP_E_UNSUPPORTED, "not supported: sparse_keys needs a closed-form `every A -> B` pattern whose int / long "
                                          "partition key is used only as the key, on one shard");
      uint64_t tc = 1;
      while (tc < 2 * (uint64_t)kc) tc <<= 1;
      rt.sparse = true;
      rt.table_cap = tc;
      if (!dev_ensure(&rt.tkey, tc * 8, a->stream, false) || !dev_ensure(&rt.tval, tc * 4, a->stream, false) ||
          !dev_ensure(&rt.krev, (size_t)kc * 8, a->stream, false) || !dev_ensure(&rt.kcount, 64, a->stream, false))
        return fail(a, CEP_E_DEVICE, "out of device memory (key map)");
      hipMemset(rt.tkey.p, 0, tc * 8);
      hipMemset(rt.tval.p, 0xff, tc * 4);
      hipMemset(rt.kcount.p, 0, 4);
      hipMemset((char*)rt.kcount.p + 4, 0xff, 4);
    }
    // `within` makes a pattern's result depend on event-time order (App. A.3
    // prunes on every event of the waiting state's stream); a sequence keeps
    // every row of its streams and prunes by |ts - ts(s1)| in any order, an
    // aggregation has no window: neither needs the re-run
    rt.order_sensitive = p.within >= 0 && !agg && !(q.nfa && q.sequence);
    a->pats.push_back(std::move(rt));
  }
  for (size_t qi = 0; qi < app.queries.size(); ++qi) {
    const Query& q = app.queries[qi];
    if (q.kind != Q_JOIN) continue;
    const bool timed = q.join_side[0].win_kind == WIN_TIME || q.join_side[1].win_kind == WIN_TIME;
    // A time window's rows are found by their position in the ts-ordered list
    // of kept rows; with ts in any order Siddhi's window is positional (a late
    // small ts sits behind a front row that blocks it) and the two differ.
    if (timed && a->opt.ts_order != 1)
      return fail(a, CEP_E_UNSUPPORTED, "a join with #window.time is not supported with ts_order = 0: the window "
                                        "is a suffix of the side's rows only for non-decreasing timestamps "
                                        "(set ts_order = 1)");
    if (a->opt.key_stride > 1)
      return fail(a, CEP_E_UNSUPPORTED, "a join is not supported with key_stride > 1: its windows are global "
                                        "and cannot be sharded by key");
    JoinRT rt;
    rt.q = (int)qi;
    JoinArgs& j = rt.ja;
    j.stream[0] = q.a_stream;
    j.stream[1] = q.b_stream;
    for (int s = 0; s < 2; ++s) {
      j.filter_prog[s] = q.join_side[s].filter.off;
      j.filter_terms[s] = q.join_side[s].filter_terms;
      j.win_kind[s] = q.join_side[s].win_kind;
      j.win_param[s] = q.join_side[s].win_param;
      rt.mark_vm |= j.filter_prog[s] >= 0 && j.filter_terms[s].n < 0;
    }
    j.nw = (int)q.rec_cols_a.size();
    for (int w = 0; w < j.nw; ++w) j.rec[w] = q.rec_cols_a[w];
    j.ew = 2 + j.nw;
    j.on_prog = q.join_on.off;
    j.nterms = std::max(0, q.join_nterms);
    for (int i = 0; i < j.nterms; ++i) j.terms[i] = q.join_terms[i];
    j.check_order = timed ? 1 : 0;
    rt.on_vm = q.join_nterms < 0;
    for (auto& it : q.select) rt.sel_vm |= it.src == SRC_VM;
    int64_t chunk = std::max<int64_t>(a->opt.chunk_events, kJoinBlockRows);
    chunk = std::min<int64_t>(chunk, kJoinMaxChunk);
    chunk = (chunk / kJoinBlockRows) * kJoinBlockRows;
    rt.chunk = chunk;
    const int64_t nblk = chunk / kJoinBlockRows, npb = chunk / kJoinThreads;
    bool ok = dev_ensure(&rt.flag, (size_t)chunk, a->stream, false) &&
              dev_ensure(&rt.bsum, (size_t)nblk * 8, a->stream, false) &&
              dev_ensure(&rt.boff, (size_t)nblk * 8, a->stream, false) &&
              dev_ensure(&rt.probe, (size_t)chunk * 8, a->stream, false) &&
              dev_ensure(&rt.pcnt, (size_t)chunk * 4, a->stream, false) &&
              dev_ensure(&rt.pbsum, (size_t)npb * 4, a->stream, false) &&
              dev_ensure(&rt.pboff, (size_t)npb * 4, a->stream, false) &&
              dev_ensure(&rt.st, sizeof(JoinState), a->stream, false) && host_ensure(&rt.total, 64);
    for (int s = 0; s < 2 && ok; ++s) {
      // tail (length: N rows, time: kJoinTailCap) + one chunk's kept rows
      rt.list_cap[s] = (j.win_kind[s] == WIN_LENGTH ? j.win_param[s] : (int64_t)kJoinTailCap) + chunk;
      for (int b = 0; b < 2 && ok; ++b)
        ok = dev_ensure(&rt.list[s][b], (size_t)rt.list_cap[s] * j.ew * 8, a->stream, false);
    }
    if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (join state)");
    hipMemset(rt.st.p, 0, sizeof(JoinState));
    a->joins.push_back(std::move(rt));
  }
  // event tables: per table one pipeline over all its operations
  if (!app.tables.empty()) {
    if (a->opt.sparse_keys)
      return fail(a, CEP_E_UNSUPPORTED, "sparse_keys is not supported for an app that holds a table: a table's keys "
                                        "are its primary-key values themselves (dense, no key map)");
    if (!dev_ensure(&a->tab_dropped, 64, a->stream, false)) return fail(a, CEP_E_DEVICE, "out of device memory");
    hipMemset(a->tab_dropped.p, 0, 64);
  }
  for (size_t ti = 0; ti < app.tables.size(); ++ti) {
    const TableDef& T = app.tables[ti];
    if (T.ops.empty()) continue;   // nobody reads or writes it
    TableRT rt;
    rt.tab = (int)ti;
    PatternArgs& p = rt.pa;
    p.a_stream = T.a_stream;
    p.b_stream = -1;
    p.f_prog = p.g_raw_prog = p.g_walk_prog = -1;
    p.within = -1;
    p.having_prog = -1;
    p.nrec_a = (int)T.rec_a.size();
    p.nrec_b = (int)T.rec_b.size();
    for (int i = 0; i < p.nrec_a; ++i) p.rec_a[i] = T.rec_a[i];
    for (int i = 0; i < p.nrec_b; ++i) p.rec_b[i] = T.rec_b[i];
    p.rec_words = 2 + std::max(p.nrec_a, p.nrec_b);
    p.key_capacity = a->opt.key_capacity;
    p.key_stride = std::max(1, a->opt.key_stride);
    p.key_offset = a->opt.key_offset;
    int lg = std::max(0, std::min(12, a->opt.buckets_log2));
    while ((p.key_capacity >> lg) > kWalkMaxKeys && lg < 12) ++lg;
    if ((p.key_capacity + (1 << lg) - 1) >> lg > kWalkMaxKeys)
      return fail(a, CEP_E_CAPACITY, "key_capacity exceeds 1024 * 4096 keys");
    p.buckets_log2 = lg;
    const int64_t kpb = (p.key_capacity + (1 << lg) - 1) >> lg;
    rt.kstride = kpb << lg;
    // operation j stands where state j of an N-state pattern stands
    p.nfa_mode = 1;
    p.nstates = (int)T.ops.size();
    for (int i = 0; i < 8; ++i) p.key_col_s[i] = T.key_col_s[i];
    p.key_col_a = p.key_col_b = T.key_col_s[T.a_stream];
    TabArgs& ta = rt.ta;
    ta.nops = p.nstates;
    ta.nwords = (int)T.schema.attrs.size();
    for (int j = 0; j < p.nstates; ++j) {
      const Query& q = app.queries[T.ops[j]];
      p.st_stream[j] = q.in_stream;
      p.st_min[j] = p.st_max[j] = 1;
      p.st_raw[j] = q.filter.off;
      p.st_walk[j] = -1;
      p.stream_mask |= 1 << q.in_stream;
      TabOp& op = ta.op[j];
      op.kind = q.tab_op;
      op.negate = q.tab_negate ? 1 : 0;
      op.on_prog = q.tab_on.off;
      op.reader = (q.tab_op == TOP_JOIN || q.tab_op == TOP_IN) ? 1 : 0;
      for (int w = 0; w < kMaxCaps; ++w) {
        op.ins[w] = q.tab_ins[w];
        op.set[w] = q.tab_set[w];
      }
      if (op.reader) {
        ++ta.nreaders;
        if (rt.run_at < 0) rt.run_at = T.ops[j];
        rt.vm |= q.tab_on.valid();
        for (auto& it : q.select) rt.vm |= it.src == SRC_VM;
      }
    }
    if (rt.run_at < 0) rt.run_at = T.ops[0];
    // the rows are the one state here that grows with a plan constant
    const double bytes = (double)rt.kstride * (4 + 8.0 * ta.nwords);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > (double)free_b)
      return fail(a, CEP_E_CAPACITY, "table " + T.schema.id + ": state of " + std::to_string((unsigned long long)bytes) +
                                         " bytes (" + std::to_string(rt.kstride) + " keys x " +
                                         std::to_string(ta.nwords) + " words) exceeds the GPU's free memory: lower "
                                         "key_capacity");
    int64_t chunk = std::max<int64_t>(a->opt.chunk_events, kPartThreads * kPartItems);
    chunk = std::min<int64_t>(chunk, (int64_t)kWalkMaxTiles * kPartThreads * kPartItems);
    chunk = (chunk / (kPartThreads * kPartItems)) * (kPartThreads * kPartItems);
    rt.pipe.chunk = chunk;
    const int64_t ntiles = chunk / (kPartThreads * kPartItems);
    const bool ok = dev_ensure(&rt.thdr, (size_t)rt.kstride * 4, a->stream, false) &&
                    dev_ensure(&rt.tword, (size_t)rt.kstride * ta.nwords * 8, a->stream, false) &&
                    rt.pipe.alloc((size_t)chunk * p.rec_words * 8 + 16, (size_t)ntiles * ((1 << lg) + 1) * 2, a->stream);
    if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (table " + T.schema.id + ")");
    hipMemset(rt.thdr.p, 0, (size_t)rt.kstride * 4);
    hipMemset(rt.tword.p, 0, (size_t)rt.kstride * ta.nwords * 8);
    a->tabs.push_back(std::move(rt));
  }
  {
    const int64_t none = INT64_MIN;
    if (!dev_ensure(&a->last_ts_dev, 64, a->stream, false) ||
        hipMemcpy(a->last_ts_dev.p, &none, 8, hipMemcpyHostToDevice) != hipSuccess)
      return fail(a, CEP_E_DEVICE, "out of device memory");
  }
  if (std::getenv("CEP_STAMPS") && !dev_ensure(&a->stamps, (size_t)2 * 4096 * 16 * 8, a->stream, false))
    return fail(a, CEP_E_DEVICE, "out of device memory (stamps)");
  hipStreamSynchronize(a->stream);
  return CEP_OK;
}

const StreamSchema* find_schema(cep_app* a, const char* id) {
  if (!id) return nullptr;
  int i = a->app.input_index(id);
  if (i >= 0) return &a->app.inputs[i];
  i = a->app.output_index(id);
  if (i >= 0) return &a->app.outputs[i];
  i = a->app.table_index(id);   // (cep_stream_schema also describes a table)
  if (i >= 0) return &a->app.tables[i].schema;
  return nullptr;
}

int fill_attrs(const StreamSchema* s, cep_attr* out, int cap, int* n) {
  if (n) *n = (int)s->attrs.size();
  for (int i = 0; i < (int)s->attrs.size() && i < cap; ++i) {
    std::snprintf(out[i].name, sizeof(out[i].name), "%s", s->attrs[i].name.c_str());
    out[i].type = s->attrs[i].type;
  }
  return CEP_OK;
}

// Run one filter query over a device batch.
int run_filter(cep_app* a, const Query& q, const RowsArgs& rows) {
  OutStream& o = a->outs[a->app.output_index(q.out_stream)];
  o.bound += rows.n;
  int rc = ensure_out_cap(a, o, o.bound);
  if (rc) return rc;
  constexpr int64_t kTile = kFilterThreads * kFilterItems;
  const int64_t ntiles = (rows.n + kTile - 1) / kTile;
  if (ntiles == 0) return CEP_OK;
  // look-back words for k_filter's or k_filterc's (smaller) tiles
  const int64_t fcr = filterc_rows_per_tile();
  const int64_t nflags = std::max<int64_t>(ntiles, (rows.n + fcr - 1) / fcr);
  if (!dev_ensure(&a->tile_state, (size_t)nflags * 8, a->stream, false))
    return fail(a, CEP_E_DEVICE, "out of device memory (tile state)");
  hipMemsetAsync(a->tile_state.p, 0, (size_t)nflags * 8, a->stream);
  hipMemsetAsync(a->ticket.p, 0, 16, a->stream);
  FilterArgs fa{};
  fa.rows = rows;
  fa.vm = {(const Ins*)a->code.p, (const uint64_t*)a->konst.p};
  fa.in_stream = q.in_stream;
  fa.filter_prog = q.filter.off;
  fa.filter_terms = q.filter_terms;
  fa.out = out_args(o, q);
  fa.tile_state = (unsigned long long*)a->tile_state.p;
  fa.ticket = (unsigned int*)a->ticket.p;
  fa.err = (unsigned int*)a->err.p;
  bool vm = q.filter.off >= 0 && q.filter_terms.n < 0;
  for (auto& it : q.select) vm |= it.src < SRC_REC || it.src >= SRC_TS;
  // k_filterc (filter.hip): term-list predicate over at most 3 distinct
  // columns, plain projection, pair loads aligned (8-byte columns at 16
  // bytes, 4-byte at 8, 1-byte at 2 from the slice's first row, which is
  // even).  CEP_NO_FILTERC=1 keeps k_filter.
  static const bool no_fc = std::getenv("CEP_NO_FILTERC") != nullptr;
  bool fc = !vm && !no_fc && (rows.row0 & 1) == 0;
  if (fc) {
    fa.npref = 0;
    for (int i = 0; fc && i < std::max(0, q.filter_terms.n); ++i) {
      const int c = q.filter_terms.t[i].col;
      int slot = -1;
      for (int k = 0; k < fa.npref; ++k)
        if (fa.pcol[k] == c) slot = k;
      if (slot < 0) {
        if (fa.npref == 3) {
          fc = false;
          break;
        }
        slot = fa.npref;
        fa.pcol[fa.npref++] = c;
      }
      fa.fslot[i] = slot;
    }
    if (fa.npref == 0) fa.pcol[fa.npref++] = 0;   // no predicate: one (unused) column
    auto al = [&](const void* ptr, int w) {
      return (((uintptr_t)ptr + (uintptr_t)(rows.row0 * w)) & (uintptr_t)(2 * w - 1)) == 0;
    };
    for (int k = 0; fc && k < fa.npref; ++k)
      fc = al(rows.cols.p[fa.pcol[k]], type_width(rows.cols.t[fa.pcol[k]]));
    if (fc && rows.stream) fc = al(rows.stream, 1);
  }
  LaunchTimer t(a, CEP_K_FILTER);
  if (fc) {
    const int64_t tr = filterc_rows_per_tile();
    const int64_t nt = (rows.n + tr - 1) / tr;
    launch_filterc(fa, nt, a->stream);
  } else {
    launch_filter(fa, ntiles, vm, a->stream);
  }
  return CEP_OK;
}

// 16-byte loads need every prefetched column (and ts) 16-byte aligned at
// each lane's first row (lanes start at multiples of 8 rows; 1-byte columns:
// 8-byte aligned, the hardware takes dword-aligned x4 loads)
bool pref_aligned(const PrefPlan& pf, const RowsArgs& rows) {
  auto al = [&](const void* ptr, int w) {
    const uintptr_t need = w == 1 ? 7u : 15u;
    return (((uintptr_t)ptr + (uintptr_t)(rows.row0 * w)) & need) == 0;
  };
  bool ok = al(rows.ts, 8) && (!rows.stream || al(rows.stream, 1));
  for (int i = 0; i < pf.n; ++i) {
    const int c = pf.col[i];
    ok = ok && al(rows.cols.p[c], type_width(rows.cols.t[c]));
  }
  return ok;
}

// Per-batch layout of the closed-form fast path's records: carried columns
// whose buffer is the batch's event-ts buffer are rebuilt from the record ts.
bool cf_plan(const PatternRT& rt, const RowsArgs& rows, CfPlan* cf, bool from_records = false) {
  const PatternArgs& p = rt.pa;
  std::memset(cf, 0, sizeof(*cf));
  int a_phys[kMaxCaps], b_phys[kMaxCaps];
  int na = 0, nb = 0;
  auto alias = [&](int col) {
    return !from_records && rows.cols.p[col] == (const void*)rows.ts && rows.cols.t[col] == T_LONG;
  };
  for (int c = 0; c < p.nrec_a; ++c) {
    a_phys[c] = alias(p.rec_a[c]) ? -1 : na;
    if (a_phys[c] >= 0) {
      cf->a_log[na] = c;
      cf->a_slot[na++] = rt.pref.reca_slot[c];
    }
  }
  for (int c = 0; c < p.nrec_b; ++c) {
    b_phys[c] = alias(p.rec_b[c]) ? -1 : nb;
    if (b_phys[c] >= 0) {
      cf->b_log[nb] = c;
      cf->b_slot[nb++] = rt.pref.recb_slot[c];
    }
  }
  cf->nw = std::max(na, nb);
  if (cf->nw > 2) return false;
  for (int w = na; w < 2; ++w) cf->a_slot[w] = 0;
  for (int w = nb; w < 2; ++w) cf->b_slot[w] = 0;
  for (int i = 0; i < kMaxCaps; ++i) cf->cap_phys[i] = i < p.ncap ? a_phys[p.cap_from_rec[i]] : 0;
  for (int c = 0; c < kMaxCaps; ++c) cf->bcol_phys[c] = c < p.nrec_b ? b_phys[c] : 0;
  return true;
}

// A prefetch slot whose column IS the batch's event-ts buffer holds a copy of
// the ts registers (E x 2 VGPRs).  When the column is only carried (rebuilt
// from the record ts: cap_phys / bcol_phys = -1) and is neither the key nor a
// term's column, nothing reads that copy: the partition is launched without
// the slot, with the later slots moved down by one (config 3: the NP = 3
// instance, which does not spill, instead of NP = 4).
void cf_drop_ts_slot(CfPartArgs* pa) {
  const int ts = pa->ts_slot;
  PrefPlan& pf = pa->pref;
  if (ts < 0 || pa->in_recs || pf.n < 2 || pf.key_slot == ts) return;
  const PatternArgs& p = pa->pat;
  const int nf = p.f_prog >= 0 ? p.f_terms.n : 0, ng = p.g_raw_prog >= 0 ? p.g_terms.n : 0;
  for (int i = 0; i < nf; ++i)
    if (pf.f_slot[i] == ts) return;
  for (int i = 0; i < ng; ++i)
    if (pf.g_slot[i] == ts) return;
  // (cf_plan lists only the physical carried words: a ts alias is not among
  // them; words past the stream's own count are padding nobody reads)
  for (int w = 0; w < pa->cf.nw; ++w)
    if (pa->cf.a_slot[w] == ts || pa->cf.b_slot[w] == ts) return;
  auto down = [&](int32_t& s) {
    if (s > ts) --s;
  };
  for (int i = ts; i + 1 < pf.n; ++i) pf.col[i] = pf.col[i + 1];
  --pf.n;
  for (int i = pf.n; i < kPref; ++i) pf.col[i] = pf.col[0];
  for (int i = 0; i < nf; ++i) down(pf.f_slot[i]);
  for (int i = 0; i < ng; ++i) down(pf.g_slot[i]);
  for (int w = 0; w < 2; ++w) {
    down(pa->cf.a_slot[w]);
    down(pa->cf.b_slot[w]);
  }
  down(pf.key_slot);
  pa->ts_slot = -1;
}

// Closed-form fast path: k_cfpart(c) then k_cfwalk(c) per chunk (double-
// buffered arenas; CEP_OVERLAP=1 runs the partitions on the side stream).
// tol: the order-tolerant closed form (ts in any order: g-failing B rows kept
// as expiry-only records, no pruning at A arrivals; hot keys through the
// hot kernels' order-tolerant scans).
int run_pattern_cf(cep_app* a, PatternRT& rt, const Query& q, OutStream& o,
                   const RowsArgs& rows_all, const CfPlan& cf,
                   const uint64_t* in_recs = nullptr, int in_rec_words = 0, bool tol = false) {
  const int P = 1 << rt.pa.buckets_log2;
  const bool hot_ok = rt.hot;
  ChunkPipe& pipe = rt.pipe;   // (its events, chunk_base and parity; the arenas are cf_recs / cf_toff)
  hipStream_t side = pipe.open_cf(a);
  const bool overlap = pipe.events;   // CEP_OVERLAP=1
  // Hot-key probe: until diversion has been decided once, the first chunk is
  // short (kHotProbeRows) and followed by one stream sync, so a skewed
  // stream's hottest keys are diverted from the second chunk on instead of
  // one workgroup walking a hot key's whole run of a full chunk (seconds at
  // Zipf s = 1.1).  Uniform streams pay one short chunk and one sync per
  // runtime.
  constexpr int64_t kHotProbeRows = 1 << 20;
  for (int64_t r0 = 0, step = 0; r0 < rows_all.n; r0 += step) {
    const int b = pipe.begin(side);
    const bool probe = hot_ok && !rt.hot_on && !rt.hot_probed;
    step = std::min<int64_t>(probe ? std::min<int64_t>(kHotProbeRows, rt.cf_chunk) : rt.cf_chunk, rows_all.n - r0);
    RowsArgs rows = rows_all;
    rows.row0 = rows_all.row0 + r0;
    rows.n = step;
    if (r0 > 0) rows.prev_ts = INT64_MIN;   // checked inside the kernel via ts[row-1]
    const int64_t ntiles = (rows.n + kCfTile - 1) / kCfTile;
    CfPartArgs pa{};
    pa.rows = rows;
    pa.pref = rt.pref;
    pa.ts_slot = -1;
    pa.in_recs = in_recs;
    pa.in_rec_words = in_rec_words;
    for (int i = 0; i < rt.pref.n && !in_recs; ++i)
      if (rows.cols.p[rt.pref.col[i]] == (const void*)rows.ts && rows.cols.t[rt.pref.col[i]] == T_LONG)
        pa.ts_slot = i;
    pa.pat = rt.pa;
    pa.pat.tolerant = tol ? 1 : 0;
    pa.cf = cf;
    cf_drop_ts_slot(&pa);
    pa.chunk_base = (int64_t*)pipe.chunk_base[b].p;
    pa.recs = (uint64_t*)rt.cf_recs[b].p;
    pa.tile_off = (uint16_t*)rt.cf_toff[b].p;
    pa.ntiles = (int32_t)ntiles;
    pa.err = (unsigned int*)a->err.p;
    // staggered first round (k_cfpart): 32 steps over about one tile's
    // duration (~40 k ticks at config 3; measured 320 / 640 / 1280 / 2000
    // ticks per step: 293 / 285 / 281 / 286 us), and only when
    // every CU runs several tiles, so a short chunk does not pay the delay
    // (CEP_CF_STAGGER: ticks per step, 0 = off)
    static const int stagger = std::getenv("CEP_CF_STAGGER") ? std::atoi(std::getenv("CEP_CF_STAGGER")) : 1280;
    pa.stagger = ntiles >= 4 * kCfStaggerBlocks ? stagger : 0;
    pa.one_wg = a->cf_one_wg ? 1 : 0;
    // the pool cursor of this chunk's walk: zeroed by the partition (serial
    // mode), or by a fill on the walk's stream when the partition may run
    // beside the previous walk (CEP_OVERLAP)
    pa.pool_cursor = overlap ? nullptr : (unsigned long long*)rt.pool_cur.p;
    if (overlap) hipMemsetAsync(rt.pool_cur.p, 0, 8, a->stream);
    if (a->stamps.p) pa.stamps = (uint64_t*)a->stamps.p + 4096 * 16;
    // hot keys: diversion starts once the device reported a slot in use (the
    // pinned word is refreshed asynchronously after every walk)
    const bool hot = hot_ok;
    if (hot && !rt.hot_on && *(volatile uint32_t*)rt.hot_active_host.p > 0) {
      const int rw = 1 + cf.nw;
      const int64_t cc = rt.cf_chunk, ntmax = cc / kCfTile;
      rt.hot_blocks = (int)((cc + kHotBlock - 1) / kHotBlock);
      const bool ok = dev_ensure(&rt.hot_gbase, (kCfHotMax + 1) * 4, a->stream, false) &&
                      dev_ensure(&rt.hoff, (size_t)kCfHotMax * ntmax * 4, a->stream, false) &&
                      dev_ensure(&rt.harr, (size_t)cc * rw * 8, a->stream, false) &&
                      dev_ensure(&rt.hrow, (size_t)cc * 4, a->stream, false) &&
                      dev_ensure(&rt.hnb, (size_t)cc * 4, a->stream, false) &&
                      dev_ensure(&rt.bsum, (size_t)rt.hot_blocks * 16, a->stream, false) &&
                      dev_ensure(&rt.bcnt, (size_t)rt.hot_blocks * 4, a->stream, false) &&
                      dev_ensure(&rt.boff, (size_t)rt.hot_blocks * 4, a->stream, false) &&
                      dev_ensure(&rt.hcm, kCfHotMax * 3 * 4, a->stream, false) &&
                      dev_ensure(&rt.hobase, 64, a->stream, false) &&
                      dev_ensure(&rt.htmn, (size_t)cc * 4, a->stream, false) &&
                      dev_ensure(&rt.htmx, (size_t)cc * 4, a->stream, false) &&
                      dev_ensure(&rt.hflag, (size_t)cc, a->stream, false) &&
                      dev_ensure(&rt.btol, (size_t)rt.hot_blocks * 12, a->stream, false);
      if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (hot-key arenas)");
      rt.hot_on = true;
    }
    const bool divert = hot && rt.hot_on;
    pa.hot_id = divert ? (const uint16_t*)rt.hot_id.p : nullptr;
    pa.nhot = divert ? kCfHotMax : 0;
    // ts_order 0: an in-order chunk (checked on the device against the
    // high-water mark of every earlier row) runs the adaptive build at
    // event-time cost; one that is not sets the gate and the order-tolerant
    // kernels queued behind it take it.  Not with hot-key diversion or
    // received records (those chunks run the order-tolerant build).
    static const bool no_atol = std::getenv("CEP_NO_ATOL") != nullptr;
    const bool atol = tol && !in_recs && !divert && rt.atol_ok && rt.hwm.p && !no_atol &&
                      (2 << rt.pa.buckets_log2) <= kCfMaxBuckets && q.a_stream != q.b_stream;
    uint32_t gseq = 0;
    if (tol && rt.hwm.p) {
      const int par = (int)(rt.tol_chunks++ & 1);
      pa.hwm_rd = (const unsigned long long*)rt.hwm.p + (par ^ 1) * 64;
      pa.hwm_wr = (unsigned long long*)rt.hwm.p + par * 64;
    }
    if (atol) {
      if (++rt.atol_seq == 0) ++rt.atol_seq;
      gseq = rt.atol_seq;
      pa.gate = (uint32_t*)rt.atol_gate.p;
      pa.gate_seq = gseq;
    }
    // hot keys: k_cfpart reads hot_id, which the previous chunk's
    // k_hot_update rewrites on the main stream (walk_done is recorded after
    // it), so with diversion candidates the partition waits for that chunk
    if (overlap && hot && pipe.used[b ^ 1]) hipStreamWaitEvent(side, pipe.walk_done[b ^ 1], 0);
    if (atol) {
      CfPartArgs aa = pa;
      aa.atol = 1;
      aa.pat.tolerant = 0;
      aa.nhot = P;   // the P expiry-entry twins of the key buckets
      aa.hot_id = nullptr;
      LaunchTimer t(a, CEP_K_CF_PARTITION, side);
      launch_cf_partition(aa, ntiles, side);
    }
    {
      // (adaptive chunk: the order-tolerant fallback, which returns at once
      // when the chunk was in order)
      LaunchTimer t(a, atol ? CEP_K_OTHER : CEP_K_CF_PARTITION, side);
      if (cf_partition_2wg(pa)) a->launches[CEP_K_CF_PARTITION_2WG]++;   // (k_cfpart2: counted under both)
      launch_cf_partition(pa, ntiles, side);
    }
    pipe.partitioned(b, side, a->stream);
    CfWalkArgs wa{};
    wa.pat = pa.pat;
    wa.cf = cf;
    wa.recs = pa.recs;
    wa.tile_off = pa.tile_off;
    wa.ntiles = (int32_t)ntiles;
    wa.chunk_base = (const int64_t*)pipe.chunk_base[b].p;
    wa.khdr = (uint32_t*)rt.khdr.p;
    wa.kslot = (uint64_t*)rt.kslot.p;
    wa.kstride = rt.kstride;
    wa.kext = (uint64_t*)rt.kext.p;
    wa.pool_rd = (const uint64_t*)rt.pool[rt.pool_side].p;
    wa.pool_wr = (uint64_t*)rt.pool[rt.pool_side ^ 1].p;
    wa.pool_cursor = (unsigned long long*)rt.pool_cur.p;
    wa.pool_cap = (uint64_t)rt.pool_cap;
    wa.key_rev = rt.sparse ? (const uint64_t*)rt.krev.p : nullptr;
    wa.out = out_args(o, q);
    wa.err = pa.err;
    HotArgs ha{};
    if (hot) {
      ha.pat = pa.pat;   // (tolerant flag included)
      ha.cf = cf;
      ha.recs = pa.recs;
      ha.tile_off = pa.tile_off;
      ha.ntiles = (int32_t)ntiles;
      ha.chunk_base = (const int64_t*)pipe.chunk_base[b].p;
      ha.hot_id = (uint16_t*)rt.hot_id.p;
      ha.hot_key = (int32_t*)rt.hot_key.p;
      ha.hot_m = (uint32_t*)rt.hot_m.p;
      ha.hot_gbase = (uint32_t*)rt.hot_gbase.p;
      ha.hoff = (uint32_t*)rt.hoff.p;
      ha.cand = (uint64_t*)rt.cand.p;
      ha.ncand = (uint32_t*)rt.ncand.p;
      ha.cand_cap = kCfHotMax * 4;
      ha.thresh = rt.hot_thresh;
      ha.harr = (uint64_t*)rt.harr.p;
      ha.hrow = (uint32_t*)rt.hrow.p;
      ha.hnb = (uint32_t*)rt.hnb.p;
      ha.bsum = (uint32_t*)rt.bsum.p;
      ha.bcnt = (uint32_t*)rt.bcnt.p;
      ha.boff = (uint32_t*)rt.boff.p;
      ha.hcm = (uint32_t*)rt.hcm.p;
      ha.obase = (unsigned long long*)rt.hobase.p;
      ha.htmn = (uint32_t*)rt.htmn.p;
      ha.htmx = (uint32_t*)rt.htmx.p;
      ha.hflag = (uint8_t*)rt.hflag.p;
      ha.btol = (uint32_t*)rt.btol.p;
      ha.max_blocks = rt.hot_blocks;
      ha.khdr = wa.khdr;
      ha.kslot = wa.kslot;
      ha.kstride = wa.kstride;
      ha.kext = wa.kext;
      ha.pool_rd = wa.pool_rd;
      ha.pool_wr = wa.pool_wr;
      ha.pool_cursor = wa.pool_cursor;
      ha.pool_cap = wa.pool_cap;
      ha.key_rev = wa.key_rev;
      ha.out = wa.out;
      ha.active = (uint32_t*)rt.hot_active.p;
      ha.in_seq = in_recs ? in_recs + rows.row0 * in_rec_words + 1 : nullptr;
      ha.in_rec_words = in_rec_words;
      static const int hot_ablate = std::getenv("CEP_HOT_ABLATE") ? std::atoi(std::getenv("CEP_HOT_ABLATE")) : 0;
      ha.ablate = hot_ablate;
      ha.err = pa.err;
      wa.hot_cand = ha.cand;
      wa.hot_ncand = ha.ncand;
      wa.hot_thresh = rt.hot_thresh;
      wa.hot_id = divert ? ha.hot_id : nullptr;
    }
    // the hot kernels run on the side stream beside the walk: disjoint keys,
    // shared output / pool cursors are atomics (CEP_HOT_SERIAL=1: main stream)
    static const bool hot_serial = std::getenv("CEP_HOT_SERIAL") != nullptr;
    hipStream_t hs = hot_serial ? a->stream : a->side;
    if (divert) {
      if (!hot_serial) {
        hipEventRecord(rt.hot_fork, a->stream);
        hipStreamWaitEvent(hs, rt.hot_fork, 0);
      }
      {
        LaunchTimer t(a, CEP_K_HOT, hs);
        launch_hot_match(ha, hs);
      }
      if (!hot_serial) hipEventRecord(rt.hot_join, hs);
    }
    wa.in_seq = in_recs ? in_recs + rows.row0 * in_rec_words + 1 : nullptr;
    wa.in_rec_words = in_rec_words;
    static const int ablate = std::getenv("CEP_ABLATE") ? std::atoi(std::getenv("CEP_ABLATE")) : 0;
    wa.ablate = ablate;
    if (a->stamps.p) {
      wa.stamps = (uint64_t*)a->stamps.p;
      hipMemsetAsync(wa.stamps, 0, (size_t)4096 * 16 * 8, a->stream);
    }
    if (atol) {
      CfWalkArgs aw = wa;
      aw.atol = 1;
      aw.pat.tolerant = 0;
      aw.hot_id = nullptr;
      aw.gate = (const uint32_t*)rt.atol_gate.p;
      aw.gate_seq = gseq;
      {
        LaunchTimer t(a, CEP_K_CF_WALK);
        launch_cf_walk(aw, P, a->stream);
      }
      // the pool this walk wrote is what the fallback must read (it returns
      // at once when this one ran, and reads nothing)
      wa.gate = aw.gate;
      wa.gate_seq = gseq;
    }
    {
      LaunchTimer t(a, atol ? CEP_K_OTHER : CEP_K_CF_WALK);
      launch_cf_walk(wa, P, a->stream);
    }
    if (hot) {
      if (divert && !hot_serial) hipStreamWaitEvent(a->stream, rt.hot_join, 0);
      launch_hot_update(ha, divert ? 1 : 0, a->stream);
      // slots in use, for the next batch's diversion check and cep_stats:
      // once per batch (and after the probe), not per chunk — each copy is
      // a blit on the engine stream between two walks
      if (probe || r0 + step >= rows_all.n)
        hipMemcpyAsync(rt.hot_active_host.p, rt.hot_active.p, 4, hipMemcpyDeviceToHost, a->stream);
      if (probe) {   // the probe's verdict decides the next chunk's diversion
        hipStreamSynchronize(a->stream);
        rt.hot_probed = true;
      }
    }
    rt.pool_side ^= 1;   // this launch's write pool holds every run now
    pipe.walked(b, a->stream);
  }
  return CEP_OK;
}

// The order-tolerant form of a pattern (rows whose ts may go backwards).
// Every row of the waiting state's stream may expire partials, so the
// partition keeps them all; the walk's closed form (event-time order, only
// g-passing B's) is off.  A 2-state pattern is walked by the N-state walk on
// its own record roles and state layout (nfa_pair): that walk keeps lists
// longer than pending_slots in the pending pool, as the closed-form path does.
PatternArgs tolerant_args(const PatternRT& rt, const Query& q) {
  PatternArgs p = rt.pa;
  p.tolerant = 1;
  p.closed_form = 0;
  if (!p.nfa_mode && !p.agg_mode) {
    p.nfa_mode = 1;
    p.nfa_pair = 1;
    p.nfa_seq = 0;
    p.nstates = 2;
    p.st_stream[0] = q.a_stream;
    p.st_stream[1] = q.b_stream;
    for (int j = 0; j < 2; ++j) {
      p.st_min[j] = p.st_max[j] = 1;
      p.st_raw[j] = -1;
      p.st_walk[j] = -1;
    }
    p.st_tail_opt[0] = 0;
    p.st_tail_opt[1] = 1;
    p.stream_mask = (1 << q.a_stream) | (1 << q.b_stream);
    for (int i = 0; i < 8; ++i) p.key_col_s[i] = -1;
    p.key_col_s[q.a_stream] = q.key_col_a;
    p.key_col_s[q.b_stream] = q.key_col_b;
    for (int i = 0; i < p.ncap; ++i) {   // s1's captures, from the A record
      p.cap_state[i] = 0;
      p.cap_index[i] = -1;
      p.cap_word[i] = p.cap_from_rec[i];
      p.cap_null[i] = 0;
    }
  }
  return p;
}

// tolerant: run on the order-tolerant path (rows whose ts may go backwards:
// a watermark release holding late rows, or the re-run after a descent).
int run_pattern(cep_app* a, PatternRT& rt, const RowsArgs& rows_in, const uint64_t* in_recs, int in_rec_words,
                bool tolerant) {
  const Query& q = a->app.queries[rt.q];
  OutStream& o = a->outs[a->app.output_index(q.out_stream)];
  if (o.bound == 0) o.bound = rt.extra_bound;
  o.bound += rows_in.n;
  int rc = ensure_out_cap(a, o, o.bound);
  if (rc) return rc;
  // Timestamps in any order (cep_options.ts_order = 0): a pattern with
  // `within` runs the order-tolerant path, whose state is exactly the
  // oracle's (App. A.3: partials pruned only by |ts - ts(s1)| > W on events
  // of the stream they wait on); the event-time fast paths (closed form,
  // push-down of g-failing B's, pruning at A arrivals) need ts_order = 1.
  // A sequence prunes by |ts - ts(s1)| on every row of its streams in any
  // order: tolerant only drops its order check.  The multi-GPU record / row
  // shuffles always take the event-time paths.
  // Received shuffle records take the tolerant path too: an order-tolerant
  // sender (same ts_order) ships every B-stream row (route_batch).
  if (!tolerant && a->opt.ts_order == 0 && rt.pa.within >= 0 && (rt.order_sensitive || rt.pa.nfa_seq) &&
      !rows_in.seq)
    tolerant = true;
  const RowsArgs& rows_all = rows_in;
  // case (c) of the window queries (one window per group standing in for
  // Siddhi's global one) holds for non-decreasing ts only: released late rows
  // are not
  if (tolerant && rt.win.kind != WIN_NONE && q.win_global)
    return fail(a, CEP_E_UNSUPPORTED, "group by with #window.time outside a partition is not supported for late rows "
                                      "(late_policy 2): partition the query");
  // ts in any order on the closed form (k_cfpart / k_cfwalk TOL builds);
  // CEP_TOL_GENERAL=1 keeps the N-state walk (nfa_pair) for these runs
  static const bool tol_general = std::getenv("CEP_TOL_GENERAL") != nullptr;
  if (rt.sparse && tolerant && tol_general)
    return fail(a, CEP_E_UNSUPPORTED, "sparse_keys with CEP_TOL_GENERAL (the N-state walk has no key map)");
  if (rt.sparse) {
    // partition values -> dense slots (keymap.hip); the pattern then reads
    // the dense column in place of the key column
    if (in_recs || rows_all.seq) return fail(a, CEP_E_UNSUPPORTED, "sparse_keys with the multi-GPU key shuffle");
    const int kcol = rows_all.input == q.b_stream ? q.key_col_b : q.key_col_a;
    if (!dev_ensure(&rt.dense, (size_t)std::max<int64_t>(rows_all.n, 1) * 4 + 16, a->stream, false))
      return fail(a, CEP_E_DEVICE, "out of device memory (dense keys)");
    KeyMapArgs ka{};
    ka.key = rows_all.cols.p[kcol];
    ka.key_is_long = rows_all.cols.t[kcol] == T_LONG ? 1 : 0;
    ka.stream = rows_all.stream;
    ka.input = rows_all.input;
    ka.a_stream = q.a_stream;
    ka.b_stream = q.b_stream;
    ka.row0 = rows_all.row0;
    ka.n = rows_all.n;
    ka.tkey = (unsigned long long*)rt.tkey.p;
    ka.tval = (uint32_t*)rt.tval.p;
    ka.table_cap = rt.table_cap;
    ka.rev = (uint64_t*)rt.krev.p;
    ka.count = (unsigned int*)rt.kcount.p;
    ka.minus_one = (unsigned int*)rt.kcount.p + 1;
    ka.cap = (uint32_t)rt.pa.key_capacity;
    ka.out = (int32_t*)rt.dense.p;
    ka.err = (unsigned int*)a->err.p;
    {
      LaunchTimer t(a, CEP_K_OTHER);
      launch_keymap(ka, a->stream);
    }
    RowsArgs rows = rows_all;
    // the dense column is indexed from the slice's first row
    rows.cols.p[kcol] = (const int32_t*)rt.dense.p - rows_all.row0;
    rows.cols.t[kcol] = T_INT;
    CfPlan cf;
    if (!pref_aligned(rt.pref, rows) || !cf_plan(rt, rows, &cf, false))
      return fail(a, CEP_E_ARG, "sparse_keys needs 16-byte aligned columns");
    // (ts_order 0: the closed form's order-tolerant build over the dense keys)
    return run_pattern_cf(a, rt, q, o, rows, cf, nullptr, 0, tolerant);
  }
  if (rt.cf && !tolerant && !rows_all.seq && (in_recs || pref_aligned(rt.pref, rows_all))) {
    CfPlan cf;
    if (cf_plan(rt, rows_all, &cf, in_recs != nullptr))
      return run_pattern_cf(a, rt, q, o, rows_all, cf, in_recs, in_rec_words);
  }
  if (rt.cf && tolerant && !tol_general && !rows_all.seq && (in_recs || pref_aligned(rt.pref, rows_all))) {
    CfPlan cf;
    if (cf_plan(rt, rows_all, &cf, in_recs != nullptr))
      return run_pattern_cf(a, rt, q, o, rows_all, cf, in_recs, in_rec_words, true);
  }
  const int P = 1 << rt.pa.buckets_log2;
  rt.atol_ok = false;   // this path keeps no high-water mark: adaptive chunks off for good
  ChunkPipe& pipe = rt.pipe;
  hipStream_t side = pipe.open(a);
  const int64_t cstep = tolerant ? rt.chunk_tol : pipe.chunk;
  for (int64_t r0 = 0; r0 < rows_all.n; r0 += cstep) {
    const int b = pipe.begin(side);
    RowsArgs rows = rows_all;
    rows.row0 = rows_all.row0 + r0;
    rows.n = std::min<int64_t>(cstep, rows_all.n - r0);
    if (r0 > 0) rows.prev_ts = INT64_MIN;   // checked inside the kernel via ts[row-1]
    const int64_t ntiles = (rows.n + kPartThreads * kPartItems - 1) / (kPartThreads * kPartItems);
    PartArgs pa{};
    pa.rows = rows;
    pa.pref = rt.pref;
    if (in_recs) {   // received shuffle records (cep_send_records)
      pa.from_records = 1;
      pa.in_recs = in_recs;
      pa.in_rec_words = in_rec_words;
      pa.pref.n = -1;
    }
    if (pa.pref.n >= 0 && !pref_aligned(pa.pref, rows)) pa.pref.n = -1;
    if (r0 > 0) pa.rows.prev_ts = INT64_MIN;
    pa.vm = {(const Ins*)a->code.p, (const uint64_t*)a->konst.p};
    pa.pat = tolerant ? tolerant_args(rt, q) : rt.pa;
    pa.tile_rows = kPartThreads * kPartItems;
    pa.recs = (uint64_t*)pipe.recs[b].p;
    pa.tile_off = (uint16_t*)pipe.tile_off[b].p;
    pa.chunk_base = (int64_t*)pipe.chunk_base[b].p;
    pa.err = (unsigned int*)a->err.p;
    if (a->stamps.p) pa.stamps = (uint64_t*)a->stamps.p + 4096 * 16;
    {
      LaunchTimer t(a, CEP_K_PARTITION, side);
      launch_partition(pa, ntiles, rt.part_vm, side);
    }
    pipe.partitioned(b, side, a->stream);
    WalkArgs wa{};
    wa.vm = pa.vm;
    wa.pat = pa.pat;
    wa.recs = pa.recs;
    wa.tile_off = pa.tile_off;
    wa.ntiles = (int)ntiles;
    wa.tile_rows = pa.tile_rows;
    wa.chunk_base = (const int64_t*)pipe.chunk_base[b].p;
    if (a->stamps.p) {
      // keep the last chunk's stamps (diagnostics only)
      wa.stamps = (uint64_t*)a->stamps.p;
    }
    wa.khdr = (uint32_t*)rt.khdr.p;
    wa.kslot = (uint64_t*)rt.kslot.p;
    wa.kstride = rt.kstride;
    wa.out = out_args(o, q);
    wa.err = pa.err;
    if (rt.win.kind != WIN_NONE) {
      WinArgs ww = rt.win;
      ww.vm = pa.vm;
      ww.pat = pa.pat;
      ww.recs = pa.recs;
      ww.tile_off = pa.tile_off;
      ww.ntiles = (int)ntiles;
      ww.tile_rows = pa.tile_rows;
      ww.chunk_base = wa.chunk_base;
      ww.khdr = wa.khdr;
      ww.kslot = wa.kslot;
      ww.kstride = wa.kstride;
      ww.out = wa.out;
      ww.err = wa.err;
      {
        LaunchTimer t(a, CEP_K_AGG);
        launch_winwalk(ww, P, rt.win_vm, a->stream);
      }
      pipe.walked(b, a->stream);
      continue;
    }
    if (rt.bat.kind != WIN_NONE) {
      BatchArgs bw = rt.bat;
      bw.vm = pa.vm;
      bw.pat = pa.pat;
      bw.recs = pa.recs;
      bw.tile_off = pa.tile_off;
      bw.ntiles = (int)ntiles;
      bw.tile_rows = pa.tile_rows;
      bw.chunk_base = wa.chunk_base;
      bw.khdr = wa.khdr;
      bw.kslot = wa.kslot;
      bw.kstride = wa.kstride;
      bw.out = wa.out;
      bw.err = wa.err;
      {
        LaunchTimer t(a, CEP_K_AGG);
        launch_batchwalk(bw, P, rt.win_vm, a->stream);
      }
      pipe.walked(b, a->stream);
      continue;
    }
    const bool pool = (q.nfa || pa.pat.nfa_pair) && rt.kext.p;
    if (pool) {
      wa.kext = (uint64_t*)rt.kext.p;
      wa.pool_rd = (const uint64_t*)rt.pool[rt.pool_side].p;
      wa.pool_wr = (uint64_t*)rt.pool[rt.pool_side ^ 1].p;
      wa.pool_cursor = (unsigned long long*)rt.pool_cur.p;
      wa.pool_cap = (uint64_t)rt.pool_cap;
      hipMemsetAsync(rt.pool_cur.p, 0, 8, a->stream);
    }
    {
      LaunchTimer t(a, CEP_K_WALK);
      launch_walk(wa, P, rt.walk_vm || pa.pat.nfa_pair, a->stream);
    }
    if (pool) rt.pool_side ^= 1;   // this launch's write pool holds every run now
    pipe.walked(b, a->stream);
  }
  return CEP_OK;
}

// One batch through a multi-query group: per chunk, k_mqpart on the side
// stream (double-buffered arenas: the partition of chunk c+1 overlaps the
// walk of chunk c) and k_mqwalk on the main stream.
int run_mq(cep_app* a, MqRT& g, const RowsArgs& rows_all) {
  const CompiledApp& app = a->app;
  // output capacity: at most one row per query per input row
  for (size_t i = 0; i < g.qs.size(); ++i) {
    const Query& q = app.queries[g.qs[i]];
    OutStream& o = a->outs[app.output_index(q.out_stream)];
    o.bound += rows_all.n;
    const int rc = ensure_out_cap(a, o, o.bound);
    if (rc) return rc;
    MqQuery& d = g.hq[i];
    int64_t* oseq = o.write_seq ? (int64_t*)o.seq.p : nullptr;   // not read: not stored
    bool same = d.out_ts == (int64_t*)o.ts.p && d.out_seq == oseq && d.out_count == o.count &&
                d.out_cap == o.cap;
    for (int c = 0; c < d.nsel; ++c) same = same && d.out_col[c] == o.cols[c].p;
    if (!same) {
      for (int c = 0; c < d.nsel; ++c) d.out_col[c] = o.cols[c].p;
      d.out_ts = (int64_t*)o.ts.p;
      d.out_seq = oseq;
      d.out_count = o.count;
      d.out_cap = o.cap;
      g.dq_dirty = true;
    }
  }
  if (g.dq_dirty) {   // rare (output growth): the walks in flight read the old table
    hipStreamSynchronize(a->stream);
    hipMemcpy(g.dq.p, g.hq.data(), g.hq.size() * sizeof(MqQuery), hipMemcpyHostToDevice);
    g.dq_dirty = false;
  }
  // this batch's column layout: a carried column whose buffer IS the event-ts
  // buffer is not carried (its value is the record's ts)
  const std::vector<int> pc = mq_pref_cols(g);
  MqPartArgs pa{};
  pa.pref.n = (int)pc.size();
  for (int i = 0; i < kPref; ++i) pa.pref.col[i] = i < pa.pref.n ? pc[i] : pc[0];
  pa.ts_slot = -1;
  for (int i = 0; i < pa.pref.n; ++i)
    if (rows_all.cols.p[pc[i]] == (const void*)rows_all.ts && rows_all.cols.t[pc[i]] == T_LONG) pa.ts_slot = i;
  MqWalkArgs wa{};
  int nphys = 0;
  for (size_t w = 0; w < g.carry.size(); ++w) {
    const int col = g.carry[w];
    if (rows_all.cols.p[col] == (const void*)rows_all.ts && rows_all.cols.t[col] == T_LONG) {
      wa.lmap[w] = -1;
      continue;
    }
    if (nphys >= kMqMaxPhys)
      return fail(a, CEP_E_UNSUPPORTED, "multi-query group carries more than " + std::to_string(kMqMaxPhys) + " columns");
    wa.lmap[w] = nphys;
    for (int i = 0; i < pa.pref.n; ++i)
      if (pc[i] == col) pa.phys_slot[nphys] = i;
    ++nphys;
  }
  if (nphys > std::min<int>((int)g.carry.size(), kMqMaxPhys)) return fail(a, CEP_E_DEVICE, "record arena too small");
  pa.stream_mask = g.stream_mask;
  pa.key_slot = 0;
  for (int s = 0; s < 8; ++s) pa.ncond[s] = g.ncond[s];
  pa.conds = (const MqCond*)g.dconds.p;
  pa.nphys = nphys;
  // the group's sequences prune by |ts - ts(s1)| on every row of their
  // streams (any order); the check stays for callers that asked for it
  pa.check_order = (g.check_order && a->opt.ts_order == 1 && !a->force_tolerant) ? 1 : 0;
  pa.key_capacity = g.key_capacity;
  pa.key_stride = g.key_stride;
  pa.key_offset = g.key_offset;
  pa.buckets_log2 = g.lg;
  pa.err = (unsigned int*)a->err.p;
  wa.q = (const MqQuery*)g.dq.p;
  wa.nq = (int)g.qs.size();
  wa.units = (const MqUnit*)g.du.p;
  wa.nunits = (int)g.units.size();
  wa.nphys = nphys;
  wa.buckets_log2 = g.lg;
  wa.kpb = g.kpb;
  wa.key_stride = g.key_stride;
  wa.key_offset = g.key_offset;
  wa.state = (uint64_t*)g.state.p;
  wa.kstride = g.kstride;
  wa.words = g.words;
  static const int mq_ablate = std::getenv("CEP_MQ_ABLATE") ? std::atoi(std::getenv("CEP_MQ_ABLATE")) : 0;
  wa.ablate = mq_ablate;
  wa.err = pa.err;
  if (a->stamps.p && (1 << g.lg) * 16 <= 2 * 4096 * 16) {
    wa.stamps = (uint64_t*)a->stamps.p;
    hipMemsetAsync(wa.stamps, 0, (size_t)(1 << g.lg) * 16 * 8, a->stream);
  }
  ChunkPipe& pipe = g.pipe;
  hipStream_t side = pipe.open(a);
  for (int64_t r0 = 0; r0 < rows_all.n; r0 += pipe.chunk) {
    const int b = pipe.begin(side);
    RowsArgs rows = rows_all;
    rows.row0 = rows_all.row0 + r0;
    rows.n = std::min<int64_t>(pipe.chunk, rows_all.n - r0);
    const int ntiles = (int)((rows.n + kMqTile - 1) / kMqTile);
    pa.rows = rows;
    pa.ntiles = ntiles;
    pa.chunk_base = (int64_t*)pipe.chunk_base[b].p;
    pa.recs = (uint64_t*)pipe.recs[b].p;
    pa.tile_off = (uint16_t*)pipe.tile_off[b].p;
    {
      LaunchTimer t(a, CEP_K_MQ_PARTITION, side);
      launch_mq_partition(pa, side);
    }
    pipe.partitioned(b, side, a->stream);
    wa.recs = pa.recs;
    wa.tile_off = pa.tile_off;
    wa.ntiles = ntiles;
    wa.chunk_base = pa.chunk_base;
    wa.in_seq = rows.seq ? rows.seq + rows.row0 : nullptr;
    {
      LaunchTimer t(a, CEP_K_MQ_WALK);
      launch_mq_walk(wa, 1 << g.lg, a->stream);
    }
    pipe.walked(b, a->stream);
  }
  return CEP_OK;
}

// Query chaining: view `vi` of the slice (derive.hip).  One k_derive launch
// per chain depth; stage k reads stage k-1's view.  The view keeps the
// slice's n, ts, arrival numbers and row positions; its handle column and
// the columns that are not same-position plain copies are the app's buffers,
// laid out so that row0 has the alignment a 256-byte-aligned caller column
// has there (run_filter's pair-load test and pref_aligned decide as for the
// batch itself).  A stage none of whose producers can see a row of the slice
// (no handle column, another input) is skipped.
int build_view(cep_app* a, int vi, const RowsArgs& rows, RowsArgs* out) {
  const CompiledApp& app = a->app;
  const View& v = app.views[vi];
  if (a->views.size() < app.views.size()) a->views.resize(app.views.size());
  auto& stages = a->views[vi];
  if ((int)stages.size() < v.stages) stages.resize(v.stages);
  RowsArgs cur = rows;
  for (int st = 1; st <= v.stages; ++st) {
    DeriveArgs da{};
    bool seen = cur.stream != nullptr;
    for (int di : v.derived) {
      const Derived& d = app.derived[di];
      if (d.stage != st) continue;
      // a slice of another layout holds no row of this producer's source (a
      // mixed batch mixes identical definitions); its columns are not the
      // ones the producer's programs index
      const auto& sa = app.inputs[d.source].attrs;
      bool same = (int)sa.size() == cur.cols.n;
      for (int c = 0; same && c < cur.cols.n; ++c) same = sa[c].type == cur.cols.t[c];
      if (!same) continue;
      seen = seen || d.source == cur.input;
      const Query& q = app.queries[d.producer];
      DeriveProd& p = da.prod[da.nprod++];
      p.src = d.source;
      p.dst = d.stream;
      p.filter_prog = q.filter.off;
      p.terms = q.filter_terms;
      for (size_t c = 0; c < q.select.size(); ++c) {
        p.item_src[c] = q.select[c].src;
        p.item_prog[c] = q.select[c].prog.off;
      }
      da.ncols = (int)q.select.size();
      for (int c = 0; c < da.ncols; ++c) da.out_type[c] = q.select[c].type;
    }
    if (!seen || da.nprod == 0) continue;
    auto& bufs = stages[st - 1];
    // a caller column p is 256-byte aligned: p + row0 * w sits at (row0 * w) % 256
    auto place = [&](DevBuf* b, int w) -> char* {
      const size_t pad = (size_t)((cur.row0 * w) & 255);
      if (!dev_ensure(b, pad + (size_t)cur.n * w + 256, a->stream, false)) return nullptr;
      return (char*)b->p + pad - cur.row0 * w;
    };
    da.rows = cur;
    da.vm = {(const Ins*)a->code.p, (const uint64_t*)a->konst.p};
    da.err = (unsigned int*)a->err.p;
    da.stream_out = (uint8_t*)place(&bufs.stream, 1);
    if (!da.stream_out) return fail(a, CEP_E_DEVICE, "out of device memory (view)");
    // columns the term-list instance loads once per row
    bool vm = false, wide = false;
    da.npref = 0;
    for (int c = 0; c < kMaxCols; ++c) da.col_slot[c] = -1;
    auto slot_of = [&](int col) {
      for (int k = 0; k < da.npref; ++k)
        if (da.pcol[k] == col) return k;
      if (da.npref == kDerivePref) {
        wide = true;
        return 0;
      }
      da.pcol[da.npref] = col;
      da.col_slot[col] = da.npref;
      return da.npref++;
    };
    // a program the interpreter runs: every column it loads is prefetched
    auto prog_cols = [&](int off) {
      vm = true;
      for (int pc = off; pc >= 0 && pc < (int)app.code.size() && app.code[pc].op != OP_END; ++pc)
        if (app.code[pc].op == OP_LDCOL) slot_of((int)app.code[pc].imm);
    };
    for (int i = 0; i < da.nprod; ++i) {
      DeriveProd& p = da.prod[i];
      if (p.filter_prog >= 0 && p.terms.n < 0) prog_cols(p.filter_prog);
      for (int t = 0; t < std::max(0, p.terms.n); ++t) p.fslot[t] = slot_of(p.terms.t[t].col);
    }
    for (int c = 0; c < da.ncols; ++c) {
      bool alias = c < cur.cols.n && cur.cols.t[c] == da.out_type[c];
      for (int i = 0; i < da.nprod; ++i) alias = alias && da.prod[i].item_src[c] == SRC_REC + c;
      da.own_col[c] = (c < cur.cols.n && cur.cols.t[c] == da.out_type[c]) ? c : -1;
      da.own_slot[c] = -1;
      if (alias) continue;
      da.col_out[c] = place(&bufs.col[c], type_width(da.out_type[c]));
      if (!da.col_out[c]) return fail(a, CEP_E_DEVICE, "out of device memory (view)");
      if (da.own_col[c] >= 0) da.own_slot[c] = slot_of(da.own_col[c]);
      for (int i = 0; i < da.nprod; ++i) {
        const int src = da.prod[i].item_src[c];
        if (src >= SRC_REC && src < SRC_TS) da.prod[i].item_slot[c] = slot_of(src - SRC_REC);
        else prog_cols(da.prod[i].item_prog[c]);
      }
    }
    for (int k = da.npref; k < kDerivePref; ++k) da.pcol[k] = da.npref ? da.pcol[0] : 0;
    auto al = [&](const void* ptr, int w) {
      return (((uintptr_t)ptr + (uintptr_t)(cur.row0 * w)) & (uintptr_t)(w == 1 ? 7 : 15)) == 0;
    };
    bool vec = al(da.stream_out, 1) && (cur.stream ? al(cur.stream, 1) : true);
    for (int k = 0; k < da.npref; ++k) vec = vec && al(cur.cols.p[da.pcol[k]], type_width(cur.cols.t[da.pcol[k]]));
    for (int c = 0; c < da.ncols; ++c)
      if (da.col_out[c]) vec = vec && al(da.col_out[c], type_width(da.out_type[c]));
    da.vec = vec ? 1 : 0;
    {
      LaunchTimer t(a, CEP_K_OTHER);
      launch_derive(da, vm, wide, a->stream);
    }
    RowsArgs nx = cur;
    nx.stream = da.stream_out;
    nx.cols.n = da.ncols;
    for (int c = 0; c < da.ncols; ++c) {
      nx.cols.t[c] = da.out_type[c];
      nx.cols.p[c] = da.col_out[c] ? da.col_out[c] : cur.cols.p[c];
    }
    cur = nx;
  }
  *out = cur;
  return CEP_OK;
}

// One join over a device batch, chunk by chunk (join_kernels.hip).  The number
// of rows a chunk emits depends on the data (up to window size x rows), so it
// is read back (8 bytes, one sync per chunk) between the count and the emit
// pass and the output grows to hold exactly that.
int run_join(cep_app* a, JoinRT& rt, const RowsArgs& rows_in) {
  const Query& q = a->app.queries[rt.q];
  OutStream& o = a->outs[a->app.output_index(q.out_stream)];
  for (int64_t off = 0; off < rows_in.n; off += rt.chunk) {
    JoinArgs j = rt.ja;
    j.rows = rows_in;
    j.rows.row0 = rows_in.row0 + off;
    j.rows.n = std::min<int64_t>(rt.chunk, rows_in.n - off);
    j.vm = {(const Ins*)a->code.p, (const uint64_t*)a->konst.p};
    j.flag = (uint8_t*)rt.flag.p;
    j.bsum = (uint32_t*)rt.bsum.p;
    j.boff = (uint32_t*)rt.boff.p;
    for (int s = 0; s < 2; ++s) {
      j.list[s] = (uint64_t*)rt.list[s][rt.cur].p;
      j.next[s] = (uint64_t*)rt.list[s][rt.cur ^ 1].p;
      j.list_cap[s] = rt.list_cap[s];
    }
    j.probe = (uint64_t*)rt.probe.p;
    j.pcnt = (uint32_t*)rt.pcnt.p;
    j.pbsum = (uint32_t*)rt.pbsum.p;
    j.pboff = (uint32_t*)rt.pboff.p;
    j.st = (JoinState*)rt.st.p;
    j.err = (unsigned int*)a->err.p;
    j.out = out_args(o, q);
    {
      LaunchTimer t(a, CEP_K_JOIN);
      launch_join_mark(j, rt.mark_vm, a->stream);
    }
    {
      LaunchTimer t(a, CEP_K_JOIN);
      if (rt.on_vm) a->launches[CEP_K_JOIN_VM]++;
      launch_join_count(j, rt.on_vm, a->stream);
    }
    uint64_t* total = (uint64_t*)rt.total.p;
    if (hipMemcpyAsync(total, &((JoinState*)rt.st.p)->total, 8, hipMemcpyDeviceToHost, a->stream) != hipSuccess ||
        hipStreamSynchronize(a->stream) != hipSuccess)
      return fail(a, CEP_E_DEVICE, "device failure during processing (join)");
    if (*total > 0) {
      o.bound += (int64_t)*total;
      const int rc = ensure_out_cap(a, o, o.bound);
      if (rc) return rc;
      j.out = out_args(o, q);
      LaunchTimer t(a, CEP_K_JOIN);
      launch_join_emit(j, rt.on_vm, rt.sel_vm, a->stream);
    }
    {
      LaunchTimer t(a, CEP_K_JOIN);
      launch_join_tail(j, a->stream);
    }
    rt.cur ^= 1;
  }
  return CEP_OK;
}

// One table's operations over a device batch, chunk by chunk: k_partition (its
// N-state record form) on the side stream, k_tabwalk on the main stream,
// double-buffered arenas as in run_pattern.  A reader emits at most one row
// per row of its stream: the outputs are sized before the launch.
int run_table(cep_app* a, TableRT& rt, const RowsArgs& rows_all) {
  const TableDef& T = a->app.tables[rt.tab];
  if (!rows_all.stream && !((rt.pa.stream_mask >> rows_all.input) & 1)) return CEP_OK;   // no operation reads it
  if (rows_all.seq)
    return fail(a, CEP_E_UNSUPPORTED, "row shuffle of an app that holds a table is not supported");
  for (int j = 0; j < rt.ta.nops; ++j) {
    if (!rt.ta.op[j].reader) continue;
    const Query& q = a->app.queries[T.ops[j]];
    OutStream& o = a->outs[a->app.output_index(q.out_stream)];
    o.bound += rows_all.n;
    const int rc = ensure_out_cap(a, o, o.bound);
    if (rc) return rc;
  }
  const int P = 1 << rt.pa.buckets_log2;
  ChunkPipe& pipe = rt.pipe;
  hipStream_t side = pipe.open(a);
  for (int64_t r0 = 0; r0 < rows_all.n; r0 += pipe.chunk) {
    const int b = pipe.begin(side);
    RowsArgs rows = rows_all;
    rows.row0 = rows_all.row0 + r0;
    rows.n = std::min<int64_t>(pipe.chunk, rows_all.n - r0);
    rows.prev_ts = INT64_MIN;   // timestamps play no part: no order check
    rows.prev_ts_dev = nullptr;
    const int64_t ntiles = (rows.n + kPartThreads * kPartItems - 1) / (kPartThreads * kPartItems);
    PartArgs pa{};
    pa.rows = rows;
    pa.pref.n = -1;
    pa.vm = {(const Ins*)a->code.p, (const uint64_t*)a->konst.p};
    pa.pat = rt.pa;
    pa.tile_rows = kPartThreads * kPartItems;
    pa.recs = (uint64_t*)pipe.recs[b].p;
    pa.tile_off = (uint16_t*)pipe.tile_off[b].p;
    pa.chunk_base = (int64_t*)pipe.chunk_base[b].p;
    pa.err = (unsigned int*)a->err.p;
    {
      LaunchTimer t(a, CEP_K_PARTITION, side);
      launch_partition(pa, ntiles, true, side);   // (the N-state record form is the interpreter build's)
    }
    pipe.partitioned(b, side, a->stream);
    TabArgs ta = rt.ta;
    ta.vm = pa.vm;
    ta.pat = pa.pat;
    ta.recs = pa.recs;
    ta.tile_off = pa.tile_off;
    ta.ntiles = (int)ntiles;
    ta.tile_rows = pa.tile_rows;
    ta.chunk_base = pa.chunk_base;
    ta.thdr = (uint32_t*)rt.thdr.p;
    ta.tword = (uint64_t*)rt.tword.p;
    ta.kstride = rt.kstride;
    for (int j = 0; j < ta.nops; ++j) {
      if (!ta.op[j].reader) continue;
      const Query& q = a->app.queries[T.ops[j]];
      ta.out[j] = out_args(a->outs[a->app.output_index(q.out_stream)], q);
    }
    ta.dropped = (unsigned long long*)a->tab_dropped.p;
    ta.err = pa.err;
    {
      LaunchTimer t(a, CEP_K_TABLE);
      if (rt.vm) a->tab_vm_launches++;
      launch_tabwalk(ta, P, rt.vm, a->stream);
    }
    pipe.walked(b, a->stream);
  }
  return CEP_OK;
}

int send_device_rows(cep_app* a, const RowsArgs& rows_in) {
  // query chaining: each view is built once per slice, before its first reader
  std::vector<RowsArgs> views(a->app.views.size());
  std::vector<char> built(a->app.views.size(), 0);
  auto rows_of = [&](int view, const RowsArgs** r) -> int {
    *r = &rows_in;
    if (view < 0) return CEP_OK;
    if (!built[view]) {
      const int rc = build_view(a, view, rows_in, &views[view]);
      if (rc) return rc;
      built[view] = 1;
    }
    *r = &views[view];
    return CEP_OK;
  };
  for (auto& g : a->mqs) {
    const RowsArgs* r;
    int rc = rows_of(g.view, &r);
    if (!rc) rc = run_mq(a, g, *r);
    if (rc) return rc;
  }
  for (size_t qi = 0; qi < a->app.queries.size(); ++qi) {
    const Query& q = a->app.queries[qi];
    if (a->in_mq[qi]) continue;
    const RowsArgs* rp;
    int rc = rows_of(q.view, &rp);
    if (rc) return rc;
    const RowsArgs& rows = *rp;
    if (q.kind == Q_FILTER) {
      rc = run_filter(a, q, rows);
    } else if (q.kind == Q_PATTERN || q.kind == Q_AGG) {
      for (auto& rt : a->pats)
        if (rt.q == (int)qi) rc = run_pattern(a, rt, rows, nullptr, 0, a->force_tolerant);
    } else if (q.kind == Q_JOIN) {
      for (auto& rt : a->joins)
        if (rt.q == (int)qi) rc = run_join(a, rt, rows);
    } else if (q.kind == Q_TABLE) {
      // every operation of the table runs in one pipeline, at its first reader
      for (auto& rt : a->tabs)
        if (rt.run_at == (int)qi) rc = run_table(a, rt, rows);
    }
    if (rc) return rc;
  }
  // the batch's last ts: the next batch's first-row order check (device
  // batches; the host does not see their ts)
  const RowsArgs& rows = rows_in;
  if (rows.n > 0 && rows.prev_ts_dev)
    hipMemcpyAsync(a->last_ts_dev.p, rows.ts + rows.row0 + rows.n - 1, 8, hipMemcpyDeviceToDevice, a->stream);
  return CEP_OK;
}


int device_error(cep_app* a, unsigned int e);

int check_device_error(cep_app* a) {
  unsigned int e = 0;
  hipMemcpy(&e, a->err.p, sizeof(e), hipMemcpyDeviceToHost);
  return device_error(a, e);
}

int error_status(cep_app* a, unsigned int e);

// Error flags read back -> status (the flags are cleared).
int device_error(cep_app* a, unsigned int e) {
  if (!e) return CEP_OK;
  hipMemset(a->err.p, 0, 64);
  return error_status(a, e);
}

// Status of device error flags (the flags are not touched).
int error_status(cep_app* a, unsigned int e) {
  if (!e) return CEP_OK;
  if (e & ERR_ORDER)   // root cause first: out-of-order input also defeats `within` pruning
    return fail(a, CEP_E_ARG, "events not in event-time order: `within` requires non-decreasing timestamps "
                              "(so do group by with #window.time outside a partition and a join with #window.time)");
  // before the capacity flags: a time that did not fit its 32-bit field was
  // stored truncated, so partials and window rows stop expiring and the lists
  // overflow as a consequence
  if (e & ERR_TS_SPAN)
    return fail(a, CEP_E_ARG, "timestamps of one chunk lie more than 2^31 ms apart (lower chunk_events)");
  if (e & ERR_PENDING)
    return fail(a, CEP_E_CAPACITY, "per-key pending partial capacity exceeded (raise pending_slots)");
  if (e & ERR_POOL)
    return fail(a, CEP_E_CAPACITY, "pending overflow pool exhausted (raise pending_pool_log2)");
  if (e & ERR_KEYMAP)
    return fail(a, CEP_E_CAPACITY, "more distinct partition values than key_capacity (sparse_keys)");
  if (e & ERR_KEY_RANGE)
    return fail(a, CEP_E_CAPACITY, "partition key outside [0, key_capacity) or not owned by this shard");
  if (e & ERR_SHUFFLE_CAP)
    return fail(a, CEP_E_CAPACITY,
                "padded key shuffle: an owner's records overflowed the padded segment (seg_cap) and, with "
                "a spill buffer, the spill (spill_cap) too; the excess records were dropped (raise seg_cap / "
                "spill_cap or use the two-phase exchange)");
  if (e & ERR_DERIVE)
    return fail(a, CEP_E_UNSUPPORTED, "a row passed the filters of two derived streams that one query reads "
                                      "(it would be two events of that query; make the producers' filters disjoint)");
  if (e & ERR_JOIN_TAIL)
    return fail(a, CEP_E_CAPACITY, "a join's #window.time held more than " + std::to_string(kJoinTailCap) +
                                       " live rows at the end of a chunk (the oldest were dropped)");
  if (e & ERR_OUT_CAP) return fail(a, CEP_E_DEVICE, "output capacity exceeded");
  return fail(a, CEP_E_DEVICE, "device error flags " + std::to_string(e));
}

}  // namespace cep

// ======================================================================= C ABI
extern "C" {

void cep_default_options(cep_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->device = 0;
  o->pending_slots = 16;
  o->key_capacity = 1 << 20;
  o->chunk_events = 1 << 22;
  o->buckets_log2 = 10;
  o->profile = 0;
  o->ordered_output = 1;
  o->key_stride = 1;
  o->key_offset = 0;
  o->pending_pool_log2 = 20;
  o->late_policy = 2;
  o->ts_order = 0;
}

int cep_validate(const char* plan, char* err, size_t errlen) {
  if (!plan) {
    set_err(err, errlen, "plan is null");
    return CEP_E_ARG;
  }
  CompiledApp app;
  std::string m;
  int rc = compile_app(plan, &app, &m);
  if (rc) set_err(err, errlen, m);
  else set_err(err, errlen, "");
  return rc;
}

int cep_plan_schema(const char* plan, const char* stream_id, cep_attr* out, int cap, int* n,
                    char* err, size_t errlen) {
  if (!plan || !stream_id) {
    set_err(err, errlen, "null argument");
    return CEP_E_ARG;
  }
  CompiledApp app;
  std::string m;
  int rc = compile_app(plan, &app, &m);
  if (rc) {
    set_err(err, errlen, m);
    return rc;
  }
  const StreamSchema* s = nullptr;
  int i = app.input_index(stream_id);
  if (i >= 0) s = &app.inputs[i];
  i = app.output_index(stream_id);
  if (!s && i >= 0) s = &app.outputs[i];
  if (!s) {
    set_err(err, errlen, std::string("Unknown stream id ") + stream_id);
    return CEP_E_UNDEFINED_STREAM;
  }
  return fill_attrs(s, out, cap, n);
}

cep_app* cep_create(const char* plan, const cep_options* opt, char* err, size_t errlen) {
  return cep::create_app(plan, opt, nullptr, err, errlen);
}

}  // extern "C"

cep_app* cep::create_app(const char* plan, const cep_options* opt, const std::vector<std::string>* dict_seed,
                         char* err, size_t errlen) {
  if (!plan) {
    set_err(err, errlen, "plan is null");
    return nullptr;
  }
  auto* a = new cep_app();
  if (opt) a->opt = *opt;
  else cep_default_options(&a->opt);
  if (a->opt.key_stride <= 0) a->opt.key_stride = 1;
  std::string m;
  int rc = compile_app(plan, &a->app, &m, dict_seed);
  if (rc) {
    set_err(err, errlen, m);
    delete a;
    return nullptr;
  }
  // pending_slots sizes the walks' LDS lists (kMaxPending); an app whose only
  // per-key lists are #window.time rings (HBM) may ask for up to kWinMaxRing
  bool has_pattern = false, has_window = false;
  for (auto& q : a->app.queries) {
    has_pattern |= q.kind == Q_PATTERN;
    has_window |= q.win_kind == WIN_LENGTH || q.win_kind == WIN_TIME;   // (a batch window keeps no ring)
  }
  const int max_pending = (has_window && !has_pattern) ? kWinMaxRing : kMaxPending;
  if (a->opt.pending_slots <= 0 || a->opt.pending_slots > max_pending) {
    set_err(err, errlen, "pending_slots must be in [1, " + std::to_string(max_pending) + "]");
    delete a;
    return nullptr;
  }
  for (auto& s : a->app.strings) cep_dict_intern(a, s.c_str());
  rc = create_runtime(a);
  if (rc) {
    set_err(err, errlen, a->last_error);
    cep_destroy(a);
    return nullptr;
  }
  set_err(err, errlen, "");
  return a;
}

extern "C" {

void cep_destroy(cep_app* a) {
  if (!a) return;
  // every stream idle before anything is freed (the members' destructors free;
  // their order is documented at cep_app)
  for (hipStream_t s : {a->stream.h, a->copy.h, a->side.h, a->rstream.h})
    if (s) hipStreamSynchronize(s);
  dump_stamps(a);
  harvest_timers(a);
  delete a;
}

int cep_stream_schema(cep_app* a, const char* stream_id, cep_attr* out, int cap, int* n) {
  if (!a) return CEP_E_ARG;
  const StreamSchema* s = find_schema(a, stream_id);
  if (!s) return fail(a, CEP_E_UNDEFINED_STREAM, std::string("Stream ") + (stream_id ? stream_id : "(null)") + " not defined");
  return fill_attrs(s, out, cap, n);
}

int cep_input(cep_app* a, const char* stream_id) {
  if (!a || !stream_id) return -CEP_E_ARG;
  int i = a->app.input_index(stream_id);
  if (i < 0) {
    fail(a, CEP_E_UNDEFINED_STREAM, std::string("Stream ") + stream_id + " not defined");
    return -CEP_E_UNDEFINED_STREAM;
  }
  return i;
}

int cep_set_callback(cep_app* a, const char* out_id, cep_emit_fn fn, void* user) {
  if (!a || !out_id) return CEP_E_ARG;
  int i = a->app.output_index(out_id);
  if (i < 0) return fail(a, CEP_E_UNDEFINED_STREAM, std::string("Stream ") + out_id + " not defined");
  a->outs[i].fn = fn;
  a->outs[i].user = user;
  return CEP_OK;
}

}  // extern "C"

namespace cep {

// Batch -> device rows (host batches are staged into device memory: the
// PCIe-inclusive path).  Validates the handle and the column count.
// *slot: the host staging slot the batch went to (-1: device batch);
// *direct: its columns are DMA'd straight from pinned caller memory.
int batch_rows(cep_app* a, const cep_batch* b, RowsArgs* out, int* slot, bool* direct) {
  *slot = -1;
  *direct = false;
  if (b->n < 0 || (b->n > 0 && !b->ts)) return fail(a, CEP_E_ARG, "bad batch");
  if (b->input < 0 || b->input >= (int)a->app.inputs.size())
    return fail(a, CEP_E_UNDEFINED_STREAM, "undefined input handle");
  const StreamSchema& sd = a->app.inputs[b->input];
  if (b->ncols != (int)sd.attrs.size() || b->ncols > kMaxCols)
    return fail(a, CEP_E_ARG, "batch has " + std::to_string(b->ncols) + " columns, stream " +
                                  sd.id + " defines " + std::to_string(sd.attrs.size()));
  RowsArgs rows{};
  rows.cols.n = b->ncols;
  for (int c = 0; c < b->ncols; ++c) rows.cols.t[c] = sd.attrs[c].type;
  rows.input = b->input;
  rows.row0 = 0;
  rows.n = b->n;
  rows.seq0 = a->events_in;
  rows.prev_ts = a->last_ts;
  rows.prev_ts_dev = (const int64_t*)a->last_ts_dev.p;
  if (b->on_device) {
    for (int c = 0; c < b->ncols; ++c) rows.cols.p[c] = b->cols[c];
    rows.ts = b->ts;
    rows.stream = b->stream;
    // cross-batch order checks would need a sync to read the last ts; the
    // in-batch check covers the hot path
    a->last_ts = INT64_MIN;
  } else {
    // One staging slot holds the whole batch (columns, ts, stream; 256-B
    // aligned pieces).  Pinned caller buffers are DMA'd directly; pageable
    // ones are first copied by the CPU into the slot's pinned arena (that
    // copy is the batch's consumption: the call returns without waiting for
    // the device).  The DMA waits for the kernels that last read the slot.
    auto& h = a->hs[a->hs_next];
    *slot = a->hs_next;
    a->hs_next ^= 1;
    if (!h.dma_done && (!h.dma_done.create() || !h.free.create()))
      return fail(a, CEP_E_DEVICE, "hipEventCreate failed");
    const int nc = b->ncols;
    size_t off[kMaxCols + 2], len[kMaxCols + 2];
    const void* src[kMaxCols + 2];
    size_t total = 0;
    auto piece = [&](int i, const void* p, size_t bytes) {
      off[i] = total;
      len[i] = bytes;
      src[i] = p;
      total += (bytes + 255) & ~(size_t)255;
    };
    for (int c = 0; c < nc; ++c) piece(c, b->cols[c], (size_t)b->n * type_width(sd.attrs[c].type));
    piece(nc, b->ts, (size_t)b->n * 8);
    piece(nc + 1, b->stream, b->stream ? (size_t)b->n : 0);
    bool pinned = true;
    for (int i = 0; i < nc + 2 && pinned; ++i) pinned = !len[i] || is_pinned(src[i]);
    // the slot's previous DMA (two batches ago) must be done before its
    // pinned arena or device arena is rewritten
    if (h.used) hipEventSynchronize(h.dma_done);
    if (h.dev.bytes < total) {
      if (h.used) hipStreamSynchronize(a->stream);   // the old arena may still be read
      if (!dev_ensure(&h.dev, total, a->stream, false))
        return fail(a, CEP_E_DEVICE, "out of device memory (staging)");
    }
    if (!pinned) {
      if (!host_ensure(&h.pinned, total)) return fail(a, CEP_E_DEVICE, "out of pinned host memory");
      for (int i = 0; i < nc + 2; ++i)
        if (len[i]) std::memcpy((char*)h.pinned.p + off[i], src[i], len[i]);
    }
    if (h.used) hipStreamWaitEvent(a->copy, h.free, 0);   // kernels done with the device arena
    if (!pinned) {
      hipMemcpyAsync(h.dev.p, h.pinned.p, total, hipMemcpyHostToDevice, a->copy);
    } else {
      for (int i = 0; i < nc + 2; ++i)
        if (len[i]) hipMemcpyAsync((char*)h.dev.p + off[i], src[i], len[i], hipMemcpyHostToDevice, a->copy);
    }
    hipEventRecord(h.dma_done, a->copy);
    hipStreamWaitEvent(a->stream, h.dma_done, 0);
    h.used = true;
    *direct = pinned;
    for (int c = 0; c < nc; ++c) rows.cols.p[c] = (char*)h.dev.p + off[c];
    rows.ts = (const int64_t*)((char*)h.dev.p + off[nc]);
    rows.stream = b->stream ? (const uint8_t*)((char*)h.dev.p + off[nc + 1]) : nullptr;
    a->last_ts = b->ts[b->n - 1];
  }
  *out = rows;
  return CEP_OK;
}

}  // namespace cep

extern "C" {

int cep_send_batch(cep_app* a, const cep_batch* b) {
  if (!a || !b) return CEP_E_ARG;
  if (!a->enabled) return CEP_OK;   // AbstractSiddhiOperator.java:128
  if (b->n == 0) return CEP_OK;
  RowsArgs rows{};
  int slot;
  bool direct;
  int rc = batch_rows(a, b, &rows, &slot, &direct);
  if (rc) return rc;
  a->events_in += b->n;
  a->batches++;
  rc = send_device_rows(a, rows);
  if (slot >= 0) {
    hipEventRecord(a->hs[slot].free, a->stream);
    // caller's pinned buffers: consumed once their DMA is done (the kernels
    // keep running); pageable buffers were consumed by the staging memcpy
    if (direct) hipEventSynchronize(a->hs[slot].dma_done);
  }
  return rc;
}

// ---- event-time reorder (AbstractSiddhiOperator.java:222-231 processElement
// offers to the PriorityQueue; :238-247 processWatermark drains ts <= mark)
int cep_buffer_batch(cep_app* a, const cep_batch* b) {
  if (!a || !b || b->n < 0) return CEP_E_ARG;
  if (b->n == 0) return CEP_OK;
  if (b->input < 0 || b->input >= (int)a->app.inputs.size())
    return fail(a, CEP_E_UNDEFINED_STREAM, "undefined input handle");
  const StreamSchema& sd = a->app.inputs[b->input];
  if (b->ncols != (int)sd.attrs.size() || b->ncols > kMaxCols)
    return fail(a, CEP_E_ARG, "batch has " + std::to_string(b->ncols) + " columns, stream " + sd.id +
                                  " defines " + std::to_string(sd.attrs.size()));
  auto& r = a->ro;
  if (r.n > 0 && (r.input != b->input || r.has_stream != (b->stream != nullptr)))
    return fail(a, CEP_E_ARG, "the reorder buffer holds rows of another input layout: call cep_watermark first");
  if (r.n + b->n > (int64_t)INT32_MAX) return fail(a, CEP_E_CAPACITY, "reorder buffer holds at most 2^31-1 rows");
  r.input = b->input;
  r.has_stream = b->stream != nullptr;
  const int64_t need = r.n + b->n;
  const hipMemcpyKind kind = b->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  bool ok = true;
  for (int c = 0; c < b->ncols && ok; ++c) {
    const int w = type_width(sd.attrs[c].type);
    ok = dev_ensure(&r.col[c], (size_t)need * w, a->stream, true);
    if (ok) hipMemcpyAsync((char*)r.col[c].p + r.n * w, b->cols[c], (size_t)b->n * w, kind, a->stream);
  }
  ok = ok && dev_ensure(&r.ts, (size_t)need * 8, a->stream, true);
  if (ok) hipMemcpyAsync((char*)r.ts.p + r.n * 8, b->ts, (size_t)b->n * 8, kind, a->stream);
  if (ok && b->stream) {
    ok = dev_ensure(&r.stream, (size_t)need, a->stream, true);
    if (ok) hipMemcpyAsync((char*)r.stream.p + r.n, b->stream, (size_t)b->n, kind, a->stream);
  }
  if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (reorder buffer)");
  r.n = need;
  if (!b->on_device) hipStreamSynchronize(a->stream);   // host buffers may be reused
  return CEP_OK;
}

int64_t cep_buffered(cep_app* a) { return a ? a->ro.n : -1; }

int cep_watermark(cep_app* a, int64_t mark) {
  if (!a) return CEP_E_ARG;
  auto& r = a->ro;
  if (r.n == 0) return CEP_OK;
  const StreamSchema& sd = a->app.inputs[r.input];
  const int nc = (int)sd.attrs.size();
  const int64_t n = r.n;
  const size_t tb = reorder_temp_bytes(n);
  if (!dev_ensure(&r.keys, (size_t)n * 8, a->stream, false) ||
      !dev_ensure(&r.idx_in, (size_t)n * 4, a->stream, false) ||
      !dev_ensure(&r.idx_out, (size_t)n * 4, a->stream, false) || !dev_ensure(&r.temp, tb + 16, a->stream, false) ||
      !dev_ensure(&r.bound, 64, a->stream, false))
    return fail(a, CEP_E_DEVICE, "out of device memory (reorder sort)");
  if (reorder_sort(r.temp.p, r.temp.bytes, (const int64_t*)r.ts.p, (int64_t*)r.keys.p, (int32_t*)r.idx_in.p,
                   (int32_t*)r.idx_out.p, n, a->stream))
    return fail(a, CEP_E_DEVICE, "reorder sort failed");
  launch_upper_bound((const int64_t*)r.keys.p, n, mark, (int64_t*)r.bound.p, a->stream);
  // rows older than one already released (late events) sort first: count them
  const bool any_released = r.released_max != INT64_MIN;
  if (any_released)
    launch_upper_bound((const int64_t*)r.keys.p, n, r.released_max - 1, (int64_t*)r.bound.p + 3, a->stream);
  int64_t hb[6] = {0, 0, 0, 0, 0, 0};
  if (hipMemcpyAsync(hb, r.bound.p, sizeof(hb), hipMemcpyDeviceToHost, a->stream) != hipSuccess ||
      hipStreamSynchronize(a->stream) != hipSuccess)
    return fail(a, CEP_E_DEVICE, "device failure during processing");
  const int64_t rel = hb[0];
  if (rel == 0) return CEP_OK;
  // A row older than an earlier watermark's release arrived late.  The
  // reference offers it to its PriorityQueue like any row, and this
  // watermark's drain hands it to Siddhi first (smallest ts), behind rows it
  // has already processed (AbstractSiddhiOperator.java:222-231, 238-245).
  // late_policy 2 (default) does the same: the released prefix, late rows
  // included, in (ts, arrival) order, on the order-tolerant path.  Policies
  // 0 / 1 drop them (counted in cep_stats.late_events).
  const int64_t late_n = any_released ? std::min(hb[3], rel) : 0;
  const bool deliver_late = a->opt.late_policy == 2;
  // ts_order 1 promises non-decreasing ts to the event-time fast paths, whose
  // state is not the oracle's once a late row can follow: they prune partials
  // at A arrivals and never see g-failing B's, and App. A.3 lets a late B
  // complete a partial that such pruning removed (or that a g-failing B would
  // have expired).  Delivering late rows there would be inexact, so the
  // release is refused before anything is consumed (the rows stay buffered);
  // ts_order 0 delivers them exactly.
  if (deliver_late && late_n > 0 && a->opt.ts_order == 1) {
    bool sensitive = false;
    for (auto& rt : a->pats) sensitive = sensitive || rt.order_sensitive;
    if (sensitive)
      return fail(a, CEP_E_ARG, std::to_string(late_n) + " late event(s) with ts_order 1: a `within` pattern's "
                                "event-time state cannot take them exactly (use ts_order 0, or late_policy 0 / 1 "
                                "to drop them)");
  }
  a->late_events += late_n;
  const int64_t late = deliver_late ? 0 : late_n;   // rows dropped from the release
  const int32_t* perm = (const int32_t*)r.idx_out.p;
  bool ok = true;
  for (int c = 0; c < nc && ok; ++c) {
    const int w = type_width(sd.attrs[c].type);
    ok = dev_ensure(&r.out[c], (size_t)n * w, a->stream, false);
    if (ok) launch_gather(r.col[c].p, r.out[c].p, perm, 0, n, w, a->stream);
  }
  ok = ok && dev_ensure(&r.ots, (size_t)n * 8, a->stream, false);
  if (ok) hipMemcpyAsync(r.ots.p, r.keys.p, (size_t)n * 8, hipMemcpyDeviceToDevice, a->stream);
  if (ok && r.has_stream) {
    ok = dev_ensure(&r.ostream, (size_t)n, a->stream, false);
    if (ok) launch_gather(r.stream.p, r.ostream.p, perm, 0, n, 1, a->stream);
  }
  if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (reorder gather)");
  // the held-back rows stay buffered, now in (ts, arrival) order
  const int64_t keep = n - rel;
  for (int c = 0; c < nc; ++c) {
    const int w = type_width(sd.attrs[c].type);
    hipMemcpyAsync(r.col[c].p, (char*)r.out[c].p + rel * w, (size_t)keep * w, hipMemcpyDeviceToDevice, a->stream);
  }
  hipMemcpyAsync(r.ts.p, (char*)r.ots.p + rel * 8, (size_t)keep * 8, hipMemcpyDeviceToDevice, a->stream);
  if (r.has_stream)
    hipMemcpyAsync(r.stream.p, (char*)r.ostream.p + rel, (size_t)keep, hipMemcpyDeviceToDevice, a->stream);
  r.n = keep;
  const int input = r.input;
  if (keep == 0) r.input = -1;
  // the released prefix minus the late rows is a device batch in event-time order
  const void* cols[kMaxCols];
  for (int c = 0; c < nc; ++c) cols[c] = (const char*)r.out[c].p + late * type_width(sd.attrs[c].type);
  cep_batch bb{};
  bb.n = rel - late;
  bb.ts = (const int64_t*)r.ots.p + late;
  bb.stream = r.has_stream ? (const uint8_t*)r.ostream.p + late : nullptr;
  bb.input = input;
  bb.ncols = nc;
  bb.cols = cols;
  bb.on_device = 1;
  a->last_ts = r.released_max;   // the kernel's order check spans the watermark
  const int64_t rmax = hb[2];
  a->force_tolerant = deliver_late && late_n > 0;
  int rc = cep_send_batch(a, &bb);
  a->force_tolerant = false;
  if (rc == CEP_OK) r.released_max = std::max(r.released_max, rmax);
  // the sorted batch buffers are reused by the next watermark: finish first
  hipStreamSynchronize(a->stream);
  if (rc == CEP_OK && late > 0 && a->opt.late_policy == 1)
    return fail(a, CEP_E_ARG, std::to_string(late) + " late event(s) dropped (older than rows an earlier watermark "
                              "released; the reference would hand them to Siddhi out of order)");
  return rc;
}

int cep_flush(cep_app* a) {
  if (!a) return CEP_E_ARG;
  // the error word, every output cursor and (ordered_output) every delivered
  // output's seq range / descents in one pinned readback, one sync
  const size_t no = a->outs.size();
  const bool order = a->opt.ordered_output != 0;
  if (!host_ensure(&a->flush_words, (no * 4 + 1) * 8)) return fail(a, CEP_E_DEVICE, "out of pinned host memory");
  uint64_t* fw = (uint64_t*)a->flush_words.p;
  uint64_t* fst = fw + 1 + no;   // 3 words per output
  fw[0] = 0;
  if (order) {
    if (!dev_ensure(&a->ostats, no * 3 * 8, a->stream, false)) return fail(a, CEP_E_DEVICE, "out of device memory");
    hipMemsetAsync(a->ostats.p, 0, no * 3 * 8, a->stream);
    for (size_t i = 0; i < no; ++i)
      if (a->outs[i].fn)
        launch_seq_stats((const int64_t*)a->outs[i].seq.p, a->outs[i].count, a->outs[i].cap,
                         (unsigned long long*)a->ostats.p + 3 * i, a->stream);
  }
  hipMemcpyAsync(fw, a->err.p, 4, hipMemcpyDeviceToHost, a->stream);
  if (no) hipMemcpyAsync(fw + 1, a->out_counts.p, no * 8, hipMemcpyDeviceToHost, a->stream);
  if (order) hipMemcpyAsync(fst, a->ostats.p, no * 3 * 8, hipMemcpyDeviceToHost, a->stream);
  if (hipStreamSynchronize(a->stream) != hipSuccess)
    return fail(a, CEP_E_DEVICE, "device failure during processing");
  harvest_timers(a);
  int rc = device_error(a, (unsigned int)fw[0]);
  // an output cursor past its capacity is a hard failure before any count
  // is used (the rows beyond cap were never written)
  for (size_t i = 0; i < no; ++i) {
    auto& o = a->outs[i];
    const unsigned long long cnt = fw[1 + i];
    if (cnt > (unsigned long long)o.cap && rc == CEP_OK)
      rc = fail(a, CEP_E_DEVICE, "output capacity exceeded on " + o.id + ": " + std::to_string(cnt) +
                                     " rows > " + std::to_string(o.cap));
  }
  // Rows of every output are consumed by this flush, delivered or not: a
  // failure part-way stops delivery, records the first error and still resets
  // every cursor below, so a later flush never hands the same rows out again.
  const bool want_seq = !a->opt.omit_seq;
  auto deliver = [&](OutStream& o, size_t i, size_t n) -> int {
    const void* src_ts = o.ts.p;
    const void* src_seq = o.seq.p;
    std::vector<const void*> src(o.cols.size());
    for (size_t c = 0; c < o.cols.size(); ++c) src[c] = o.cols[c].p;
    if (order && fst[3 * i + 2] > 0) {
      // Siddhi's emission order (StreamOutputHandler.java:63-92 receives
      // each completing event's matches in turn): by completing event, then
      // pending order, which the walk already keeps contiguous per key — a
      // stable sort on seq over the window's seq range, then one gather
      // per column, all on the device.
      if (n > (size_t)INT32_MAX) return fail(a, CEP_E_DEVICE, "too many rows to order in one flush");
      const uint64_t bias = 0x8000000000000000ull;
      const int64_t lo = (int64_t)(~fst[3 * i] ^ bias), hi = (int64_t)(fst[3 * i + 1] ^ bias);
      const uint64_t range = (uint64_t)hi - (uint64_t)lo;
      const int bits = range ? 64 - __builtin_clzll(range) : 1;
      const size_t tb = order_temp_bytes((int64_t)n);
      bool ok = dev_ensure(&a->okeys[0], n * 8, a->stream, false) && dev_ensure(&a->okeys[1], n * 8, a->stream, false) &&
                dev_ensure(&a->oidx[0], n * 4, a->stream, false) && dev_ensure(&a->oidx[1], n * 4, a->stream, false) &&
                dev_ensure(&a->otemp, tb, a->stream, false) && dev_ensure(&o.sts, n * 8, a->stream, false) &&
                (!want_seq || dev_ensure(&o.sseq, n * 8, a->stream, false));
      o.scols.resize(o.cols.size());
      for (size_t c = 0; c < o.cols.size() && ok; ++c)
        ok = dev_ensure(&o.scols[c], n * type_width(o.types[c]), a->stream, false);
      if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (output ordering)");
      if (order_sort(a->otemp.p, a->otemp.bytes, (const int64_t*)o.seq.p, (int64_t)n, lo, bits, a->okeys[0].p,
                     a->okeys[1].p, (int32_t*)a->oidx[0].p, (int32_t*)a->oidx[1].p, a->stream) != 0)
        return fail(a, CEP_E_DEVICE, "output ordering sort failed");
      const int32_t* perm = (const int32_t*)a->oidx[1].p;
      for (size_t c = 0; c < o.cols.size(); ++c) {
        launch_gather(o.cols[c].p, o.scols[c].p, perm, 0, (int64_t)n, type_width(o.types[c]), a->stream);
        src[c] = o.scols[c].p;
      }
      launch_gather(o.ts.p, o.sts.p, perm, 0, (int64_t)n, 8, a->stream);
      src_ts = o.sts.p;
      if (want_seq) {
        launch_gather(o.seq.p, o.sseq.p, perm, 0, (int64_t)n, 8, a->stream);
        src_seq = o.sseq.p;
      }
    }
    // one async D2H per column into pinned buffers, one sync; the seq column
    // only when the consumer reads it (cep_options.omit_seq)
    o.hcols.resize(o.cols.size());
    bool ok = host_ensure(&o.hts, n * 8) && (!want_seq || host_ensure(&o.hseq, n * 8));
    for (size_t c = 0; c < o.cols.size() && ok; ++c) ok = host_ensure(&o.hcols[c], n * type_width(o.types[c]));
    if (!ok) return fail(a, CEP_E_DEVICE, "out of pinned host memory (output delivery)");
    hipMemcpyAsync(o.hts.p, src_ts, n * 8, hipMemcpyDeviceToHost, a->stream);
    if (want_seq) hipMemcpyAsync(o.hseq.p, src_seq, n * 8, hipMemcpyDeviceToHost, a->stream);
    for (size_t c = 0; c < o.cols.size(); ++c)
      hipMemcpyAsync(o.hcols[c].p, src[c], n * type_width(o.types[c]), hipMemcpyDeviceToHost, a->stream);
    if (hipStreamSynchronize(a->stream) != hipSuccess) return fail(a, CEP_E_DEVICE, "output delivery failed");
    std::vector<const void*> ptrs(o.cols.size());
    for (size_t c = 0; c < o.cols.size(); ++c) ptrs[c] = o.hcols[c].p;
    cep_rows rows{};
    rows.stream_id = o.id.c_str();
    rows.n = (int64_t)n;
    rows.ncols = (int32_t)o.cols.size();
    rows.ts = (const int64_t*)o.hts.p;
    rows.seq = want_seq ? (const int64_t*)o.hseq.p : nullptr;
    rows.cols = ptrs.data();
    o.fn(o.user, &rows);
    return CEP_OK;
  };
  if (a->seq_poison && rc == CEP_OK) {
    for (size_t i = 0; i < no && rc == CEP_OK; ++i) {
      const auto& o = a->outs[i];
      if (o.write_seq || o.cap == 0) continue;
      std::vector<uint64_t> h((size_t)o.cap);
      hipMemcpy(h.data(), o.seq.p, h.size() * 8, hipMemcpyDeviceToHost);
      for (size_t j = 0; j < h.size(); ++j)
        if (h[j] != 0xa5a5a5a5a5a5a5a5ull) {
          rc = fail(a, CEP_E_DEVICE, "a kernel stored arrival numbers of " + o.id + " (row " + std::to_string(j) +
                                         ") although write_seq is 0");
          break;
        }
    }
  }
  for (size_t i = 0; i < no; ++i) {
    auto& o = a->outs[i];
    const unsigned long long cnt = rc == CEP_OK ? fw[1 + i] : 0ull;
    a->matches_out += (int64_t)cnt;
    if (o.fn && cnt > 0 && rc == CEP_OK) rc = deliver(o, i, (size_t)cnt);
    o.bound = 0;
  }
  if (no) hipMemsetAsync(a->out_counts.p, 0, no * 8, a->stream);
  return rc;
}

int cep_output_device(cep_app* a, const char* out_id, cep_rows* rows) {
  if (!a || !out_id || !rows) return CEP_E_ARG;
  int i = a->app.output_index(out_id);
  if (i < 0) return fail(a, CEP_E_UNDEFINED_STREAM, std::string("Stream ") + out_id + " not defined");
  if (hipStreamSynchronize(a->stream) != hipSuccess) return fail(a, CEP_E_DEVICE, "device failure");
  harvest_timers(a);
  int rc = check_device_error(a);
  if (rc) return rc;
  OutStream& o = a->outs[i];
  unsigned long long cnt = 0;
  hipMemcpy(&cnt, o.count, sizeof(cnt), hipMemcpyDeviceToHost);
  if (cnt > (unsigned long long)o.cap)
    return fail(a, CEP_E_DEVICE, "output capacity exceeded on " + o.id);
  static thread_local std::vector<const void*> ptrs;
  ptrs.assign(o.cols.size(), nullptr);
  for (size_t c = 0; c < o.cols.size(); ++c) ptrs[c] = o.cols[c].p;
  rows->stream_id = o.id.c_str();
  rows->n = (int64_t)cnt;
  rows->ncols = (int32_t)o.cols.size();
  rows->ts = (const int64_t*)o.ts.p;
  // omit_seq with unordered output: the kernels need not write them
  rows->seq = (a->opt.omit_seq && !a->opt.ordered_output) ? nullptr : (const int64_t*)o.seq.p;
  rows->cols = ptrs.data();
  return CEP_OK;
}

int cep_reset_output(cep_app* a) {
  if (!a) return CEP_E_ARG;
  for (auto& o : a->outs) {
    hipMemsetAsync(o.count, 0, sizeof(unsigned long long), a->stream);
    o.bound = 0;
  }
  return CEP_OK;
}

int cep_stream_wait(cep_app* a, void* hip_stream) {
  if (!a) return CEP_E_ARG;
  if (hipEventRecord(a->ext_ready, (hipStream_t)hip_stream) != hipSuccess ||
      hipStreamWaitEvent(a->stream, a->ext_ready, 0) != hipSuccess ||
      hipStreamWaitEvent(a->rstream, a->ext_ready, 0) != hipSuccess)
    return fail(a, CEP_E_DEVICE, "cep_stream_wait: invalid stream");
  return CEP_OK;
}

int cep_stream_signal(cep_app* a, void* hip_stream) {
  if (!a) return CEP_E_ARG;
  if (hipEventRecord(a->out_ready, a->stream) != hipSuccess ||
      hipStreamWaitEvent((hipStream_t)hip_stream, a->out_ready, 0) != hipSuccess ||
      hipEventRecord(a->r_ready, a->rstream) != hipSuccess ||
      hipStreamWaitEvent((hipStream_t)hip_stream, a->r_ready, 0) != hipSuccess)
    return fail(a, CEP_E_DEVICE, "cep_stream_signal: invalid stream");
  return CEP_OK;
}

int cep_route_signal(cep_app* a, void* hip_stream) {
  if (!a) return CEP_E_ARG;
  if (hipEventRecord(a->r_ready, a->rstream) != hipSuccess ||
      hipStreamWaitEvent((hipStream_t)hip_stream, a->r_ready, 0) != hipSuccess)
    return fail(a, CEP_E_DEVICE, "cep_route_signal: invalid stream");
  return CEP_OK;
}

int cep_set_enabled(cep_app* a, int enabled) {
  if (!a) return CEP_E_ARG;
  a->enabled = enabled != 0;
  return CEP_OK;
}

int32_t cep_dict_intern(cep_app* a, const char* s) {
  if (!a || !s) return -1;
  auto it = a->dict_index.find(s);
  if (it != a->dict_index.end()) return it->second;
  int32_t id = (int32_t)a->dict.size();
  a->dict.push_back(s);
  a->dict_index.emplace(s, id);
  return id;
}

const char* cep_dict_lookup(cep_app* a, int32_t id) {
  if (!a || id < 0 || id >= (int32_t)a->dict.size()) return nullptr;
  return a->dict[id].c_str();
}

int cep_stats(cep_app* a, cep_stats_t* s) {
  if (!a || !s) return CEP_E_ARG;
  hipStreamSynchronize(a->stream);
  harvest_timers(a);
  std::memset(s, 0, sizeof(*s));
  s->events_in = a->events_in;
  s->matches_out = a->matches_out;
  s->batches = a->batches;
  s->late_events = a->late_events;
  for (auto& p : a->pats)
    if (p.hot) s->hot_keys += *(volatile uint32_t*)p.hot_active_host.p;
  s->table_vm_launches = a->tab_vm_launches;
  if (a->tab_dropped.p) {
    unsigned long long d = 0;
    hipMemcpy(&d, a->tab_dropped.p, 8, hipMemcpyDeviceToHost);
    s->table_dropped = (int64_t)d;
  }
  for (int i = 0; i < 16; ++i) {
    s->kernel_launches[i] = a->launches[i];
    s->kernel_ms[i] = a->kernel_ms[i];
    s->kernel_timed[i] = a->kernel_timed[i];
  }
  return CEP_OK;
}

const char* cep_last_error(cep_app* a) { return a ? a->last_error.c_str() : "null app"; }

void cep_free(void* p) { std::free(p); }

}  // extern "C"

// Snapshots: the byte format and its validation live in snapshot.h /
// snapshot.cpp; here device state is pulled into, or committed from, a SnapImage.
static SnapGeometry snap_geometry(cep_app* a) {
  SnapGeometry g;
  g.plan_hash = plan_hash(a->app);
  g.hdr_ovf = kHdrOvf;
  g.join_tail_cap = kJoinTailCap;
  for (auto& rt : a->pats)
    g.pats.push_back({rt.pa.key_capacity, rt.kstride, rt.pool_cap, rt.pa.buckets_log2, (uint32_t)rt.pa.pending_slots,
                      (uint32_t)rt.pa.slot_words, rt.kext.p != nullptr, rt.sparse, rt.table_cap});
  for (auto& m : a->mqs) g.groups.push_back({m.key_capacity, m.kstride, m.lg, m.kpb, (uint32_t)m.words});
  for (auto& jr : a->joins)
    g.joins.push_back({(uint32_t)jr.ja.ew, {jr.ja.win_kind[0], jr.ja.win_kind[1]}, {jr.ja.win_param[0], jr.ja.win_param[1]}});
  for (auto& tr : a->tabs)
    g.tabs.push_back({tr.pa.key_capacity, tr.kstride, tr.pa.buckets_log2, (uint32_t)tr.ta.nwords});
  for (auto& in : a->app.inputs) {
    g.inputs.emplace_back();
    for (auto& at : in.attrs) g.inputs.back().push_back(type_width(at.type));
  }
  return g;
}

template <class T>
static void pull(std::vector<T>& v, size_t n, const void* dev) {
  v.resize(n);
  if (n) hipMemcpy(v.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost);
}

template <class T>
static void push(void* dev, const std::vector<T>& v) {
  if (!v.empty()) hipMemcpy(dev, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

extern "C" {

int cep_snapshot(cep_app* a, uint8_t** buf, size_t* len) {
  if (!a || !buf || !len) return CEP_E_ARG;
  if (hipStreamSynchronize(a->stream) != hipSuccess) return fail(a, CEP_E_DEVICE, "device failure");
  SnapImage img;
  img.geo = snap_geometry(a);
  img.events_in = a->events_in;
  img.pats.resize(a->pats.size());
  for (size_t pi = 0; pi < a->pats.size(); ++pi) {
    const PatternRT& rt = a->pats[pi];
    auto& p = img.pats[pi];
    const size_t ks = (size_t)rt.kstride, sw = (size_t)rt.pa.slot_words;
    pull(p.hdr, ks, rt.khdr.p);
    pull(p.slots, ks * rt.pa.pending_slots * sw, rt.kslot.p);
    if (rt.kext.p) {
      pull(p.ext, ks, rt.kext.p);
      pull(p.pool, (size_t)rt.pool_cap * sw, rt.pool[rt.pool_side].p);
    }
    if (rt.sparse) {
      hipMemcpy(p.kcount, rt.kcount.p, 8, hipMemcpyDeviceToHost);
      p.kcount[0] = std::min<uint32_t>(p.kcount[0], (uint32_t)rt.pa.key_capacity);
      pull(p.krev, p.kcount[0], rt.krev.p);
    }
  }
  {
    const auto& r = a->ro;
    img.ro.input = r.input;
    img.ro.has_stream = r.has_stream;
    img.ro.n = r.n;
    img.ro.released_max = r.released_max;
    if (r.n > 0) {
      const StreamSchema& sd = a->app.inputs[r.input];
      std::vector<uint8_t> tmp;
      auto col = [&](const DevBuf& b, size_t bytes) {
        pull(tmp, bytes, b.p);
        img.ro.rows.insert(img.ro.rows.end(), tmp.begin(), tmp.end());
      };
      for (size_t c = 0; c < sd.attrs.size(); ++c) col(r.col[c], (size_t)r.n * type_width(sd.attrs[c].type));
      col(r.ts, (size_t)r.n * 8);
      if (r.has_stream) col(r.stream, (size_t)r.n);
    }
  }
  img.groups.resize(a->mqs.size());
  for (size_t gi = 0; gi < a->mqs.size(); ++gi)
    pull(img.groups[gi], (size_t)a->mqs[gi].words * a->mqs[gi].kstride, a->mqs[gi].state.p);
  img.joins.resize(a->joins.size());
  for (size_t ji = 0; ji < a->joins.size(); ++ji) {
    const JoinRT& jr = a->joins[ji];
    JoinState st;
    hipMemcpy(&st, jr.st.p, sizeof(st), hipMemcpyDeviceToHost);
    for (int sd = 0; sd < 2; ++sd) {
      img.joins[ji].kept[sd] = st.kept[sd];
      img.joins[ji].tail[sd] = std::min<uint64_t>(st.tail[sd], (uint64_t)jr.list_cap[sd]);
      pull(img.joins[ji].rows[sd], (size_t)img.joins[ji].tail[sd] * jr.ja.ew, jr.list[sd][jr.cur].p);
    }
  }
  img.tabs.resize(a->tabs.size());
  for (size_t ti = 0; ti < a->tabs.size(); ++ti) {
    pull(img.tabs[ti].hdr, (size_t)a->tabs[ti].kstride, a->tabs[ti].thdr.p);
    pull(img.tabs[ti].words, (size_t)a->tabs[ti].kstride * a->tabs[ti].ta.nwords, a->tabs[ti].tword.p);
  }
  if (a->tab_dropped.p) hipMemcpy(&img.tab_dropped, a->tab_dropped.p, 8, hipMemcpyDeviceToHost);
  const std::vector<uint8_t> out = snapshot_encode(img);
  *buf = (uint8_t*)std::malloc(out.size());
  if (!*buf) return fail(a, CEP_E_DEVICE, "out of host memory");
  std::memcpy(*buf, out.data(), out.size());
  *len = out.size();
  return CEP_OK;
}

int cep_restore(cep_app* a, const uint8_t* buf, size_t len) {
  if (!a || (!buf && len)) return CEP_E_ARG;
  // decode and validate everything into a host image; nothing on the device
  // changes until the whole snapshot is known to be good
  SnapImage img;
  std::string why;
  if (const int rc = snapshot_decode(snap_geometry(a), buf, len, &img, &why)) return fail(a, rc, why);
  // commit (device allocations first, so a failure leaves the runtime as it was)
  auto& r = a->ro;
  const int64_t n = img.ro.n;
  const StreamSchema* sd = n > 0 ? &a->app.inputs[img.ro.input] : nullptr;
  if (n > 0) {
    bool ok = true;
    for (size_t c = 0; c < sd->attrs.size() && ok; ++c)
      ok = dev_ensure(&r.col[c], (size_t)n * type_width(sd->attrs[c].type), a->stream, false);
    ok = ok && dev_ensure(&r.ts, (size_t)n * 8, a->stream, false);
    if (img.ro.has_stream) ok = ok && dev_ensure(&r.stream, (size_t)n, a->stream, false);
    if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (reorder buffer)");
  }
  hipStreamSynchronize(a->stream);
  for (size_t pi = 0; pi < a->pats.size(); ++pi) {
    PatternRT& rt = a->pats[pi];
    const auto& p = img.pats[pi];
    push(rt.khdr.p, p.hdr);
    push(rt.kslot.p, p.slots);
    if (rt.hwm.p) {   // no restored partial lies above the mark
      std::vector<uint64_t> h(128, 0ull);
      h[0] = h[64] = (uint64_t)p.ts_max ^ (1ull << 63);
      push(rt.hwm.p, h);
    }
    if (rt.kext.p) {
      push(rt.kext.p, p.ext);
      push(rt.pool[rt.pool_side].p, p.pool);
    }
  }
  r.n = 0;
  r.input = -1;
  r.released_max = img.ro.released_max;
  if (n > 0) {
    const uint8_t* src = img.ro.rows.data();
    for (size_t c = 0; c < sd->attrs.size(); ++c) {
      const size_t bytes = (size_t)n * type_width(sd->attrs[c].type);
      hipMemcpy(r.col[c].p, src, bytes, hipMemcpyHostToDevice);
      src += bytes;
    }
    hipMemcpy(r.ts.p, src, (size_t)n * 8, hipMemcpyHostToDevice);
    if (img.ro.has_stream) hipMemcpy(r.stream.p, src + (size_t)n * 8, (size_t)n, hipMemcpyHostToDevice);
    r.input = img.ro.input;
    r.has_stream = img.ro.has_stream;
    r.n = n;
  }
  for (size_t pi = 0; pi < a->pats.size(); ++pi) {
    PatternRT& rt = a->pats[pi];
    if (!rt.sparse) continue;
    push(rt.tkey.p, img.pats[pi].tkey);
    push(rt.tval.p, img.pats[pi].tval);
    push(rt.krev.p, img.pats[pi].krev);
    hipMemcpy(rt.kcount.p, img.pats[pi].kcount, 8, hipMemcpyHostToDevice);
  }
  for (size_t gi = 0; gi < a->mqs.size(); ++gi) push(a->mqs[gi].state.p, img.groups[gi]);
  for (size_t ji = 0; ji < a->joins.size(); ++ji) {
    JoinRT& jr = a->joins[ji];
    JoinState st{};
    for (int s = 0; s < 2; ++s) {
      st.kept[s] = img.joins[ji].kept[s];
      st.tail[s] = st.n[s] = img.joins[ji].tail[s];
      push(jr.list[s][jr.cur].p, img.joins[ji].rows[s]);
    }
    hipMemcpy(jr.st.p, &st, sizeof(st), hipMemcpyHostToDevice);
  }
  for (size_t ti = 0; ti < a->tabs.size(); ++ti) {
    push(a->tabs[ti].thdr.p, img.tabs[ti].hdr);
    push(a->tabs[ti].tword.p, img.tabs[ti].words);
  }
  if (a->tab_dropped.p) hipMemcpy(a->tab_dropped.p, &img.tab_dropped, 8, hipMemcpyHostToDevice);
  a->events_in = img.events_in;
  return CEP_OK;
}

// The live rows of table `table_id`, ordered by primary key, columns = the
// table's attributes (ts / seq NULL).  On a shard: the keys it owns.
int cep_table_rows(cep_app* a, const char* table_id, cep_emit_fn fn, void* user) {
  if (!a || !table_id || !fn) return CEP_E_ARG;
  const int ti = a->app.table_index(table_id);
  if (ti < 0) return fail(a, CEP_E_UNDEFINED_STREAM, std::string("Table ") + table_id + " not defined");
  if (hipStreamSynchronize(a->stream) != hipSuccess) return fail(a, CEP_E_DEVICE, "device failure");
  harvest_timers(a);
  const TableDef& T = a->app.tables[ti];
  const TableRT* tr = nullptr;
  for (auto& t : a->tabs)
    if (t.tab == ti) tr = &t;
  const size_t nc = T.schema.attrs.size();
  std::vector<std::vector<uint8_t>> cols(nc);
  int64_t n = 0;
  if (tr) {
    const int64_t ks = tr->kstride, kc = tr->pa.key_capacity;
    const int lg = tr->pa.buckets_log2;
    const int64_t kpb = ks >> lg;
    std::vector<uint32_t> hdr(ks);
    std::vector<uint64_t> words((size_t)ks * nc);
    if (hipMemcpy(hdr.data(), tr->thdr.p, hdr.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(words.data(), tr->tword.p, words.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(a, CEP_E_DEVICE, "device failure (table rows)");
    // dense keys ascending = primary keys ascending (key = dense * stride + offset)
    for (int64_t key = 0; key < kc; ++key) {
      const int64_t idx = (key & ((1 << lg) - 1)) * kpb + (key >> lg);
      if (!(hdr[idx] & 1u)) continue;
      for (size_t c = 0; c < nc; ++c) {
        const uint64_t v = words[c * (size_t)ks + idx];
        const int w = type_width(T.schema.attrs[c].type);
        uint8_t bytes[8];
        if (w == 1) bytes[0] = (uint8_t)(v & 1u);
        else if (w == 4) { const uint32_t x = (uint32_t)v; std::memcpy(bytes, &x, 4); }
        else std::memcpy(bytes, &v, 8);
        cols[c].insert(cols[c].end(), bytes, bytes + w);
      }
      ++n;
    }
  }
  if (n == 0) return CEP_OK;
  std::vector<const void*> ptrs(nc);
  for (size_t c = 0; c < nc; ++c) ptrs[c] = cols[c].data();
  cep_rows rows{};
  rows.stream_id = T.schema.id.c_str();
  rows.n = n;
  rows.ncols = (int32_t)nc;
  rows.ts = nullptr;
  rows.seq = nullptr;
  rows.cols = ptrs.data();
  fn(user, &rows);
  return CEP_OK;
}


int cep_plan_partition_keys(const char* plan, const char* stream_id, char* buf, size_t len) {
  if (!plan || !stream_id || !buf || !len) return CEP_E_ARG;
  CompiledApp app;
  std::string m;
  const int rc = compile_app(plan, &app, &m);
  if (rc) return rc;
  const int in = app.input_index(stream_id);
  if (in < 0) return CEP_E_UNDEFINED_STREAM;
  // SiddhiExecutionPlanner.parse (utils/SiddhiExecutionPlanner.java:76-140,
  // retrievePartition :172-189): each query reading the stream names its
  // group-by attributes; queries that name different non-empty lists are
  // incompatible partitions.  Extension: the reference's planner rejects
  // `partition with` blocks; here a partitioned query names its partition
  // attribute of the stream.
  // Query chaining: a keyed query on a derived stream M needs the rows of one
  // key on one operator instance just as well, so its key on M, followed back
  // through plain-copy select items to an attribute of this stream, counts as
  // a key of this stream (the reference's planner looks at each query's own
  // input only and cannot see this).  A computed key names nothing.
  const auto& attrs = app.inputs[in].attrs;
  std::vector<int> keys;
  for (auto& q : app.queries) {
    for (int s : query_streams(q)) {
      std::vector<int> k;
      if (q.in_stream == s) {
        k = q.group_cols;
        if (k.empty() && q.part_col >= 0) k.push_back(q.part_col);
      } else if (q.nfa) {
        if (s < (int)q.key_col_s.size() && q.key_col_s[s] >= 0) k.push_back(q.key_col_s[s]);
      } else if (q.a_stream == s || q.b_stream == s) {
        const int c = q.a_stream == s ? q.key_col_a : q.key_col_b;
        if (c >= 0) k.push_back(c);
      }
      if (s != in) {   // a derived stream of this one: translate, or nothing
        std::vector<int> t;
        for (int c : k) {
          int ss = s, cc = c;
          if (source_column(app, &ss, &cc) && ss == in) t.push_back(cc);
        }
        if (t.size() != k.size()) t.clear();
        k = t;
      }
      if (k.empty()) continue;
      if (!keys.empty() && keys != k) {
        std::snprintf(buf, len, "incompatible partitions on stream %s: [%s] vs [%s]", stream_id,
                      attrs[keys[0]].name.c_str(), attrs[k[0]].name.c_str());
        return CEP_E_PARSE;
      }
      keys = k;
    }
  }
  std::string s;
  for (int c : keys) {
    if (!s.empty()) s += '\n';
    s += attrs[c].name;
  }
  std::snprintf(buf, len, "%s", s.c_str());
  return s.size() < len ? CEP_OK : CEP_E_CAPACITY;
}

int cep_partition_channels(cep_app* a, const cep_batch* b, const char* key_field, int nchan, int64_t seq0,
                           int32_t* chan_dev, int64_t* keys_dev) {
  if (!a || !b || nchan <= 0 || !chan_dev || !b->on_device || b->stream) return CEP_E_ARG;
  if (b->input < 0 || b->input >= (int)a->app.inputs.size()) return fail(a, CEP_E_UNDEFINED_STREAM, "undefined input handle");
  const StreamSchema& sd = a->app.inputs[b->input];
  RouteKeyArgs ra{};
  ra.n = b->n;
  ra.nchan = nchan;
  ra.seq0 = seq0;
  ra.keys = keys_dev;
  ra.chan = chan_dev;
  if (key_field && *key_field) {
    int c = -1;
    for (size_t i = 0; i < sd.attrs.size(); ++i)
      if (sd.attrs[i].name == key_field) c = (int)i;
    if (c >= b->ncols) return fail(a, CEP_E_ARG, "batch has fewer columns than the stream definition");
    if (c < 0) {
      // AddRouteOperator.java:84-91: a key the stream lacks sums no field -> key 0
      hipMemsetAsync(chan_dev, 0, (size_t)b->n * 4, a->stream);
      if (keys_dev) hipMemsetAsync(keys_dev, 0, (size_t)b->n * 8, a->stream);
      return hipGetLastError() == hipSuccess ? CEP_OK : fail(a, CEP_E_DEVICE, "memset failed");
    }
    ra.col = b->cols[c];
    ra.type = sd.attrs[c].type;
    if (ra.type == T_STRING) {
      // String.hashCode over UTF-16 code units of each dictionary entry
      std::vector<int32_t> h(a->dict.size());
      for (size_t i = 0; i < a->dict.size(); ++i) {
        const std::string& u = a->dict[i];
        uint32_t x = 0;
        for (size_t j = 0; j < u.size();) {
          uint32_t cp = (uint8_t)u[j];
          int extra = cp >= 0xf0 ? 3 : cp >= 0xe0 ? 2 : cp >= 0xc0 ? 1 : 0;
          cp = extra == 3 ? (cp & 7) : extra == 2 ? (cp & 15) : extra == 1 ? (cp & 31) : cp;
          for (int k = 1; k <= extra && j + k < u.size(); ++k) cp = (cp << 6) | ((uint8_t)u[j + k] & 63);
          j += 1 + extra;
          if (cp >= 0x10000) {   // surrogate pair
            cp -= 0x10000;
            x = x * 31u + (0xd800u + (cp >> 10));
            x = x * 31u + (0xdc00u + (cp & 0x3ff));
          } else {
            x = x * 31u + cp;
          }
        }
        h[i] = (int32_t)x;
      }
      if (!dev_ensure(&a->str_hash, std::max<size_t>(h.size(), 1) * 4, a->stream, false))
        return fail(a, CEP_E_DEVICE, "out of device memory");
      if (!h.empty()) hipMemcpyAsync(a->str_hash.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, a->stream);
      hipStreamSynchronize(a->stream);
      ra.str_hash = (const int32_t*)a->str_hash.p;
      ra.nstr = (int32_t)h.size();
    }
  }
  launch_route_keys(ra, a->stream);
  return hipGetLastError() == hipSuccess ? CEP_OK : fail(a, CEP_E_DEVICE, "route key kernel failed");
}

int cep_generate(int64_t first, int64_t n, uint64_t seed, int64_t keys, int64_t rate, int64_t t0,
                 int single_stream, int32_t* key, int64_t* ts, uint8_t* stream, int32_t* id,
                 double* price, void* hip_stream) {
  if (n < 0 || keys <= 0 || rate <= 0) return CEP_E_ARG;
  launch_generate(first, n, seed, keys, rate, t0, single_stream, key, ts, stream, id, price,
                  (hipStream_t)hip_stream);
  return hipGetLastError() == hipSuccess ? CEP_OK : CEP_E_DEVICE;
}

}  // extern "C"
