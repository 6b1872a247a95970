// The multi-GPU key / row shuffle ABI: senders (cep_route_*) and receivers
// (cep_send_records*, cep_send_rows*) of include/cep.h.
#include "rt.h"

using namespace cep;

extern "C" {

static const char* kTableShuffle = "the key / row shuffle of an app that holds a table is not supported";

int cep_record_words(cep_app* a) {
  if (a && !a->app.tables.empty()) {
    fail(a, CEP_E_UNSUPPORTED, kTableShuffle);
    return -CEP_E_UNSUPPORTED;
  }
  if (a && !a->joins.empty()) {
    fail(a, CEP_E_UNSUPPORTED, "key shuffle of an app that holds a join is not supported: its windows are global, "
                               "not per key");
    return -CEP_E_UNSUPPORTED;
  }
  if (!a || a->pats.size() != 1) return -CEP_E_UNSUPPORTED;
  return a->pats[0].pa.rec_words + 1;   // wide record: [hdr, seq, ts, carried...]
}

// seg_cap == 0: owner-contiguous output, counts read back (cep_route_batch);
// seg_cap > 0: padded owner segments with in-band counts, nothing read back
// (cep_route_batch_padded).
struct SpillArgs {
  void* out = nullptr;         // nullptr: records past seg_cap are dropped (and flagged)
  int64_t cap = 0;             // records the spill holds
  int64_t* counts = nullptr;   // device: spilled records per owner
};

// The sender's arenas: record words, per tile and owner counts / offsets, per owner totals.
static bool route_arenas(cep_app* a, int64_t words, int64_t tile_owners, int world, hipStream_t rs) {
  return dev_ensure(&a->route_arena, (size_t)words * 8, rs, false) &&
         dev_ensure(&a->route_tcount, (size_t)tile_owners * 4, rs, false) &&
         dev_ensure(&a->route_toffs, (size_t)tile_owners * 4, rs, false) &&
         dev_ensure(&a->route_dcount, (size_t)world * 8, rs, false);
}

// Behind the route kernels (key shuffle, or rows: the row shuffle).  Padded
// (seg_cap > 0): nothing is read back, the route's error bits travel in the
// segment headers (every owner reports them at its next flush) and are cleared
// behind the pad kernel.  Otherwise the per-owner counts, W words, are read
// back on the route stream only (the all-to-all's split sizes are host
// values; the engine stream keeps going), with the route kernels' own error
// word, read and cleared on the route stream (the walk's belongs to cep_flush).
static int route_finish(cep_app* a, const cep_batch* b, int world, int64_t seg_cap, int slot, hipStream_t rs,
                        int64_t* counts_host, bool rows) {
  if (slot >= 0) hipEventRecord(a->hs[slot].free, rs);
  if (seg_cap > 0) {
    hipMemsetAsync(a->rerr.p, 0, 64, rs);
    a->batches++;
    return hipGetLastError() == hipSuccess
               ? CEP_OK
               : fail(a, CEP_E_DEVICE, rows ? "padded row route launch failed" : "padded route launch failed");
  }
  std::vector<unsigned long long> dc(world);
  unsigned int re = 0;
  hipMemcpyAsync(dc.data(), a->route_dcount.p, world * 8, hipMemcpyDeviceToHost, rs);
  hipMemcpyAsync(&re, a->rerr.p, 4, hipMemcpyDeviceToHost, rs);
  if (hipStreamSynchronize(rs) != hipSuccess) return fail(a, CEP_E_DEVICE, rows ? "row route failed" : "route failed");
  int64_t total = 0;
  for (int d = 0; d < world; ++d) {
    counts_host[d] = (int64_t)dc[d];
    total += (int64_t)dc[d];
  }
  if (total > b->n)
    return fail(a, CEP_E_DEVICE, rows ? "route produced more rows than the batch" : "route produced more records than rows");
  if (re) {
    hipMemsetAsync(a->rerr.p, 0, 64, rs);
    hipStreamSynchronize(rs);
    return error_status(a, re);
  }
  a->batches++;
  return CEP_OK;
}

static int route_batch(cep_app* a, const cep_batch* b, int world, int64_t seq0, void* rec_out,
                       int64_t rec_cap, int64_t* counts_host, int64_t seg_cap, const SpillArgs& sp = SpillArgs()) {
  if (!a || !b || world <= 0 || (seg_cap == 0 && !counts_host) || seg_cap < 0) return CEP_E_ARG;
  if (world > kMaxWorld) return fail(a, CEP_E_ARG, "world exceeds " + std::to_string(kMaxWorld));
  if (!a->app.derived.empty())
    return fail(a, CEP_E_UNSUPPORTED, "key shuffle of an app with query chaining (derived streams) is not supported: "
                                      "the sender needs the key in source columns");
  if (!a->app.tables.empty()) return fail(a, CEP_E_UNSUPPORTED, kTableShuffle);
  if (!a->joins.empty())
    return fail(a, CEP_E_UNSUPPORTED, "key shuffle of an app that holds a join is not supported: its windows are "
                                      "global, not per key");
  if (a->pats.size() != 1 || a->app.queries.size() != 1)
    return fail(a, CEP_E_UNSUPPORTED, "key shuffle needs an app with exactly one keyed pattern");
  PatternRT& rt = a->pats[0];
  const Query& q = a->app.queries[rt.q];
  if (q.key_col_a < 0 || q.key_col_b < 0)
    return fail(a, CEP_E_UNSUPPORTED, "key shuffle needs a partitioned pattern");
  if (seg_cap == 0) {
    for (int d = 0; d < world; ++d) counts_host[d] = 0;
    if (b->n == 0) return CEP_OK;
    // the gather writes rec_out as soon as it runs: at most n records are
    // routed, so a buffer of n records can never overrun (checked up front)
    if (!rec_out || rec_cap < b->n)
      return fail(a, CEP_E_ARG, "rec_out must hold at least n records (" + std::to_string(b->n) + ")");
  } else {
    // every rank ships world segments each step, so the null records need a
    // ts / seq of this batch (its first and last rows)
    if (b->n == 0) return fail(a, CEP_E_ARG, "padded key shuffle needs a non-empty batch");
    if (!rec_out || rec_cap < (int64_t)world * (1 + seg_cap))
      return fail(a, CEP_E_ARG, "rec_out must hold world * (1 + seg_cap) records");
  }
  RowsArgs rows{};
  int slot;
  bool direct;
  int rc = batch_rows(a, b, &rows, &slot, &direct);
  if (rc) return rc;
  // fast route (k_cfroute) when every column the pattern reads is prefetchable
  // and f / g are term lists (the k_cfpart load path); CEP_NO_CF=1 forces k_route
  static const bool no_cf = std::getenv("CEP_NO_CF") != nullptr;
  const bool fast = !no_cf && !rt.part_vm && rt.pref.n >= 0 && rt.pref.key_slot <= 0 &&
                    rt.pa.rec_words + 1 <= 5 && pref_aligned(rt.pref, rows);
  const int64_t tile_rows = fast ? kCfTile : kPartThreads * kPartItems;
  const int64_t ntiles = (b->n + tile_rows - 1) / tile_rows;
  const int wrw = rt.pa.rec_words + 1;
  // device batches route on the route stream (ordered after the producer by
  // cep_stream_wait), so the walk of the previous batch keeps running; host
  // batches were staged on the engine stream and route there
  hipStream_t rs = b->on_device ? a->rstream : a->stream;
  if (!route_arenas(a, ntiles * tile_rows * wrw, ntiles * world, world, rs))
    return fail(a, CEP_E_DEVICE, "out of device memory (route arena)");
  RouteArgs ra{};
  ra.rows = rows;
  ra.vm = {(const Ins*)a->code.p, (const uint64_t*)a->konst.p};
  ra.pat = rt.pa;
  // ts_order 0: the owners run the order-tolerant path, which needs every
  // B-stream row (a g-failing B expires partials, App. A.3), so no B is
  // pushed down; sender and owners share the app's options
  ra.pat.tolerant = (a->opt.ts_order == 0 && rt.order_sensitive) ? 1 : 0;
  ra.world = world;
  ra.wrw = wrw;
  ra.tile_rows = (int32_t)tile_rows;
  ra.seq0 = seq0;
  ra.arena = (uint64_t*)a->route_arena.p;
  ra.tcount = (uint32_t*)a->route_tcount.p;
  ra.err = (unsigned int*)a->rerr.p;
  ra.seg_cap = seg_cap;
  ra.spill = (uint64_t*)sp.out;
  ra.spill_cap = sp.cap;
  ra.spill_counts = sp.counts;
  {
    LaunchTimer t(a, CEP_K_ROUTE, rs);
    if (fast) {
      CfRouteArgs ca{};
      ca.r = ra;
      ca.pref = rt.pref;
      ca.ts_slot = -1;
      for (int i = 0; i < rt.pref.n; ++i)
        if (rows.cols.p[rt.pref.col[i]] == (const void*)rows.ts && rows.cols.t[rt.pref.col[i]] == T_LONG)
          ca.ts_slot = i;
      launch_cf_route(ca, ntiles, rs);
      launch_route_collect(ra, ntiles, (uint32_t*)a->route_toffs.p,
                           (unsigned long long*)a->route_dcount.p, (uint64_t*)rec_out, rs);
    } else {
      launch_route(ra, ntiles, rt.part_vm, (uint32_t*)a->route_toffs.p,
                   (unsigned long long*)a->route_dcount.p, (uint64_t*)rec_out, rs);
    }
    if (seg_cap > 0) launch_route_pad(ra, (const unsigned long long*)a->route_dcount.p, (uint64_t*)rec_out, rs);
  }
  return route_finish(a, b, world, seg_cap, slot, rs, counts_host, false);
}

int cep_route_batch(cep_app* a, const cep_batch* b, int world, int64_t seq0, void* rec_out,
                    int64_t rec_cap, int64_t* counts_host) {
  return route_batch(a, b, world, seq0, rec_out, rec_cap, counts_host, 0);
}

// A host batch is staged and routed on the engine stream; join that into the
// route stream so cep_route_signal (which records on the route stream) also
// orders a consumer after it (the padded routes read nothing back).
static int route_join_host(cep_app* a, const cep_batch* b, int rc) {
  if (rc != CEP_OK || !b || b->on_device) return rc;
  if (hipEventRecord(a->r_host, a->stream) != hipSuccess ||
      hipStreamWaitEvent(a->rstream, a->r_host, 0) != hipSuccess)
    return fail(a, CEP_E_DEVICE, "route: stream join failed");
  return rc;
}

int cep_route_batch_padded(cep_app* a, const cep_batch* b, int world, int64_t seq0, void* seg_out,
                           int64_t seg_out_cap, int64_t seg_cap) {
  if (seg_cap <= 0) return CEP_E_ARG;
  return route_join_host(a, b, route_batch(a, b, world, seq0, seg_out, seg_out_cap, nullptr, seg_cap));
}

int cep_route_batch_padded_spill(cep_app* a, const cep_batch* b, int world, int64_t seq0, void* seg_out,
                                 int64_t seg_out_cap, int64_t seg_cap, void* spill_out, int64_t spill_cap,
                                 int64_t* spill_counts) {
  if (seg_cap <= 0 || !spill_out || spill_cap < 0 || !spill_counts) return CEP_E_ARG;
  SpillArgs sp;
  sp.out = spill_out;
  sp.cap = spill_cap;
  sp.counts = spill_counts;
  return route_join_host(a, b, route_batch(a, b, world, seq0, seg_out, seg_out_cap, nullptr, seg_cap, sp));
}

// Row shuffle plan: per input handle the owner key column (-1: any owner,
// the stream feeds stateless filters only; -2: no query reads it).  Every
// query that keeps per-key state must key each stream it reads on one
// attribute, the same for all such queries; the shipped streams must share
// one column layout (the owner unpacks them into one multi-stream batch).
static int row_route_plan(cep_app* a, int32_t (&kc)[8], int* layout) {
  const CompiledApp& app = a->app;
  const int ni = (int)app.inputs.size();
  if (ni > 8) return fail(a, CEP_E_UNSUPPORTED, "row shuffle supports at most 8 input streams");
  if (!app.tables.empty()) return fail(a, CEP_E_UNSUPPORTED, kTableShuffle);
  if (!a->joins.empty())
    return fail(a, CEP_E_UNSUPPORTED, "row shuffle of an app that holds a join is not supported: its windows are "
                                      "global, not per key");
  for (int i = 0; i < 8; ++i) kc[i] = -2;
  auto need = [&](int s, int col) -> int {
    if (s < 0 || s >= ni) return CEP_OK;
    if (col < 0) return fail(a, CEP_E_UNSUPPORTED, "row shuffle: query state on stream " + app.inputs[s].id +
                                                     " is not keyed (needs `partition with` or group by)");
    if (kc[s] >= 0 && kc[s] != col)
      return fail(a, CEP_E_UNSUPPORTED, "row shuffle: stream " + app.inputs[s].id + " is keyed on two attributes");
    kc[s] = col;
    return CEP_OK;
  };
  for (auto& q : app.queries) {
    int rc = CEP_OK;
    if (q.kind == Q_FILTER) {
      if (q.in_stream >= 0 && kc[q.in_stream] == -2) kc[q.in_stream] = -1;
      continue;
    }
    if (q.kind == Q_AGG) {
      rc = need(q.in_stream, q.key_col);
    } else if (q.nfa) {
      for (auto& st : q.nstates) {
        rc = need(st.stream, st.stream >= 0 && st.stream < (int)q.key_col_s.size() ? q.key_col_s[st.stream] : -1);
        if (rc) break;
      }
    } else {
      rc = need(q.a_stream, q.key_col_a);
      if (!rc) rc = need(q.b_stream, q.key_col_b);
    }
    if (rc) return rc;
  }
  // a keyed stream also read by a filter keeps its key (filters are stateless)
  *layout = -1;
  for (int s = 0; s < ni; ++s) {
    if (kc[s] == -2) continue;
    if (*layout < 0) {
      *layout = s;
      continue;
    }
    const auto& x = app.inputs[*layout].attrs;
    const auto& y = app.inputs[s].attrs;
    bool same = x.size() == y.size();
    for (size_t c = 0; same && c < x.size(); ++c) same = x[c].type == y[c].type;
    if (!same)
      return fail(a, CEP_E_UNSUPPORTED, "row shuffle: streams " + app.inputs[*layout].id + " and " +
                                            app.inputs[s].id + " have different column types");
  }
  if (*layout < 0) return fail(a, CEP_E_UNSUPPORTED, "row shuffle: no query reads any input stream");
  return CEP_OK;
}

int cep_send_records(cep_app* a, const void* recs, int64_t n, int64_t events_represented) {
  if (!a || (n > 0 && !recs) || n < 0) return CEP_E_ARG;
  if (!a->enabled) return CEP_OK;
  if (a->pats.size() != 1 || a->app.queries.size() != 1)
    return fail(a, CEP_E_UNSUPPORTED, "records need an app with exactly one keyed pattern");
  a->events_in += events_represented;
  if (n == 0) return CEP_OK;
  PatternRT& rt = a->pats[0];
  RowsArgs rows{};
  rows.n = n;
  rows.row0 = 0;
  rows.input = rt.pa.a_stream;
  a->batches++;
  return run_pattern(a, rt, rows, (const uint64_t*)recs, rt.pa.rec_words + 1);
}

int cep_send_records_padded(cep_app* a, const void* segs, int world, int64_t seg_cap,
                            int64_t events_represented) {
  if (!a || !segs || world <= 0 || world > kMaxWorld || seg_cap <= 0) return CEP_E_ARG;
  if (!a->enabled) return CEP_OK;
  if (a->pats.size() != 1 || a->app.queries.size() != 1)
    return fail(a, CEP_E_UNSUPPORTED, "records need an app with exactly one keyed pattern");
  a->events_in += events_represented;
  PatternRT& rt = a->pats[0];
  const int wrw = rt.pa.rec_words + 1;
  // the headers' counts / error bits -> this engine's error word (reported
  // by the next flush); the null records flow through the partitions, which
  // skip role-0 records, so no count is read back here
  launch_route_check((const uint64_t*)segs, world, seg_cap, wrw, 0, (unsigned int*)a->err.p, a->stream);
  RowsArgs rows{};
  rows.n = (int64_t)world * (1 + seg_cap);
  rows.row0 = 0;
  rows.input = rt.pa.a_stream;
  a->batches++;
  return run_pattern(a, rt, rows, (const uint64_t*)segs, wrw);
}

int cep_row_words(cep_app* a) {
  if (!a) return -CEP_E_ARG;
  int32_t kc[8];
  int layout;
  const int rc = row_route_plan(a, kc, &layout);
  if (rc) return -rc;
  return 3 + (int)a->app.inputs[layout].attrs.size();
}

// seg_cap == 0: owner-contiguous rows, counts read back (cep_route_rows);
// seg_cap > 0: padded owner segments, counts in-band (cep_route_rows_padded).
static int route_rows(cep_app* a, const cep_batch* b, int world, int64_t seq0, void* rec_out, int64_t rec_cap,
                      int64_t* counts_host, int64_t seg_cap, const SpillArgs& sp = SpillArgs()) {
  if (!a || !b || world <= 0 || seg_cap < 0 || (seg_cap == 0 && !counts_host)) return CEP_E_ARG;
  if (world > kMaxWorld) return fail(a, CEP_E_ARG, "world exceeds " + std::to_string(kMaxWorld));
  if (!a->app.derived.empty())
    return fail(a, CEP_E_UNSUPPORTED, "row shuffle of an app with query chaining (derived streams) is not supported: "
                                      "the sender needs the key in source columns");
  int32_t kc[8];
  int layout;
  int rc = row_route_plan(a, kc, &layout);
  if (rc) return rc;
  if (seg_cap == 0) {
    for (int d = 0; d < world; ++d) counts_host[d] = 0;
    if (b->n == 0) return CEP_OK;
    if (!rec_out || rec_cap < b->n)
      return fail(a, CEP_E_ARG, "rec_out must hold at least n rows (" + std::to_string(b->n) + ")");
  } else {
    if (b->n == 0) return fail(a, CEP_E_ARG, "padded row shuffle needs a non-empty batch");
    if (!rec_out || rec_cap < (int64_t)world * (1 + seg_cap))
      return fail(a, CEP_E_ARG, "seg_out must hold world * (1 + seg_cap) rows");
  }
  if (b->stream) {
    // a multi-stream batch needs one layout for all its streams (batch_rows)
  } else if (kc[b->input] != -2) {
    const auto& x = a->app.inputs[layout].attrs;
    const auto& y = a->app.inputs[b->input].attrs;
    bool same = x.size() == y.size();
    for (size_t c = 0; same && c < x.size(); ++c) same = x[c].type == y[c].type;
    if (!same) return fail(a, CEP_E_UNSUPPORTED, "row shuffle: batch stream layout differs");
  }
  RowsArgs rows{};
  int slot;
  bool direct;
  rc = batch_rows(a, b, &rows, &slot, &direct);
  if (rc) return rc;
  const int64_t tile_rows = kPartThreads * kPartItems;
  const int64_t ntiles = (b->n + tile_rows - 1) / tile_rows;
  const int wrw = 3 + rows.cols.n;
  hipStream_t rs = b->on_device ? a->rstream : a->stream;
  if (!route_arenas(a, ntiles * tile_rows * wrw, ntiles * world, world, rs))
    return fail(a, CEP_E_DEVICE, "out of device memory (route arena)");
  RowRouteArgs ra{};
  ra.rows = rows;
  ra.world = world;
  ra.wrw = wrw;
  ra.tile_rows = (int32_t)tile_rows;
  ra.seq0 = seq0;
  for (int i = 0; i < 8; ++i) ra.key_col_s[i] = kc[i];
  ra.arena = (uint64_t*)a->route_arena.p;
  ra.tcount = (uint32_t*)a->route_tcount.p;
  ra.err = (unsigned int*)a->rerr.p;
  ra.seg_cap = seg_cap;
  ra.spill = (uint64_t*)sp.out;
  ra.spill_cap = sp.cap;
  ra.spill_counts = sp.counts;
  {
    LaunchTimer t(a, CEP_K_ROUTE, rs);
    launch_route_rows(ra, ntiles, (uint32_t*)a->route_toffs.p, (unsigned long long*)a->route_dcount.p,
                      (uint64_t*)rec_out, rs);
  }
  return route_finish(a, b, world, seg_cap, slot, rs, counts_host, true);
}

int cep_route_rows(cep_app* a, const cep_batch* b, int world, int64_t seq0, void* rec_out, int64_t rec_cap,
                   int64_t* counts_host) {
  return route_rows(a, b, world, seq0, rec_out, rec_cap, counts_host, 0);
}

int cep_route_rows_padded(cep_app* a, const cep_batch* b, int world, int64_t seq0, void* seg_out,
                          int64_t seg_out_cap, int64_t seg_cap) {
  if (seg_cap <= 0) return CEP_E_ARG;
  return route_join_host(a, b, route_rows(a, b, world, seq0, seg_out, seg_out_cap, nullptr, seg_cap));
}

int cep_route_rows_padded_spill(cep_app* a, const cep_batch* b, int world, int64_t seq0, void* seg_out,
                                int64_t seg_out_cap, int64_t seg_cap, void* spill_out, int64_t spill_cap,
                                int64_t* spill_counts) {
  if (seg_cap <= 0 || !spill_out || spill_cap < 0 || !spill_counts) return CEP_E_ARG;
  SpillArgs sp;
  sp.out = spill_out;
  sp.cap = spill_cap;
  sp.counts = spill_counts;
  return route_join_host(a, b, route_rows(a, b, world, seq0, seg_out, seg_out_cap, nullptr, seg_cap, sp));
}

int cep_send_rows_padded(cep_app* a, const void* segs, int world, int64_t seg_cap, int64_t events_represented) {
  if (!a || !segs || world <= 0 || world > kMaxWorld || seg_cap <= 0) return CEP_E_ARG;
  if (!a->enabled) return CEP_OK;
  const int w = cep_row_words(a);
  if (w < 0) return -w;
  // headers -> this engine's error word; header and null rows carry stream
  // handle kRowNullStream, which no query reads
  launch_route_check((const uint64_t*)segs, world, seg_cap, w, 1, (unsigned int*)a->err.p, a->stream);
  return cep_send_rows(a, segs, (int64_t)world * (1 + seg_cap), events_represented);
}

int cep_send_rows(cep_app* a, const void* recs, int64_t n, int64_t events_represented) {
  if (!a || (n > 0 && !recs) || n < 0) return CEP_E_ARG;
  if (!a->enabled) return CEP_OK;
  int32_t kc[8];
  int layout;
  int rc = row_route_plan(a, kc, &layout);
  if (rc) return rc;
  a->events_in += events_represented;
  if (n == 0) return CEP_OK;
  const StreamSchema& sd = a->app.inputs[layout];
  const int nc = (int)sd.attrs.size();
  RowUnpackArgs ua{};
  ua.recs = (const uint64_t*)recs;
  ua.n = n;
  ua.wrw = 3 + nc;
  ua.ncols = nc;
  bool ok = true;
  for (int c = 0; c < nc && ok; ++c) {
    ok = dev_ensure(&a->rr_col[c], (size_t)n * type_width(sd.attrs[c].type) + 16, a->stream, false);
    ua.col[c] = a->rr_col[c].p;
    ua.type[c] = sd.attrs[c].type;
  }
  ok = ok && dev_ensure(&a->rr_ts, (size_t)n * 8, a->stream, false) &&
       dev_ensure(&a->rr_stream, (size_t)n + 16, a->stream, false) &&
       dev_ensure(&a->rr_seq, (size_t)n * 8, a->stream, false);
  if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (received rows)");
  ua.ts = (int64_t*)a->rr_ts.p;
  ua.stream = (uint8_t*)a->rr_stream.p;
  ua.seq = (int64_t*)a->rr_seq.p;
  {
    LaunchTimer t(a, CEP_K_OTHER);
    launch_unpack_rows(ua, a->stream);
  }
  RowsArgs rows{};
  rows.cols.n = nc;
  for (int c = 0; c < nc; ++c) {
    rows.cols.p[c] = ua.col[c];
    rows.cols.t[c] = sd.attrs[c].type;
  }
  rows.ts = ua.ts;
  rows.stream = ua.stream;
  rows.input = layout;
  rows.row0 = 0;
  rows.n = n;
  rows.seq0 = 0;
  rows.seq = ua.seq;
  rows.prev_ts = INT64_MIN;
  a->last_ts = INT64_MIN;
  a->batches++;
  return send_device_rows(a, rows);
}

}  // extern "C"
