// Host runtime of libcep: owning HIP resource types, the chunk pipeline, the
// runtime structs behind a cep_app and the helpers the host files share
// (engine.cpp, mq_plan.cpp, route.cpp, stamps.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/cep.h"
#include "frontend.h"
#include "kernels.h"

namespace cep {

// Move-only owner of a block of device (hipFree) or pinned host (hipHostFree)
// memory.  p / bytes are public: kernels' arguments are built from them.
template <hipError_t (*Free)(void*)>
struct Buf {
  void* p = nullptr;
  size_t bytes = 0;
  Buf() = default;
  Buf(Buf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  Buf& operator=(Buf&& o) noexcept {   // (o's destructor frees the old block)
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { reset(); }
  void reset() {
    if (p) Free(p);
    p = nullptr;
    bytes = 0;
  }
};
using DevBuf = Buf<hipFree>;
// Pinned (page-locked) host memory: DMA at PCIe speed, no driver bounce.
using HostBuf = Buf<hipHostFree>;

// Grows to max(bytes, 2 x old); keep: the old contents are copied over on s;
// s is synchronised before the old block is freed.
inline bool dev_ensure(DevBuf* b, size_t bytes, hipStream_t s, bool keep) {
  if (b->bytes >= bytes && b->p) return true;
  size_t nb = std::max(bytes, b->bytes * 2);
  void* p = nullptr;
  if (hipMalloc(&p, nb) != hipSuccess) return false;
  if (keep && b->p && b->bytes) hipMemcpyAsync(p, b->p, b->bytes, hipMemcpyDeviceToDevice, s);
  if (b->p) {
    hipStreamSynchronize(s);
    hipFree(b->p);
  }
  b->p = p;
  b->bytes = nb;
  return true;
}

inline bool host_ensure(HostBuf* b, size_t bytes) {
  if (b->bytes >= bytes && b->p) return true;
  // pinning hundreds of MB takes ~100 ms: grow with headroom, so a delivery
  // buffer sized by one flush's rows is not re-pinned when the next flush
  // brings a few more
  const size_t nb = std::max(bytes + bytes / 2, b->bytes * 2);
  b->reset();
  if (hipHostMalloc(&b->p, nb, hipHostMallocDefault) != hipSuccess) return false;
  b->bytes = nb;
  return true;
}

// Move-only owner of one HIP event / stream, convertible to the raw handle.
template <class T, hipError_t (*Destroy)(T)>
struct Handle {
  T h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
  Handle& operator=(Handle&& o) noexcept {
    std::swap(h, o.h);
    return *this;
  }
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() {
    if (h) Destroy(h);
  }
  operator T() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
  bool create(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&h, flags) == hipSuccess; }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  bool create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking) == hipSuccess; }
};

// The double-buffered partition / walk pipeline of one runtime: the partition
// of chunk c+1 fills arena b^1 on the side stream while the walk of chunk c
// reads arena b on the main stream.  Per batch: open(); per chunk: begin(),
// the partition launch, partitioned(), the walk launch, walked().
struct ChunkPipe {
  DevBuf recs[2], tile_off[2], chunk_base[2];
  Event part_done[2], walk_done[2];
  bool used[2] = {false, false};
  int cur = 0;            // arena of the next chunk
  int64_t chunk = 0;      // rows per chunk
  bool events = true;     // this batch's passes are ordered by events (open / open_cf)

  bool alloc(size_t rec_bytes, size_t toff_bytes, hipStream_t s) {
    bool ok = true;
    for (int b = 0; b < 2 && ok; ++b)
      ok = dev_ensure(&recs[b], rec_bytes, s, false) && dev_ensure(&tile_off[b], toff_bytes, s, false) &&
           dev_ensure(&chunk_base[b], 64, s, false) && part_done[b].create() && walk_done[b].create();
    return ok;
  }
  // The side stream starts after everything already queued on the main stream
  // (host-batch staging copies, earlier queries).  Returns the partition's
  // stream: the side stream, or the main stream with CEP_NO_OVERLAP=1
  // (diagnostics; the events are still issued).
  hipStream_t open(cep_app* a);
  // The closed form (run_pattern_cf) differs: both passes on the main stream
  // and no event at all unless CEP_OVERLAP=1, which makes it open() without
  // the CEP_NO_OVERLAP lookup.
  hipStream_t open_cf(cep_app* a);
  int begin(hipStream_t side) {
    const int b = cur;
    cur ^= 1;
    if (events && used[b]) hipStreamWaitEvent(side, walk_done[b], 0);   // arena b is free
    return b;
  }
  void partitioned(int b, hipStream_t side, hipStream_t main) {
    if (!events) return;
    hipEventRecord(part_done[b], side);
    hipStreamWaitEvent(main, part_done[b], 0);
  }
  void walked(int b, hipStream_t main) {
    if (events) hipEventRecord(walk_done[b], main);
    used[b] = true;
  }
};

struct OutStream {
  std::string id;
  std::vector<int> types;
  std::vector<DevBuf> cols;
  DevBuf ts, seq;
  unsigned long long* count = nullptr;   // device cursor
  int64_t cap = 0;                       // allocated rows
  int64_t bound = 0;                     // upper bound of rows since last flush
  bool write_seq = true;                 // the kernels store arrival numbers (someone reads them)
  cep_emit_fn fn = nullptr;
  void* user = nullptr;
  // pinned host copies for callback delivery (D2H at PCIe speed)
  std::vector<HostBuf> hcols;
  HostBuf hts, hseq;
  // ordered_output: the rows permuted into Siddhi's emission order on the
  // device (stable sort on seq) before the D2H
  std::vector<DevBuf> scols;
  DevBuf sts, sseq;
};

struct PatternRT {
  int q = -1;
  PatternArgs pa{};
  DevBuf khdr, kslot;        // per-key state, SoA over the bucket-major key index
  int64_t kstride = 0;       // keys_per_bucket * buckets
  // the general path's chunk arenas.  The closed form's arenas below share
  // the pipe's chunk_base, events and `cur`: a batch takes one path or the
  // other, chunk_base[b] is written by either path's partition and read by its
  // walk, so whichever path ran last, walk_done[b] / used[b] are what the next
  // partition into side b has to wait for
  ChunkPipe pipe;
  PrefPlan pref;               // fast partition path (n < 0: generic)
  int64_t chunk_tol = 0;       // chunk of the order-tolerant form (walked by the VM build: up to 16 Mi rows)
  int64_t extra_bound = 0;   // pending partials that may still complete
  bool part_vm = true;       // partition pass needs the interpreter
  bool walk_vm = true;       // walk needs the interpreter (g on s1, computed select items)
  // closed-form fast path (cf_kernels.hip): its own, larger chunk arenas
  bool cf = false;
  int64_t cf_chunk = 0;
  DevBuf cf_recs[2], cf_toff[2];
  // pending lists longer than S (closed-form path): per-key count + run
  // offset, and two pools of overflow slots swapped per walk launch
  DevBuf kext, pool[2], pool_cur;
  int pool_side = 0;           // pool[pool_side] holds the current runs
  int64_t pool_cap = 0;        // slots per pool
  // sparse partition keys (cep_options.sparse_keys): value -> dense slot map
  bool sparse = false;
  uint64_t table_cap = 0;
  DevBuf tkey, tval, krev, kcount, dense;
  // hot keys (hot.hip): keys that would make their bucket a straggler are
  // matched by grid-wide scans; the walk reports candidates, diversion starts
  // (sticky) once the device has put a key into a hot slot
  bool hot = false;            // candidate collection on (closed-form path, P + kCfHotMax buckets fit)
  bool hot_on = false;         // diversion active: hot arenas allocated
  // ts_order 0 on the closed form: in-order chunks take the adaptive build
  // (CfPartArgs::atol); atol_ok goes false for good once another path has
  // run the pattern (it keeps no high-water mark)
  bool atol_ok = true;
  uint32_t atol_seq = 0;       // gate value of the current adaptive chunk
  int64_t tol_chunks = 0;      // high-water-mark shard set parity
  DevBuf atol_gate;            // 64 B: the gate word
  DevBuf hwm;                  // 2 x 64 u64: high-water-mark shard sets
  bool hot_probed = false;     // the first (short) chunk ran and its candidates were read back
  uint32_t hot_thresh = 0;     // records per key per launch that make a key hot
  int hot_blocks = 0;
  DevBuf hot_id, hot_key, hot_m, hot_gbase, hoff, cand, ncand, harr, hrow, hnb, bsum, bcnt, boff, hcm, hobase,
      hot_active, htmn, htmx, hflag, btol;   // (the last four: order-tolerant runs)
  HostBuf hot_active_host;     // pinned: slots in use (read without a sync)
  Event hot_fork, hot_join;    // hot kernels on the side stream, beside the walk
  // a pattern whose result depends on event-time order (`within`, not a
  // sequence): with cep_options.ts_order = 0 it runs the order-tolerant path
  bool order_sensitive = false;
  // sliding-window aggregate (win_kernels.hip): the window fields of WinArgs
  // (kind, param, ring, entry layout); win.kind = WIN_NONE: not a window query
  WinArgs win{};
  bool win_vm = false;         // k_winwalk needs the interpreter (having, computed select items)
  // tumbling-window aggregate (batch_kernels.hip): the window and state-layout
  // fields of BatchArgs; bat.kind = WIN_NONE: not a batch-window query.  Its
  // interpreter flag is win_vm too (a query has one window).
  BatchArgs bat{};
};

// Multi-query group (mq_kernels.hip): keyed queries of one app sharing a
// key column, run by one partition pass + one walk per chunk.
struct MqRT {
  std::vector<int> qs;                   // query indices, plan order
  std::vector<MqQuery> hq;               // host copy of the device descriptors
  DevBuf dq, dconds;
  std::vector<MqCond> conds;             // [8][kMqMaxCond]
  int32_t ncond[8] = {0};
  uint32_t stream_mask = 0;
  int key_col = -1;
  int view = -1;                         // query chaining: the view its queries read (-1: the batch)
  std::vector<int> carry;                // logical carried columns
  std::vector<int> cond_cols;            // columns the conditions read
  bool check_order = false;
  int64_t key_capacity = 0, kstride = 0;
  int lg = 0, kpb = 0;
  int key_stride = 1, key_offset = 0;
  DevBuf state;
  int64_t words = 0;                     // state words per key (all queries)
  ChunkPipe pipe;
  bool dq_dirty = true;
  std::vector<int> classes_kind, classes_n;   // shape classes in descriptor order (MqUnit kinds, sizes)
  std::vector<MqUnit> units;
  DevBuf du;
};

// Windowed stream join (join_kernels.hip): both sides' kept-row lists (double
// buffered: k_jointail moves the surviving rows into the other buffer), the
// chunk's flag / probe scratch and the device state words.
struct JoinRT {
  int q = -1;
  JoinArgs ja{};               // the plan's part of the kernel arguments
  bool mark_vm = false;        // a side filter needs the interpreter
  bool on_vm = false;          // `on` needs the interpreter
  bool sel_vm = false;         // a select item is computed
  int64_t chunk = 0;
  int64_t list_cap[2] = {0, 0};
  DevBuf list[2][2];           // [side][buffer]
  int cur = 0;                 // buffer holding the current lists
  DevBuf flag, bsum, boff, probe, pcnt, pbsum, pboff, st;
  HostBuf total;               // pinned: the chunk's row total (read back before the emit pass)
};

// Event table (tab_kernels.hip): one pipeline per table holding every
// operation on it.  The generic partition pass (N-state record form: one
// "state" per operation) and k_tabwalk, chunk by chunk, double buffered like a
// pattern's arenas.  State: a present bit and the row's words per key.
struct TableRT {
  int tab = -1;                // index into CompiledApp::tables
  int run_at = -1;             // query index at which the pipeline runs (its first reader, else its first operation)
  PatternArgs pa{};            // k_partition's view of the operations
  TabArgs ta{};                // the plan's part of the walk's arguments
  bool vm = false;             // k_tabwalk needs the interpreter
  DevBuf thdr, tword;
  int64_t kstride = 0;
  ChunkPipe pipe;
};

struct TimedLaunch {
  int kind;
  Event a, b;
};

}  // namespace cep

// Members are destroyed in reverse order: every buffer and event below goes
// before the four streams at the top are destroyed (cep_destroy has
// synchronised them), which is the order the hand-written teardown kept.
struct cep_app {
  cep::Stream stream;
  cep::Stream copy;              // H2D of host batches
  cep::Stream side;              // partition pass of the next chunk
  // Shuffle sender (cep_route_batch of device batches) runs on its own stream:
  // routing step s+1 overlaps the walk of step s (it touches no walk state)
  cep::Stream rstream;
  cep::Event in_ready;
  cep::Event ext_ready;          // cep_stream_wait: producer stream of device inputs
  cep::Event out_ready;          // cep_stream_signal: the engine's work so far
  cep::Event r_ready;
  cep::Event r_host;             // a host batch's route (engine stream) joined into the route stream
  cep::CompiledApp app;
  cep_options opt{};
  bool enabled = true;
  std::string last_error;
  std::vector<std::string> dict;
  std::unordered_map<std::string, int32_t> dict_index;
  cep::DevBuf code, konst;
  std::vector<cep::OutStream> outs;
  std::vector<cep::PatternRT> pats;
  std::vector<cep::MqRT> mqs;          // multi-query groups
  std::vector<cep::JoinRT> joins;      // windowed stream joins
  std::vector<cep::TableRT> tabs;      // event tables
  cep::DevBuf tab_dropped;             // inserts dropped on an existing key (device counter, every table)
  std::vector<char> in_mq;             // per query: served by a multi-query group
  cep::DevBuf tile_state, ticket, err;
  cep::DevBuf route_arena, route_tcount, route_toffs, route_dcount;   // key shuffle (sender)
  cep::DevBuf rerr;                 // error word of the route kernels (route stream; the walk's is `err`)
  cep::DevBuf stamps;               // CEP_STAMPS=1: walk phase stamps (diagnostics)
  cep::DevBuf str_hash;             // Java String.hashCode per dictionary id (dynamic routing)
  cep::HostBuf flush_words;         // cep_flush: error word + output cursors + seq stats (pinned)
  cep::DevBuf out_counts;           // every output's row cursor (OutStream::count points here)
  cep::DevBuf ostats;               // cep_flush: per output {~min seq, max seq, descents} (k_seq_stats)
  cep::DevBuf okeys[2], oidx[2], otemp;   // cep_flush: emission-order sort scratch (shared by the outputs)
  cep::DevBuf rr_col[cep::kMaxCols], rr_ts, rr_stream, rr_seq;   // cep_send_rows: unpacked rows
  // query chaining: per view (CompiledApp::views) and stage, the handle column
  // and the materialised columns of the last batch (stateless: rebuilt per batch)
  struct ViewStage {
    cep::DevBuf stream, col[cep::kMaxCols];
  };
  std::vector<std::vector<ViewStage>> views;
  // host batches: two staging slots (pinned host arena + device arena); a
  // batch's H2D copy runs on the copy stream while the previous batch's
  // kernels run on the main stream
  struct HostSlot {
    cep::HostBuf pinned;
    cep::DevBuf dev;
    cep::Event dma_done, free;   // created with the slot's first batch
    bool used = false;
  } hs[2];
  int hs_next = 0;
  // event-time reorder buffer (cep_buffer_batch / cep_watermark): rows of
  // one input layout since the last watermark, SoA in arrival order
  struct Reorder {
    int input = -1;            // layout owner (-1: empty)
    bool has_stream = false;
    int64_t n = 0, cap = 0;
    int64_t released_max = INT64_MIN;   // latest ts handed to the engine
    cep::DevBuf col[cep::kMaxCols], ts, stream;  // buffered rows
    cep::DevBuf out[cep::kMaxCols], ots, ostream;   // sorted released rows (a device batch)
    cep::DevBuf keys, idx_in, idx_out, temp, bound;
  } ro;
  int64_t events_in = 0, matches_out = 0, batches = 0, late_events = 0;
  int64_t tab_vm_launches = 0;   // k_tabwalk launches of the interpreter build
  int64_t last_ts = INT64_MIN;
  cep::DevBuf last_ts_dev;     // last ts of the previous batch (RowsArgs::prev_ts_dev)
  bool force_tolerant = false; // this batch holds late rows (cep_watermark, late_policy 2)
  bool seq_poison = false;     // diagnostics (CEP_SEQ_POISON=1): unread seq columns hold a pattern the flush checks
  bool cf_one_wg = false;      // CEP_CF_PART=1 (read at creation): k_cfpart where k_cfpart2 would run
  int64_t launches[16] = {0};
  double kernel_ms[16] = {0};
  int64_t kernel_timed[16] = {0};
  std::vector<cep::TimedLaunch> timed;
  std::vector<cep::Event> event_pool;   // timing events of LaunchTimer, reused
  std::vector<std::unique_ptr<char[]>> name_store;
};

namespace cep {

inline int fail(cep_app* a, int code, const std::string& m) {
  if (a) a->last_error = m;
  return code;
}

inline Event pool_event(cep_app* a) {
  Event e;
  if (!a->event_pool.empty()) {
    e = std::move(a->event_pool.back());
    a->event_pool.pop_back();
  } else {
    e.create(hipEventDefault);
  }
  return e;
}

struct LaunchTimer {
  cep_app* a;
  int kind;
  hipStream_t st;
  Event s;
  // profile = k: HIP events around every k-th launch of each kernel kind
  // (each event between two kernels widens the gap between them by ~5 us)
  LaunchTimer(cep_app* app, int k, hipStream_t on = nullptr)
      : a(app), kind(k), st(on ? on : (hipStream_t)app->stream) {
    const bool timed = a->opt.profile > 0 && a->launches[k] % a->opt.profile == 0;
    a->launches[k]++;
    if (timed) {
      s = pool_event(a);
      hipEventRecord(s, st);
    }
  }
  ~LaunchTimer() {
    if (s) {
      Event e = pool_event(a);
      hipEventRecord(e, st);
      a->timed.push_back({kind, std::move(s), std::move(e)});
    }
  }
};

// engine.cpp
void harvest_timers(cep_app* a);
int ensure_out_cap(cep_app* a, OutStream& o, int64_t need);
OutArgs out_args(OutStream& o, const Query& q);
bool pref_aligned(const PrefPlan& pf, const RowsArgs& rows);
int run_pattern(cep_app* a, PatternRT& rt, const RowsArgs& rows_in, const uint64_t* in_recs = nullptr,
                int in_rec_words = 0, bool tolerant = false);
int batch_rows(cep_app* a, const cep_batch* b, RowsArgs* out, int* slot, bool* direct);
int send_device_rows(cep_app* a, const RowsArgs& rows_in);
int check_device_error(cep_app* a);
int error_status(cep_app* a, unsigned int e);
// mq_plan.cpp: multi-query groups of an app (plan-time grouping, device state)
int build_mq_groups(cep_app* a);
std::vector<int> mq_pref_cols(const MqRT& g);
// stamps.cpp: the CEP_STAMPS / CEP_WAVESTAMP report of the last launches
void dump_stamps(cep_app* a);

}  // namespace cep
