// Snapshot codec (snapshot.h): SnapImage <-> bytes, and the plan hash.
#include "snapshot.h"

#include <algorithm>
#include <cstring>
#include <functional>

#include "../../include/cep.h"

namespace cep {
namespace {

// One pass over the format (snap_io) serves both directions: Ar<true> appends
// the image's fields to `out`, Ar<false> fills them from untrusted bytes, every
// read bounds-checked (false past the end).
template <bool W>
struct Ar {
  std::vector<uint8_t>* out;
  const uint8_t* buf;
  size_t len, off;
  size_t left() const { return len - off; }
  bool raw(void* p, size_t n) {
    if (W) {
      out->insert(out->end(), (const uint8_t*)p, (const uint8_t*)p + n);
      return true;
    }
    if (n > len - off) return false;
    if (n) std::memcpy(p, buf + off, n);
    off += n;
    return true;
  }
  template <class T>
  bool operator()(T& v) { return raw(&v, sizeof(v)); }
};

struct Fail {
  std::string* why;
  int operator()(int code, const char* m) const {
    *why = m;
    return code;
  }
};

// One "live keys" section: u32 n_live (the caller's), then per live key,
// ascending in the key index, u32 dense key, (patterns) u64 header and u32 n,
// n x nw words.  A pattern keeps n partials per key, inline slots then a run of
// the pending pool; groups and tables keep one run of nw words.
struct Keys {
  int64_t kc, ks, kpb;
  int lg;
  uint32_t nw;
  std::function<uint64_t&(int64_t i, uint32_t j, uint32_t w)> word;
  const SnapGeometry::Pattern* pg;   // patterns
  SnapImage::Pattern* pat;
  std::vector<uint32_t>* present;    // tables: bit 0 per key (groups: live = a word is not zero)
  uint32_t ovf_bit;

  bool live(int64_t i) const {
    if (pat) return pat->hdr[i] != 0;
    if (present) return ((*present)[i] & 1u) != 0;
    for (uint32_t w = 0; w < nw; ++w)
      if (word(i, 0, w)) return true;
    return false;
  }
  uint32_t count() const {
    uint32_t n = 0;
    for (int64_t i = 0; i < ks; ++i) n += live(i) ? 1 : 0;
    return n;
  }
};

template <bool W>
int keys_io(Ar<W>& ar, const Keys& s, uint32_t nlive, uint32_t ver, const Fail& fail) {
  int64_t next = 0;
  for (uint32_t k = 0; k < nlive; ++k) {
    int64_t i = 0;
    uint32_t key = 0, n = 1;
    uint64_t h = 0;
    if (W) {
      while (!s.live(next)) ++next;
      i = next++;
      key = dense_key(i, s.kpb, s.lg);
      if (s.pat) {
        const bool ovf = (s.pat->hdr[i] & s.ovf_bit) && !s.pat->ext.empty();
        h = s.pat->hdr[i] & ~(uint64_t)s.ovf_bit;
        n = ovf ? (uint32_t)s.pat->ext[i] : (s.pat->hdr[i] & 0xff);
      }
    }
    if (!ar(key) || (s.pat && !ar(h))) return fail(CEP_E_STATE, s.pat ? "corrupt snapshot" : "truncated snapshot");
    if (!W && ((int64_t)key >= s.kc || (h & s.ovf_bit))) return fail(CEP_E_STATE, "corrupt snapshot");
    if (s.pat) {
      if (ver < 4) n = (uint32_t)(h & 0xff);
      else if (!ar(n)) return fail(CEP_E_STATE, "truncated snapshot");
      if (!W && (uint64_t)n * s.nw > ar.left() / 8) return fail(CEP_E_STATE, "truncated snapshot");
    }
    if (!W) {
      i = key_index(key, s.kpb, s.lg);
      if (s.present) (*s.present)[i] = 1;
    }
    if (!W && s.pat) {
      SnapImage::Pattern& p = *s.pat;
      const uint32_t S = s.pg->S;
      uint32_t hw = ((uint32_t)h & ~0xffu) | std::min(n, S);
      if (n > S) {   // overflow run: the pending pool (closed-form runtimes only)
        const uint64_t used = p.pool.size() / s.nw;
        if (p.ext.empty()) return fail(CEP_E_CAPACITY, "snapshot holds more than pending_slots partials for a key");
        if (used + (n - S) > (uint64_t)s.pg->pool_cap)
          return fail(CEP_E_CAPACITY, "snapshot's overflow partials exceed the pending pool");
        p.ext[i] = (uint64_t)n | (used << 32);
        p.pool.resize((used + (n - S)) * s.nw);
        hw |= s.ovf_bit;
      }
      p.hdr[i] = hw;
    }
    for (uint32_t j = 0; j < n; ++j)
      for (uint32_t w = 0; w < s.nw; ++w) {
        uint64_t& v = s.word(i, j, w);
        if (!ar(v)) return fail(CEP_E_STATE, "truncated snapshot");
        if (!W && s.pat && w == 0) s.pat->ts_max = std::max(s.pat->ts_max, (int64_t)v);
      }
  }
  return CEP_OK;
}

Keys pattern_keys(const SnapGeometry::Pattern& g, SnapImage::Pattern& p, uint32_t ovf_bit) {
  const uint32_t S = g.S, sw = g.slot_words;
  const int64_t ks = g.kstride;
  auto word = [&p, S, sw, ks, ovf_bit](int64_t i, uint32_t j, uint32_t w) -> uint64_t& {
    if (j < S) return p.slots[((size_t)j * sw + w) * ks + i];
    const uint64_t run = (p.hdr[i] & ovf_bit) && !p.ext.empty() ? p.ext[i] >> 32 : 0;
    return p.pool[(run + j - S) * sw + w];
  };
  return {g.key_capacity, ks, ks >> g.lg, g.lg, sw, word, &g, &p, nullptr, ovf_bit};
}

// state word w of bucket-major key index i = b * kpb + k lives at
// (b * words + w) * kpb + k (each bucket's state is one contiguous block)
Keys group_keys(const SnapGeometry::Group& g, std::vector<uint64_t>& st) {
  const int64_t kpb = g.kpb;
  const uint32_t nw = g.words;
  auto word = [&st, kpb, nw](int64_t i, uint32_t, uint32_t w) -> uint64_t& {
    return st[(size_t)(((i / kpb) * nw + w) * kpb + i % kpb)];
  };
  return {g.key_capacity, g.kstride, kpb, g.lg, nw, word, nullptr, nullptr, nullptr, 0};
}

Keys table_keys(const SnapGeometry::Table& g, SnapImage::Table& t) {
  const int64_t ks = g.kstride;
  auto word = [&t, ks](int64_t i, uint32_t, uint32_t w) -> uint64_t& { return t.words[(size_t)w * ks + i]; };
  return {g.key_capacity, ks, ks >> g.lg, g.lg, g.nwords, word, nullptr, nullptr, &t.hdr, 0};
}

// The sparse-key map as the device's hash table (same hash and probing as
// keymap.hip; any valid placement serves lookups).
void rehash_keys(uint64_t table_cap, SnapImage::Pattern* m) {
  m->tkey.assign(table_cap, 0);
  m->tval.assign(table_cap, 0xffffffffu);
  for (uint32_t id = 0; id < m->kcount[0]; ++id) {
    if (id == m->kcount[1]) continue;   // the value -1 has its own word
    const uint64_t v = m->krev[id];
    uint64_t z = v + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    uint64_t h = (z ^ (z >> 31)) & (table_cap - 1);
    while (m->tkey[h]) h = (h + 1) & (table_cap - 1);
    m->tkey[h] = v + 1;
    m->tval[h] = id;
  }
}

// i64 key_capacity, u32 words, u32 n_live of a group or table section, then its keys.
template <bool W>
int keyed_io(Ar<W>& ar, const Keys& s, uint32_t ver, const char* geometry, const Fail& fail) {
  int64_t kc = s.kc;
  uint32_t nw = s.nw, nl = W ? s.count() : 0;
  if (!ar(kc) || !ar(nw) || !ar(nl)) return fail(CEP_E_STATE, "truncated snapshot");
  if (kc != s.kc || nw != s.nw || nl > (uint64_t)kc) return fail(CEP_E_STATE, geometry);
  if (!W && (uint64_t)nl * (4 + 8ull * nw) > ar.left()) return fail(CEP_E_STATE, "truncated snapshot");
  return keys_io(ar, s, nl, ver, fail);
}

template <bool W>
int snap_io(Ar<W>& ar, const SnapGeometry& geo, SnapImage& img, const Fail& fail) {
  char magic[4] = {'C', 'E', 'P', 'S'};
  // 3: + the event-time reorder buffer; 4: + pending counts (overflow runs); 5: + groups; 6: + joins; 7: + tables
  uint32_t ver = !geo.tabs.empty() ? 7 : geo.joins.empty() ? 5 : 6, np = (uint32_t)geo.pats.size();
  uint64_t h = geo.plan_hash;
  if (!ar.raw(magic, 4) || std::memcmp(magic, "CEPS", 4) || !ar(ver) || ver < 2 || ver > 7 || !ar(h) ||
      !ar(img.events_in) || !ar(np))
    return fail(CEP_E_STATE, "not a libcep snapshot");
  if (!W) img.version = ver;
  if (h != geo.plan_hash || np != geo.pats.size())
    return fail(CEP_E_STATE, "snapshot was taken with a different plan (or a build that compiled it "
                             "differently: 2-state patterns with s1-dependent conditions need CEP_PAIR_WALK=1 "
                             "to restore snapshots of builds before round 4)");
  if (!W) {
    img.pats.resize(geo.pats.size());
    img.groups.resize(geo.groups.size());
    img.joins.resize(geo.joins.size());
    img.tabs.resize(geo.tabs.size());
  }
  for (size_t pi = 0; pi < geo.pats.size(); ++pi) {
    const auto& g = geo.pats[pi];
    auto& p = img.pats[pi];
    if (!W) {
      p.hdr.assign(g.kstride, 0);
      p.slots.assign((size_t)g.kstride * g.S * g.slot_words, 0);
      if (g.has_kext) p.ext.assign(g.kstride, 0);
    }
    const Keys s = pattern_keys(g, p, geo.hdr_ovf);
    int64_t kc = g.key_capacity;
    uint32_t S = g.S, sw = g.slot_words, live = W ? s.count() : 0;
    if (!ar(kc) || !ar(S) || !ar(sw) || !ar(live)) return fail(CEP_E_STATE, "truncated snapshot");
    if (kc != g.key_capacity || S != g.S || sw != g.slot_words)
      return fail(CEP_E_STATE, "snapshot geometry differs from this runtime");
    if ((uint64_t)live > (uint64_t)kc) return fail(CEP_E_STATE, "corrupt snapshot (live keys)");
    if (const int rc = keys_io(ar, s, live, ver, fail)) return rc;
  }
  // rows waiting for a watermark (the operator checkpoints its PriorityQueue
  // as "queuedRecordsState": AbstractSiddhiOperator.java:98, 396-404)
  if (ver >= 3) {
    auto& ro = img.ro;
    int32_t in = ro.n > 0 ? ro.input : -1;
    uint8_t hs = ro.has_stream ? 1 : 0;
    if (!ar(in) || !ar(hs) || !ar(ro.n) || !ar(ro.released_max) || ro.n < 0 || ro.n > (int64_t)INT32_MAX ||
        (ro.n > 0 && (in < 0 || in >= (int)geo.inputs.size())))
      return fail(CEP_E_STATE, "corrupt snapshot (reorder buffer)");
    if (!W) ro.input = in, ro.has_stream = hs != 0;
    if (ro.n > 0) {
      size_t row_bytes = 8 + (hs ? 1 : 0);
      for (int w : geo.inputs[in]) row_bytes += (size_t)w;
      if (!W && (uint64_t)ro.n > ar.left() / row_bytes) return fail(CEP_E_STATE, "truncated snapshot (reorder buffer)");
      if (!W) ro.rows.resize((size_t)ro.n * row_bytes);
      if (!ar.raw(ro.rows.data(), ro.rows.size())) return fail(CEP_E_STATE, "truncated snapshot (reorder buffer)");
    }
  }
  // (version 4) per pattern: the sparse-key map, dense slot -> value
  for (size_t pi = 0; pi < geo.pats.size(); ++pi) {
    const auto& g = geo.pats[pi];
    auto& m = img.pats[pi];
    if (ver < 4) {
      if (g.sparse) return fail(CEP_E_STATE, "snapshot has no key map (version < 4)");
      continue;
    }
    uint8_t sp = g.sparse ? 1 : 0;
    if (!ar(sp) || (sp != 0) != g.sparse) return fail(CEP_E_STATE, "snapshot key map does not match");
    if (!sp) continue;
    if (!ar.raw(m.kcount, 8) || (!W && (m.kcount[0] > (uint64_t)g.key_capacity || m.kcount[0] > ar.left() / 8)))
      return fail(CEP_E_STATE, "corrupt snapshot (key map)");
    if (!W) m.krev.resize(m.kcount[0]);
    if (!ar.raw(m.krev.data(), m.krev.size() * 8)) return fail(CEP_E_STATE, "corrupt snapshot (key map)");
    if (!W) rehash_keys(g.table_cap, &m);
  }
  // (version 5) multi-query groups: per group every key whose state is not
  // all zero, with the group's state words (query by query, plan order)
  if (ver >= 5) {
    uint32_t ng = (uint32_t)geo.groups.size();
    if (!ar(ng) || ng != geo.groups.size()) return fail(CEP_E_STATE, "snapshot multi-query groups do not match");
    for (size_t gi = 0; gi < geo.groups.size(); ++gi) {
      const auto& g = geo.groups[gi];
      if (!W) img.groups[gi].assign((size_t)g.words * g.kstride, 0);
      if (const int rc = keyed_io(ar, group_keys(g, img.groups[gi]), ver, "snapshot geometry differs from this runtime", fail))
        return rc;
    }
  } else if (!geo.groups.empty()) {
    // v2-v4 kept these queries on per-query runtimes: a runtime created with
    // CEP_NO_MQ=1 has that layout and restores the snapshot
    return fail(CEP_E_STATE, "snapshot has no multi-query group state (version < 5): "
                             "create the runtime with CEP_NO_MQ=1 to restore it on per-query state");
  }
  // (version 6) joins: each side's live rows (the list's tail) and counts
  if (ver >= 6) {
    uint32_t nj = (uint32_t)geo.joins.size();
    if (!ar(nj) || nj != geo.joins.size()) return fail(CEP_E_STATE, "snapshot joins do not match");
    for (size_t ji = 0; ji < geo.joins.size(); ++ji) {
      const auto& g = geo.joins[ji];
      auto& j = img.joins[ji];
      uint32_t ew = g.ew;
      if (!ar(ew) || ew != g.ew) return fail(CEP_E_STATE, "snapshot geometry differs from this runtime (join rows)");
      for (int sd = 0; sd < 2; ++sd) {
        if (!ar(j.kept[sd]) || !ar(j.tail[sd])) return fail(CEP_E_STATE, "truncated snapshot");
        const uint64_t tail = j.tail[sd];
        const uint64_t max_tail = g.win_kind[sd] == WIN_LENGTH ? (uint64_t)g.win_param[sd] : geo.join_tail_cap;
        if (!W && (tail > max_tail || tail * ew > ar.left() / 8)) return fail(CEP_E_STATE, "corrupt snapshot (join rows)");
        if (!W) j.rows[sd].resize((size_t)tail * ew);
        if (!ar.raw(j.rows[sd].data(), j.rows[sd].size() * 8)) return fail(CEP_E_STATE, "corrupt snapshot (join rows)");
      }
    }
  } else if (!geo.joins.empty()) {
    return fail(CEP_E_STATE, "snapshot has no join state (version < 6)");
  }
  // (version 7) tables: per table its live rows, by dense key
  if (ver >= 7) {
    uint32_t nt = (uint32_t)geo.tabs.size();
    if (!ar(nt) || nt != geo.tabs.size()) return fail(CEP_E_STATE, "snapshot tables do not match");
    for (size_t ti = 0; ti < geo.tabs.size(); ++ti) {
      const auto& g = geo.tabs[ti];
      if (!W) {
        img.tabs[ti].hdr.assign(g.kstride, 0);
        img.tabs[ti].words.assign((size_t)g.kstride * g.nwords, 0);
      }
      if (const int rc = keyed_io(ar, table_keys(g, img.tabs[ti]), ver,
                                  "snapshot geometry differs from this runtime (table rows)", fail))
        return rc;
    }
    if (!ar(img.tab_dropped)) return fail(CEP_E_STATE, "truncated snapshot");
  } else if (!geo.tabs.empty()) {
    return fail(CEP_E_STATE, "snapshot has no table state (version < 7)");
  }
  return CEP_OK;
}

}  // namespace

std::vector<uint8_t> snapshot_encode(const SnapImage& img) {
  std::vector<uint8_t> out;
  std::string why;
  Ar<true> ar{&out, nullptr, 0, 0};
  snap_io(ar, img.geo, const_cast<SnapImage&>(img), Fail{&why});   // (writing reads the image only)
  return out;
}

int snapshot_decode(const SnapGeometry& geo, const uint8_t* buf, size_t len, SnapImage* img, std::string* why) {
  *img = SnapImage();
  img->geo = geo;
  Ar<false> ar{nullptr, buf, len, 0};
  return snap_io(ar, geo, *img, Fail{why});
}

uint64_t plan_hash(const CompiledApp& app) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  };
  mix(app.code.data(), app.code.size() * sizeof(Ins));
  mix(app.konst.data(), app.konst.size() * 8);
  // window kind and parameter (plans without a window hash as before)
  for (size_t qi = 0; qi < app.queries.size(); ++qi) {
    const Query& q = app.queries[qi];
    if (q.win_kind == WIN_NONE) continue;
    const int64_t w[4] = {(int64_t)qi, q.win_kind, q.win_param, q.win_global ? 1 : 0};
    mix(w, sizeof(w));
    // tumbling windows: the time attribute's column (sliding plans hash as before)
    if (win_is_batch(q.win_kind)) {
      const int64_t c = q.win_col;
      mix(&c, sizeof(c));
    }
  }
  // joins: sides, windows, carried columns (plans without a join hash as before)
  for (size_t qi = 0; qi < app.queries.size(); ++qi) {
    const Query& q = app.queries[qi];
    if (q.kind != Q_JOIN) continue;
    const int64_t w[8] = {-3, (int64_t)qi, q.a_stream, q.b_stream, q.join_side[0].win_kind, q.join_side[0].win_param,
                          q.join_side[1].win_kind, q.join_side[1].win_param};
    mix(w, sizeof(w));
    for (int c : q.rec_cols_a) mix(&c, sizeof(c));
  }
  // tables: definitions and operations (plans without a table hash as before)
  for (size_t ti = 0; ti < app.tables.size(); ++ti) {
    const TableDef& T = app.tables[ti];
    const int64_t w[4] = {-4, (int64_t)ti, T.pk, (int64_t)T.schema.attrs.size()};
    mix(w, sizeof(w));
    mix(T.schema.id.data(), T.schema.id.size());
    for (auto& at : T.schema.attrs) {
      mix(at.name.data(), at.name.size());
      mix(&at.type, sizeof(at.type));
    }
    for (int qi : T.ops) {
      const Query& q = app.queries[qi];
      const int64_t o[6] = {-5, qi, q.tab_op, q.in_stream, q.tab_key_col, q.tab_negate ? 1 : 0};
      mix(o, sizeof(o));
      mix(q.tab_ins, sizeof(q.tab_ins));
      mix(q.tab_set, sizeof(q.tab_set));
    }
  }
  // logical pattern states: `A -> B and C` and `A -> B or C` compile to the
  // same code (plans without one hash as before)
  for (size_t qi = 0; qi < app.queries.size(); ++qi) {
    const Query& q = app.queries[qi];
    bool any = false;
    for (auto& st : q.nstates) any = any || st.logic != 0;
    if (!any) continue;
    const int64_t w[2] = {-6, (int64_t)qi};
    mix(w, sizeof(w));
    for (auto& st : q.nstates) mix(&st.logic, sizeof(st.logic));
  }
  // count states in patterns: `B<2:4>` and `B<2:5>` compile to the same code
  // (a sequence's counts stay out, and every other plan hashes as before)
  for (size_t qi = 0; qi < app.queries.size(); ++qi) {
    const Query& q = app.queries[qi];
    bool any = false;
    for (auto& st : q.nstates) any = any || st.min_count != 1 || st.max_count != 1;
    if (!any || q.sequence) continue;
    const int64_t w[2] = {-7, (int64_t)qi};
    mix(w, sizeof(w));
    for (auto& st : q.nstates) {
      mix(&st.min_count, sizeof(st.min_count));
      mix(&st.max_count, sizeof(st.max_count));
    }
  }
  // query chaining (plans without derived streams hash as before)
  for (auto& d : app.derived) {
    const int64_t w[5] = {-1, d.stream, d.producer, d.source, d.stage};
    mix(w, sizeof(w));
  }
  for (size_t qi = 0; qi < app.queries.size(); ++qi) {
    if (app.queries[qi].view < 0) continue;
    const int64_t w[3] = {-2, (int64_t)qi, app.queries[qi].view};
    mix(w, sizeof(w));
    for (int di : app.views[app.queries[qi].view].derived) mix(&di, sizeof(di));
  }
  return h;
}

}  // namespace cep
