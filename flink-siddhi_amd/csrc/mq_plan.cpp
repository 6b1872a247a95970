// Multi-query groups: plan-time grouping of an app's keyed queries and the
// groups' device descriptors, state and chunk arenas (run by engine.cpp run_mq).
#include <cstring>

#include "rt.h"

namespace cep {

// ---- multi-query groups (mq_kernels.hip) ------------------------------------
// A query joins a group when its per-event work is interpreter-free and keyed
// on the group's key column: group-by aggregations (term-list filter, plain
// column arguments, select items key / aggregate / column, having on one
// output item) and sequences of the one-live-partial shape (a single start
// event on a stream no later state reads) with own-column term-list
// conditions and first / last captures.  Queries of one group share the
// partition pass (one read of the batch, each distinct condition evaluated
// once per row) and the walk (AbstractSiddhiOperator.java:283-287: every
// event goes to every query).  CEP_NO_MQ=1: no groups (general path).
static bool same_layout(const CompiledApp& app, int s, int t) {
  const auto& x = app.inputs[s].attrs;
  const auto& y = app.inputs[t].attrs;
  if (x.size() != y.size()) return false;
  for (size_t c = 0; c < x.size(); ++c)
    if (x[c].type != y[c].type) return false;
  return true;
}

static bool same_terms(const TermList& x, const TermList& y) {
  if (x.n != y.n || x.any != y.any) return false;
  for (int i = 0; i < x.n; ++i) {
    const Term &u = x.t[i], &v = y.t[i];
    if (u.col != v.col || u.coltype != v.coltype || u.aop != v.aop || u.atype != v.atype || u.aconst != v.aconst ||
        u.cop != v.cop || u.ctype != v.ctype || u.cconst != v.cconst)
      return false;
  }
  return true;
}

// What one query adds to a group: its conditions per stream, carried columns.
struct MqNeeds {
  int key_col = -1, layout = -1;
  std::vector<std::pair<int, TermList>> conds;   // (stream, condition), n == 0: always true
  std::vector<int> carry;                        // columns carried in records
  std::vector<int> cols;                         // columns conditions read
};

static bool mq_candidate(const cep_app* a, const Query& q, MqNeeds* nd) {
  const CompiledApp& app = a->app;
  if (a->opt.sparse_keys) return false;
  auto key_ok = [&](int s, int col) {
    if (s < 0 || col < 0) return false;
    const int t = app.inputs[s].attrs[col].type;
    return t == T_INT || t == T_LONG;
  };
  auto add_cols = [&](const TermList& tl) {
    for (int i = 0; i < tl.n; ++i)
      if (std::find(nd->cols.begin(), nd->cols.end(), tl.t[i].col) == nd->cols.end()) nd->cols.push_back(tl.t[i].col);
  };
  auto carry = [&](int col) {
    if (col == nd->key_col) return;
    if (std::find(nd->carry.begin(), nd->carry.end(), col) == nd->carry.end()) nd->carry.push_back(col);
  };
  if (q.kind == Q_AGG) {
    // a windowed aggregate keeps a ring per key: its own pipeline (k_winwalk)
    if (q.win_kind != WIN_NONE) return false;
    if (q.in_stream < 0 || !key_ok(q.in_stream, q.key_col)) return false;
    if ((int)q.aggs.size() > kMqMaxAggs || !q.having_simple || (int)q.select.size() > kMqMaxSel) return false;
    if (q.f.valid() && q.f_terms.n < 0) return false;
    nd->key_col = q.key_col;
    nd->layout = q.in_stream;
    TermList f;
    f.n = 0;
    if (q.f.valid()) f = q.f_terms;
    nd->conds.push_back({q.in_stream, f});
    add_cols(f);
    for (auto& ag : q.aggs) {
      if (ag.arg.valid() && ag.word < 0) return false;
      if (ag.word >= 0) carry(q.rec_cols_a[ag.word]);
    }
    for (auto& it : q.select) {
      if (it.src == SRC_KEY || (it.src >= SRC_AGG && it.src < SRC_AGG + (int)q.aggs.size())) continue;
      if (it.src >= SRC_REC && it.src < SRC_REC + (int)q.rec_cols_a.size()) {
        carry(q.rec_cols_a[it.src - SRC_REC]);
        continue;
      }
      return false;
    }
    return true;
  }
  if (q.kind != Q_PATTERN || !q.nfa || !q.sequence) return false;
  const int n = (int)q.nstates.size();
  if (n < 1 || n > kMaxStates || q.nstates[0].min_count != 1 || q.nstates[0].max_count != 1) return false;
  if ((int)q.ncaps.size() > kMqMaxCaps || (int)q.select.size() > kMqMaxSel) return false;
  for (int j = 0; j < n; ++j) {
    const auto& st = q.nstates[j];
    if (st.logic) return false;   // logical states: the stand-alone walk only
    if (j > 0 && st.stream == q.nstates[0].stream) return false;   // one live partial per key
    if (st.walk.valid() || st.terms.n < 0 || st.min_count > 254 || st.max_count > 254) return false;
    const int col = st.stream < (int)q.key_col_s.size() ? q.key_col_s[st.stream] : -1;
    if (!key_ok(st.stream, col) || (nd->key_col >= 0 && col != nd->key_col)) return false;
    if (!same_layout(app, st.stream, q.nstates[0].stream)) return false;
    nd->key_col = col;
  }
  nd->layout = q.nstates[0].stream;
  for (int j = 0; j < n; ++j) {
    nd->conds.push_back({q.nstates[j].stream, q.nstates[j].terms});
    add_cols(q.nstates[j].terms);
  }
  for (auto& cp : q.ncaps) {
    if (cp.index != 0 && cp.index != -1) return false;
    // the group units clear a new partial's captures to 0, which is the null
    // of every type but STRING (dictionary id -1, cep.h): a STRING capture of
    // a state a match may skip stays on the stand-alone walk (cap_null)
    const auto& cs = q.nstates[cp.state];
    const int ccol = q.rec_cols_a[cp.word];
    if (cs.min_count == 0 && ccol >= 0 && ccol < (int)app.inputs[cs.stream].attrs.size() &&
        app.inputs[cs.stream].attrs[ccol].type == T_STRING)
      return false;
    carry(ccol);
  }
  for (auto& it : q.select)
    if (!(it.src == SRC_KEY || (it.src >= SRC_CAP && it.src < SRC_CAP + (int)q.ncaps.size()))) return false;
  return true;
}

static int mq_index(std::vector<int>& v, int x) {
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == x) return (int)i;
  v.push_back(x);
  return (int)v.size() - 1;
}

// Condition bit of `tl` on stream s in group g (added when new); -1: full.
static int mq_cond_bit(MqRT& g, int s, const TermList& tl, bool add) {
  if (tl.n == 0) return kMqTrueBit;
  for (int c = 0; c < g.ncond[s]; ++c)
    if (same_terms(g.conds[s * kMqMaxCond + c].tl, tl)) return c;
  if (g.ncond[s] >= kMqMaxCond) return -1;
  if (!add) return g.ncond[s];
  MqCond& mc = g.conds[s * kMqMaxCond + g.ncond[s]];
  std::memset(&mc, 0, sizeof(mc));
  mc.tl = tl;
  return g.ncond[s]++;
}

// Prefetched columns of a group: the key first, then condition and carried
// columns (k_mqpart loads each once per row).
std::vector<int> mq_pref_cols(const MqRT& g) {
  std::vector<int> v{g.key_col};
  for (int c : g.cond_cols) mq_index(v, c);
  for (int c : g.carry) mq_index(v, c);
  return v;
}

// A shape class of one group's queries (walk unit kinds, kernels.h MqUnit).
struct MqClassB {
  int kind = MQU_SEQ;
  std::string sig;
  int key_col = -1, layout = -1;
  int view = -1;
  std::vector<int> qs;
  std::vector<MqNeeds> nds;
};

// Shape signature: queries with equal signatures run as one walk unit
// (sequence classes advance bit-parallel, aggregations share the decode).
static std::string mq_signature(const cep_app* a, const Query& q, const MqNeeds& nd, int* kind) {
  const CompiledApp& app = a->app;
  std::string sg = std::to_string(nd.key_col) + "/" + std::to_string(nd.layout) + "/" + std::to_string(q.view) + "|";
  auto add = [&](int64_t v) { sg += std::to_string(v) + ","; };
  const auto& od = app.outputs[app.output_index(q.out_stream)];
  for (auto& at : od.attrs) add(at.type);
  sg += "|";
  for (auto& it : q.select) add(it.src >= SRC_REC && it.src < SRC_REC + (int)q.rec_cols_a.size()
                                    ? 1000 + q.rec_cols_a[it.src - SRC_REC] : it.src);
  sg += "|";
  if (q.kind == Q_AGG) {
    *kind = MQU_AGG;
    add(q.in_stream);
    for (auto& ag : q.aggs) {
      add(ag.fn);
      add(ag.word >= 0 ? q.rec_cols_a[ag.word] : -1);
      add(ag.arg_type);
      add(ag.out_type);
    }
    sg += "|";
    add(q.having_item);
    if (q.having_item >= 0) {
      add(q.having_cop);
      add(q.having_ctype);
    }
    return "A" + sg;
  }
  // sequences: bit-parallel when every state reads its own stream and counts
  // "one" or "one or more" (optional states allowed)
  bool bp = true;
  const int n = (int)q.nstates.size();
  for (int j = 0; j < n; ++j) {
    const auto& st = q.nstates[j];
    for (int k = 0; k < j; ++k) bp = bp && q.nstates[k].stream != st.stream;
    bp = bp && st.min_count <= 1 && (st.max_count == 1 || st.max_count < 0);
  }
  *kind = bp ? MQU_SEQ_BP : MQU_SEQ;
  add(q.every ? 1 : 0);
  add(q.within);
  for (auto& st : q.nstates) {
    add(st.stream);
    add(st.min_count);
    add(st.max_count);
  }
  sg += "|";
  for (auto& cp : q.ncaps) {
    add(cp.state);
    add(cp.index);
    add(q.rec_cols_a[cp.word]);
  }
  return "S" + sg;
}

// Record bit of a run of conditions on stream s (query order), sharing an
// identical run already placed; -1 when the stream's bits are used up.
static int mq_cond_run(MqRT& g, int s, const std::vector<TermList>& run, bool add) {
  const int n = (int)run.size();
  for (int i = 0; i + n <= g.ncond[s]; ++i) {
    bool same = true;
    for (int j = 0; j < n && same; ++j) same = same_terms(g.conds[s * kMqMaxCond + i + j].tl, run[j]);
    if (same) return i;
  }
  if (g.ncond[s] + n > kMqMaxCond) return -1;
  if (!add) return g.ncond[s];
  const int at = g.ncond[s];
  for (int j = 0; j < n; ++j) {
    MqCond& mc = g.conds[s * kMqMaxCond + at + j];
    std::memset(&mc, 0, sizeof(mc));
    mc.tl = run[j];
  }
  g.ncond[s] += n;
  return at;
}

// Place a class's conditions into group g (bit-parallel classes: one run per
// state; others: one bit per distinct condition).  false: no room.
static bool mq_place_conds(const cep_app* a, MqRT& g, const MqClassB& c) {
  const CompiledApp& app = a->app;
  if (c.kind == MQU_SEQ_BP) {
    const Query& q0 = app.queries[c.qs[0]];
    for (size_t j = 0; j < q0.nstates.size(); ++j) {
      std::vector<TermList> run;
      bool any = false;
      for (int qi : c.qs) {
        run.push_back(app.queries[qi].nstates[j].terms);
        any = any || app.queries[qi].nstates[j].terms.n > 0;
      }
      if (any && mq_cond_run(g, q0.nstates[j].stream, run, true) < 0) return false;
    }
    return true;
  }
  for (auto& nd : c.nds)
    for (auto& cd : nd.conds)
      if (cd.second.n > 0 && mq_cond_run(g, cd.first, {cd.second}, true) < 0) return false;
  return true;
}

int build_mq_groups(cep_app* a) {
  const CompiledApp& app = a->app;
  a->in_mq.assign(app.queries.size(), 0);
  if (std::getenv("CEP_NO_MQ") || app.inputs.size() > 8) return CEP_OK;
  // shape classes of the candidates, in plan order of their first query
  std::vector<MqClassB> classes;
  for (size_t qi = 0; qi < app.queries.size(); ++qi) {
    MqNeeds nd;
    if (!mq_candidate(a, app.queries[qi], &nd)) continue;
    int kind;
    const std::string sig = mq_signature(a, app.queries[qi], nd, &kind);
    MqClassB* c = nullptr;
    for (auto& x : classes)
      if (x.sig == sig && x.kind != MQU_SEQ && (int)x.qs.size() < (x.kind == MQU_SEQ_BP ? kMqMaxCond : kMqMaxQ))
        c = &x;
    if (!c) {
      classes.push_back(MqClassB());
      c = &classes.back();
      c->kind = kind;
      c->sig = sig;
      c->key_col = nd.key_col;
      c->layout = nd.layout;
      c->view = app.queries[qi].view;
    }
    c->qs.push_back((int)qi);
    c->nds.push_back(nd);
  }
  // classes into groups: a class joins the first group with room (queries,
  // carried / prefetched columns, condition bits); a class too large for an
  // empty group is halved
  std::vector<int> layouts;   // per group: a stream of its layout
  std::vector<std::vector<MqClassB>> gclasses;
  for (size_t ci = 0; ci < classes.size(); ++ci) {
    MqClassB c = classes[ci];
    auto fits = [&](MqRT& g) {
      MqRT t;
      t.key_col = g.key_col;
      t.cond_cols = g.cond_cols;
      t.carry = g.carry;
      t.conds = g.conds;
      std::copy(g.ncond, g.ncond + 8, t.ncond);
      for (auto& nd : c.nds) {
        for (int x : nd.cols) mq_index(t.cond_cols, x);
        for (int x : nd.carry) mq_index(t.carry, x);
      }
      if ((int)t.carry.size() > kMqMaxCarry || (int)mq_pref_cols(t).size() > kPref) return false;
      if ((int)(g.qs.size() + c.qs.size()) > kMqMaxQ) return false;
      if (!mq_place_conds(a, t, c)) return false;
      g.cond_cols = t.cond_cols;
      g.carry = t.carry;
      g.conds = t.conds;
      std::copy(t.ncond, t.ncond + 8, g.ncond);
      return true;
    };
    int gi = -1;
    for (size_t i = 0; i < a->mqs.size() && gi < 0; ++i)
      if (a->mqs[i].key_col == c.key_col && a->mqs[i].view == c.view && same_layout(app, layouts[i], c.layout) &&
          fits(a->mqs[i]))
        gi = (int)i;
    if (gi < 0) {
      MqRT g;
      g.key_col = c.key_col;
      g.view = c.view;
      g.conds.resize(8 * kMqMaxCond);
      if (!fits(g)) {
        if (c.qs.size() > 1) {   // halve the class and place both halves
          MqClassB h = c;
          const size_t m = c.qs.size() / 2;
          c.qs.resize(m);
          c.nds.resize(m);
          h.qs.erase(h.qs.begin(), h.qs.begin() + m);
          h.nds.erase(h.nds.begin(), h.nds.begin() + m);
          classes[ci] = c;
          classes.insert(classes.begin() + ci + 1, h);
          --ci;
        }
        continue;   // a single query that fits no group: general path
      }
      a->mqs.push_back(std::move(g));
      layouts.push_back(c.layout);
      gclasses.emplace_back();
      gi = (int)a->mqs.size() - 1;
    }
    MqRT& g = a->mqs[gi];
    for (int qi : c.qs) {
      g.qs.push_back(qi);
      a->in_mq[qi] = 1;
    }
    gclasses[gi].push_back(c);
  }
  // a group of one query stays on its own PatternRT: the key shuffle entry
  // points (cep_route_batch / cep_send_records) and v2-v4 snapshots of such
  // apps address that runtime
  for (size_t gi = a->mqs.size(); gi-- > 0;) {
    if (a->mqs[gi].qs.size() >= 2) continue;
    for (int qi : a->mqs[gi].qs) a->in_mq[qi] = 0;
    a->mqs.erase(a->mqs.begin() + gi);
    gclasses.erase(gclasses.begin() + gi);
    layouts.erase(layouts.begin() + gi);
  }
  for (size_t gi = 0; gi < a->mqs.size(); ++gi)
    for (auto& c : gclasses[gi]) {
      a->mqs[gi].classes_kind.push_back(c.kind);
      a->mqs[gi].classes_n.push_back((int)c.qs.size());
    }
  // device descriptors, state and arenas per group
  for (auto& g : a->mqs) {
    const int64_t K = a->opt.key_capacity;
    g.key_capacity = K;
    g.key_stride = std::max(1, a->opt.key_stride);
    g.key_offset = a->opt.key_offset;
    int64_t chunk = std::max<int64_t>(a->opt.chunk_events, kMqTile);
    chunk = std::min<int64_t>(chunk, (int64_t)kMqMaxTiles * kMqTile);
    g.pipe.chunk = (chunk / kMqTile) * kMqTile;
    const int nphys_max = std::min<int>((int)g.carry.size(), kMqMaxPhys);
    const int W = mq_window(nphys_max);
    // keys per bucket: about half a window of records per bucket per chunk
    int64_t kpb = 64;
    while (kpb * 2 <= kMqMaxKpb && (double)g.pipe.chunk * (double)(kpb * 2) / (double)K <= W / 2) kpb *= 2;
    int lg = 0;
    while (((K + (1 << lg) - 1) >> lg) > kpb) ++lg;
    while (lg > 0 && (1 << lg) > kMqMaxBuckets) --lg;
    kpb = (K + (1 << lg) - 1) >> lg;
    if (kpb > kMqMaxKpb) return fail(a, CEP_E_CAPACITY, "key_capacity too large for a multi-query group");
    g.lg = lg;
    g.kpb = (int)kpb;
    g.kstride = kpb << lg;
    // descriptors (class order), then the walk units
    int64_t off = 0;
    std::vector<int> qkind;   // per descriptor: its class's unit kind
    for (size_t ci = 0; ci < g.classes_kind.size(); ++ci)
      for (int i = 0; i < g.classes_n[ci]; ++i) qkind.push_back(g.classes_kind[ci]);
    for (int qi : g.qs) {
      const Query& q = app.queries[qi];
      MqQuery d;
      std::memset(&d, 0, sizeof(d));
      d.st_off = off;
      const int oi = app.output_index(q.out_stream);
      const auto& od = app.outputs[oi];
      d.nsel = (int)q.select.size();
      for (int i = 0; i < d.nsel; ++i) d.sel_type[i] = od.attrs[i].type;
      d.hav_item = -1;
      auto lword = [&](int col) { return col == g.key_col ? (int)MQ_SRC_KEY : mq_index(g.carry, col); };
      if (q.kind == Q_AGG) {
        d.kind = MQ_AGG;
        d.in_stream = q.in_stream;
        d.stream_mask = 1u << q.in_stream;
        TermList f;
        f.n = 0;
        if (q.f.valid()) f = q.f_terms;
        d.filter_bit = mq_cond_bit(g, q.in_stream, f, false);
        d.nagg = (int)q.aggs.size();
        for (int i = 0; i < d.nagg; ++i) {
          d.agg_fn[i] = q.aggs[i].fn;
          d.agg_arg_type[i] = q.aggs[i].arg_type;
          d.agg_out_type[i] = q.aggs[i].out_type;
          d.agg_src[i] = q.aggs[i].word >= 0 ? lword(q.rec_cols_a[q.aggs[i].word]) : (int)MQ_SRC_KEY;
        }
        for (int i = 0; i < d.nsel; ++i) {
          const int src = q.select[i].src;
          d.sel_src[i] = (src >= SRC_REC && src < SRC_REC + (int)q.rec_cols_a.size())
                             ? SRC_REC + lword(q.rec_cols_a[src - SRC_REC])
                             : src;
        }
        if (q.having_item >= 0) {
          d.hav_item = q.having_item;
          d.hav_cop = q.having_cop;
          d.hav_ctype = q.having_ctype;
          d.hav_cconst = q.having_cconst;
        }
        d.nwords = 1 + d.nagg;
      } else {
        d.kind = MQ_SEQ;
        d.nstates = (int)q.nstates.size();
        d.every = q.every ? 1 : 0;
        d.within = q.within;
        for (int j = 0; j < d.nstates; ++j) {
          const auto& st = q.nstates[j];
          d.stream_mask |= 1u << st.stream;
          d.st_stream |= (uint32_t)st.stream << (3 * j);
          d.st_bit |= (uint64_t)mq_cond_bit(g, st.stream, st.terms, false) << (6 * j);
          d.st_min |= (uint64_t)st.min_count << (8 * j);
          d.st_max |= (uint64_t)(st.max_count < 0 ? 0xff : st.max_count) << (8 * j);
          bool opt = true;
          for (int k = j + 1; k < d.nstates; ++k) opt = opt && q.nstates[k].min_count == 0;
          if (opt) d.tail_opt |= 1u << j;
        }
        d.ncap = (int)q.ncaps.size();
        for (int i = 0; i < d.ncap; ++i) {
          d.cap_state[i] = q.ncaps[i].state;
          d.cap_last[i] = q.ncaps[i].index < 0 ? 1 : 0;
          d.cap_src[i] = lword(q.rec_cols_a[q.ncaps[i].word]);
        }
        for (int i = 0; i < d.nsel; ++i) d.sel_src[i] = q.select[i].src;
        d.nwords = 2 + d.ncap;
      }
      for (int i = 0; i < d.nsel; ++i) {
        const int src = d.sel_src[i];
        d.sel_vi[i] = (src >= SRC_CAP && src < SRC_CAP + kMqMaxCaps) ? 1 + (src - SRC_CAP)
                      : (src >= SRC_AGG && src < SRC_AGG + kMqMaxAggs) ? 1 + (src - SRC_AGG)
                      : (src >= SRC_REC && src < SRC_REC + kMqMaxCarry) ? 5 + (src - SRC_REC)
                                                                         : 0;
        d.sel_w[i] = type_width(d.sel_type[i]);
      }
      d.hav_vi = d.hav_item >= 0 ? d.sel_vi[d.hav_item] : 0;
      g.stream_mask |= d.stream_mask;
      g.check_order = g.check_order || (d.kind == MQ_SEQ && d.within >= 0);
      if (qkind[g.hq.size()] == MQU_SEQ_BP) d.nwords = 0;   // class state (unit)
      off += d.nwords;
      g.hq.push_back(d);
    }
    g.units.clear();
    for (size_t ci = 0, q0 = 0; ci < g.classes_kind.size(); q0 += g.classes_n[ci], ++ci) {
      const int n = g.classes_n[ci];
      MqUnit u;
      std::memset(&u, 0, sizeof(u));
      u.kind = g.classes_kind[ci];
      u.q0 = (int)q0;
      if (u.kind == MQU_SEQ) {
        for (int i = 0; i < n; ++i) {
          u.q0 = (int)q0 + i;
          u.nq = 1;
          g.units.push_back(u);
        }
      } else if (u.kind == MQU_SEQ_BP) {
        const Query& q = app.queries[g.qs[q0]];
        const int N = (int)q.nstates.size();
        u.nq = n;
        u.st_off = off;
        off += 4 + (int64_t)q.ncaps.size();   // live mask, started mask, state, start ts, captures
        u.keep_last = q.nstates[N - 1].max_count < 0 ? 1 : 0;
        for (int j = 0; j < N; ++j) {
          const auto& st = q.nstates[j];
          u.st_of_stream |= (uint32_t)(j + 1) << (4 * st.stream);
          for (int t = 0; t < N; ++t) {
            bool ok = (t == j && st.max_count < 0);
            if (t > j) {
              ok = true;
              for (int k = j + 1; k < t; ++k) ok = ok && q.nstates[k].min_count == 0;
            }
            if (ok) u.allow |= 1ull << (j * 8 + t);
          }
          std::vector<TermList> run;
          bool any = false;
          for (int i = 0; i < n; ++i) {
            run.push_back(app.queries[g.qs[q0 + i]].nstates[j].terms);
            any = any || run.back().n > 0;
          }
          const uint64_t cb = any ? (uint64_t)mq_cond_run(g, st.stream, run, false) : 0xffull;
          u.cbase |= cb << (8 * j);
        }
        for (int j = N; j < 8; ++j) u.cbase |= 0xffull << (8 * j);
        g.units.push_back(u);
      } else {
        const Query& q = app.queries[g.qs[q0]];
        int na = 0;
        for (auto& ag : q.aggs) na += ag.fn != AGG_COUNT ? 1 : 0;
        int nu = na <= 1 ? 8 : na == 2 ? 4 : 2;   // k_mqwalk's mq_agg_unit widths
        static const int nu_cap = std::getenv("CEP_MQ_NU") ? std::atoi(std::getenv("CEP_MQ_NU")) : 8;
        if (nu_cap == 4 || nu_cap == 2) nu = std::min(nu, nu_cap);   // diagnostics: narrower units
        // mq_agg_fast: at most one non-count accumulator, having compared as
        // a double or an integer (not a float)
        const MqQuery& d0 = g.hq[q0];
        int fast = 0;
        if (na <= 1 && (d0.hav_item < 0 || d0.hav_ctype == T_DOUBLE || d0.hav_ctype == T_LONG ||
                        d0.hav_ctype == T_INT)) {
          fast = 9;
          for (int y = 0; y < d0.nagg; ++y) {
            const int fn = d0.agg_fn[y], t = d0.agg_arg_type[y];
            if (fn == AGG_COUNT) continue;
            const int acmp = (t == T_LONG || t == T_INT) ? 0 : t == T_FLOAT ? 1 : 2;
            (void)acmp;   // min / max: generic mq_agg_unit (fast shapes 3-8 are not built)
            fast = (fn == AGG_MIN || fn == AGG_MAX) ? 0 : (fn == AGG_SUM && d0.agg_out_type[y] == T_LONG) ? 2 : 1;
          }
        }
        static const bool no_fast = std::getenv("CEP_MQ_GENERIC") != nullptr;   // diagnostics
        if (fast && !no_fast) nu = std::min(nu, 4);   // mq_agg_fast is built 4 queries wide
        for (int i = 0; i < n; i += nu) {
          u.q0 = (int)q0 + i;
          u.nq = std::min(nu, n - i);
          u.nu = nu;
          u.fast = no_fast ? 0 : fast;
          g.units.push_back(u);
        }
      }
    }
    g.words = off;
    const int ntiles = (int)(g.pipe.chunk / kMqTile);
    bool ok = dev_ensure(&g.dq, g.hq.size() * sizeof(MqQuery), a->stream, false) &&
              dev_ensure(&g.du, g.units.size() * sizeof(MqUnit), a->stream, false) &&
              dev_ensure(&g.dconds, g.conds.size() * sizeof(MqCond), a->stream, false) &&
              dev_ensure(&g.state, (size_t)g.words * g.kstride * 8, a->stream, false);
    ok = ok && g.pipe.alloc((size_t)g.pipe.chunk * (2 + nphys_max) * 8 + 16,
                            (size_t)((1 << lg) + 1) * ntiles * 2 + 16, a->stream);
    if (!ok) return fail(a, CEP_E_DEVICE, "out of device memory (multi-query group)");
    hipMemset(g.state.p, 0, (size_t)g.words * g.kstride * 8);
    // condition slots: the prefetch slot of each term's column
    const std::vector<int> pc = mq_pref_cols(g);
    for (auto& mc : g.conds)
      for (int i = 0; i < mc.tl.n && i < kMaxTerms; ++i)
        for (size_t sl = 0; sl < pc.size(); ++sl)
          if (pc[sl] == mc.tl.t[i].col) mc.slot[i] = (int32_t)sl;
    hipMemcpy(g.dconds.p, g.conds.data(), g.conds.size() * sizeof(MqCond), hipMemcpyHostToDevice);
    hipMemcpy(g.du.p, g.units.data(), g.units.size() * sizeof(MqUnit), hipMemcpyHostToDevice);
  }
  return CEP_OK;
}

}  // namespace cep
