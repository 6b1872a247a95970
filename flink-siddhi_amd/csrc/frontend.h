// SiddhiQL-subset front end: parse + bind + compile.
//
// Replaces the plan-side uses of Siddhi that flink-siddhi makes:
//   SiddhiManager.validateSiddhiApp      (AbstractSiddhiOperator.java:292-299)
//   SiddhiCompiler.parse                 (SiddhiExecutionPlanner.java:76)
//   SiddhiAppRuntime.getStreamDefinitionMap for output-type inference
//                                         (SiddhiTypeFactory.java:64-112)
// Unsupported-but-valid SiddhiQL (outer / unidirectional joins, windows other
// than sliding #window.length / #window.time and tumbling #window.lengthBatch /
// #window.externalTimeBatch, tables without a primary key or
// addressed by anything but that key, extensions) fails with
// CEP_E_UNSUPPORTED so the Java shim can fall back to real Siddhi.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "plan.h"

namespace cep {

struct AttrDef {
  std::string name;
  int type;
};

struct StreamSchema {
  std::string id;
  std::vector<AttrDef> attrs;
  int index(const std::string& n) const {
    for (size_t i = 0; i < attrs.size(); ++i)
      if (attrs[i].name == n) return (int)i;
    return -1;
  }
};

enum QueryKind { Q_FILTER = 0, Q_PATTERN = 1, Q_AGG = 2, Q_JOIN = 3, Q_TABLE = 4 };


struct AggSpec {
  int fn;
  int arg_type;         // input type (after evaluation of arg program)
  int out_type;
  Prog arg;             // argument program over the current event (unused for count)
  int word = -1;        // device: carried record word holding the argument (-1: count)
};

struct OutItem {
  std::string name;
  int type;
  Prog prog;
  int32_t src = SRC_VM;          // direct copy source when the item is a plain attribute
};

struct Query {
  int kind = Q_FILTER;
  std::string out_stream;
  std::vector<OutItem> select;   // output attributes in definition order
  Prog having;                   // over LDOUT / LDCOL / LDAGG
  // interpreter-free having (multi-query walk): `<select item> cop constant`;
  // having_item -1 with having_simple = true: no having
  bool having_simple = true;
  int having_item = -1;
  int having_cop = 0, having_ctype = 0;
  uint64_t having_cconst = 0;

  // ---- filter / aggregation (single input stream)
  int in_stream = -1;
  Prog filter;                   // conjunction of all [..] filters, invalid = true
  TermList filter_terms;
  int key_col = -1;              // partition / group key column (-1: none)
  int part_col = -1;             // `partition with` column (-1: none)
  std::vector<Prog> group_progs; // group-by expressions (host path when not a column)
  std::vector<int> group_cols;   // group-by attribute columns (routing keys)
  std::vector<AggSpec> aggs;
  // sliding window in front of the aggregates (#window.length(N) / #window.time(T)):
  // the engine keeps one window per key
  int win_kind = WIN_NONE;
  int64_t win_param = 0;         // rows (length) / ms (time)
  // tumbling windows (#window.lengthBatch(N) / #window.externalTimeBatch(c, T),
  // batch_kernels.hip): win_kind is WIN_LENGTH_BATCH / WIN_TIME_BATCH; win_col
  // is c's column, carried as record word win_word (-1: lengthBatch)
  int win_col = -1, win_word = -1;
  bool win_global = false;       // Siddhi's window spans every group (group by without a
                                 // partition): per-key windows are equivalent only for
                                 // #window.time over non-decreasing ts (engine.cpp)

  // ---- 2-state pattern `[every] s1=A[f] -> s2=B[g] [within W]`
  int a_stream = -1, b_stream = -1;
  Prog f;                        // over A's columns (LDCOL = raw column)
  Prog g_raw;                    // g over B's raw columns (valid iff !g_in_walk)
  TermList f_terms, g_terms;     // interpreter-free forms of f / g_raw
  Prog g_walk;                   // g in the walk: LDCOL = record word, LDCAP = s1 capture
  bool g_in_walk = false;
  bool every = false;
  int64_t within = -1;           // ms, -1 = none
  int key_col_a = -1, key_col_b = -1;  // partition key columns (-1: unpartitioned)
  std::vector<int> rec_cols_a;   // raw columns carried in A-stream records
  std::vector<int> rec_cols_b;   // raw columns carried in B-stream records
  std::vector<int> cap_from_rec; // pending capture word i <- A-record word cap_from_rec[i]

  // ---- N-state pattern / sequence (general NFA walk): `nfa` queries keep
  // every event of the states' streams (sequences) or every event some
  // state's own condition accepts (patterns) as records carrying rec_cols_a
  struct NState {
    int stream = -1;
    int min_count = 1, max_count = 1;   // max -1: unbounded
    int logic = 0;   // first side of a logical position: 1 `and` / 2 `or` with the next state
    Prog raw;      // condition over the event's own columns (partition pass)
    Prog walk;     // condition reading earlier states (walk: LDCOL word, LDCAP capture)
    TermList terms;   // interpreter-free form of raw (n = 0: no condition, -1: not expressible)
  };
  struct NCap {
    int state, index, word;           // index: k-th event of the state (0 = first), -1 = last
  };
  bool nfa = false;
  bool sequence = false;
  std::vector<NState> nstates;
  std::vector<NCap> ncaps;
  std::vector<int> key_col_s;    // per input stream handle: partition key column (-1)

  // ---- windowed stream join `A[f]#window.x as a join B[g]#window.y as b on C`
  // (Q_JOIN, join_kernels.hip): a_stream / b_stream are the two sides; both
  // have one definition, so kept rows of either side carry rec_cols_a.  The
  // side filters read raw columns; join_on and the select programs read the
  // A-side row's carried word w as LDCOL w (SRC_REC + w) and the B-side row's
  // as LDCAP w (SRC_CAP + w), whichever of the two rows triggered the match.
  struct JoinSide {
    Prog filter;                 // conjunction of the side's filters, invalid = true
    TermList filter_terms;
    int win_kind = WIN_NONE;
    int64_t win_param = 0;       // rows (length) / ms (time)
  };
  JoinSide join_side[2];
  Prog join_on;                  // invalid: no `on` (every pair joins)
  int join_nterms = -1;          // >= 0: `on` as direct comparisons (join_terms), -1: interpreter only
  JoinTerm join_terms[kMaxTerms];

  // ---- event-table operation (Q_TABLE, tab_kernels.hip): a
  // writer (`insert into T`, `update or insert into T`, `update T`, `delete
  // T`: no output stream) or a reader (lookup join, `in`) over in_stream.
  // `filter` is the operation's own-row filter over raw columns (without the
  // `in` conjunct).  Rows of in_stream carry rec_cols_a in the table
  // pipeline's records (TableDef::rec of the stream); tab_on and the select
  // programs read carried word w of the stream row as LDCOL w (SRC_REC + w)
  // and attribute w of the table row as LDCAP w (SRC_CAP + w).
  int tab = -1;                  // index into CompiledApp::tables
  int tab_op = -1;               // TabOpKind
  int tab_key_col = -1;          // column of in_stream that equals the primary key
  bool tab_negate = false;       // TOP_IN under `not`
  Prog tab_on;                   // TOP_JOIN: the `on` conjuncts beside the key equality (invalid: none)
  // writers, per table attribute w: the carried word stored when the key is
  // absent (tab_ins) / present (tab_set); -1: none
  int tab_ins[kMaxCaps], tab_set[kMaxCaps];

  // ---- query chaining (derive.hip): the query reads derived streams through
  // view `view` of CompiledApp::views (-1: it reads the batch as sent)
  int view = -1;
  bool in_partition = false;     // written inside a `partition with` block
};

// A producer of a derived stream: a plain filter / projection query whose
// output stream some query reads.  Its rows reach the readers as a masked
// view of the batch (engine.cpp build_view), not through its OutStream.
struct Derived {
  int stream;      // input handle of the derived stream
  int producer;    // query index
  int source;      // input handle the producer reads
  int stage;       // 1 + depth of the source (raw inputs: depth 0)
};

// The derived streams one query (or several) reads: every producer behind
// them, in stage order.  Stage k's producers read stage k-1's view.
struct View {
  std::vector<int> derived;      // indices into CompiledApp::derived, stage order
  int stages = 0;
};

// `@PrimaryKey('k') define table T (...)`: per-key state of one pipeline that
// holds every operation on T (plan order).
struct TableDef {
  StreamSchema schema;
  int pk = -1;                   // primary-key attribute
  std::vector<int> ops;          // query indices (Q_TABLE), plan order
  // records: rows of stream a_stream carry rec_a, rows of every other stream
  // rec_b (k_partition's two carried-column lists)
  int a_stream = -1;
  std::vector<int> rec_a, rec_b;
  int key_col_s[8];              // per input handle: the column that maps to the key (-1)
};

constexpr int kMaxChainDepth = 4;
constexpr int kMaxDerived = 8;
constexpr int kMaxStageProducers = 4;   // producers sharing one k_derive pass

struct CompiledApp {
  std::vector<StreamSchema> inputs;     // defined input streams
  std::vector<StreamSchema> outputs;    // output streams (inferred)
  std::vector<Query> queries;
  std::vector<Ins> code;
  std::vector<uint64_t> konst;
  std::vector<std::string> strings;     // string literals (dictionary order)
  std::vector<Derived> derived;         // query chaining: producers of read derived streams
  std::vector<View> views;
  std::vector<std::string> read_ids;    // stream ids the plan's queries read (compile_app)
  std::vector<TableDef> tables;         // event tables, definition order

  int input_index(const std::string& id) const {
    for (size_t i = 0; i < inputs.size(); ++i)
      if (inputs[i].id == id) return (int)i;
    return -1;
  }
  bool is_derived(int handle) const {
    for (auto& d : derived)
      if (d.stream == handle) return true;
    return false;
  }
  int table_index(const std::string& id) const {
    for (size_t i = 0; i < tables.size(); ++i)
      if (tables[i].schema.id == id) return (int)i;
    return -1;
  }
  int output_index(const std::string& id) const {
    for (size_t i = 0; i < outputs.size(); ++i)
      if (outputs[i].id == id) return (int)i;
    return -1;
  }
};

// Status codes mirror include/cep.h.
// dict_seed: strings that take dictionary ids 0..n-1 before the plan's own
// literals (plans of one operator share their ids, operator.cpp).
int compile_app(const std::string& text, CompiledApp* out, std::string* err,
                const std::vector<std::string>* dict_seed = nullptr);

}  // namespace cep

struct cep_app;
struct cep_options;
namespace cep {
// cep_create with a dictionary seed (engine.cpp).
cep_app* create_app(const char* plan, const cep_options* opt, const std::vector<std::string>* dict_seed,
                    char* err, size_t errlen);

const char* type_name(int t);

// Input streams some query reads (InputStream.getUniqueStreamIds over the
// plan's queries), in definition order.
std::vector<int> read_inputs(const CompiledApp& app);

// Input handles one query reads.
std::vector<int> query_streams(const Query& q);

// Query chaining: the attribute of raw input `*stream` that column `*col` of a
// derived stream is a plain copy of, through every producer on the way
// (false: some producer computes it, or the stream has several producers).
bool source_column(const CompiledApp& app, int* stream, int* col);

}  // namespace cep
