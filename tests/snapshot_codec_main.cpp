// Stand-alone check of the snapshot codec (csrc/snapshot.h), built and run by
// tests/test_snapshot_codec.py under AddressSanitizer + UBSan.  Exit status 0:
// every check passed.  No GPU, no HIP.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../include/cep.h"
#include "snapshot.h"

using namespace cep;

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

constexpr uint32_t kOvf = 1u << 9;

// Decode from a heap block of exactly len bytes, so that any read past the
// end is the sanitizer's to report.
static int decode(const SnapGeometry& g, const std::vector<uint8_t>& b, size_t len, SnapImage* img, std::string* why) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
  if (len) std::memcpy(exact.get(), b.data(), len);
  return snapshot_decode(g, exact.get(), len, img, why);
}

// A pattern of 8 keys in 2 buckets, S = 2, 3 slot words; key 5 holds S + 3
// partials (an overflow run), key 2 one; a sparse map holding the value -1;
// reorder rows; a group of 2 buckets x 4 keys x 3 words; a join with a length
// and a time side; a table of 2 words.
static SnapImage make_image(bool group, bool join, bool table, bool has_stream, bool sparse) {
  SnapImage im;
  SnapGeometry& g = im.geo;
  g.plan_hash = 0x1234567890abcdefull;
  g.hdr_ovf = kOvf;
  g.join_tail_cap = 65536;
  g.inputs = {{4, 8, 1}, {8}};
  im.events_in = 4242;
  g.pats.push_back({8, 8, 16, 1, 2, 3, true, sparse, 16});
  SnapImage::Pattern p;
  p.hdr.assign(8, 0);
  p.slots.assign(8 * 2 * 3, 0);
  p.ext.assign(8, 0);
  auto slot = [&](int64_t i, int j, int w) -> uint64_t& { return p.slots[((size_t)j * 3 + w) * 8 + i]; };
  const int64_t i5 = key_index(5, 4, 1), i2 = key_index(2, 4, 1);
  p.hdr[i5] = 0x100u | 2u | kOvf;
  p.ext[i5] = 5;   // 5 partials, run at pool slot 0
  for (int j = 0; j < 2; ++j)
    for (int w = 0; w < 3; ++w) slot(i5, j, w) = 1000 + 10 * j + w;
  for (int j = 2; j < 5; ++j)
    for (int w = 0; w < 3; ++w) p.pool.push_back(1000 + 10 * j + w);
  p.hdr[i2] = 0x100u | 1u;
  for (int w = 0; w < 3; ++w) slot(i2, 0, w) = 77 + w;
  if (sparse) {
    p.kcount[0] = 3, p.kcount[1] = 1;
    p.krev = {100, ~0ull, 7};
  }
  im.pats.push_back(p);
  im.ro.input = 0;
  im.ro.has_stream = has_stream;
  im.ro.n = 3;
  im.ro.released_max = 999;
  im.ro.rows.resize(3 * (4 + 8 + 1 + 8 + (has_stream ? 1 : 0)));
  for (size_t i = 0; i < im.ro.rows.size(); ++i) im.ro.rows[i] = (uint8_t)(i * 7 + 1);
  if (group) {
    g.groups.push_back({8, 8, 1, 4, 3});
    std::vector<uint64_t> st(24, 0);
    st[(0 * 3 + 1) * 4 + 2] = 5;                    // bucket 0, word 1, key 2 of the bucket
    for (int w = 0; w < 3; ++w) st[(1 * 3 + w) * 4 + 3] = 90 + w;   // bucket 1, key 3
    im.groups.push_back(st);
  }
  if (join) {
    g.joins.push_back({3, {WIN_LENGTH, WIN_TIME}, {4, 1000}});
    SnapImage::Join j;
    j.kept[0] = 11, j.kept[1] = 12, j.tail[0] = 2, j.tail[1] = 3;
    for (int i = 0; i < 6; ++i) j.rows[0].push_back(200 + i);
    for (int i = 0; i < 9; ++i) j.rows[1].push_back(300 + i);
    im.joins.push_back(j);
  }
  if (table) {
    g.tabs.push_back({8, 8, 1, 2});
    SnapImage::Table t;
    t.hdr.assign(8, 0);
    t.words.assign(16, 0);
    for (uint32_t key : {0u, 3u, 6u}) {
      const int64_t i = key_index(key, 4, 1);
      t.hdr[i] = 1;
      t.words[i] = 500 + key, t.words[8 + i] = 600 + key;
    }
    im.tabs.push_back(t);
    im.tab_dropped = 9;
  }
  return im;
}

static bool same(const SnapImage& a, const SnapImage& b) {
  bool ok = a.events_in == b.events_in && a.pats.size() == b.pats.size() && a.groups == b.groups &&
            a.joins.size() == b.joins.size() && a.tabs.size() == b.tabs.size() && a.tab_dropped == b.tab_dropped &&
            a.ro.input == b.ro.input && a.ro.has_stream == b.ro.has_stream && a.ro.n == b.ro.n &&
            a.ro.released_max == b.ro.released_max && a.ro.rows == b.ro.rows;
  for (size_t i = 0; ok && i < a.pats.size(); ++i)
    ok = a.pats[i].hdr == b.pats[i].hdr && a.pats[i].slots == b.pats[i].slots && a.pats[i].ext == b.pats[i].ext &&
         a.pats[i].pool == b.pats[i].pool && a.pats[i].krev == b.pats[i].krev &&
         !std::memcmp(a.pats[i].kcount, b.pats[i].kcount, 8);
  for (size_t i = 0; ok && i < a.joins.size(); ++i)
    for (int s = 0; s < 2; ++s)
      ok = ok && a.joins[i].kept[s] == b.joins[i].kept[s] && a.joins[i].tail[s] == b.joins[i].tail[s] &&
           a.joins[i].rows[s] == b.joins[i].rows[s];
  for (size_t i = 0; ok && i < a.tabs.size(); ++i) ok = a.tabs[i].hdr == b.tabs[i].hdr && a.tabs[i].words == b.tabs[i].words;
  return ok;
}

struct Field {
  const char* name;
  size_t off;
  int width;       // bytes
  uint64_t max;
};

template <class T>
static T rd(const std::vector<uint8_t>& b, size_t off) {
  T v;
  std::memcpy(&v, &b[off], sizeof(v));
  return v;
}

// The count and size fields of a well-formed snapshot, found by walking the
// documented layout.
static std::vector<Field> fields(const SnapImage& im, const std::vector<uint8_t>& b) {
  std::vector<Field> f;
  const SnapGeometry& g = im.geo;
  const uint32_t ver = rd<uint32_t>(b, 4);
  size_t o = 28;
  auto keys = [&](const char* what, uint64_t kc, uint32_t nw, bool headed) {
    const uint32_t live = rd<uint32_t>(b, o);
    f.push_back({what, o, 4, kc});
    o += 4;
    for (uint32_t k = 0; k < live; ++k) {
      o += 4;
      uint32_t n = 1;
      if (headed) {
        n = rd<uint32_t>(b, o + 8);
        f.push_back({"pattern n", o + 8, 4, 2 + 16});
        o += 12;
      }
      o += (size_t)n * nw * 8;
    }
  };
  for (auto& p : g.pats) {
    o += 16;
    keys("pattern live", p.key_capacity, p.slot_words, true);
  }
  f.push_back({"reorder n", o + 5, 8, (uint64_t)INT32_MAX});
  o += 21 + im.ro.rows.size();
  for (auto& p : g.pats) {
    if (p.sparse) {
      f.push_back({"key map count", o + 1, 4, (uint64_t)p.key_capacity});
      o += 8 + 8 * rd<uint32_t>(b, o + 1);
    }
    o += 1;
  }
  o += 4;
  for (auto& gr : g.groups) {
    o += 12;
    keys("group nl", gr.key_capacity, gr.words, false);
  }
  if (ver >= 6) {
    o += 4;
    for (auto& j : g.joins) {
      o += 4;
      for (int s = 0; s < 2; ++s) {
        f.push_back({"join tail", o + 8, 8, j.win_kind[s] == WIN_LENGTH ? (uint64_t)j.win_param[s] : g.join_tail_cap});
        o += 16 + (size_t)rd<uint64_t>(b, o + 8) * j.ew * 8;
      }
    }
  }
  if (ver >= 7) {
    o += 4;
    for (auto& t : g.tabs) {
      o += 12;
      keys("table live", t.key_capacity, t.nwords, false);
    }
    o += 8;
  }
  CHECK(o == b.size());   // the walk and the encoder agree on the layout
  return f;
}

static void check_image(const SnapImage& im, uint32_t want_ver) {
  const std::vector<uint8_t> b = snapshot_encode(im);
  CHECK(b.size() > 8 && rd<uint32_t>(b, 4) == want_ver);
  SnapImage out;
  std::string why;
  CHECK(decode(im.geo, b, b.size(), &out, &why) == CEP_OK);
  CHECK(out.version == want_ver && same(im, out));
  CHECK(snapshot_encode(out) == b);
  // every proper prefix is refused with a state error
  for (size_t len = 0; len < b.size(); ++len) {
    const int rc = decode(im.geo, b, len, &out, &why);
    if (rc != CEP_E_STATE) {
      std::fprintf(stderr, "prefix %zu of %zu: status %d (%s)\n", len, b.size(), rc, why.c_str());
      ++failures;
    }
  }
  // each count / size field forced to an edge value: refused, or decoded into
  // an image that encodes and decodes again
  for (const Field& f : fields(im, b)) {
    const uint64_t edge[4] = {0, f.max, 0xffffffffull, f.width == 8 ? (uint64_t)INT32_MAX : f.max + 1};
    for (uint64_t v : edge) {
      std::vector<uint8_t> m = b;
      std::memcpy(&m[f.off], &v, f.width);
      if (decode(im.geo, m, m.size(), &out, &why) != CEP_OK) continue;
      const std::vector<uint8_t> again = snapshot_encode(out);
      SnapImage out2;
      const bool ok = decode(im.geo, again, again.size(), &out2, &why) == CEP_OK && same(out, out2);
      if (!ok) std::fprintf(stderr, "field %s at %zu = %llu: inconsistent\n", f.name, f.off, (unsigned long long)v);
      CHECK(ok);
    }
  }
}

static void expect(const SnapGeometry& g, const std::vector<uint8_t>& b, int status, const char* text) {
  SnapImage out;
  std::string why;
  const int rc = decode(g, b, b.size(), &out, &why);
  if (rc != status || why.compare(0, std::strlen(text), text) != 0) {
    std::fprintf(stderr, "expected %d \"%s\", got %d \"%s\"\n", status, text, rc, why.c_str());
    ++failures;
  }
}

static void check_refusals() {
  const SnapImage im = make_image(true, true, true, true, true);
  const std::vector<uint8_t> b = snapshot_encode(im);
  auto bytes = [&](size_t off, uint32_t v) {
    std::vector<uint8_t> m = b;
    std::memcpy(&m[off], &v, 4);
    return m;
  };
  expect(im.geo, bytes(0, 0x53504544), CEP_E_STATE, "not a libcep snapshot");
  expect(im.geo, bytes(4, 1), CEP_E_STATE, "not a libcep snapshot");
  expect(im.geo, bytes(4, 8), CEP_E_STATE, "not a libcep snapshot");
  expect(im.geo, bytes(8, 1), CEP_E_STATE, "snapshot was taken with a different plan");
  auto with = [&](void (*change)(SnapGeometry&)) {
    SnapGeometry g = im.geo;
    change(g);
    return g;
  };
  const char* geom = "snapshot geometry differs from this runtime";
  expect(with([](SnapGeometry& g) { g.pats.push_back(g.pats[0]); }), b, CEP_E_STATE, "snapshot was taken with a different plan");
  expect(with([](SnapGeometry& g) { g.pats[0].key_capacity = 16; }), b, CEP_E_STATE, geom);
  expect(with([](SnapGeometry& g) { g.pats[0].S = 4; }), b, CEP_E_STATE, geom);
  expect(with([](SnapGeometry& g) { g.pats[0].slot_words = 2; }), b, CEP_E_STATE, geom);
  expect(with([](SnapGeometry& g) { g.pats[0].has_kext = false; }), b, CEP_E_CAPACITY,
         "snapshot holds more than pending_slots partials for a key");
  expect(with([](SnapGeometry& g) { g.pats[0].pool_cap = 2; }), b, CEP_E_CAPACITY,
         "snapshot's overflow partials exceed the pending pool");
  expect(with([](SnapGeometry& g) { g.inputs.clear(); }), b, CEP_E_STATE, "corrupt snapshot (reorder buffer)");
  expect(with([](SnapGeometry& g) { g.pats[0].sparse = false; }), b, CEP_E_STATE, "snapshot key map does not match");
  expect(with([](SnapGeometry& g) { g.groups.clear(); }), b, CEP_E_STATE, "snapshot multi-query groups do not match");
  expect(with([](SnapGeometry& g) { g.groups[0].words = 4; }), b, CEP_E_STATE, geom);
  expect(with([](SnapGeometry& g) { g.joins.clear(); }), b, CEP_E_STATE, "snapshot joins do not match");
  expect(with([](SnapGeometry& g) { g.joins[0].ew = 4; }), b, CEP_E_STATE,
         "snapshot geometry differs from this runtime (join rows)");
  expect(with([](SnapGeometry& g) { g.joins[0].win_param[0] = 1; }), b, CEP_E_STATE, "corrupt snapshot (join rows)");
  expect(with([](SnapGeometry& g) { g.tabs.clear(); }), b, CEP_E_STATE, "snapshot tables do not match");
  expect(with([](SnapGeometry& g) { g.tabs[0].nwords = 3; }), b, CEP_E_STATE,
         "snapshot geometry differs from this runtime (table rows)");
  // an older version than the runtime's state needs
  const SnapImage v5 = make_image(true, false, false, false, false);
  const std::vector<uint8_t> b5 = snapshot_encode(v5);
  SnapGeometry g = v5.geo;
  g.joins = im.geo.joins;
  expect(g, b5, CEP_E_STATE, "snapshot has no join state (version < 6)");
  g = v5.geo;
  g.tabs = im.geo.tabs;
  expect(g, b5, CEP_E_STATE, "snapshot has no table state (version < 7)");
}

static void check_key_mapping() {
  for (int64_t kpb : {1, 2, 128, 512})
    for (int lg : {0, 1, 5, 11}) {
      const int64_t ks = kpb << lg;
      std::vector<char> seen(ks, 0);
      bool ok = true;
      for (int64_t i = 0; i < ks && ok; ++i) {
        const uint32_t key = dense_key(i, kpb, lg);
        ok = (int64_t)key < ks && !seen[key] && key_index(key, kpb, lg) == i;
        if (ok) seen[key] = 1;
      }
      CHECK(ok);
    }
}

// Versions 2 - 4, assembled by hand: no n per key (2, 3: n = header & 0xff),
// no reorder section (2), no key map (2, 3), no group section.
static void check_old_versions() {
  SnapGeometry g = make_image(false, false, false, false, false).geo;
  for (uint32_t ver = 2; ver <= 4; ++ver) {
    std::vector<uint8_t> b;
    auto put = [&](const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
    auto u32 = [&](uint32_t v) { put(&v, 4); };
    auto u64 = [&](uint64_t v) { put(&v, 8); };
    put("CEPS", 4);
    u32(ver), u64(g.plan_hash), u64(31), u32(1);
    u64(8), u32(2), u32(3), u32(1);           // key_capacity, S, slot_words, one live key
    u32(6), u64(0x100u | 2u);                 // key 6, header: 2 partials
    if (ver >= 4) u32(2);
    for (uint64_t w = 0; w < 6; ++w) u64(40 + w);
    if (ver >= 3) {
      const int32_t in = 1;
      const uint8_t hs = 0;
      put(&in, 4), put(&hs, 1), u64(2), u64(17);   // input 1 (one i64 column), 2 rows, released_max
      for (uint64_t w = 0; w < 4; ++w) u64(w);     // the column, then ts
    }
    if (ver >= 4) b.push_back(0);                  // not sparse
    SnapImage out;
    std::string why;
    CHECK(decode(g, b, b.size(), &out, &why) == CEP_OK);
    const int64_t i6 = key_index(6, 4, 1);
    CHECK(out.version == ver && out.events_in == 31 && out.pats[0].hdr[i6] == (0x100u | 2u));
    CHECK(out.pats[0].slots[((size_t)1 * 3 + 2) * 8 + i6] == 45 && out.pats[0].ts_max == 43);
    CHECK(out.ro.n == (ver >= 3 ? 2 : 0) && out.ro.released_max == (ver >= 3 ? 17 : INT64_MIN));
    for (size_t len = 0; len < b.size(); ++len) CHECK(decode(g, b, len, &out, &why) == CEP_E_STATE);
    // a runtime with groups, joins or a sparse map cannot take them
    SnapGeometry g2 = g;
    g2.groups.push_back({8, 8, 1, 4, 3});
    expect(g2, b, CEP_E_STATE, "snapshot has no multi-query group state (version < 5)");
    if (ver < 4) {
      g2 = g;
      g2.pats[0].sparse = true;
      expect(g2, b, CEP_E_STATE, "snapshot has no key map (version < 4)");
    }
  }
}

int main() {
  for (int hs = 0; hs < 2; ++hs)
    for (int sp = 0; sp < 2; ++sp) {
      check_image(make_image(false, false, false, hs, sp), 5);
      check_image(make_image(true, false, false, hs, sp), 5);
      check_image(make_image(true, true, false, hs, sp), 6);
      check_image(make_image(true, false, true, hs, sp), 7);
      check_image(make_image(true, true, true, hs, sp), 7);
    }
  check_refusals();
  check_key_mapping();
  check_old_versions();
  if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
  return failures ? 1 : 0;
}
