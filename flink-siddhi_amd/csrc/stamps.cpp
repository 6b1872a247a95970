// CEP_STAMPS=1 diagnostics: the phase stamps the last walk / partition launches
// left on the device, printed when the app is destroyed (scripts/ parse the text).
#include <cstdio>

#include "rt.h"

namespace cep {

void dump_stamps(cep_app* a) {
  if (a->stamps.p && !a->pats.empty()) {
    // diagnostics: mean duration of each k_walk phase over the last launch's blocks
    const int nb = 1 << a->pats[0].pa.buckets_log2;
    std::vector<uint64_t> st((size_t)4096 * 16);
    hipMemcpy(st.data(), a->stamps.p, st.size() * 8, hipMemcpyDeviceToHost);
    // phases 1..7 of window 0, then phases 2..7 of window 1 (stamps 10..15,
    // relative to window 0's last stamp); blocks with one window have zeros
    double sum[16] = {0};
    int n1 = 0;
    for (int b = 0; b < nb; ++b) {
      const uint64_t* t = &st[(size_t)b * 16];
      for (int i = 1; i < 8; ++i)
        if (t[i] && t[i - 1]) sum[i] += (double)(t[i] - t[i - 1]);
      if (t[10] && t[7]) {
        ++n1;
        sum[10] += (double)(t[10] - t[7]);
        for (int i = 11; i < 16; ++i)
          if (t[i] && t[i - 1]) sum[i] += (double)(t[i] - t[i - 1]);
      }
    }
    {   // slowest blocks (stragglers): first stamp to the last one written
      std::vector<std::pair<uint64_t, int>> dur;
      for (int b = 0; b < nb; ++b) {
        const uint64_t* t = &st[(size_t)b * 16];
        uint64_t hi = 0;
        for (int i = 0; i < 16; ++i) hi = std::max(hi, t[i]);
        if (t[0] && hi > t[0]) dur.push_back({hi - t[0], b});
      }
      std::sort(dur.rbegin(), dur.rend());
      std::fprintf(stderr, "[cep stamps] slowest walk blocks (ticks):");
      for (size_t i = 0; i < dur.size() && i < 6; ++i) std::fprintf(stderr, " b%d=%llu", dur[i].second,
                                                                   (unsigned long long)dur[i].first);
      if (!dur.empty()) std::fprintf(stderr, " median=%llu", (unsigned long long)dur[dur.size() / 2].first);
      std::fprintf(stderr, "\n");
    }
    {   // every stamp against the previous one (both kernels' layouts)
      double dsum[16] = {0};
      int dn[16] = {0};
      for (int b = 0; b < nb; ++b) {
        const uint64_t* t = &st[(size_t)b * 16];
        for (int i = 1; i < 16; ++i)
          if (t[i] && t[i - 1]) {
            dsum[i] += (double)(t[i] - t[i - 1]);
            ++dn[i];
          }
      }
      std::fprintf(stderr, "[cep stamps] walk deltas ticks/block:");
      for (int i = 1; i < 16; ++i) std::fprintf(stderr, " d%d=%.0f(%d)", i, dn[i] ? dsum[i] / dn[i] : 0.0, dn[i]);
      std::fprintf(stderr, "\n");
    }
    if (std::getenv("CEP_WAVESTAMP")) {   // -DCF_WAVESTAMP build: per-wave ends vs slot 0
      double m[16] = {0};
      int c[16] = {0};
      for (int b = 0; b < nb; ++b) {
        const uint64_t* t = &st[(size_t)b * 16];
        if (!t[0]) continue;
        for (int i = 1; i < 16; ++i)
          if (t[i]) {
            m[i] += (double)(int64_t)(t[i] - t[0]);
            ++c[i];
          }
      }
      std::fprintf(stderr, "[cep wavestamps] commit end per wave:");
      for (int i = 1; i <= 8; ++i) std::fprintf(stderr, " w%d=%.0f", i - 1, c[i] ? m[i] / c[i] : 0.0);
      std::fprintf(stderr, "\n[cep wavestamps] emission end per wave:");
      for (int i = 9; i < 16; ++i) std::fprintf(stderr, " w%d=%.0f", i - 9, c[i] ? m[i] / c[i] : 0.0);
      std::fprintf(stderr, "\n");
    }
    std::fprintf(stderr, "[cep stamps] walk window0 ticks/block:");
    for (int i = 1; i < 8; ++i) std::fprintf(stderr, " p%d=%.0f", i, sum[i] / nb);
    std::fprintf(stderr, "\n[cep stamps] walk window1 (%d blocks):", n1);
    for (int i = 10; i < 16; ++i) std::fprintf(stderr, " p%d=%.0f", i - 8, n1 ? sum[i] / n1 : 0.0);
    std::fprintf(stderr, "\n");
    const uint64_t* c = &st[(size_t)4095 * 16];
    if (nb <= 4095 && c[0] && !c[5 + 8])
      std::fprintf(stderr, "[cep counters] walk2 active keys=%llu n>2=%llu n>4=%llu n>6=%llu n>8=%llu | waves: n>2=%llu n>4=%llu of %llu\n",
                   (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
                   (unsigned long long)c[3], (unsigned long long)c[4], (unsigned long long)c[5],
                   (unsigned long long)c[6], (unsigned long long)c[7]);
    if (nb <= 4095 && (c[5] || c[7]))
      std::fprintf(stderr, "[cep counters] walk: carried=%llu all=%llu keylanes_n>2=%llu drop_n>2=%llu "
                   "slot_st>=2=%llu windows=%llu keylanes=%llu\n",
                   (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
                   (unsigned long long)c[3], (unsigned long long)c[4], (unsigned long long)c[5],
                   (unsigned long long)c[7]);
    const bool cf = a->pats[0].cf;
    const int nt = (int)std::min<int64_t>(4096, cf ? a->pats[0].cf_chunk / kCfTile
                                                   : a->pats[0].pipe.chunk / (kPartThreads * kPartItems));
    std::vector<uint64_t> pt((size_t)nt * 16);
    hipMemcpy(pt.data(), (uint64_t*)a->stamps.p + 4096 * 16, pt.size() * 8, hipMemcpyDeviceToHost);
    double ps[16] = {0};
    uint64_t plo = UINT64_MAX, phi = 0;
    for (int b = 0; b < nt; ++b) {
      for (int i = 1; i < 8; ++i)
        if (pt[b * 16 + i] && pt[b * 16 + i - 1]) ps[i] += (double)(pt[b * 16 + i] - pt[b * 16 + i - 1]);
      if (pt[b * 16]) plo = std::min(plo, pt[b * 16]);
      for (int i = 0; i < 8; ++i) phi = std::max(phi, pt[b * 16 + i]);
    }
    std::fprintf(stderr, "[cep stamps] partition phase ticks/block:");
    for (int i = 1; i < 8; ++i) std::fprintf(stderr, " p%d=%.0f", i, ps[i] / nt);
    std::fprintf(stderr, " span=%.0f\n", (double)(phi - plo));
  }
  if (a->stamps.p && !a->mqs.empty()) {
    // diagnostics: mean ticks per multi-query walk phase over the last launch's buckets
    const int nb = 1 << a->mqs[0].lg;
    std::vector<uint64_t> st((size_t)nb * 16);
    hipMemcpy(st.data(), a->stamps.p, st.size() * 8, hipMemcpyDeviceToHost);
    double sum[8] = {0}, ut[8] = {0}, p1 = 0, rs = 0;
    for (int b = 0; b < nb; ++b) {
      const uint64_t* x = &st[(size_t)b * 16];
      for (int i = 1; i < 5; ++i)
        if (x[i] && x[i - 1]) sum[i] += (double)(x[i] - x[i - 1]);
      if (x[5] && x[2]) p1 += (double)(x[5] - x[2]);
      if (x[3] && x[5]) rs += (double)(x[3] - x[5]);
      for (int i = 0; i < 8; ++i) ut[i] += (double)x[8 + i];
    }
    std::fprintf(stderr, "[cep stamps] mq walk ticks/bucket: gather=%.0f sort=%.0f count=%.0f (pass1 %.0f, "
                 "reserve %.0f) emit=%.0f\n", sum[1] / nb, sum[2] / nb, sum[3] / nb, p1 / nb, rs / nb, sum[4] / nb);
    std::fprintf(stderr, "[cep stamps] mq unit ticks/bucket (units 0-3) pass1: %.0f %.0f %.0f %.0f pass2: %.0f %.0f "
                 "%.0f %.0f\n", ut[0] / nb, ut[1] / nb, ut[2] / nb, ut[3] / nb, ut[4] / nb, ut[5] / nb,
                 ut[6] / nb, ut[7] / nb);
  }
}

}  // namespace cep
