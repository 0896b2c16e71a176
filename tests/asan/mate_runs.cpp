// The shared walk of a mate's M runs (csrc/gk_materuns.h) and the shared bootstrap draw (csrc/gk_draw.h) on the host.  A
// stand-alone program: built for the host with AddressSanitizer and UBSan by tests/test_mate_runs_host.py.
//   (1) records are built from mate descriptions in both forms -- 128-byte gk_mate records and the compact words of
//       gk_mates_compact_host -- in heap blocks of exactly their size, so a read past a record, past the last compact
//       word or past the wide array is the sanitizer's to report;
//   (2) every mate is walked by both walkers (the staged one twice) into plain difference arrays, which must equal what
//       expect() below, an independent restatement that reads the descriptions and never a record, marks;
//   (3) gk_boot_draw is printed for a few hundred (seed, i, b, g, n): the Python test holds the lines against
//       tests/boot_reference.py.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "gk_draw.h"
#include "gk_materuns.h"

static char g_err[512];
void gk_set_error(const char* fmt, ...) {      // gk_sampack.cpp reports through it
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {

using Ops = std::vector<std::pair<int, uint32_t>>;      // (GK_CIG_*, length)

struct MateSpec {
  uint32_t pos0;
  int ref;
  Ops ops;            // the operations stored: at most GK_MAX_CIG (plain) / GK_WIDE_CIG (wide)
  int n_cig;          // the count field: may exceed what is stored (the walk clamps it)
};

struct PairSpec {
  MateSpec mate[2];
  bool wide = false;
  uint32_t slot = 0;      // of a wide pair: its place in the wide array as the record names it
};

constexpr int kGenes = 2;
const int64_t kGeneOff[kGenes + 1] = {0, 300, 450};      // backbones of 300 and 150 positions

Ops repeat(int n, int op, uint32_t len) { return Ops((size_t)n, {op, len}); }

// plain mates: every class of the issue's list; each is used on both sides (pairs are made by cycling)
std::vector<MateSpec> plainMates() {
  const int M = GK_CIG_M, D = GK_CIG_D, I = GK_CIG_I, S = GK_CIG_S;
  std::vector<MateSpec> v;
  v.push_back({10, 0, {}, 0});                                                              // no operation
  v.push_back({10, 0, {{M, 50}}, 1});
  v.push_back({0, 0, {{M, 50}}, 1});                                                        // pos0 = 0
  v.push_back({5, 0, {{S, 3}, {M, 20}, {I, 2}, {M, 10}, {D, 4}, {M, 7}, {S, 5}}, 7});       // mixed
  v.push_back({7, 1, repeat(13, M, 3), 13});                                                // an odd count: half a word
  v.push_back({7, 1, repeat(14, M, 3), 14});                                                // a full record
  {
    Ops o = repeat(14, M, 2);
    o[3] = {D, 9};
    o[8] = {I, 1};
    for (int n : {15, 100, 254}) v.push_back({20, 0, o, n});                                // counts beyond the record
  }
  v.push_back({250, 0, {{M, 50}}, 1});                                                      // ends exactly at len
  v.push_back({100, 1, {{M, 20}, {D, 10}, {M, 20}}, 3});                                    // the last run ends at len (150)
  v.push_back({280, 0, {{M, 50}}, 1});                                                      // straddles len
  v.push_back({140, 1, {{M, 5}, {M, 20}, {M, 5}}, 3});                                      // 2nd straddles, 3rd beyond
  v.push_back({300, 0, {{M, 10}, {D, 5}, {M, 10}}, 3});                                     // starts at len
  v.push_back({100000, 1, {{M, 10}, {M, 4095}}, 2});                                        // starts far beyond len
  v.push_back({0xFFFFFF00u, 0, {{M, 4095}, {D, 4095}, {M, 4095}}, 3});                      // the largest pos0 of a record
  v.push_back({10, 5, {{M, 50}}, 1});                                                       // a reference that is no gene
  v.push_back({149, 1, {{D, 1}, {M, 1}}, 2});                                               // D to len: nothing left
  v.push_back({148, 1, {{I, 30}, {S, 30}, {M, 2}}, 3});                                     // I and S do not advance
  return v;
}

std::vector<MateSpec> wideMates() {
  const int M = GK_CIG_M, D = GK_CIG_D, I = GK_CIG_I;
  std::vector<MateSpec> v;
  v.push_back({10, 0, {}, 0});
  v.push_back({0, 0, {{M, 100000}}, 1});                                                    // longer than a record's 4095
  v.push_back({3, 1, repeat(128, M, 1), 128});
  {
    Ops o = repeat(128, M, 2);
    for (int k = 1; k < 128; k += 3) o[(size_t)k] = {k % 2 ? D : I, 1};
    v.push_back({40, 0, o, 200});                                                           // clamped to 128
  }
  v.push_back({120, 1, {{M, 20}, {D, 10}, {M, 40}}, 3});                                    // straddles len
  return v;
}

void putPlain(const MateSpec& m, gk_mate& r) {
  memset(&r, 0, sizeof r);
  r.pos0 = m.pos0;
  r.flag = 3;
  r.ref = (uint8_t)m.ref;
  r.nh = 1;
  r.n_cig = (uint8_t)m.n_cig;
  for (size_t k = 0; k < m.ops.size(); ++k) r.cig[k] = (uint16_t)(m.ops[k].second << 4 | (uint32_t)m.ops[k].first);
}

void putWide(const MateSpec& m, uint32_t slot, gk_mate& r, gk_mate_wide* x) {
  memset(&r, 0, sizeof r);
  r.pos0 = m.pos0;
  r.flag = 3;
  r.ref = (uint8_t)m.ref;
  r.nh = 1;
  r.n_cig = GK_SPILLED;
  r.ins[0] = slot;
  if (!x) return;
  memset(x, 0, sizeof *x);
  x->pos0 = m.pos0;
  x->ref = (uint8_t)m.ref;
  x->n_cig = (uint16_t)m.n_cig;
  for (size_t k = 0; k < m.ops.size(); ++k) x->cig[k] = m.ops[k].second << 4 | (uint32_t)m.ops[k].first;
}

// The restatement: what mate `m` marks, from its description alone.  `wide`: the pair is in the wide array.
void expect(const MateSpec& m, bool wide, std::vector<uint32_t>& d) {
  if (m.ref >= kGenes) return;
  const int64_t base = kGeneOff[m.ref], len = kGeneOff[m.ref + 1] - base;
  const size_t n = std::min<size_t>({(size_t)m.n_cig, m.ops.size(), (size_t)(wide ? GK_WIDE_CIG : GK_MAX_CIG)});
  int64_t at = m.pos0;
  for (size_t k = 0; k < n; ++k) {
    const int64_t run = m.ops[k].second;
    if (m.ops[k].first == GK_CIG_M && at < len) { d[(size_t)(base + at)] += 1; d[(size_t)(base + std::min(at + run, len))] -= 1; }
    if (m.ops[k].first == GK_CIG_M || m.ops[k].first == GK_CIG_D) at += run;
  }
}

int g_failed = 0;
void fail(const char* what, bool compact, bool no_wide, int64_t row, int side) {
  printf("FAIL %s: %s records%s, valid row %lld, side %d\n", what, compact ? "compact" : "128-byte",
         no_wide ? ", no wide array" : "", (long long)row, side);
  ++g_failed;
}

struct Tab {      // what gk_mate_sample reads of a gk_tab
  int64_t n_pairs, n_valid, n_spill;
  int32_t* d_pair_src;
  uint8_t* d_pair_nh;
  gk_mate_wide* d_wide;
};

template <bool kCompact>
void walkAll(const GkMateSample& s, const std::vector<PairSpec>& pairs, bool no_wide) {
  const int64_t total = kGeneOff[kGenes];
  for (int64_t i = 0; i < s.n_valid; ++i) {
    for (int side = 0; side < 2; ++side) {
      std::vector<uint32_t> want((size_t)total + 1, 0u), one = want, two = want, again = want;
      const int64_t src = s.pair_src[i];
      const bool taken = src >= 0 && src < s.n_pairs;
      if (taken) {
        const PairSpec& p = pairs[(size_t)src];
        if (!p.wide || (!no_wide && p.slot < (uint32_t)s.n_spill)) expect(p.mate[side], p.wide, want);
      }
      GkMateRuns m;
      const bool found = gk_mate_find<kCompact>(s, i, side, [](uint32_t ref) { return (int)ref < kGenes; }, m);
      if (found != (taken && pairs[(size_t)src].mate[side].ref < kGenes)) fail("gk_mate_find", kCompact, no_wide, i, side);
      if (found) {
        const int64_t base = kGeneOff[m.ref], len = kGeneOff[m.ref + 1] - base;
        gk_mate_walk<kCompact>(s, m, side, len, [&](int64_t a, int64_t e) { one[(size_t)(base + a)] += 1; one[(size_t)(base + e)] -= 1; });
        GkMateCigar cig;
        if (gk_mate_stage<kCompact>(s, m, side, cig)) {
          gk_mate_walk_staged(m, cig, len, [&](int64_t a, int64_t e) { two[(size_t)(base + a)] += 1; two[(size_t)(base + e)] -= 1; });
          gk_mate_walk_staged(m, cig, len, [&](int64_t a, int64_t e) { again[(size_t)(base + a)] += 1; again[(size_t)(base + e)] -= 1; });
        }
      }
      if (one != want) fail("gk_mate_walk", kCompact, no_wide, i, side);
      if (two != want) fail("gk_mate_walk_staged", kCompact, no_wide, i, side);
      if (again != two) fail("gk_mate_walk_staged, second walk", kCompact, no_wide, i, side);
    }
  }
}

void walks() {
  // pairs: every plain mate on both sides, every wide mate on both sides; then the pairs at the edges of the arrays
  std::vector<PairSpec> pairs;
  const std::vector<MateSpec> plain = plainMates(), wides = wideMates();
  for (size_t k = 0; k < plain.size(); ++k) {
    PairSpec p;
    p.mate[0] = plain[k];
    p.mate[1] = plain[(k + 1) % plain.size()];
    pairs.push_back(p);
  }
  const uint32_t n_spill = (uint32_t)wides.size();
  for (size_t k = 0; k < wides.size(); ++k) {
    PairSpec p;
    p.wide = true;
    p.slot = (uint32_t)k;      // the last one: slot == n_spill - 1, taken
    p.mate[0] = wides[k];
    p.mate[1] = wides[(k + 1) % wides.size()];
    pairs.push_back(p);
  }
  {
    PairSpec p;      // a wide pair whose place is one past the wide array: refused
    p.wide = true;
    p.slot = n_spill;
    p.mate[0] = p.mate[1] = wides[1];
    pairs.push_back(p);
  }
  {
    PairSpec p;      // the last record of the buffer: a compact mate that ends with its last CIGAR word
    p.mate[0] = plain[4];
    p.mate[1] = plain[1];      // one operation: one CIGAR word of the seven a full record has
    pairs.push_back(p);
  }
  const int64_t n_pairs = (int64_t)pairs.size();

  // heap blocks of exactly the arrays' sizes
  gk_mate* mates = (gk_mate*)malloc((size_t)(2 * n_pairs) * sizeof(gk_mate));
  gk_mate_wide* wide = (gk_mate_wide*)malloc((size_t)(2 * n_spill) * sizeof(gk_mate_wide));
  for (int64_t k = 0; k < n_pairs; ++k)
    for (int side = 0; side < 2; ++side) {
      const PairSpec& p = pairs[(size_t)k];
      if (p.wide) putWide(p.mate[side], p.slot, mates[2 * k + side], p.slot < n_spill ? wide + 2 * p.slot + side : nullptr);
      else putPlain(p.mate[side], mates[2 * k + side]);
    }
  int64_t n_words = 0;
  if (gk_mates_compact_size(mates, 2 * n_pairs, 1, &n_words) != GK_OK) { printf("FAIL gk_mates_compact_size: %s\n", g_err); exit(1); }
  const int64_t cap = 2 * n_pairs + 1 + n_words;
  uint32_t* compact = (uint32_t*)malloc((size_t)cap * sizeof(uint32_t));
  if (gk_mates_compact_host(mates, 2 * n_pairs, 1, compact, cap) != GK_OK) { printf("FAIL gk_mates_compact_host: %s\n", g_err); exit(1); }
  if (compact[2 * n_pairs] != (uint32_t)n_words || compact[2 * n_pairs] - compact[2 * n_pairs - 1] != kGkCigWord + 1) {
    printf("FAIL the last compact mate does not end with its last CIGAR word\n");
    exit(1);
  }

  // valid rows: every pair, last to first, then a pair_src below and one above the pairs
  std::vector<int32_t> src;
  for (int64_t k = n_pairs - 1; k >= 0; --k) src.push_back((int32_t)k);      // n_pairs - 1: taken
  src.push_back(-1);
  src.push_back((int32_t)n_pairs);
  const int64_t n_valid = (int64_t)src.size();
  int32_t* pair_src = (int32_t*)malloc((size_t)n_valid * sizeof(int32_t));
  memcpy(pair_src, src.data(), (size_t)n_valid * sizeof(int32_t));
  uint8_t* pair_nh = (uint8_t*)malloc((size_t)n_valid);
  memset(pair_nh, 1, (size_t)n_valid);

  for (int no_wide = 0; no_wide < 2; ++no_wide) {
    Tab tab = {n_pairs, n_valid, (int64_t)n_spill, pair_src, pair_nh, no_wide ? nullptr : wide};
    const GkMateSample full = gk_mate_sample(&tab, (gk_dptr)(uintptr_t)mates, 0);
    const GkMateSample comp = gk_mate_sample(&tab, 0, (gk_dptr)(uintptr_t)compact);
    if (full.c_off || full.c_words || comp.mates || comp.c_words != compact + 2 * n_pairs + 1 || comp.pair_nh != pair_nh ||
        full.n_valid != n_valid || full.n_pairs != n_pairs || full.n_spill != (int64_t)n_spill) {
      printf("FAIL gk_mate_sample\n");
      exit(1);
    }
    walkAll<false>(full, pairs, no_wide != 0);
    walkAll<true>(comp, pairs, no_wide != 0);
  }
  printf("walked %lld valid rows x 2 sides x 2 forms, with and without the wide array (%u wide pairs)\n", (long long)n_valid, n_spill);
  free(pair_nh);
  free(pair_src);
  free(compact);
  free(wide);
  free(mates);
}

void draws() {
  const uint64_t seeds[] = {0ull, 1ull, 0x123456789ABCDEFull, ~0ull};
  const uint32_t ns[] = {1u, 2u, 7u, 1000u, 1u << 20, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
  for (uint64_t seed : seeds)
    for (uint32_t n : ns)
      for (uint64_t b : {0ull, 3ull, 9999ull})
        for (uint64_t g : {0ull, 13ull}) {
          const uint64_t is[] = {0ull, 1ull, n / 2, (uint64_t)n - 1};
          for (uint64_t i : is) {
            const uint32_t j = gk_boot_draw(seed, i, b, g, n);
            if (j >= n) { printf("FAIL a draw of %u reads gave read %u\n", n, j); ++g_failed; }
            printf("draw %llu %llu %llu %llu %u %u\n", (unsigned long long)seed, (unsigned long long)i, (unsigned long long)b,
                   (unsigned long long)g, n, j);
          }
        }
}

}  // namespace

int main() {
  walks();
  draws();
  if (g_failed) {
    printf("mate runs: %d FAILED\n", g_failed);
    return 1;
  }
  printf("mate runs: ok\n");
  return 0;
}
