// The M runs of a packed mate, read in ONE place for the kernels that count aligned bases per position: depth_mark
// (gk_depth.hip), callcov_mark / callcov_mark_lds (gk_callcov.hip), depthw_mark (gk_depthboot.hip).  `__host__ __device__`,
// no heap, no std::, fixed-size state; tests/asan/mate_runs.cpp runs it on the host.
//
// A mate counts as `samtools depth` counts it: every M run [cur, cur + n) of its CIGAR, clipped to [0, len) of its
// backbone, is one marked interval; M and D advance cur, every other operation does not.  A pair in the wide format
// (n_cig == GK_SPILLED) takes its CIGAR from the tabulation's wide records and marks nothing when there are none.  A
// pair_src outside [0, n_pairs) and a wide slot >= n_spill mark nothing: no array is indexed with an unchecked number.
// What stays with a kernel: which rows it takes, the NH filter, the gene test and what a mark does (+1 / -1 to HBM or
// LDS, +w / -w).  So a kernel goes  gk_mate_find, with its gene test -> one of the two walkers, with its mark.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "graphkir_hip.h"

#ifndef GK_HD
#define GK_HD __host__ __device__
#endif

// ---- the layout facts: header words 0 - 2 (pos0, flag | ref | nh, nm | n_cig | n_mm | n_ins), then the CIGAR
constexpr int kGkCigWord = 3;                                // the first CIGAR word; of a compact wide mate: its pair's place
constexpr int kGkCigWords = GK_MAX_CIG / 2;                  // uint16 operations, two to a word
constexpr int kGkInsWord = offsetof(gk_mate, ins) / 4;       // ins[0] of a 128-byte record: a wide pair's place there
static_assert(offsetof(gk_mate, pos0) == 0 && offsetof(gk_mate, cig) == 4 * kGkCigWord && sizeof(gk_mate) == 128 &&
              GK_MAX_CIG % 2 == 0, "gk_mate layout: header words, then the CIGAR as whole words");

struct GkMateSample {                // the records of a tabulated sample in one of two forms, and the valid pairs' map to them
  const gk_mate* mates;              // the 128-byte records, or
  const uint32_t* c_off;             // the compact form: word offsets [2 * n_pairs + 1] ...
  const uint32_t* c_words;           // ... and the words
  const gk_mate_wide* wide;
  const int32_t* pair_src;
  const uint8_t* pair_nh;
  int64_t n_valid, n_pairs, n_spill;
};

template <class Tab>      // gk_tab (gk_common.h), of which this header knows the name only
static inline GkMateSample gk_mate_sample(const Tab* tab, gk_dptr d_mates, gk_dptr d_compact) {
  const uint32_t* c_off = reinterpret_cast<const uint32_t*>(static_cast<uintptr_t>(d_compact));
  return {reinterpret_cast<const gk_mate*>(static_cast<uintptr_t>(d_mates)), c_off, c_off ? c_off + 2 * tab->n_pairs + 1 : nullptr,
          tab->d_wide, tab->d_pair_src, tab->d_pair_nh, tab->n_valid, tab->n_pairs, tab->n_spill};
}

struct GkMateRuns {                  // one mate, found and its header decoded
  const uint32_t* w;                 // the record's words
  uint32_t pos0, ref, n_ops;         // n_ops: the record's n_cig, GK_SPILLED for a pair in the wide array
};

// Mate `side` of valid pair i (0 <= i < s.n_valid): its words and header fields; false: nothing to mark.  on_gene(ref) is
// the kernel's gene test, asked as soon as the header is read (asked after the call it cost callcov_mark two registers).
template <bool kCompact, class OnGene>
GK_HD static inline bool gk_mate_find(const GkMateSample& s, int64_t i, int side, OnGene on_gene, GkMateRuns& m) {
  const int64_t src = s.pair_src[i];
  if (src < 0 || src >= s.n_pairs) return false;
  const int64_t at = 2 * src + side;
  m.w = kCompact ? s.c_words + s.c_off[at] : reinterpret_cast<const uint32_t*>(s.mates + at);
  const uint32_t w0 = m.w[0], w1 = m.w[1], w2 = m.w[2];
  m.pos0 = w0;
  m.ref = (w1 >> 16) & 0xFFu;
  m.n_ops = (w2 >> 8) & 0xFFu;
  return on_gene(m.ref);
}

// The wide record of a mate with n_ops == GK_SPILLED: its CIGAR is there.  null: nothing to mark.
template <bool kCompact>
GK_HD static inline const gk_mate_wide* gk_mate_far(const GkMateSample& s, const GkMateRuns& m, int side) {
  if (!s.wide) return nullptr;
  const int64_t slot = kCompact ? m.w[kGkCigWord] : m.w[kGkInsWord];
  if (slot >= s.n_spill) return nullptr;
  return s.wide + 2 * slot + side;
}

GK_HD static inline int gk_far_ops(const gk_mate_wide* far) { return far->n_cig < GK_WIDE_CIG ? far->n_cig : GK_WIDE_CIG; }
GK_HD static inline int gk_mate_ops(const GkMateRuns& m) { return m.n_ops < GK_MAX_CIG ? (int)m.n_ops : GK_MAX_CIG; }

// The clip rule: operation `op` of length n at `cur` on a backbone of `len` positions.  mark(a, e) for a non-empty
// clipped M run [a, e); M and D advance cur.
template <class Mark>
GK_HD static inline void gk_mate_run(int64_t& cur, uint32_t op, uint32_t n, int64_t len, Mark& mark) {
  if (op == GK_CIG_M) {
    const int64_t a = cur < 0 ? 0 : cur, e = cur + n > len ? len : cur + n;
    if (e > a) mark(a, e);
    cur += n;
  } else if (op == GK_CIG_D) {
    cur += n;
  }
}

// Walker 1: the operations are read from the record as the walk goes.
template <bool kCompact, class Mark>
GK_HD static inline void gk_mate_walk(const GkMateSample& s, const GkMateRuns& m, int side, int64_t len, Mark mark) {
  int64_t cur = m.pos0;
  if (m.n_ops == GK_SPILLED) {
    const gk_mate_wide* far = gk_mate_far<kCompact>(s, m, side);
    if (!far) return;
    const int n_cig = gk_far_ops(far);
    for (int c = 0; c < n_cig; ++c) gk_mate_run(cur, far->cig[c] & 15u, far->cig[c] >> 4, len, mark);
    return;
  }
  const int n_cig = gk_mate_ops(m);
  for (int c = 0; c < n_cig; ++c) {      // uint16 operations, two to a word
    const uint32_t x = m.w[kGkCigWord + (c >> 1)];
    const uint32_t cg = (c & 1) ? (x >> 16) : (x & 0xFFFFu);
    gk_mate_run(cur, cg & 15u, cg >> 4, len, mark);
  }
}

// Walker 2, for a kernel that walks one mate several times: gk_mate_stage reads the CIGAR words of a 128-byte / compact
// record once into kGkCigWords registers (a wide pair's operations, up to GK_WIDE_CIG and rare, are read from its record
// at every walk); false: nothing to mark.  Only the words the operations take are read: a compact mate ends with them.
struct GkMateCigar {
  const gk_mate_wide* far;           // the wide record whose CIGAR counts, or null: the CIGAR is in cw
  int n_cig;
  uint32_t cw[kGkCigWords];
};

template <bool kCompact>
GK_HD static inline bool gk_mate_stage(const GkMateSample& s, const GkMateRuns& m, int side, GkMateCigar& c) {
  c.far = nullptr;
  if (m.n_ops == GK_SPILLED) {
    c.far = gk_mate_far<kCompact>(s, m, side);
    if (!c.far) return false;
    c.n_cig = gk_far_ops(c.far);
  } else {
    c.n_cig = gk_mate_ops(m);
#pragma unroll
    for (int k = 0; k < kGkCigWords; ++k) c.cw[k] = 2 * k < c.n_cig ? m.w[kGkCigWord + k] : 0u;
  }
  return true;
}

template <class Mark>
GK_HD static inline void gk_mate_walk_staged(const GkMateRuns& m, const GkMateCigar& c, int64_t len, Mark mark) {
  int64_t cur = m.pos0;
  if (c.far) {
    for (int k = 0; k < c.n_cig; ++k) gk_mate_run(cur, c.far->cig[k] & 15u, c.far->cig[k] >> 4, len, mark);
  } else {
#pragma unroll
    for (int k = 0; k < GK_MAX_CIG; ++k) {
      if (k < c.n_cig) {
        const uint32_t cg = (k & 1) ? (c.cw[k >> 1] >> 16) : (c.cw[k >> 1] & 0xFFFFu);
        gk_mate_run(cur, cg & 15u, cg >> 4, len, mark);
      }
    }
  }
}
