// One decoder of a PLAIN mate pair in BAM form, written for the host and for the device alike (`__host__ __device__`):
// the decode step of the device ingest, which sits between the two halves of gk_packer_feed_records (gk_ingest.h).
// ingest_decode_pairs (gk_ingest_decode.hip) runs it, one lane per mate; on the host it is held against the decoder it restates.
//
// It restates, for records as they lie in a BAM stream, what bam_pack_impl's `full` (gk_bamread.cpp), walk_alignment<BamSource>
// and decode_records (gk_sampack.cpp) do for a pair that needs nothing but two gk_mate records: the fixed fields, the tag
// scan (the LAST integer NM, the FIRST integer NH >= 0, the first Z of MD and of Zs), passes() of both mates before either
// is walked, header-only records when it fails for either, the CIGAR / MD / Zs co-walk with every consumption check, the
// clamps of nh and nm and the capacity test of gk_mate (readPair / filterRead / getNH / recordToRawVariant:
// hisat2.py:228-276, 551-569, 95-100, 279-515).
//
// The verdict per pair is GK_DECODE_DONE (both 128-byte records complete, every byte written, unused bytes zero) or
// GK_DECODE_HOST (the host decodes the pair as before).  The rule is asymmetric: a wrong HOST costs time, a wrong DONE is
// a wrong result, so everything that is not restated exactly is HOST -- any CIGAR op other than M or D, no CIGAR, no SEQ,
// a record shorter than its fixed part, a reference that is no backbone, a tag scan that does not end at the record's
// end, an MD number of more than 9 digits, a Zs entry that is not `1-9 digits | one character | ...`, any failed check of
// the walk (the host reports it with its line) and anything beyond gk_mate (the host spills the pair or refuses it).
// tests/asan/mate_decode.cpp holds the two decoders against each other.
//
// No heap, no std::, fixed-size state.  Record bytes are read through an accessor type `B` with `uint32_t u8(uint64_t at)`
// (`at` = byte offset in the stream): GkPlainBytes reads bytes, GkWordBytes aligned 32-bit words (BAM records are not
// aligned, and the name's length shifts everything behind it).
#pragma once
#include <stdint.h>

#include "graphkir_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GK_HD __host__ __device__
#else
#define GK_HD
#endif

enum { GK_DECODE_DONE = 0, GK_DECODE_HOST = 1 };

struct GkPlainBytes {
  const uint8_t* p;
  GK_HD uint32_t u8(uint64_t at) const { return p[at]; }
};

// aligned words of a stream whose base is 4-byte aligned and whose allocation is a whole number of words; the last
// word read is kept, which serves a walk over neighbouring bytes
struct GkWordBytes {
  const uint32_t* w;
  mutable uint64_t have = ~0ull;
  mutable uint32_t word = 0;
  GK_HD uint32_t u8(uint64_t at) const {
    const uint64_t i = at >> 2;
    if (i != have) { have = i; word = w[i]; }
    return (word >> ((uint32_t)(at & 3u) << 3)) & 0xFFu;
  }
};

template <typename B> GK_HD static inline uint32_t gk_rd16(const B& b, uint64_t at) { return b.u8(at) | b.u8(at + 1) << 8; }
template <typename B> GK_HD static inline uint32_t gk_rd32(const B& b, uint64_t at) {
  return b.u8(at) | b.u8(at + 1) << 8 | b.u8(at + 2) << 16 | b.u8(at + 3) << 24;
}

// what the scan of one record leaves for the walk
struct GkMateScan {
  uint32_t pos0 = 0;
  uint16_t flag = 0;
  uint8_t ref = 0, nh = 1, nm = GK_NM_ABSENT;
  bool passes = false;             // flag & 2, NM present, NM <= 4
  bool has_md = false, has_zs = false;
  uint32_t n_cig = 0, l_seq = 0;
  uint64_t cig = 0, seq = 0;       // stream offsets of the CIGAR words and of the packed bases
  uint64_t md = 0, zs = 0;         // ... and of the MD / Zs text (without the NUL)
  uint32_t md_len = 0, zs_len = 0;
};

// Fixed fields and tag scan of the record at [off, off + size).  gene_of_ref [n_ref]: reference id of the file -> backbone
// ordinal of the index, < 0 when it is none.  false: HOST.
template <typename B>
GK_HD static inline bool gk_mate_scan(const B& b, uint64_t off, uint32_t size, const int32_t* gene_of_ref, int32_t n_ref,
                                      GkMateScan& s) {
  if (size < 32u) return false;
  const uint32_t l_name = b.u8(off + 8), n_cig = gk_rd16(b, off + 12), l_seq = gk_rd32(b, off + 16);
  const uint64_t fixed = 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + l_seq;
  if (fixed > size || n_cig == 0 || l_seq == 0) return false;
  const int32_t ref_id = (int32_t)gk_rd32(b, off);
  if (ref_id < 0 || ref_id >= n_ref) return false;
  const int32_t gene = gene_of_ref[ref_id];
  if (gene < 0) return false;
  s.pos0 = gk_rd32(b, off + 4);
  s.flag = (uint16_t)gk_rd16(b, off + 14);
  s.ref = (uint8_t)gene;
  s.n_cig = n_cig;
  s.l_seq = l_seq;
  s.cig = off + 32 + l_name;
  s.seq = s.cig + 4ull * n_cig;
  s.has_md = s.has_zs = false;
  bool has_nm = false, has_nh = false;
  int64_t nm = 0, nh = 1;
  uint64_t t = off + fixed;
  const uint64_t end = off + size;
  while (t + 3 <= end) {
    const uint32_t t0 = b.u8(t), t1 = b.u8(t + 1), type = b.u8(t + 2);
    const uint64_t v = t + 3;
    const uint64_t avail = end - v;
    uint64_t used = 0;
    int64_t ival = 0;
    bool is_int = true;
    switch (type) {
      case 'A': used = 1; is_int = false; break;
      case 'c': if (avail < 1) return false; used = 1; ival = (int8_t)b.u8(v); break;
      case 'C': if (avail < 1) return false; used = 1; ival = b.u8(v); break;
      case 's': if (avail < 2) return false; used = 2; ival = (int16_t)gk_rd16(b, v); break;
      case 'S': if (avail < 2) return false; used = 2; ival = gk_rd16(b, v); break;
      case 'i': if (avail < 4) return false; used = 4; ival = (int32_t)gk_rd32(b, v); break;
      case 'I': if (avail < 4) return false; used = 4; ival = (int64_t)gk_rd32(b, v); break;
      case 'f': used = 4; is_int = false; break;
      case 'Z': case 'H': {
        uint64_t n = 0;
        while (n < avail && b.u8(v + n) != 0) ++n;
        if (n == avail) return false;              // no NUL inside the record
        if (type == 'Z' && t0 == 'M' && t1 == 'D' && !s.has_md) { s.has_md = true; s.md = v; s.md_len = (uint32_t)n; }
        if (type == 'Z' && t0 == 'Z' && t1 == 's' && !s.has_zs) { s.has_zs = true; s.zs = v; s.zs_len = (uint32_t)n; }
        used = n + 1; is_int = false;
        break;
      }
      case 'B': {
        if (avail < 5) return false;
        const uint32_t sub = b.u8(v);
        const uint64_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
        used = 5 + (uint64_t)gk_rd32(b, v + 1) * w; is_int = false;
        break;
      }
      default: return false;
    }
    if (used > avail) return false;
    if (is_int && t0 == 'N' && t1 == 'M') { has_nm = true; nm = ival; }
    if (is_int && t0 == 'N' && t1 == 'H' && !has_nh && ival >= 0) { has_nh = true; nh = ival; }
    t = v + used;
  }
  if (t != end) return false;                      // the host keeps what it found so far: not restated
  s.nh = (uint8_t)(nh < 255 ? nh : 255);
  s.nm = has_nm ? (uint8_t)(nm < 0 ? 0 : nm > 254 ? 254 : nm) : (uint8_t)GK_NM_ABSENT;
  s.passes = (s.flag & 2u) && has_nm && nm <= 4;
  return true;
}

// every byte of the record: the header fields, the rest zero
GK_HD static inline void gk_mate_header(const GkMateScan& s, gk_mate& r) {
  uint32_t* w = reinterpret_cast<uint32_t*>(&r);
  for (int i = 0; i < (int)(sizeof(gk_mate) / 4); ++i) w[i] = 0;
  r.pos0 = s.pos0; r.flag = s.flag; r.ref = s.ref; r.nh = s.nh; r.nm = s.nm;
}

namespace gk_decode_detail {

// MD as a stream of tokens with one token of look-ahead: a run of digits is a number, anything else one character
template <typename B>
struct MdStream {
  const B& b;
  uint64_t at, end;
  bool has = false, bad = false;   // a current token / a number of more than 9 digits was met
  bool is_num = false;
  int64_t num = 0;
  uint32_t ch = 0;
  GK_HD MdStream(const B& b_, uint64_t a, uint64_t e) : b(b_), at(a), end(e) { next(); }
  GK_HD void next() {
    if (at >= end) { has = false; return; }
    has = true;
    uint32_t c = b.u8(at);
    if (c >= '0' && c <= '9') {
      is_num = true;
      num = 0;
      int digits = 0;
      while (c >= '0' && c <= '9') {
        if (digits < 9) num = num * 10 + (int64_t)(c - '0');
        ++digits; ++at;
        if (at >= end) break;
        c = b.u8(at);
      }
      if (digits > 9) bad = true;
    } else {
      is_num = false;
      ch = c;
      ++at;
    }
  }
  GK_HD bool zero() const { return has && is_num && num == 0; }
  GK_HD bool acgt() const { return has && !is_num && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'); }
};

// Zs entries `gap|kind|...` between commas, one entry of look-ahead
template <typename B>
struct ZsStream {
  const B& b;
  uint64_t at, end;
  bool has = false, bad = false;
  int64_t gap = 0;
  uint32_t kind = 0;
  GK_HD ZsStream(const B& b_, uint64_t a, uint64_t e, bool present) : b(b_), at(a), end(e) {
    if (present && a < e) next(); else at = end + 1;
  }
  // entries are separated by commas: after the last one `at` is end + 1
  GK_HD void next() {
    if (at > end) { has = false; return; }
    has = true;
    int digits = 0;
    gap = 0;
    while (at < end) {
      const uint32_t c = b.u8(at);
      if (c < '0' || c > '9') break;
      gap = gap * 10 + (int64_t)(c - '0');
      ++digits; ++at;
      if (digits > 9) break;
    }
    if (digits < 1 || digits > 9 || at >= end || b.u8(at) != '|') { bad = true; return; }
    ++at;
    if (at >= end) { bad = true; return; }
    kind = b.u8(at);
    if (kind == '|' || kind == ',') { bad = true; return; }
    ++at;
    if (at >= end || b.u8(at) != '|') { bad = true; return; }
    ++at;
    while (at < end && b.u8(at) != ',') ++at;
    ++at;                          // past the comma, or to end + 1
  }
};

}  // namespace gk_decode_detail

// The co-walk of a mate whose pair passes: CIGAR words, mismatches and counts into `r` (gk_mate_header first).  false: HOST.
template <typename B>
GK_HD static inline bool gk_mate_walk(const B& b, const GkMateScan& s, gk_mate& r) {
  gk_mate_header(s, r);
  for (uint32_t k = 0; k < s.n_cig; ++k) {         // the host takes any other op elsewhere (strings, clips, errors)
    const uint32_t op = b.u8(s.cig + 4ull * k) & 15u;
    if (op != 0u && op != 2u) return false;
  }
  if (s.n_cig > (uint32_t)GK_MAX_CIG) return false;
  gk_decode_detail::MdStream<B> md(b, s.md, s.has_md ? s.md + s.md_len : s.md);
  gk_decode_detail::ZsStream<B> zs(b, s.zs, s.zs + s.zs_len, s.has_zs);
  const int64_t seq_size = (int64_t)s.l_seq;
  int64_t ref = 0, ri = 0, owed = 0, zpos = 0;
  uint32_t n_mm = 0, n_del = 0;
  for (uint32_t k = 0; k < s.n_cig; ++k) {
    const uint32_t v = gk_rd32(b, s.cig + 4ull * k);
    const int64_t n = (int64_t)(v >> 4);
    if (n > 4095) return false;                    // not a gk_mate
    if (md.zero()) md.next();
    if ((v & 15u) == 0u) {
      r.cig[k] = (uint16_t)((uint32_t)n << 4 | GK_CIG_M);
      int64_t done = 0;
      for (;;) {
        if (owed <= done && md.has && md.is_num) { owed += md.num; md.next(); }
        if (owed >= n) { owed -= n; break; }
        if (ri + owed >= seq_size || !md.has) return false;
        const int64_t q = ri + owed;
        const uint32_t code = (b.u8(s.seq + (uint64_t)(q >> 1)) >> ((~(uint32_t)q & 1u) << 2)) & 15u;
        // "=ACMGRSVTWYHKDBN"
        const uint64_t half = code < 8u ? 0x565352474D43413Dull : 0x4E42444B48595754ull;
        const uint32_t base = (uint32_t)(half >> ((code & 7u) << 3)) & 0xFFu;
        if (md.zero()) md.next();
        if (!md.has) return false;
        if (!md.acgt()) return false;
        if (md.ch == base) return false;
        md.next();
        if (zs.has && !zs.bad && zs.kind == 'S' && ri + owed == zpos + zs.gap) { zpos += zs.gap + 1; zs.next(); }
        const int64_t at = ref + owed;
        if (at > 0xFFFF || n_mm >= (uint32_t)GK_MAX_MM) return false;
        r.mm[n_mm].ref_off = (uint16_t)at;
        r.mm[n_mm].base = (uint8_t)base;
        ++n_mm;
        owed += 1;
        done = owed;
        if (owed == n) { owed = 0; break; }
      }
      ref += n;
      ri += n;
    } else {
      r.cig[k] = (uint16_t)((uint32_t)n << 4 | GK_CIG_D);
      ++n_del;
      if (!(md.has && !md.is_num && md.ch == '^')) return false;
      md.next();
      while (md.acgt()) md.next();
      if (zs.has && !zs.bad && zs.kind == 'D' && ri + owed == zpos + zs.gap) { zpos += zs.gap; zs.next(); }
      ref += n;
    }
    if (md.bad || zs.bad) return false;
  }
  if (md.zero()) md.next();
  if (md.bad || zs.bad) return false;
  if (zs.has) return false;                        // Zs entries do not line up with the alignment
  if (md.has) return false;                        // MD not fully consumed
  if (ri != seq_size) return false;                // CIGAR does not cover the read
  if (n_mm + n_del > (uint32_t)GK_MAX_EVENTS) return false;
  r.n_cig = (uint8_t)s.n_cig;
  r.n_mm = (uint8_t)n_mm;
  r.n_ins = 0;
  return true;
}

// Both mates of a pair, one after the other (a kernel would run the two in neighbouring lanes and exchange `passes`
// and the verdict between them -- every lane taking part in the exchange, whatever it has found itself).  left /
// right: stream offset and size of the two records.  GK_DECODE_DONE: out[0] (left) and out[1] (right) are complete.
template <typename B>
GK_HD static inline int gk_pair_decode(const B& b, uint64_t left_off, uint32_t left_size, uint64_t right_off,
                                       uint32_t right_size, const int32_t* gene_of_ref, int32_t n_ref, gk_mate* out) {
  GkMateScan s[2];
  if (!gk_mate_scan(b, left_off, left_size, gene_of_ref, n_ref, s[0])) return GK_DECODE_HOST;
  if (!gk_mate_scan(b, right_off, right_size, gene_of_ref, n_ref, s[1])) return GK_DECODE_HOST;
  const bool both = s[0].passes && s[1].passes;
  for (int m = 0; m < 2; ++m) {
    if (!both) { gk_mate_header(s[m], out[m]); continue; }
    if (!gk_mate_walk(b, s[m], out[m])) return GK_DECODE_HOST;
  }
  return GK_DECODE_DONE;
}
