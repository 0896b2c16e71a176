// The shared decoder of a plain mate pair (csrc/gk_mate_decode.h) against the host decoder it restates (gk_bamread.cpp:
// the tag scan of bam_pack_impl; gk_sampack.cpp: walk_alignment<BamSource>, decode_records), on BAM records built in
// memory.  A stand-alone program: built for the host with AddressSanitizer and UBSan by tests/test_mate_decode_host.py.
//   (1) DONE  =>  the host decoded the pair without error, without spill and without strings, and the 2 x 128 bytes agree;
//   (2) every pair of the plain classes is DONE;  (3) every pair of the non-plain classes is HOST;
//   (4) (1) over single-byte mutations and truncations of plain records, on a fixed seed.
// The shared decoder reads a copy of the two records that ends with the (mutated, truncated) record's last byte, so a read
// past a record's end is the sanitizer's to report; it is run through both accessors (bytes, aligned words at every
// residue of the record's start mod 4), which must agree.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "gk_bamread.cpp"   // struct gk_bam: the records are handed over as an open file would hold them
#include "gk_mate_decode.h"

static char g_err[512];
void gk_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {

using Cigar = std::vector<std::pair<char, uint32_t>>;

struct Mate {
  std::string name = "r";
  uint32_t flag = 0;
  int32_t ref = 0, pos0 = 100;
  Cigar cigar;
  std::string seq;
  std::string tags;                 // raw bytes
  int32_t next_ref = 0, next_pos0 = 100;
};

void w32(std::string& s, uint32_t v) { for (int i = 0; i < 4; ++i) s.push_back((char)(v >> (8 * i))); }
void w16(std::string& s, uint32_t v) { for (int i = 0; i < 2; ++i) s.push_back((char)(v >> (8 * i))); }

std::string tagInt(const char* name, char type, long v) {
  std::string s(name, 2);
  s.push_back(type);
  const int n = (type == 'c' || type == 'C') ? 1 : (type == 's' || type == 'S') ? 2 : 4;
  for (int i = 0; i < n; ++i) s.push_back((char)((unsigned long)v >> (8 * i)));
  return s;
}
std::string tagZ(const char* name, const std::string& v, char type = 'Z') {
  std::string s(name, 2);
  s.push_back(type);
  s += v;
  s.push_back('\0');
  return s;
}

std::string encode(const Mate& m) {   // the record without its length word, as gk_bam holds it
  static const std::string kBase = "=ACMGRSVTWYHKDBN", kOps = "MIDNSHP=X";
  std::string s;
  w32(s, (uint32_t)m.ref); w32(s, (uint32_t)m.pos0);
  s.push_back((char)(m.name.size() + 1)); s.push_back(0);
  w16(s, 0); w16(s, (uint32_t)m.cigar.size()); w16(s, m.flag);
  w32(s, (uint32_t)m.seq.size());
  w32(s, (uint32_t)m.next_ref); w32(s, (uint32_t)m.next_pos0); w32(s, 0);
  s += m.name; s.push_back('\0');
  for (auto& op : m.cigar) w32(s, op.second << 4 | (uint32_t)kOps.find(op.first));
  for (size_t i = 0; i < m.seq.size(); i += 2) {
    const uint32_t hi = (uint32_t)kBase.find(m.seq[i]), lo = i + 1 < m.seq.size() ? (uint32_t)kBase.find(m.seq[i + 1]) : 0;
    s.push_back((char)(hi << 4 | lo));
  }
  s.append(m.seq.size(), (char)30);
  s += m.tags;
  return s;
}

// An alignment of M and D ops with mismatches at chosen read offsets: SEQ and a standard MD (a number, 0 included,
// between any two non-numbers) are generated.
struct Plain {
  Cigar cigar;
  std::string seq, md;
  int n_mm = 0;
};
Plain plain(const Cigar& cigar, const std::vector<int>& mism) {
  Plain p;
  p.cigar = cigar;
  long run = 0, ri = 0;
  size_t at = 0;
  for (auto& op : cigar) {
    if (op.first == 'M') {
      for (uint32_t k = 0; k < op.second; ++k, ++ri) {
        const char base = "ACGT"[(ri * 7 + 3) % 4];
        p.seq.push_back(base);
        if (at < mism.size() && mism[at] == ri) {
          p.md += std::to_string(run);
          p.md.push_back(base == 'A' ? 'C' : 'A');
          run = 0; ++at; ++p.n_mm;
        } else {
          ++run;
        }
      }
    } else if (op.first == 'D') {
      p.md += std::to_string(run);
      p.md.push_back('^');
      for (uint32_t k = 0; k < op.second && k < 3; ++k) p.md.push_back("ACGT"[k % 4]);   // the walk skips any number of bases
      run = 0;
    } else {                         // other ops take read bases without a word in MD
      if (op.first == 'I' || op.first == 'S')
        for (uint32_t k = 0; k < op.second; ++k, ++ri) p.seq.push_back("ACGT"[(ri * 7 + 3) % 4]);
    }
  }
  p.md += std::to_string(run);
  return p;
}

Mate mateOf(const Plain& p, bool left, long nm = 0) {
  Mate m;
  m.flag = 2u | 1u | (left ? 128u : 64u);
  m.cigar = p.cigar;
  m.seq = p.seq;
  m.tags = tagInt("NM", 'c', nm) + tagZ("MD", p.md);
  return m;
}

struct Pair { std::string what; std::string left, right; uint32_t left_size, right_size; };
Pair pairOf(const std::string& what, const Mate& left, const Mate& right) {
  Pair p{what, encode(left), encode(right), 0, 0};
  p.left_size = (uint32_t)p.left.size();
  p.right_size = (uint32_t)p.right.size();
  return p;
}

struct HostResult {
  bool emitted = false, error = false, spilled = false, strings = false;
  gk_mate rec[2];
};

constexpr size_t kSlack = 1u << 19;   // the host reader trusts the record index: room behind a damaged record

HostResult hostDecode(const Pair& p) {
  HostResult r;
  static gk_bam* b = nullptr;
  if (!b) {
    b = new gk_bam();
    b->ref_names = {"G0", "G1", "X"};
    b->name_sorted = b->collated = true;
    b->data.resize(kSlack * 2);
    memset(b->data.data(), 0, b->data.size());
  }
  // the earlier record is the right one
  if (p.left.size() + p.right.size() > kSlack) { fprintf(stderr, "pair too large\n"); exit(2); }
  memcpy(b->data.data(), p.right.data(), p.right.size());
  memcpy(b->data.data() + p.right.size(), p.left.data(), p.left.size());
  memset(b->data.data() + p.right.size() + p.left.size(), 0, 4096);
  b->recs.resize(2);
  b->recs[0] = {0, p.right_size};
  b->recs[1] = {p.right.size(), p.left_size};
  const char* genes[2] = {"G0", "G1"};
  gk_packer* pk = nullptr;
  if (gk_packer_create(genes, 2, nullptr, 0, &pk) != GK_OK) exit(2);
  gk_bam_pack(b, pk);
  int32_t kind = 0;
  int64_t line = 0, n_pairs = 0, n_strings = 0, n_spill = 0;
  gk_packer_error(pk, &kind, &line);
  gk_packer_counts(pk, nullptr, nullptr, &n_pairs, nullptr, &n_strings);
  gk_packer_spilled(pk, &n_spill);
  r.error = kind != 0;
  r.emitted = r.error || n_pairs == 1;
  r.spilled = n_spill != 0;
  r.strings = n_strings != 0;
  if (n_pairs == 1) gk_packer_records(pk, r.rec, nullptr);
  gk_packer_destroy(pk);
  return r;
}

const int32_t kGeneOfRef[3] = {0, 1, -1};

// the shared decoder on an exact copy: [right][left] or [left][right], the record `last` (0 left, 1 right) at the end
int sharedDecode(const Pair& p, int last, gk_mate* out) {
  const std::string& a = last == 0 ? p.right : p.left;
  const std::string& z = last == 0 ? p.left : p.right;
  const uint32_t z_size = last == 0 ? p.left_size : p.right_size;
  const uint32_t a_size = last == 0 ? p.right_size : p.left_size;
  const size_t n = a.size() + z_size;
  uint8_t* buf = (uint8_t*)malloc(n);
  memcpy(buf, a.data(), a.size());
  memcpy(buf + a.size(), z.data(), z_size);
  const uint64_t left_off = last == 0 ? a.size() : 0, right_off = last == 0 ? 0 : a.size();
  const uint32_t left_size = last == 0 ? z_size : a_size, right_size = last == 0 ? a_size : z_size;
  const int verdict = gk_pair_decode(GkPlainBytes{buf}, left_off, left_size, right_off, right_size, kGeneOfRef, 3, out);
  // the word accessor, the copy starting at every residue mod 4 and ending in whole words
  for (int shift = 0; shift < 4; ++shift) {
    const size_t words = (shift + n + 3) / 4;
    uint32_t* w = (uint32_t*)calloc(words ? words : 1, 4);
    memcpy((uint8_t*)w + shift, buf, n);
    gk_mate again[2];
    memset(again, 0xAB, sizeof(again));
    const int v2 = gk_pair_decode(GkWordBytes{w}, left_off + shift, left_size, right_off + shift, right_size, kGeneOfRef, 3, again);
    if (v2 != verdict || (verdict == GK_DECODE_DONE && memcmp(again, out, sizeof(again)))) {
      fprintf(stderr, "%s: the word accessor at shift %d disagrees with the byte accessor\n", p.what.c_str(), shift);
      exit(1);
    }
    free(w);
  }
  free(buf);
  return verdict;
}

int g_failures = 0;
void complain(const Pair& p, const char* why) {
  fprintf(stderr, "FAIL %s: %s\n", p.what.c_str(), why);
  ++g_failures;
}

// (1), and what the pair came to: DONE or HOST; -1 when the host never emitted the pair (nothing to compare)
int check(const Pair& p, int last = 0) {
  gk_mate out[2];
  memset(out, 0xCD, sizeof(out));
  const int verdict = sharedDecode(p, last, out);
  const HostResult h = hostDecode(p);
  if (!h.emitted) return -1;
  if (verdict == GK_DECODE_DONE) {
    if (h.error) complain(p, "DONE, but the host reports an error");
    else if (h.spilled) complain(p, "DONE, but the host spilled the pair");
    else if (h.strings) complain(p, "DONE, but the host interned a string");
    else if (memcmp(out, h.rec, sizeof(out))) complain(p, "DONE, but the records differ from the host's");
  }
  return verdict;
}

Cigar alternating(int n_ops, uint32_t m_len, uint32_t d_len) {
  Cigar c;
  for (int i = 0; i < n_ops; ++i) c.push_back(i % 2 == 0 ? std::make_pair('M', m_len) : std::make_pair('D', d_len));
  return c;
}

std::vector<int> firstN(int n) { std::vector<int> v; for (int i = 0; i < n; ++i) v.push_back(i); return v; }

}  // namespace

int main() {
  std::vector<Pair> plains, others;
  const Plain clean = plain({{'M', 50}}, {});
  auto both = [&](const std::string& what, const Plain& p, long nm = 0) {
    plains.push_back(pairOf(what, mateOf(p, true, nm), mateOf(clean, false)));
    plains.push_back(pairOf(what + " (right mate)", mateOf(clean, true), mateOf(p, false, nm)));
  };
  auto bothOther = [&](const std::string& what, const Plain& p, long nm = 0) {
    others.push_back(pairOf(what, mateOf(p, true, nm), mateOf(clean, false)));
    others.push_back(pairOf(what + " (right mate)", mateOf(clean, true), mateOf(p, false, nm)));
  };
  // ---- plain classes
  both("no mismatch", clean);
  for (int len = 1; len <= 8; ++len) {       // record starts and field offsets on every residue mod 4
    Mate l = mateOf(clean, true), r = mateOf(clean, false);
    l.name = r.name = std::string((size_t)len, 'q');
    plains.push_back(pairOf("name of " + std::to_string(len), l, r));
  }
  both("l_seq 1", plain({{'M', 1}}, {}));
  both("l_seq 1, mismatched", plain({{'M', 1}}, {0}), 1);
  both("l_seq odd", plain({{'M', 51}}, {50}), 1);
  both("mismatch at the first and last base", plain({{'M', 50}}, {0, 49}), 2);
  both("0A0C0", plain({{'M', 2}}, {0, 1}), 2);
  both("^AC0T", plain({{'M', 10}, {'D', 2}, {'M', 10}}, {10}), 3);
  both("CIGAR ending in D", plain({{'M', 10}, {'D', 2}}, {}), 2);
  both("14 ops", plain(alternating(14, 5, 1), {}), 4);
  both("16 mismatches", plain({{'M', 40}}, firstN(16)), 4);
  both("22 events", plain(alternating(13, 5, 1), firstN(16)), 4);
  both("an op of 4095", plain({{'M', 4095}}, {4094}), 1);
  both("a D of 4095 and a far mismatch", plain({{'M', 1}, {'D', 4095}, {'M', 4095}, {'D', 4095}, {'M', 5}}, {4100}), 3);
  {
    const char types[6] = {'c', 'C', 's', 'S', 'i', 'I'};
    for (char t : types) {
      Mate l = mateOf(clean, true), r = mateOf(clean, false);
      l.tags = tagInt("NM", t, 3) + tagZ("MD", clean.md);
      plains.push_back(pairOf(std::string("NM of type ") + t, l, r));
      r.tags = tagZ("MD", clean.md) + tagInt("NM", t, 200) + tagInt("NM", t, 4);   // the last NM counts
      plains.push_back(pairOf(std::string("two NM of type ") + t, l, r));
    }
    Mate l = mateOf(clean, true), r = mateOf(clean, false);
    l.tags = tagInt("NM", 'c', -3) + tagZ("MD", clean.md);
    r.tags = tagInt("NM", 'i', -70000) + tagZ("MD", clean.md);
    plains.push_back(pairOf("NM negative", l, r));
    l = mateOf(clean, true);
    l.tags += tagInt("NH", 'S', 300);
    plains.push_back(pairOf("NH > 255", l, mateOf(clean, false)));
    l = mateOf(clean, true);
    l.tags = tagInt("NH", 'c', -2) + l.tags + tagInt("NH", 'C', 7) + tagInt("NH", 'C', 9);
    plains.push_back(pairOf("a negative NH, then two NH", l, mateOf(clean, false)));
    l = mateOf(clean, true);
    l.tags += tagZ("MD", "7") + std::string("XBBs") + std::string("\x02\0\0\0", 4) + std::string("\x01\0\x02\0", 4) +
              tagZ("XH", "1AE3", 'H') + std::string("XAAq") + std::string("XFf") + std::string("\0\0\x80\x3f", 4) +
              tagZ("MD", "x", 'H');
    plains.push_back(pairOf("a second MD, B, H, A and f tags", l, mateOf(clean, false)));
    // Zs entries of kind S and D that line up
    const Plain z = plain({{'M', 10}, {'D', 2}, {'M', 10}}, {3});
    l = mateOf(z, true, 3);
    l.tags += tagZ("Zs", "3|S|hv1,6|D|hv2");
    r = mateOf(z, false, 3);
    r.tags = tagZ("Zs", "3|S|hv1,6|D|hv2") + r.tags + tagZ("Zs", "9|S|never read");
    plains.push_back(pairOf("Zs of kind S and D", l, r));
    l = mateOf(clean, true);
    l.tags = tagInt("NM", 'c', 0) + tagZ("MD", "60");
    plains.push_back(pairOf("MD longer than the M (the walk leaves the rest owed)", l, mateOf(clean, false)));
    l = mateOf(clean, true);
    l.tags += tagZ("Zs", "");
    plains.push_back(pairOf("an empty Zs", l, mateOf(clean, false)));
  }
  // header-only pairs, each cause on one mate only
  for (int side = 0; side < 2; ++side) {
    const Plain busy = plain({{'M', 10}, {'D', 2}, {'M', 10}}, {3});
    for (int cause = 0; cause < 4; ++cause) {
      Mate m[2] = {mateOf(busy, true, 2), mateOf(busy, false, 2)};
      Mate& x = m[side];
      const char* what = "";
      if (cause == 0) { x.tags = tagInt("NM", 'c', 5) + tagZ("MD", busy.md); what = "NM = 5"; }
      if (cause == 1) { x.tags = tagZ("MD", busy.md); what = "NM absent"; }
      if (cause == 2) { x.flag &= ~2u; what = "flag without bit 2"; }
      if (cause == 3) { x.tags = tagInt("NM", 'c', 5); x.cigar = {{'M', 5}, {'I', 2}, {'H', 3}}; x.seq = "ACGTACG"; what = "header-only with I and H ops"; }
      plains.push_back(pairOf(std::string(what) + (side ? " on the right mate" : " on the left mate"), m[0], m[1]));
    }
  }
  // ---- non-plain classes
  bothOther("an I op", plain({{'M', 10}, {'I', 2}, {'M', 10}}, {}), 2);
  bothOther("an S op", plain({{'S', 5}, {'M', 20}}, {}));
  bothOther("15 ops", plain(alternating(15, 5, 1), {}), 4);
  bothOther("17 mismatches", plain({{'M', 40}}, firstN(17)), 4);
  bothOther("23 events", plain(alternating(14, 5, 1), firstN(16)), 4);
  bothOther("an op of 4096", plain({{'M', 4096}}, {}));
  bothOther("a mismatch at offset 65535", plain({{'M', 1}, {'D', 65534}, {'M', 5}}, {1}), 3);
  bothOther("a mismatch at offset 65536", plain({{'M', 1}, {'D', 65535}, {'M', 5}}, {1}), 3);
  bothOther("an N op", plain({{'M', 10}, {'N', 100}, {'M', 10}}, {}));
  bothOther("an H op", plain({{'M', 20}, {'H', 10}}, {}));
  {
    auto variant = [&](const std::string& what, const Plain& p, const std::string& tags, int ref = 0) {
      for (int side = 0; side < 2; ++side) {
        Mate m[2] = {mateOf(clean, true), mateOf(clean, false)};
        m[side] = mateOf(p, side == 0);
        m[side].tags = tags;
        m[0].ref = m[1].ref = m[0].next_ref = m[1].next_ref = ref;
        others.push_back(pairOf(what + (side ? " (right mate)" : ""), m[0], m[1]));
      }
    };
    const Plain one = plain({{'M', 50}}, {7});
    const std::string nm = tagInt("NM", 'c', 1);
    variant("a tag cut off at the record's end", clean, nm + tagZ("MD", "50") + std::string("XXi\x01\x02", 5));
    variant("two stray bytes behind the tags", clean, nm + tagZ("MD", "50") + std::string("XX", 2));
    variant("a Z tag without its NUL", clean, nm + std::string("MDZ50", 5));
    variant("a tag of unknown type", clean, nm + tagZ("MD", "50") + std::string("XX?\0", 4));
    variant("MD that does not cover the M", clean, nm + tagZ("MD", "40"));
    variant("no MD", clean, nm);
    variant("an MD base equal to the read base", one, nm + tagZ("MD", std::string("7") + one.seq[7] + "42"));
    variant("an MD mismatch that is no base", one, nm + tagZ("MD", "7N42"));
    variant("an MD number of 10 digits", clean, nm + tagZ("MD", "0000000050"));
    variant("Zs entries that do not line up", one, nm + tagZ("MD", one.md) + tagZ("Zs", "6|S|hv1"));
    variant("a Zs entry with a sign", one, nm + tagZ("MD", one.md) + tagZ("Zs", "+7|S|hv1"));
    variant("a Zs entry with a long kind", one, nm + tagZ("MD", one.md) + tagZ("Zs", "7|SS|hv1"));
    variant("a Zs entry without its second bar", one, nm + tagZ("MD", one.md) + tagZ("Zs", "7|S"));
    variant("a Zs ending in a comma", one, nm + tagZ("MD", one.md) + tagZ("Zs", "7|S|hv1,"));
    variant("a reference that is no backbone", clean, nm + tagZ("MD", "50"), 2);
    variant("a reference id outside the table", clean, nm + tagZ("MD", "50"), 7);
    Mate l = mateOf(clean, true), r = mateOf(clean, false);
    l.cigar.clear();
    others.push_back(pairOf("no CIGAR", l, r));
    l = mateOf(clean, true);
    l.seq.clear();
    l.cigar = {{'D', 3}};
    others.push_back(pairOf("no SEQ", l, r));
  }
  int done = 0, host = 0;
  for (const Pair& p : plains) {
    const int v = check(p);
    if (v != GK_DECODE_DONE) complain(p, v < 0 ? "a plain pair that the host never emitted" : "a plain pair that is not DONE");
    else ++done;
  }
  for (const Pair& p : others) {
    const int v = check(p);
    if (v == GK_DECODE_DONE) complain(p, "a non-plain pair that is DONE");
    else if (v < 0) complain(p, "a non-plain pair that the host never emitted");
    else ++host;
  }
  // ---- (4) mutations and truncations of plain records
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
  int compared = 0, mutated_done = 0;
  for (int it = 0; it < 6000; ++it) {
    Pair p = plains[(size_t)(next() % plains.size())];
    if (p.left.size() > 600 || p.right.size() > 600) { --it; continue; }   // the long records would spend the mutations on bases
    // a record with an op beyond S goes through the host's text form, which renders l_seq bases whatever the record's size
    if (p.what.find("I and H ops") != std::string::npos) { --it; continue; }
    const int side = (int)(next() & 1);
    std::string& rec = side == 0 ? p.left : p.right;
    uint32_t& size = side == 0 ? p.left_size : p.right_size;
    if (it % 6 == 5) {
      size -= 1 + (uint32_t)(next() % (size < 40 ? size - 1 : 40));
      p.what += " truncated to " + std::to_string(size);
    } else {
      const size_t at = (size_t)(next() % rec.size());
      const int how = (int)(next() % 3);
      const char was = rec[at];
      rec[at] = how == 0 ? (char)next() : how == 1 ? (char)(was ^ (1 << (next() % 8))) : (char)(was + (next() & 1 ? 1 : -1));
      p.what += " byte " + std::to_string(at) + " of the " + (side ? "right" : "left") + " record";
    }
    const int v = check(p, side);
    if (v >= 0) ++compared;
    if (v == GK_DECODE_DONE) ++mutated_done;
  }
  printf("plain pairs DONE: %d of %zu; non-plain pairs HOST: %d of %zu; damaged pairs compared: %d, of them DONE: %d\n", done,
         plains.size(), host, others.size(), compared, mutated_done);
  if (g_failures) { printf("mate decode: %d failures\n", g_failures); return 1; }
  if (compared < 2000 || mutated_done < 200) { printf("mate decode: the damaged pairs exercise too little\n"); return 1; }
  printf("mate decode: ok\n");
  return 0;
}
