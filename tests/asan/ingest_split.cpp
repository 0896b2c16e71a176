// The split route of the ingest (csrc/gk_ingest.h: gk_bam_pack_with; csrc/gk_sampack.cpp: gk_packer_decode_subset)
// against gk_bam_pack on BAM records built in memory.  A stand-alone program: built for the host with AddressSanitizer
// and UBSan by tests/test_ingest_split_host.py.  A stand-in for the device decoder (gk_pair_decode over the stream's
// bytes, with verdicts forced to HOST where a case wants them, and 0xAB left in every slot it flags HOST) takes the
// pairs it may; the packer decodes the rest.  Whatever the split, the packer must hold what gk_bam_pack leaves of the
// same file: records, pair_lines, counts, strings and their ids, spill records and their pair indices, error kind,
// line and message.  The empty subset goes in as (nullptr, 0) and as (pointer, 0); a subset that is not ascending is
// refused.  gk_bam_pack_plain_host, the same route with the shared decoder on the ingest threads, is held to the same.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
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
std::string tagZ(const char* name, const std::string& v) {
  std::string s(name, 2);
  s.push_back('Z');
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

// An alignment of M, D and I ops with mismatches at chosen read offsets: SEQ and a standard MD are generated.
struct Plain {
  Cigar cigar;
  std::string seq, md;
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
          run = 0; ++at;
        } else {
          ++run;
        }
      }
    } else if (op.first == 'D') {
      p.md += std::to_string(run);
      p.md.push_back('^');
      for (uint32_t k = 0; k < op.second && k < 3; ++k) p.md.push_back("ACGT"[k % 4]);
      run = 0;
    } else {                         // I: read bases without a word in MD
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

Cigar alternating(int n_ops, uint32_t m_len, uint32_t d_len) {
  Cigar c;
  for (int i = 0; i < n_ops; ++i) c.push_back(i % 2 == 0 ? std::make_pair('M', m_len) : std::make_pair('D', d_len));
  return c;
}

// ---- the kinds of pairs a file is made of
enum Kind { kClean, kBusy, kHeaderOnly, kInsA, kInsB, kSpill, kFail, kLone };

struct File {
  std::vector<std::string> recs;    // in stream order: the right (earlier) record of a pair first
  void add(Kind k) {
    const std::string name = "p" + std::to_string(1000 + recs.size());
    const Plain clean = plain({{'M', 50}}, {});
    Mate l = mateOf(clean, true), r = mateOf(clean, false);
    switch (k) {
      case kClean: break;
      case kBusy: { const Plain b = plain({{'M', 10}, {'D', 2}, {'M', 30}}, {3, 17}); l = mateOf(b, true, 4); break; }
      case kHeaderOnly: r.tags = tagInt("NM", 'c', 5) + tagZ("MD", clean.md); break;
      case kInsA: { const Plain b = plain({{'M', 10}, {'I', 2}, {'M', 10}}, {}); l = mateOf(b, true, 2); break; }
      case kInsB: { const Plain b = plain({{'M', 11}, {'I', 3}, {'M', 10}}, {}); r = mateOf(b, false, 3); break; }
      case kSpill: { const Plain b = plain(alternating(15, 5, 1), {}); l = mateOf(b, true, 4); break; }
      case kFail: {                  // an MD base equal to the read base
        const Plain one = plain({{'M', 50}}, {7});
        l = mateOf(one, true, 1);
        l.tags = tagInt("NM", 'c', 1) + tagZ("MD", std::string("7") + one.seq[7] + "42");
        break;
      }
      case kLone: break;
    }
    l.name = r.name = name;
    recs.push_back(encode(r));
    if (k == kLone) return;          // a record whose mate never comes
    recs.push_back(encode(l));
  }
};

File fileOf(const std::vector<Kind>& kinds) {
  File f;
  for (Kind k : kinds) f.add(k);
  return f;
}

gk_bam* openFile(const File& f) {
  gk_bam* b = new gk_bam();
  b->ref_names = {"G0", "G1", "X"};
  b->name_sorted = b->collated = true;
  size_t bytes = 0;
  for (auto& r : f.recs) bytes += r.size();
  b->data.resize(bytes);
  b->recs.resize(f.recs.size());
  size_t at = 0;
  for (size_t i = 0; i < f.recs.size(); ++i) {
    memcpy(b->data.data() + at, f.recs[i].data(), f.recs[i].size());
    b->recs[i] = {at, (uint32_t)f.recs[i].size()};
    at += f.recs[i].size();
  }
  return b;
}

// ---- what a packer holds, through the C ABI
struct Snapshot {
  int rc = 0;
  std::string message;
  int32_t kind = 0;
  int64_t line = -1, n_lines = 0, n_reads = 0, n_pairs = 0, n_strange = 0, n_strings = 0, n_spill = 0;
  std::vector<gk_mate> mates;
  std::vector<int64_t> pair_lines, spill_pair;
  std::vector<gk_mate_wide> wide;
  std::vector<std::string> strings;
};

Snapshot snapshot(gk_packer* pk, int rc) {
  Snapshot s;
  s.rc = rc;
  s.message = rc == GK_OK ? "" : g_err;
  gk_packer_error(pk, &s.kind, &s.line);
  gk_packer_counts(pk, &s.n_lines, &s.n_reads, &s.n_pairs, &s.n_strange, &s.n_strings);
  gk_packer_spilled(pk, &s.n_spill);
  s.mates.resize((size_t)(2 * s.n_pairs));
  s.pair_lines.resize((size_t)(2 * s.n_pairs));
  gk_packer_records(pk, s.mates.data(), s.pair_lines.data());
  s.wide.resize((size_t)(2 * s.n_spill));
  s.spill_pair.resize((size_t)s.n_spill);
  gk_packer_spill_records(pk, s.wide.data(), s.spill_pair.data());
  for (int64_t i = 0; i < s.n_strings; ++i) s.strings.push_back(gk_packer_string(pk, i));
  return s;
}

int g_failures = 0;
void complain(const std::string& what, const std::string& why) {
  fprintf(stderr, "FAIL %s: %s\n", what.c_str(), why.c_str());
  ++g_failures;
}

void compare(const std::string& what, const Snapshot& a, const Snapshot& b) {
  auto num = [&](const char* field, int64_t x, int64_t y) {
    if (x != y) complain(what, std::string(field) + ": " + std::to_string(x) + " on the host route, " + std::to_string(y));
  };
  num("return code", a.rc, b.rc);
  num("error kind", a.kind, b.kind);
  num("error line", a.line, b.line);
  num("lines", a.n_lines, b.n_lines);
  num("reads", a.n_reads, b.n_reads);
  num("pairs", a.n_pairs, b.n_pairs);
  num("strange", a.n_strange, b.n_strange);
  num("strings", a.n_strings, b.n_strings);
  num("spilled pairs", a.n_spill, b.n_spill);
  if (a.message != b.message) complain(what, "message '" + a.message + "' on the host route, '" + b.message + "'");
  if (a.n_pairs != b.n_pairs || a.n_spill != b.n_spill) return;
  for (size_t i = 0; i < a.mates.size(); ++i)
    if (memcmp(&a.mates[i], &b.mates[i], sizeof(gk_mate))) { complain(what, "record " + std::to_string(i) + " differs"); break; }
  if (a.pair_lines != b.pair_lines) complain(what, "pair_lines differ");
  if (a.spill_pair != b.spill_pair) complain(what, "pair indices of the spill differ");
  if (!a.wide.empty() && memcmp(a.wide.data(), b.wide.data(), a.wide.size() * sizeof(gk_mate_wide))) complain(what, "spill records differ");
  if (a.strings != b.strings) complain(what, "strings differ");
}

gk_packer* newPacker() {
  const char* genes[2] = {"G0", "G1"};
  const char* strings[1] = {"GG"};          // a string of the index: ids of new ones start at 1
  gk_packer* pk = nullptr;
  if (gk_packer_create(genes, 2, strings, 1, &pk) != GK_OK) exit(2);
  return pk;
}

// the stand-in for the device decoder: force(p, n) turns the verdict of pair p of n into HOST
using Force = std::function<bool(int64_t, int64_t)>;
GkPlainDecoder standIn(const Force& force, int64_t* n_done) {
  return [force, n_done](const GkBamRecords& r, const GkPairList& pairs, gk_mate* mates_out, uint8_t* verdict_out) {
    const GkBamRec* recs = (const GkBamRec*)r.recs;
    const int64_t n = (int64_t)pairs.size() / 2;
    *n_done = 0;
    for (int64_t p = 0; p < n; ++p) {
      const GkBamRec& left = recs[pairs[(size_t)(2 * p)]];
      const GkBamRec& right = recs[pairs[(size_t)(2 * p + 1)]];
      int v = gk_pair_decode(GkPlainBytes{r.data}, left.off, left.size, right.off, right.size, r.gene_of_ref.data(),
                             (int32_t)r.gene_of_ref.size(), mates_out + 2 * p);
      if (force(p, n)) v = GK_DECODE_HOST;
      if (v == GK_DECODE_HOST) memset(mates_out + 2 * p, 0xAB, 2 * sizeof(gk_mate));
      else ++*n_done;
      verdict_out[p] = (uint8_t)v;
    }
    return GK_OK;
  };
}

Snapshot hostRoute(const File& f, int64_t capacity = -1) {
  gk_bam* b = openFile(f);
  gk_packer* pk = newPacker();
  std::vector<gk_mate> ext((size_t)std::max<int64_t>(capacity, 1));
  if (capacity >= 0) gk_packer_set_output(pk, ext.data(), capacity);
  g_err[0] = 0;
  const Snapshot s = snapshot(pk, gk_bam_pack(b, pk));
  gk_packer_destroy(pk);
  gk_bam_close(b);
  return s;
}

struct SplitRun { Snapshot s; int64_t n_done = 0, n_plain = 0, n_host = 0; };
SplitRun splitRoute(const File& f, const Force& force, int64_t capacity = -1) {
  SplitRun run;
  gk_bam* b = openFile(f);
  gk_packer* pk = newPacker();
  std::vector<gk_mate> ext((size_t)std::max<int64_t>(capacity, 1));
  if (capacity >= 0) gk_packer_set_output(pk, ext.data(), capacity);
  g_err[0] = 0;
  GkSplit split;
  const int rc = gk_bam_pack_with(b, pk, standIn(force, &run.n_done), split);
  run.s = snapshot(pk, rc);
  run.n_plain = split.n_plain;
  run.n_host = (int64_t)split.host.size();
  if (split.n_plain + (int64_t)split.host.size() != split.n_pairs) complain("split", "the counts of the split do not add up");
  gk_packer_destroy(pk);
  gk_bam_close(b);
  return run;
}

// the steps of the driver by hand, for subsets the driver never makes: `which` as it is given
Snapshot byHand(const File& f, const int64_t* which, int64_t n_which) {
  gk_bam* b = openFile(f);
  gk_packer* pk = newPacker();
  g_err[0] = 0;
  GkBamRecords r;
  gk_bam_records(b, pk, r);
  GkPairList pairs;
  int64_t first_line = 0;
  int rc = gk_packer_pair_records(pk, r.n_recs, r.names_contiguous, r.key, r.soon, pairs, &first_line);
  if (rc == GK_OK) {
    const int64_t n = (int64_t)pairs.size() / 2;
    gk_mate* mates = gk_packer_reserve_pairs(pk, n);
    std::vector<uint8_t> verdict((size_t)n + 1);
    int64_t n_done = 0;
    if (mates) standIn([](int64_t, int64_t) { return false; }, &n_done)(r, pairs, mates, verdict.data());
    rc = gk_packer_decode_subset(pk, first_line, pairs, which, n_which, r.full, r.soon);
  }
  const Snapshot s = snapshot(pk, rc);
  gk_packer_destroy(pk);
  gk_bam_close(b);
  return s;
}

Snapshot plainHost(const File& f, int64_t* n_plain, int64_t* n_host) {
  gk_bam* b = openFile(f);
  gk_packer* pk = newPacker();
  g_err[0] = 0;
  const Snapshot s = snapshot(pk, gk_bam_pack_plain_host(b, pk, n_plain, n_host));
  gk_packer_destroy(pk);
  gk_bam_close(b);
  return s;
}

const Force kNatural = [](int64_t, int64_t) { return false; };
const Force kAllHost = [](int64_t, int64_t) { return true; };
const Force kOdd = [](int64_t p, int64_t) { return p % 2 == 1; };
const Force kEven = [](int64_t p, int64_t) { return p % 2 == 0; };
const Force kEnds = [](int64_t p, int64_t n) { return p == 0 || p == n - 1; };

}  // namespace

int main() {
  struct Case { std::string what; std::vector<Kind> kinds; int64_t natural_done, pairs_kept, strings, spills; int32_t kind; };
  std::vector<Kind> many;               // more pairs than one thread takes (256 per thread), every kind but the failing one
  for (int i = 0; i < 700; ++i) many.push_back(i % 97 == 5 ? kInsA : i % 89 == 7 ? kSpill : i % 83 == 11 ? kInsB : i % 5 == 0 ? kBusy : i % 7 == 0 ? kHeaderOnly : kClean);
  int64_t many_done = 0;
  for (Kind k : many) many_done += k == kClean || k == kBusy || k == kHeaderOnly;
  const std::vector<Case> cases = {
      {"zero records", {}, 0, 0, 1, 0, 0},
      {"records that pair into nothing", {kLone, kLone, kLone}, 0, 0, 1, 0, 0},
      {"one pair", {kClean}, 1, 1, 1, 0, 0},
      {"one pair that needs the host", {kInsA}, 0, 1, 2, 0, 0},
      {"every pair plain", {kClean, kBusy, kHeaderOnly, kClean, kBusy}, 5, 5, 1, 0, 0},
      {"no pair plain", {kInsA, kSpill, kInsB}, 0, 3, 3, 1, 0},
      {"a HOST pair first and a HOST pair last", {kInsA, kClean, kBusy, kClean, kInsB}, 3, 5, 3, 0, 0},
      {"the same new string twice, plain pairs between", {kClean, kInsA, kClean, kBusy, kInsA, kClean}, 4, 6, 2, 0, 0},
      {"two new strings in either order of appearance", {kInsB, kClean, kInsA, kClean, kInsB}, 2, 5, 3, 0, 0},
      {"a spilled pair between plain pairs", {kClean, kBusy, kSpill, kClean, kClean}, 4, 5, 1, 1, 0},
      {"two spilled pairs and a string", {kSpill, kClean, kInsA, kSpill, kClean}, 2, 5, 2, 2, 0},
      {"a failing pair between plain pairs", {kClean, kBusy, kClean, kFail, kClean, kClean}, 5, 3, 1, 0, 1},
      {"a failing pair behind a string and a spill, more of both behind it", {kInsA, kClean, kSpill, kFail, kInsB, kSpill, kClean}, 2, 3, 2, 1, 1},
      {"a failing pair first", {kFail, kClean, kInsA}, 1, 0, 1, 0, 1},
      {"a failing pair last", {kClean, kInsA, kFail}, 1, 2, 2, 0, 1},
      {"lone records between the pairs", {kLone, kClean, kLone, kInsA, kClean, kLone}, 2, 3, 2, 0, 0},
      {"700 pairs", many, many_done, 700, 3, 8, 0},
  };
  const std::pair<const char*, Force> plans[] = {{"natural verdicts", kNatural}, {"every pair HOST", kAllHost},
                                                 {"odd pairs HOST", kOdd}, {"even pairs HOST", kEven},
                                                 {"first and last pair HOST", kEnds}};
  int runs = 0;
  for (const Case& c : cases) {
    const File f = fileOf(c.kinds);
    const Snapshot host = hostRoute(f);
    // the case is what it claims to be
    if (host.n_pairs != c.pairs_kept) complain(c.what, "pairs kept by the host route: " + std::to_string(host.n_pairs));
    if (host.n_strings != c.strings) complain(c.what, "strings of the host route: " + std::to_string(host.n_strings));
    if (host.n_spill != c.spills) complain(c.what, "spilled pairs of the host route: " + std::to_string(host.n_spill));
    if (host.kind != c.kind) complain(c.what, "error kind of the host route: " + std::to_string(host.kind));
    if (c.kind && host.message.find("MD") == std::string::npos) complain(c.what, "the error is not the MD one: " + host.message);
    for (auto& plan : plans) {
      const std::string what = c.what + ", " + plan.first;
      const SplitRun run = splitRoute(f, plan.second);
      compare(what, host, run.s);
      if (run.n_done != run.n_plain) complain(what, "DONE verdicts and the driver's count differ");
      if (&plan == &plans[0] && run.n_plain != c.natural_done)
        complain(what, "pairs taken by the shared decoder: " + std::to_string(run.n_plain));
      if (&plan == &plans[1] && run.n_plain != 0) complain(what, "a pair was taken although every verdict was HOST");
      ++runs;
    }
    int64_t n_plain = -1, n_host = -1;
    const Snapshot rehearsal = plainHost(f, &n_plain, &n_host);
    compare(c.what + ", gk_bam_pack_plain_host", host, rehearsal);
    if (n_plain != c.natural_done) complain(c.what, "gk_bam_pack_plain_host took " + std::to_string(n_plain) + " pairs");
    ++runs;
  }
  // ---- the empty subset as (nullptr, 0) and as (pointer, 0); it decodes nothing, whatever the pointer
  {
    const File f = fileOf({kClean, kBusy, kHeaderOnly, kClean});
    const Snapshot host = hostRoute(f);
    const int64_t dummy[1] = {3};
    compare("empty subset as a null pointer", host, byHand(f, nullptr, 0));
    compare("empty subset as a pointer with count 0", host, byHand(f, dummy, 0));
    const File one = fileOf({kClean});
    compare("empty subset of one pair", hostRoute(one), byHand(one, nullptr, 0));
    // zero pairs: nothing was reserved, nothing is decoded
    const File none = fileOf({kLone, kLone});
    compare("empty subset of no pairs", hostRoute(none), byHand(none, dummy, 0));
    const int64_t every[4] = {0, 1, 2, 3};
    compare("the whole list as a subset", host, byHand(f, every, 4));
    const int64_t some[2] = {1, 3};
    compare("plain pairs decoded by the packer", host, byHand(f, some, 2));
    runs += 6;
  }
  // ---- subsets that are refused: GK_ERR_ARG, and the packer holds no record of the list
  {
    const File f = fileOf({kClean, kBusy, kClean, kClean});
    const int64_t descending[2] = {2, 1}, twice[2] = {1, 1}, beyond[1] = {4}, negative[1] = {-1}, long_list[5] = {0, 1, 2, 3, 4};
    const struct { const char* what; const int64_t* which; int64_t n; } bad[] = {
        {"a descending subset", descending, 2}, {"a pair listed twice", twice, 2}, {"a pair beyond the list", beyond, 1},
        {"a negative pair", negative, 1}, {"more items than pairs", long_list, 5}, {"a null pointer with a count", nullptr, 2},
        {"a negative count", descending, -1}};
    for (auto& c : bad) {
      const Snapshot s = byHand(f, c.which, c.n);
      if (s.rc != GK_ERR_ARG) complain(c.what, "not refused");
      if (s.n_pairs != 0 || s.kind != 0) complain(c.what, "the packer holds records or an error after the refusal");
      ++runs;
    }
  }
  // ---- a caller's buffer: just large enough, and one record short (the host route's error, in its words)
  {
    const File f = fileOf({kClean, kInsA, kClean});
    compare("a caller's buffer of 6 records", hostRoute(f, 6), splitRoute(f, kNatural, 6).s);
    const Snapshot host = hostRoute(f, 5);
    if (host.kind != 3) complain("a caller's buffer of 5 records", "the host route does not refuse it");
    compare("a caller's buffer of 5 records", host, splitRoute(f, kNatural, 5).s);
    runs += 2;
  }
  // ---- a decoder that fails, and one that declines
  {
    const File f = fileOf({kClean, kInsA, kClean});
    for (int answer : {GK_ERR_HIP, kGkDecoderDeclines}) {
      gk_bam* b = openFile(f);
      gk_packer* pk = newPacker();
      g_err[0] = 0;
      GkSplit split;
      const int rc = gk_bam_pack_with(b, pk, [answer](const GkBamRecords&, const GkPairList&, gk_mate*, uint8_t*) { return answer; }, split);
      const Snapshot s = snapshot(pk, rc);
      if (answer == GK_ERR_HIP) {
        if (rc != GK_ERR_HIP || s.n_pairs != 0 || s.kind != 0) complain("a decoder that fails", "its code is not returned over an empty packer");
      } else {
        compare("a decoder that declines", hostRoute(f), s);
        if (split.n_plain != 0 || split.host.size() != 3) complain("a decoder that declines", "the split does not say that the host took every pair");
      }
      gk_packer_destroy(pk);
      gk_bam_close(b);
      ++runs;
    }
  }
  printf("ingest split: %d runs\n", runs);
  if (g_failures) { printf("ingest split: %d failures\n", g_failures); return 1; }
  printf("ingest split: ok\n");
  return 0;
}
