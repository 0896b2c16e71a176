// Internal interface between the alignment readers and the packer (gk_sampack.cpp): what the packer
// needs to know about one alignment record, whatever it was read from.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <string_view>
#include <algorithm>
#include <cstring>
#include <exception>
#include <new>
#include <vector>

#include <chrono>
#include <cstdio>
#include <cstdlib>

#include <thread>

#include "gk_env.h"
#include "graphkir_hip.h"

struct gk_packer;

// allocator whose resize() leaves new elements uninitialised: buffers of hundreds of megabytes that the
// worker threads are about to overwrite (and first-touch in parallel)
template <typename T>
struct GkRawInit : std::allocator<T> {
  template <typename U> struct rebind { using other = GkRawInit<U>; };
  template <typename U> void construct(U* p) noexcept { ::new ((void*)p) U; }
  template <typename U, typename... A> void construct(U* p, A&&... a) { ::new ((void*)p) U(std::forward<A>(a)...); }
};

// threads of the native readers / packers / writers: GK_PACK_THREADS (default 8), at most the hardware's
inline int gk_ingest_threads() {
  const char* e = getenv("GK_PACK_THREADS");
  long n = e ? atol(e) : 8;
  const long hw = (long)std::thread::hardware_concurrency();
  if (hw > 0) n = std::min(n, hw);
  return (int)std::max<long>(1, std::min<long>(n, 64));
}

// GK_TRACE=ingest: phase times of the host ingest on stderr (development aid)
struct GkPhaseClock {
  const char* what;
  bool on;
  std::chrono::steady_clock::time_point t;
  explicit GkPhaseClock(const char* w) : what(w), on(gk_trace("ingest")), t(std::chrono::steady_clock::now()) {}
  void lap(const char* phase) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[ingest] %s %s %.1f ms\n", what, phase, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

struct GkAlnKey {            // fields of readPair's pairing rule (hisat2.py:248-258)
  std::string_view name, ref;
  long flag = 0, pos = 0, next_pos = 0;   // positions 1-based like the SAM text
  bool mate_same_ref = false;             // RNEXT is "="
};

struct GkAlnRecord {         // fields of filterRead / getNH / recordToRawVariant
  std::string_view ref, cigar, seq, md, zs;
  std::string cigar_text, seq_text;       // storage when the source is not text (views above point here)
  // A BAM source may hand over CIGAR and SEQ as they lie in the record instead of as text (bam_cigar != nullptr;
  // `cigar` / `seq` are then unset): n_bam_cigar little-endian words `len << 4 | op`, every op one of M I D N S
  // (0..4), at least one of them, and l_bam_seq >= 1 bases of 4 bits ("=ACMGRSVTWYHKDBN", high nibble first).
  // Records outside that shape (other ops, no CIGAR, no SEQ) come as text: their SAM spelling has quirks
  // under the reference's regular expression that only the text walk reproduces.
  const uint8_t* bam_cigar = nullptr;
  const uint8_t* bam_seq = nullptr;
  uint32_t n_bam_cigar = 0, l_bam_seq = 0;
  long flag = 0, pos = 0, nm = 0, nh = 1;
  bool has_nm = false, has_md = false, has_zs = false;
  // backbone ordinal of `ref` when the source knows it (BAM: reference ids map to it once per file), -1 when
  // it is no backbone of the index; kGeneByName: look `ref` up by name
  static constexpr int kGeneByName = -2;
  int gene = kGeneByName;
};

// backbone ordinal of a reference name in the packer's index, -1 when it is none
int gk_packer_gene_of(const gk_packer* pk, std::string_view ref);

// Pair n records in stream order like readPair and pack the emitted pairs (decoding on several
// threads).  key(i, k) and full(i, r) fill the fields of record i; both must be thread-safe and the
// views must stay valid until the call returns.  Line numbers reported for errors / pairs are
// first_line + i.  names_contiguous: records of one name are adjacent (a name-collated stream), which
// lets the pairing run on several threads.  soon(i, head_only), when given, announces that key(i) (head_only) or full(i)
// is about to be called (a source whose records lie scattered in memory can prefetch them).  Returns GK_OK or the packer's error code.
int gk_packer_feed_records(gk_packer* pk, int64_t n, bool names_contiguous,
                           const std::function<void(int64_t, GkAlnKey&)>& key,
                           const std::function<void(int64_t, GkAlnRecord&)>& full,
                           const std::function<void(int64_t, bool)>& soon = nullptr);

// The two halves of gk_packer_feed_records, which is the two in sequence: a later device ingest decodes most pairs of
// the list itself and must be able to sit between them.
// gk_packer_pair_records: the pairing alone -- pairs[2p], pairs[2p + 1] = left (later) and right (earlier) record of
// emitted pair p, *first_line = line number of record 0; the packer's read / pair / strange counts are updated.
// gk_packer_decode_pairs: decodes the pairs of the list into the packer, in list order.
using GkPairList = std::vector<int64_t, GkRawInit<int64_t>>;
int gk_packer_pair_records(gk_packer* pk, int64_t n, bool names_contiguous,
                           const std::function<void(int64_t, GkAlnKey&)>& key,
                           const std::function<void(int64_t, bool)>& soon, GkPairList& pairs, int64_t* first_line);
int gk_packer_decode_pairs(gk_packer* pk, int64_t first_line, const GkPairList& pairs,
                           const std::function<void(int64_t, GkAlnRecord&)>& full,
                           const std::function<void(int64_t, bool)>& soon);
// The split route: somebody else (a device ingest) writes the records of most pairs of the list and the packer decodes
// the rest.  gk_packer_reserve_pairs makes room for the n_pairs pairs of the NEXT list and returns their first slot
// (nullptr, and nothing changed: no pairs, a buffer of gk_packer_set_output that is too small, an error held);
// gk_packer_unreserve takes that back when the list is not going to come.
// gk_packer_decode_subset decodes the pairs which[0] < which[1] < ... (n_which of them, checked: GK_ERR_ARG and the
// room taken back) of the list into their slots of the whole list, and fills `pair_lines` for every pair of the
// list; strings, spills, the error and the truncation at the first failing pair are what gk_packer_decode_pairs
// makes of the same list as long as the other pairs need none of them.  The subset is a (pointer, count) pair:
// n_which == 0 decodes NOTHING (and still makes the room and fills the lines) whatever the pointer is, null included;
// "every pair" is n_which == n_pairs, never a null pointer.
gk_mate* gk_packer_reserve_pairs(gk_packer* pk, int64_t n_pairs);
void gk_packer_unreserve(gk_packer* pk);
int gk_packer_decode_subset(gk_packer* pk, int64_t first_line, const GkPairList& pairs, const int64_t* which,
                            int64_t n_which, const std::function<void(int64_t, GkAlnRecord&)>& full,
                            const std::function<void(int64_t, bool)>& soon);

// An open BAM file as the packer's callers see it: the inflated stream, the record table in output order (GkBamRec),
// the file's reference id -> backbone ordinal table for the packer's
// index (-1: no backbone) and the three callbacks of gk_packer_feed_records.  The callbacks point into this object and
// into the file handle: neither may move or go away while they are in use.
struct gk_bam;
struct GkBamRec { uint64_t off; uint32_t size; uint32_t unused; };   // a record's bytes are data[off, off + size)
struct GkBamRecords {
  const uint8_t* data = nullptr;
  size_t data_bytes = 0;
  size_t data_capacity = 0;        // bytes of the allocation behind `data` (>= data_bytes; what lies behind data_bytes is anything)
  const void* recs = nullptr;
  int64_t n_recs = 0;
  bool names_contiguous = false;
  std::vector<int32_t> gene_of_ref;
  std::function<void(int64_t, GkAlnKey&)> key;
  std::function<void(int64_t, GkAlnRecord&)> full;
  std::function<void(int64_t, bool)> soon;      // empty when the records lie in reading order
};
void gk_bam_records(gk_bam* b, gk_packer* pk, GkBamRecords& out);
bool gk_bam_records_inside(const GkBamRecords& r);   // every record of the table lies inside the stream

// The split route over an open file: gk_bam_records, gk_packer_pair_records, then `decoder` writes the
// final records of the pairs it can take into mates_out (2 per pair, the packer's own slots) and one verdict per pair
// (GK_DECODE_DONE / GK_DECODE_HOST, gk_mate_decode.h; a HOST pair may leave anything in its slots), then
// gk_packer_decode_subset over the HOST pairs.  The decoder returns GK_OK, an error code (returned as it is, the
// packer as before the call but for the counts of the pairing) or kGkDecoderDeclines: the file is not for it, and
// gk_packer_decode_pairs takes the whole list.  The packer afterwards is what gk_bam_pack leaves of the same file.
using GkPlainDecoder = std::function<int(const GkBamRecords&, const GkPairList&, gk_mate* mates_out, uint8_t* verdict_out)>;
constexpr int kGkDecoderDeclines = 1;
struct GkSplit {
  int64_t n_pairs = 0, n_plain = 0;   // pairs of the list / of them decoded by the decoder
  std::vector<int64_t> host;          // the pairs the packer decoded itself, ascending (all of them: n_plain == 0)
  gk_mate* mates = nullptr;           // first slot of the list's pairs in the packer's array (nullptr: no pairs)
};
inline int gk_bam_pack_with(gk_bam* b, gk_packer* pk, const GkPlainDecoder& decoder, GkSplit& split) {
  split = GkSplit();
  GkBamRecords r;
  gk_bam_records(b, pk, r);
  GkPairList pairs;
  int64_t first_line = 0;
  int rc = gk_packer_pair_records(pk, r.n_recs, r.names_contiguous, r.key, r.soon, pairs, &first_line);
  if (rc != GK_OK) return rc;
  const int64_t n = (int64_t)pairs.size() / 2;
  split.n_pairs = n;
  if (!n) return GK_OK;
  auto all_host = [&] {
    split.host.resize((size_t)n);
    for (int64_t p = 0; p < n; ++p) split.host[(size_t)p] = p;
    return gk_packer_decode_pairs(pk, first_line, pairs, r.full, r.soon);
  };
  gk_mate* const mates = gk_packer_reserve_pairs(pk, n);
  if (!mates) return all_host();      // no room: the host route reports it in its own words
  split.mates = mates;
  std::vector<uint8_t, GkRawInit<uint8_t>> verdict((size_t)n);
  rc = decoder(r, pairs, mates, verdict.data());
  if (rc != GK_OK) {
    gk_packer_unreserve(pk);
    return rc == kGkDecoderDeclines ? all_host() : rc;
  }
  for (int64_t p = 0; p < n; ++p)
    if (verdict[(size_t)p] != 0) split.host.push_back(p);   // GK_DECODE_DONE is 0
  split.n_plain = n - (int64_t)split.host.size();
  return gk_packer_decode_subset(pk, first_line, pairs, split.host.data(), (int64_t)split.host.size(), r.full, r.soon);
}

// the entry points that allocate with the size of the input: running out of memory is an error code, not an abort
// (an exception must not cross the C boundary)
void gk_set_error(const char* fmt, ...);
template <typename Call>
static inline int gk_guarded(const char* what, const Call& call) {
  try {
    return call();
  } catch (const std::bad_alloc&) {
    gk_set_error("%s: out of host memory", what);
    return GK_ERR_CAPACITY;
  } catch (const std::exception& e) {
    gk_set_error("%s: %s", what, e.what());
    return GK_ERR_ARG;
  }
}

// start offset of every line of a text (a final line without '\n' counts), plus the end as sentinel
inline std::vector<int64_t> gk_line_starts(std::string_view text) {
  std::vector<int64_t> starts;
  const char* base = text.data();
  size_t a = 0;
  while (a < text.size()) {
    starts.push_back((int64_t)a);
    const void* nl = memchr(base + a, '\n', text.size() - a);
    if (!nl) { a = text.size(); break; }
    a = (size_t)((const char*)nl - base) + 1;
  }
  starts.push_back((int64_t)text.size() + (text.empty() || text.back() == '\n' ? 0 : 1));
  return starts;
}

// line i without its line terminator ("\n" or "\r\n")
inline std::string_view gk_line_at(std::string_view text, const std::vector<int64_t>& starts, int64_t i) {
  if (i < 0 || (size_t)i + 1 >= starts.size()) return std::string_view();
  size_t a = (size_t)starts[(size_t)i], b = (size_t)starts[(size_t)i + 1];
  if (b > a) --b;                                   // the '\n' (or the sentinel's virtual one)
  b = std::min(b, text.size());
  std::string_view line = text.substr(a, b - a);
  if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
  return line;
}

