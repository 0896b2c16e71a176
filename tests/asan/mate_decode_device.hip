// Compile check only (tests/test_mate_decode_host.py builds the code object for gfx950 and runs nothing): the shared
// decoder of csrc/gk_mate_decode.h must stay device code -- no heap, no std::, aligned word reads.
#include <hip/hip_runtime.h>

#include "gk_mate_decode.h"

struct Rec { uint64_t off; uint32_t size; uint32_t pad; };

__global__ void decode_check(const uint32_t* stream, const Rec* recs, const int64_t* pairs, int64_t n_pairs,
                             const int32_t* gene_of_ref, int32_t n_ref, gk_mate* out, uint32_t* verdict) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const Rec l = recs[pairs[2 * p]], r = recs[pairs[2 * p + 1]];
  verdict[p] = (uint32_t)gk_pair_decode(GkWordBytes{stream}, l.off, l.size, r.off, r.size, gene_of_ref, n_ref, out + 2 * p);
}
