// Compile check only (tests/test_mate_runs_host.py builds the code object for gfx950 and runs nothing): the shared walk
// of csrc/gk_materuns.h and the draw of csrc/gk_draw.h must stay device code without gk_common.h -- no heap, no std::.
#include <hip/hip_runtime.h>

#include "gk_draw.h"
#include "gk_materuns.h"

template <bool kCompact>
__global__ void runs_check(GkMateSample s, int64_t len, uint64_t seed, uint32_t* diff, uint32_t* staged) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * s.n_valid) return;
  const int side = (int)(t & 1);
  GkMateRuns m;
  if (!gk_mate_find<kCompact>(s, t >> 1, side, [](uint32_t ref) { return ref == 0; }, m)) return;
  gk_mate_walk<kCompact>(s, m, side, len, [&](int64_t a, int64_t e) {
    atomicAdd(&diff[a], 1u);
    atomicAdd(&diff[e], 0xFFFFFFFFu);
  });
  GkMateCigar cig;
  if (!gk_mate_stage<kCompact>(s, m, side, cig)) return;
  const uint32_t w = gk_boot_draw(seed, (uint64_t)t, 0, 0, 8u) + 1;
  gk_mate_walk_staged(m, cig, len, [&](int64_t a, int64_t e) {
    atomicAdd(&staged[a], w);
    atomicAdd(&staged[e], 0u - w);
  });
}

template __global__ void runs_check<false>(GkMateSample, int64_t, uint64_t, uint32_t*, uint32_t*);
template __global__ void runs_check<true>(GkMateSample, int64_t, uint64_t, uint32_t*, uint32_t*);
