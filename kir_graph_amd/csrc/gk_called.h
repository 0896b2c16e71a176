// The called columns of a call report (gk_callfit.hip, gk_callswap.hip, gk_calldosage.hip, gk_callcov.hip): every report
// reads the K distinct called columns (1 .. 16) of the u8 mismatch table miss8[column][row] the search left in HBM.  What
// they share is here, once: the list of the columns as a kernel argument, the checks of the table and of the list at an
// entry point, the ladder from K to the columns a lane loads (KT = 1, 2, 4, 8, 16), and the small device helpers.  The row
// loops of the kernels are NOT shared: their registers are counted per kernel (see the comments at callfit_profile,
// callswap_rows and calldosage_patterns).
#pragma once
#include "gk_blocks.h"

constexpr int kCalledMaxCols = 16;

// the called columns, passed to a kernel by value; the entries beyond the list are 0
struct GkCalledCols { int32_t c[kCalledMaxCols]; };

// what every report asks of the table it reads
inline bool gk_called_table_ok(gk_dptr d_miss8, int64_t ldm, int64_t n_rows, int32_t n_table_cols) {
  return d_miss8 && d_miss8 % 16 == 0 && n_rows >= 1 && n_rows < (1ll << 31) && ldm >= n_rows && ldm % 64 == 0 &&
         n_table_cols >= 1;
}

#define GK_CALLED_REQUIRE(cond, text)                                    \
  do {                                                                   \
    if (!(cond)) {                                                       \
      gk_set_error("%s: " text " (%s:%d)", what, __FILE__, __LINE__);    \
      return GK_ERR_ARG;                                                 \
    }                                                                    \
  } while (0)

// The checks of an entry point `what` ("call fit", ...) on its table and its called columns, in the order every entry
// point makes them: the table, the number of columns, the entry point's own arguments (`between`, which returns GK_OK or
// has set the error), then every column in range and listed once.  Fills `out`, padded with 0.  Writes host memory only.
template <class Between>
inline int gk_called_cols(const char* what, gk_dptr d_miss8, int64_t ldm, int64_t n_rows, int32_t n_table_cols,
                          const int32_t* cols, int32_t n_cols, GkCalledCols* out, Between between) {
  GK_CALLED_REQUIRE(gk_called_table_ok(d_miss8, ldm, n_rows, n_table_cols),
                    "needs a 16-byte aligned table, 1 <= n_rows < 2^31 and n_rows <= ldm, a multiple of 64");
  GK_CALLED_REQUIRE(n_cols >= 1 && n_cols <= kCalledMaxCols, "the number of called columns must lie in 1 .. 16");
  if (const int rc = between()) return rc;
  for (int k = 0; k < kCalledMaxCols; ++k) out->c[k] = 0;
  for (int k = 0; k < n_cols; ++k) {
    GK_CALLED_REQUIRE(cols[k] >= 0 && cols[k] < n_table_cols, "a called column is not in the table");
    for (int j = 0; j < k; ++j) GK_CALLED_REQUIRE(cols[j] != cols[k], "a called column is listed twice");
    out->c[k] = cols[k];
  }
  return GK_OK;
}

// KT of K listed columns, and LAUNCH(KT) for it: a kernel is instantiated for 1, 2, 4, 8 and 16 columns
constexpr int calledKT(int n_cols) { return n_cols == 1 ? 1 : n_cols == 2 ? 2 : n_cols <= 4 ? 4 : n_cols <= 8 ? 8 : 16; }

#define GK_CALLED_LAUNCH(n_cols, LAUNCH) \
  switch (calledKT(n_cols)) {            \
    case 1: LAUNCH(1); break;            \
    case 2: LAUNCH(2); break;            \
    case 4: LAUNCH(4); break;            \
    case 8: LAUNCH(8); break;            \
    default: LAUNCH(16); break;          \
  }

__device__ inline uint32_t sad4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }

__device__ inline uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// the first `n` bytes (rows) of the 16 a lane holds, as masks of its four words
__device__ inline uint32_t row_mask(int n, int word) {
  const int k = n - 4 * word;
  return k >= 4 ? 0xFFFFFFFFu : k <= 0 ? 0u : (1u << (8 * k)) - 1u;
}
