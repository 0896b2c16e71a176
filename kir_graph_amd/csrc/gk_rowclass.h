// Row classes of one gene's rows (gk_rowclass.hip): which rows of the compatibility table carry the same kept
// (id, sign) sequence.  Everything is queued on the context's stream; nothing is waited for.
#pragma once
#include "gk_blocks.h"

struct gk_rowclass {
  int32_t* rep_rows = nullptr;      // [n_rows]: rows[] of the classes' representatives, in row order; *n_classes are set
  uint32_t* class_of = nullptr;     // [n_rows]: class of every row = the rank of its representative
  uint32_t* n_classes = nullptr;    // device: 1 <= *n_classes <= n_rows
  GkBlocks blocks;                  // the pool blocks behind all of it: they go back with the record
};

// n_rows > 0.  On an error `rc` is left as it was.
int gk_rowclass_enqueue(gk_ctx* ctx, gk_tab* tab, const int32_t* d_rows, int64_t n_rows, const uint8_t* d_vflag,
                        gk_rowclass* rc);
// L [n_cols][n_rows] from the compact table Lc [class][ldc] (ldc = gk_rowclass_ld(n_cols): the columns, up to a multiple of
// 8), and miss8 [n_cols][ldm], every byte of it: the counts read back from the log-likelihoods as compat_kernel reads
// them back, rows from n_rows to ldm zero
int64_t gk_rowclass_ld(int n_cols);
int gk_rowclass_expand(gk_ctx* ctx, const gk_rowclass* rc, const double* Lc, int64_t ldc, int n_cols, int64_t n_rows,
                       double* L, uint8_t* miss8, int64_t ldm);

// The class record of a table that was written through its row classes, kept beyond the table call: the class of every
// row.  The rows and the drop flags decide it, so it holds for every later pass over the table's entries.
struct GkClassOf {
  uint32_t* class_of = nullptr;     // [n_rows]; null: the table was written row by row
  int64_t n_rows = 0;
  GkBlocks blocks;
};
// gk_compat_log_miss (table_cols == nullptr) / gk_compat_log_miss_cols with an owner (may be null) for that record
int gk_compat_log_miss_owned(gk_ctx* ctx, gk_tab* tab, gk_dptr d_rows, int64_t n_rows, gk_dptr d_vflag, int32_t vbeg,
                             int32_t vend, gk_dptr d_mask, int32_t words, int32_t n_allele, int32_t keep_empty, gk_lut* lut,
                             const int32_t* table_cols, int32_t n_table_cols, gk_dptr d_log, gk_dptr d_miss8, int64_t ldm,
                             gk_dptr d_flags, GkClassOf* owner);
