// Internal: the words of device memory that a launcher or an entry point needs beside its arguments — scratch the caller hands
// over, or a temporary the callee takes itself (out of the proof's workspace while a proof runs).  Part of kernels.h, which
// includes it beside the launchers; kept free of HIP so that workspace_plan.h and a host program can sum the same numbers.
#pragma once
#include <cstddef>

namespace bj {
// stage2.hip: d_tmp of launch_copy_perm_stage2 — the chunk products [2][n_chunks][n], a total per 1024-row block, 16 spare
inline size_t copy_perm_stage2_scratch_words(unsigned n_chunks, size_t n) { return (size_t)2 * n_chunks * n + 2 * ((n + 1023) / 1024) + 16; }

// openings.hip: a workgroup of launch_barycentric_eval covers 256 * BARY_PTS consecutive points
constexpr int BARY_PTS = 32;
inline unsigned barycentric_num_blocks(size_t n) { return (unsigned)((n + 256 * BARY_PTS - 1) / (256 * BARY_PTS)); }
// openings_abi.hip: the argument block of bj_barycentric_eval_batch — [pointers][partial sums per block][values]
inline size_t barycentric_arg_words(size_t n_cols, size_t n) { return n_cols + n_cols * barycentric_num_blocks(n) * 2 + n_cols * 2; }
// openings_abi.hip: the argument block of combine_monomials and of the deep_accumulate calls — [pointers][F_p^2 coefficients]
inline size_t column_list_arg_words(size_t n_cols) { return 3 * n_cols; }
constexpr int DEEP_MAX_SETS = 3;   // opening sets one launch_deep_accumulate_multi takes

// prover.hip: the staging of all_gather_columns, [world][parts][part_len]; one device alone copies straight through
inline size_t gather_columns_staging_words(unsigned world, unsigned parts, size_t part_len) {
    return world > 1 ? (size_t)world * parts * part_len : 0;
}
}  // namespace bj
