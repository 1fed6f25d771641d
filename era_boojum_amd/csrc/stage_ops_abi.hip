// C-ABI entry points of seam S2 for the prover's second round and its quotient terms (rows a9, a10, a12 of SURVEY §8 as
// stand-alone operators): the kernels bj_prove runs, callable on caller-provided device columns so that each can be
// compared with the reference function it replaces (with oracle/prover_ops.c on satisfied circuits in tests/test_gpu_stage_ops.py,
// with the definitions in python integers on arbitrary columns in tests/test_gpu_quotient_terms.py).
#include "ctx.h"
#include "gate_program.h"

#include <string>
#include <vector>

using gl::u64;

extern "C" {

int bj_copy_perm_stage2(bj_ctx *ctx, const uint64_t *d_vars, size_t var_stride, const uint64_t *d_sigmas, size_t sig_stride,
                        const uint64_t *h_non_residues, unsigned num_vars, unsigned chunk, unsigned log_n,
                        const uint64_t *h_beta, const uint64_t *h_gamma, uint64_t *d_z, uint64_t *d_partials) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_vars || !d_sigmas || !h_non_residues || !h_beta || !h_gamma || !d_z)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_copy_perm_stage2: null pointer");
    if (num_vars == 0 || chunk == 0 || log_n > 30) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_copy_perm_stage2: bad geometry");
    const size_t n = (size_t)1 << log_n;
    if (var_stride < n || sig_stride < n) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_copy_perm_stage2: column stride below n");
    const unsigned n_chunks = (num_vars + chunk - 1) / chunk;
    if (n_chunks > 1 && !d_partials) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_copy_perm_stage2: null partial-product buffer");
    if (int rc = bj::ensure_twiddles(ctx, log_n, false)) return rc;
    bj::TmpBuf nr(true), tmp(true), dummy(true);   // freed after the stream has drained: these are test / plumbing entry points
    if (int rc = nr.alloc(ctx, num_vars)) return rc;
    if (int rc = tmp.alloc(ctx, bj::copy_perm_stage2_scratch_words(n_chunks, n))) return rc;
    u64 *partials = d_partials;
    if (!partials) {   // one chunk: the kernel still wants a valid pointer
        if (int rc = dummy.alloc(ctx, 8)) return rc;
        partials = dummy.p;
    }
    if (int rc = bj::h2d_async(ctx, nr.p, h_non_residues, 8 * (size_t)num_vars)) return rc;
    bool small_k = true;
    for (unsigned c = 0; c < num_vars; c++) small_k = small_k && gl::canon(h_non_residues[c]) < ((u64)1 << 32);
    const bj::CopyPermArg cp{{d_vars, var_stride}, {d_sigmas, sig_stride}, nr.p, num_vars, chunk, log_n, ctx->tw_fwd.p, h_beta, h_gamma, small_k};
    bj::launch_copy_perm_stage2(cp, tmp.p, d_z, partials, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

int bj_lookup_polys(bj_ctx *ctx, const uint64_t *d_lookup_vars, size_t var_stride, const uint64_t *d_table_id,
                    const uint64_t *d_tables, size_t table_stride, const uint64_t *d_multiplicities, unsigned reps, unsigned width,
                    unsigned log_n, const uint64_t *h_beta, const uint64_t *h_gamma, uint64_t *d_A, uint64_t *d_B) {
    if (int rc = bj::bind(ctx)) return rc;
    // d_table_id may be NULL: the table id is then the (width+1)-th variable column of every sub-argument
    if (!d_lookup_vars || !d_tables || !d_multiplicities || !h_beta || !h_gamma || !d_A || !d_B)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_lookup_polys: null pointer");
    if (reps == 0 || width == 0 || width > 8 || log_n > 30) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_lookup_polys: bad geometry (width 1..8)");
    const size_t n = (size_t)1 << log_n;
    if (var_stride < n || table_stride < n) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_lookup_polys: column stride below n");
    const bj::LookupArg l{{d_lookup_vars, var_stride}, {d_tables, table_stride}, d_table_id, d_multiplicities, reps, width, h_beta, h_gamma};
    bj::launch_lookup_polys(l, log_n, d_A, d_B, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

int bj_quotient_gates(bj_ctx *ctx, const uint64_t *d_vars, size_t var_stride, unsigned num_gp_vars, const uint64_t *d_consts,
                      size_t const_stride, unsigned num_constant_cols, const bj_gate_desc *gates, unsigned num_gates,
                      const uint64_t *h_alphas, size_t num_points, uint64_t *d_out0, uint64_t *d_out1) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_vars || !d_consts || !gates || !d_out0 || !d_out1) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_gates: null pointer");
    if (num_gates == 0 || num_gates > 16) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_gates: 1..16 gate types");
    if (var_stride < num_points || const_stride < num_points)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_gates: column stride below the number of points");
    // the rules of a circuit's gates (gate_list.h) over the columns given here, and two refusals of this operator's own
    const bj::GateColumns cols{num_gp_vars, num_constant_cols, ~0u};
    bj::GateList L;
    std::string err;
    for (unsigned g = 0; g < num_gates; g++) {
        const bj_gate_desc &G = gates[g];
        if (G.kind < BJ_GATE_CONSTANT_ALLOCATOR || G.kind > BJ_GATE_POSEIDON_FLATTENED)
            return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_quotient_gates: gate %u: kind %d is not evaluated here", g, G.kind);
        bj::GateShape shape;
        if (int rc = bj::resolve_gate(G, g, cols, &shape, &err, "reads past the given columns"))
            return bj::fail(ctx, rc, "bj_quotient_gates: %s", err.c_str());
        unsigned ve = 0, ce = 0, we = 0;
        if (G.kind == BJ_GATE_PROGRAM) bj::gate_program_extent(G.program, &ve, &ce, &we);
        if (we) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_quotient_gates: gate %u reads witness columns", g);
        L.push_general(shape);
    }
    const size_t n_terms = L.n_general_terms;
    if (n_terms && !h_alphas) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_gates: null alpha powers");
    std::vector<bj::DevProgram> programs(num_gates);   // op-list gates; their device copies live until their kernels are done
    auto release = [&]() {
        bool synced = false;
        for (auto &p : programs)
            if (p.block) {
                if (!synced) (void)hipStreamSynchronize(ctx->stream);
                synced = true;
                p.release();
            }
    };
    for (unsigned g = 0; g < num_gates; g++)
        if (gates[g].kind == BJ_GATE_PROGRAM)
            if (int rc = programs[g].upload(ctx, gates[g].program)) {
                release();
                return rc;
            }
    bj::TmpBuf al(true);
    int rc = al.alloc(ctx, 2 * (n_terms + 1));
    if (!rc && n_terms) rc = bj::h2d_async(ctx, al.p, h_alphas, 16 * n_terms);
    if (!rc) {
        bj::launch_general_gates(ctx, L.general.data(), programs.data(), num_gates, bj::GateCols{{d_vars, var_stride}, {d_consts, const_stride}, nullptr},
                                 bj::TermSink{al.p, num_points, d_out0, d_out1}, ctx->stream, 0.0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = bj::fail(ctx, BJ_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    }
    release();
    return rc;
}

int bj_quotient_lookup(bj_ctx *ctx, const uint64_t *d_lookup_vars, size_t var_stride, const uint64_t *d_table_id,
                       const uint64_t *d_tables, size_t table_stride, const uint64_t *d_multiplicities, const uint64_t *d_A,
                       const uint64_t *d_B, size_t stage2_stride, unsigned reps, unsigned width, const uint64_t *h_beta,
                       const uint64_t *h_gamma, const uint64_t *h_alphas, size_t num_points, uint64_t *d_out0, uint64_t *d_out1) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_lookup_vars || !d_tables || !d_multiplicities || !d_A || !d_B || !h_beta || !h_gamma || !h_alphas ||
        !d_out0 || !d_out1)   // d_table_id may be NULL (table id as the last variable column of a sub-argument)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_lookup: null pointer");
    if (reps == 0 || width == 0 || width > 8) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_lookup: bad geometry (width 1..8)");
    if (var_stride < num_points || table_stride < num_points || stage2_stride < num_points)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_lookup: column stride below the number of points");
    bj::TmpBuf al(true);
    if (int rc = al.alloc(ctx, 2 * ((size_t)reps + 1))) return rc;
    if (int rc = bj::h2d_async(ctx, al.p, h_alphas, 16 * ((size_t)reps + 1))) return rc;
    const bj::LookupArg l{{d_lookup_vars, var_stride}, {d_tables, table_stride}, d_table_id, d_multiplicities, reps, width, h_beta, h_gamma};
    bj::launch_quotient_lookup(l, d_A, d_B, stage2_stride, bj::TermSink{al.p, num_points, d_out0, d_out1}, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

int bj_quotient_copy_perm(bj_ctx *ctx, const uint64_t *d_vars, size_t var_stride, const uint64_t *d_sigmas, size_t sig_stride,
                          const uint64_t *d_stage2, size_t stage2_stride, const uint64_t *h_non_residues, unsigned num_vars,
                          unsigned chunk, unsigned log_n, unsigned log_lde, const uint64_t *h_beta, const uint64_t *h_gamma,
                          const uint64_t *h_alphas, size_t num_points, size_t first_point, uint64_t *d_out0, uint64_t *d_out1) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_vars || !d_sigmas || !d_stage2 || !h_non_residues || !h_beta || !h_gamma || !h_alphas || !d_out0 || !d_out1)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_copy_perm: null pointer");
    if (num_vars == 0 || num_vars > 4096 || chunk == 0 || log_n > 30 || log_lde > 6)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_copy_perm: bad geometry (1..4096 columns, LDE factor at most 64)");
    const size_t n = (size_t)1 << log_n;
    if (first_point + num_points > (n << log_lde)) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_copy_perm: points past the LDE domain");
    // the kernel takes the index inside the coset from the LOCAL index, and reads z(omega x) anywhere in the coset of its point
    if (first_point & (n - 1)) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_copy_perm: first_point is not a multiple of n");
    const size_t whole_cosets = (num_points + n - 1) & ~(n - 1);
    if (var_stride < whole_cosets || sig_stride < whole_cosets || stage2_stride < whole_cosets)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_quotient_copy_perm: column stride below the number of points rounded up to whole cosets");
    if (int rc = bj::ensure_twiddles(ctx, log_n + log_lde, false)) return rc;
    const unsigned n_chunks = (num_vars + chunk - 1) / chunk;
    bj::TmpBuf nr(true), al(true);
    if (int rc = nr.alloc(ctx, num_vars)) return rc;
    if (int rc = al.alloc(ctx, 2 * ((size_t)n_chunks + 1))) return rc;
    if (int rc = bj::h2d_async(ctx, nr.p, h_non_residues, 8 * (size_t)num_vars)) return rc;
    if (int rc = bj::h2d_async(ctx, al.p, h_alphas + 2, 16 * (size_t)n_chunks)) return rc;
    bool small_k = true;
    for (unsigned c = 0; c < num_vars; c++) small_k = small_k && gl::canon(h_non_residues[c]) < ((u64)1 << 32);
    const bj::CopyPermArg cp{{d_vars, var_stride}, {d_sigmas, sig_stride}, nr.p, num_vars, chunk, log_n, ctx->tw_fwd.p, h_beta, h_gamma, small_k};
    bj::launch_quotient_copy_perm(cp, bj::Cols{d_stage2, stage2_stride}, log_lde, h_alphas /* the L1 power; al: the chunks' that follow it */,
                                  bj::TermSink{al.p, num_points, d_out0, d_out1}, first_point, nullptr, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

int bj_combine_residues(bj_ctx *ctx, const uint64_t *d_residues, unsigned world, size_t residue_len, unsigned num_cols,
                        const uint64_t *h_moduli, uint64_t *d_out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_residues || !h_moduli || !d_out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_combine_residues: null pointer");
    if (world == 0 || world > 8 || residue_len == 0 || num_cols == 0 || num_cols > 65535)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_combine_residues: 1..8 residues of at least one coefficient, at most 65535 columns");
    if (!bj::launch_combine_residues(d_residues, world, residue_len, num_cols, h_moduli, d_out, ctx->stream))
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_combine_residues: the moduli x^E - a_i are not pairwise distinct");
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

}  // extern "C"
