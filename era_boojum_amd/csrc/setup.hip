// Setup creation: bj_setup_create[_sharded] and the accessors of the setup object (setup.h).  The circuit's description is
// checked, the sigma / constant / table columns are brought to the device, inverse-transformed, extended over this GPU's cosets
// of the LDE domain and committed to (setup.rs, prover.rs:211); proofs (prover.hip) only read the result.
#include "ctx.h"
#include "fri_types.h"
#include "gate_program.h"
#include "setup.h"

#include <cstring>

using gl::u64;

namespace bj {
unsigned setup_world(const bj_setup *s) { return s ? s->sh.world : 0; }
}  // namespace bj

extern "C" {

int bj_setup_set_comm(bj_setup *s, const bj_comm *comm) {
    if (!s || !comm) return BJ_ERR_INVALID_ARG;
    if (s->sh.world < 2 || comm->world != s->sh.world || comm->rank != s->sh.rank || (!comm->all_gather && !comm->all_gather_stream))
        return BJ_ERR_INVALID_ARG;   // only the transport changes: the shard this setup holds is fixed
    s->sh.comm = *comm;
    return BJ_OK;
}

void bj_setup_destroy(bj_setup *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->d_nat) (void)hipFree(s->d_nat);
    if (s->d_mono) (void)hipFree(s->d_mono);
    if (s->d_lde) (void)hipFree(s->d_lde);
    if (s->d_tree) (void)hipFree(s->d_tree);
    if (s->d_non_res) (void)hipFree(s->d_non_res);
    if (s->d_inv_xm1) (void)hipFree(s->d_inv_xm1);
    if (s->d_placement) (void)hipFree(s->d_placement);
    if (s->d_wit_placement) (void)hipFree(s->d_wit_placement);
    for (auto &p : s->programs) p.release();
    for (auto &p : s->spec_programs) p.release();
    delete s;
}

int bj_setup_create(bj_ctx *ctx, const bj_circuit *c, const uint64_t *h_sigmas, const uint64_t *h_constants,
                    const uint64_t *h_tables, const bj_proof_config *cfg, bj_setup **out) {
    return bj::setup_create_impl(ctx, c, h_sigmas, nullptr, h_constants, h_tables, cfg, nullptr, out, bj::env().setup_lean);
}

int bj_setup_create_sharded(bj_ctx *ctx, const bj_circuit *c, const uint64_t *h_sigmas, const uint64_t *h_constants,
                            const uint64_t *h_tables, const bj_proof_config *cfg, const bj_comm *comm, bj_setup **out) {
    return bj::setup_create_impl(ctx, c, h_sigmas, nullptr, h_constants, h_tables, cfg, comm, out);
}

}  // extern "C"

void bj::setup_adopt_placement(bj_setup *s, uint32_t *d_placement) { s->d_placement = d_placement; }
const uint32_t *bj::setup_placement(const bj_setup *s) { return s->d_placement; }
void bj::setup_adopt_witness_placement(bj_setup *s, uint32_t *d_placement) {
    if (s->d_wit_placement) (void)hipFree(s->d_wit_placement);   // set again: the caller has no proof of this setup in flight
    s->d_wit_placement = d_placement;
}

// The placement entries at the public input locations, from whichever placement covers the column; synchronises the context's stream.
int bj::setup_read_public_placement(bj_ctx *ctx, bj_setup *s) {
    const size_t n = (size_t)1 << s->log_n;
    s->pub_place.assign(s->pub_cols.size(), PLACEMENT_NONE);
    for (size_t i = 0; i < s->pub_cols.size(); i++) {
        const unsigned c = s->pub_cols[i];
        const uint32_t *from = c < s->V ? s->d_placement : s->d_wit_placement;
        if (!from || c >= s->V + s->Wc) continue;
        BJ_HIP(ctx, hipMemcpyAsync(&s->pub_place[i], from + (size_t)(c < s->V ? c : c - s->V) * n + s->pub_rows[i], 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BJ_OK;
}

// Everything bj_setup_create refuses about a circuit description and a proof config, without touching a device: the geometry,
// the config, the sharding requirements (comm != nullptr), and what bj::resolve_gates (gate_list.h) refuses about the gates, whose
// resolved list goes to *gates.  bj_vk_create runs the same function, so a key is refused exactly where a setup is, in the same
// words after the caller's name.
#define BJ_WHO "%s: "
#define BJ_WHO_SHARDED "%s_sharded: "
static int check_program(bj_ctx *ctx, const bj_gate_program *p) {
    bj::canon::Program C;
    std::string err;
    if (int rc = bj::canon::canonicalize(p, &C, &err)) return bj::fail(ctx, rc, "%s", err.c_str());
    if (C.num_slots > (unsigned)BJ_GATE_PROGRAM_MAX_SLOTS)
        return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "gate program: %u values live at once (at most %d)", C.num_slots, BJ_GATE_PROGRAM_MAX_SLOTS);
    return BJ_OK;
}

int bj::circuit_check(bj_ctx *ctx, const char *who, const bj_circuit *c, const bj_proof_config *cfg, bool has_tables, const bj_comm *comm,
                      bj::GateList *gates) {
    if (c->log_n < 1 || c->log_n > 26) return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "log_n out of range", who);
    if (c->num_gates == 0 || c->num_gates > 16 || !c->gates) return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "1..16 gates expected", who);
    if (!bj::is_pow2(c->quotient_degree) || !bj::is_pow2(cfg->fri_lde_factor) || cfg->fri_lde_factor < 2 ||
        !bj::is_pow2(cfg->cap_size))
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "quotient degree / fri_lde_factor / cap must be powers of two", who);
    {
        const unsigned tk = cfg->transcript ? cfg->transcript : BJ_TRANSCRIPT_POSEIDON2, hk = cfg->tree_hasher ? cfg->tree_hasher : BJ_HASHER_POSEIDON2;
        if (tk > BJ_TRANSCRIPT_KECCAK256 || hk > BJ_HASHER_POSEIDON) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, BJ_WHO "unknown transcript / tree hasher", who);
        const bool byte_hasher = hk == BJ_HASHER_BLAKE2S || hk == BJ_HASHER_KECCAK256,
                   byte_transcript = tk == BJ_TRANSCRIPT_BLAKE2S || tk == BJ_TRANSCRIPT_KECCAK256;
        if (byte_hasher != byte_transcript)   // Transcript::CompatibleCap = TreeHasher::Output (prover.rs:153-168)
            return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "a byte tree hasher (Blake2s / Keccak256) goes with a byte transcript and "
                                                     "an algebraic tree hasher (Poseidon2 / Poseidon) with an algebraic transcript", who);
    }
    if (cfg->fri_lde_factor > 64 || c->quotient_degree > 64)   // per-coset tables of the quotient kernels hold 64 entries
        return bj::fail(ctx, BJ_ERR_UNSUPPORTED, BJ_WHO "fri_lde_factor and quotient_degree are limited to 64", who);
    if (c->num_public_inputs && (!c->public_input_cols || !c->public_input_rows))
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "public input locations missing", who);
    for (unsigned i = 0; i < c->num_public_inputs; i++)
        if (c->public_input_cols[i] >= c->num_vars || (c->public_input_rows[i] >> c->log_n) != 0)
            return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "public input %u at (column %u, row %u) is outside the %u x 2^%u trace", who,
                            i, c->public_input_cols[i], c->public_input_rows[i], c->num_vars, c->log_n);
    if (cfg->pow_bits > 32 || cfg->pow_bits >= cfg->security_level)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "pow_bits must be <= 32 and below the security level (pow.rs:53, prover.rs:2293)", who);
    if (cfg->pow_runner > BJ_POW_KECCAK256)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "pow_runner %u (0 / BJ_POW_BLAKE2S256 / BJ_POW_KECCAK256)", who, cfg->pow_runner);
    const bj::CircuitShape shape = bj::circuit_shape(c, cfg);   // proof_layout.h: the table id as a constant or as a variable
    const bool tid_var = shape.tid_var;
    const unsigned lookup_cps = shape.lookup_cps;
    if (c->lookup_reps && (!has_tables || c->lookup_width == 0 || c->lookup_width > 8 || (!tid_var && c->table_id_col >= c->num_constant_cols)))
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "bad lookup parameters", who);
    if ((uint64_t)c->num_vars < (uint64_t)c->num_gp_vars + (uint64_t)lookup_cps * c->lookup_reps || !c->non_residues)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO "bad column counts", who);
    if (c->num_vars > 4096)   // the copy-permutation quotient keeps k_c * beta of every column in LDS (16 bytes per column)
        return bj::fail(ctx, BJ_ERR_UNSUPPORTED, BJ_WHO "%u copiable columns, at most 4096 are supported", who, c->num_vars);
    unsigned n_chunks = (c->num_vars + c->quotient_degree - 1) / c->quotient_degree;
    if (n_chunks < 2) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, BJ_WHO "a single copy-permutation chunk is not supported", who);
    if (comm && comm->world > 1) {
        const unsigned W = comm->world;
        if (!bj::is_pow2(W) || W > 8 || comm->rank >= W || (!comm->all_gather && !comm->all_gather_stream))
            return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO_SHARDED "world must be a power of two <= 8, rank < world, callback set", who);
        if (cfg->fri_lde_factor % W || cfg->cap_size % W || c->quotient_degree > cfg->fri_lde_factor)
            return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO_SHARDED "world must divide fri_lde_factor and cap_size, and "
                                                     "quotient_degree must not exceed fri_lde_factor", who);
        const unsigned cl = cfg->fri_lde_factor / W;
        if ((((size_t)1 << c->log_n) * cl) < cfg->cap_size / W)
            return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO_SHARDED "shard smaller than its cap fragment", who);
        const size_t Qe_rank = ((size_t)c->quotient_degree << c->log_n) / W;   // every rank evaluates q n / W points of the quotient
        if (Qe_rank < 2 || !bj::is_pow2(Qe_rank))                              // and inverse-transforms them: a power of two
            return bj::fail(ctx, BJ_ERR_INVALID_ARG, BJ_WHO_SHARDED "q n / world = %zu quotient points per rank (a power of two >= 2 is needed)", who, Qe_rank);
    }
    // every gate descriptor with the column ranges it will form, and the layout of the specialized columns (gate_list.h); the op
    // lists are canonicalised at their place in that order, and a malformed one is refused in the canonicaliser's own words
    std::string err;
    if (int rc = bj::resolve_gates(*c, lookup_cps, gates, &err, [ctx](const bj_gate_program *p) { return check_program(ctx, p); }))
        return err.empty() ? rc : bj::fail(ctx, rc, BJ_WHO "%s", who, err.c_str());
    return BJ_OK;
}
#undef BJ_WHO
#undef BJ_WHO_SHARDED

int bj::setup_create_impl(bj_ctx *ctx, const bj_circuit *c, const uint64_t *h_sigmas, const std::function<int(bj_setup *, u64 *)> &fill_sigmas,
                          const uint64_t *h_constants, const uint64_t *h_tables, const bj_proof_config *cfg, const bj_comm *comm,
                          bj_setup **out, bool lean) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_setup_create: null out pointer");
    *out = nullptr;
    if (!c || !cfg || (!h_sigmas && !fill_sigmas) || !h_constants) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_setup_create: null argument");
    bj::GateList gates;
    if (int rc = bj::circuit_check(ctx, "bj_setup_create", c, cfg, h_tables != nullptr, comm, &gates)) return rc;
    bj_setup *s = new bj_setup();
    static_cast<bj::CircuitShape &>(*s) = bj::circuit_shape(c, cfg);
    s->layout = bj::proof_layout(*s);
    s->device = ctx->device;
    bj::HasherGuard hasher_guard{ctx, ctx->hasher};
    ctx->hasher = cfg->tree_hasher ? (int)cfg->tree_hasher : BJ_HASHER_POSEIDON2;
    if (comm && comm->world > 1) {
        s->sh.rank = comm->rank;
        s->sh.world = comm->world;
        s->sh.comm = *comm;
    }
    s->gates = std::move(gates);
    auto upload = [ctx](std::vector<bj::DevProgram> &to, const bj_gate_desc *from, unsigned n) {
        to.resize(n);
        for (unsigned g = 0; g < n; g++)
            if (from[g].kind == BJ_GATE_PROGRAM)
                if (int prc = to[g].upload(ctx, from[g].program)) return prc;
        return (int)BJ_OK;
    };
    int prc = upload(s->programs, c->gates, c->num_gates);
    if (!prc) prc = upload(s->spec_programs, c->specialized_gates, c->num_specialized_gates);
    if (prc) {
        bj_setup_destroy(s);
        return prc;
    }
    s->non_residues.assign(c->non_residues, c->non_residues + c->num_vars);
    s->small_non_residues = true;
    for (u64 k : s->non_residues) s->small_non_residues = s->small_non_residues && gl::canon(k) < ((u64)1 << 32);
    for (unsigned i = 0; i < c->num_public_inputs; i++) {
        s->pub_cols.push_back(c->public_input_cols[i]);
        s->pub_rows.push_back(c->public_input_rows[i]);
    }
    s->fri_lde = cfg->fri_lde_factor; s->security = cfg->security_level; s->pow_bits = cfg->pow_bits;
    s->pow_runner = cfg->pow_runner ? cfg->pow_runner : BJ_POW_BLAKE2S256;
    s->transcript = cfg->transcript ? cfg->transcript : BJ_TRANSCRIPT_POSEIDON2;
    s->hasher = cfg->tree_hasher ? cfg->tree_hasher : BJ_HASHER_POSEIDON2;
    s->L = s->fri_lde > s->q ? s->fri_lde : s->q;   // used_lde_degree (prover.rs:313)
    s->log_L = bj::log2_exact(s->L); s->log_q = bj::log2_exact(s->q);
    const size_t n = (size_t)1 << s->log_n;
    const bj::ProofLayout &L = s->layout;
    const unsigned n_cols = L.widths[bj::ORACLE_SETUP], nT = n_cols - L.table(0);
    s->cl = s->L / s->sh.world;
    s->c0 = s->sh.rank * s->cl;
    s->Ls = (size_t)s->cl * n;
    s->Nl = n * s->fri_lde / s->sh.world;
    s->cap_l = s->cap_size / s->sh.world;
    int rc = BJ_OK;
    auto bail = [&](int code) {
        bj_setup_destroy(s);
        return code;
    };
    if (hipMalloc((void **)&s->d_nat, (size_t)n_cols * n * 8) != hipSuccess ||
        hipMalloc((void **)&s->d_lde, (size_t)n_cols * s->Ls * 8) != hipSuccess ||
        hipMalloc((void **)&s->d_non_res, s->V * 8) != hipSuccess)
        return bail(bj::fail(ctx, BJ_ERR_OOM, "bj_setup_create: device allocation failed"));
    // leaf order of the setup oracle: sigma || constants || tables (polynomial_storage.rs:667-676)
    rc = fill_sigmas ? fill_sigmas(s, s->d_nat) : bj_memcpy_h2d(ctx, s->d_nat, h_sigmas, (size_t)s->V * n * 8);
    if (!rc) rc = bj_memcpy_h2d(ctx, s->d_nat + (size_t)L.constant(0) * n, h_constants, (size_t)s->nC * n * 8);
    if (!rc && nT) rc = bj_memcpy_h2d(ctx, s->d_nat + (size_t)L.table(0) * n, h_tables, (size_t)nT * n * 8);
    if (!rc) rc = bj_memcpy_h2d(ctx, s->d_non_res, s->non_residues.data(), s->V * 8);
    if (rc) return bail(rc);
    {   // monomials (kept), LDE into d_lde
        if (hipMalloc((void **)&s->d_mono, (size_t)n_cols * n * 8) != hipSuccess)
            return bail(bj::fail(ctx, BJ_ERR_OOM, "bj_setup_create: device allocation failed"));
        s->tiled = bj::mono_tiled(s->log_n);
        rc = s->tiled ? bj::intt_to_tiled(ctx, s->d_nat, n, s->d_mono, n, s->log_n, n_cols)
                      : bj_intt_batch(ctx, s->d_nat, s->d_mono, s->log_n, n_cols, n, 1);
        if (!rc) rc = bj::lde_cosets_strided(ctx, s->d_mono, n, s->d_lde, s->Ls, s->log_n, n_cols, s->log_L, s->c0, s->cl, s->tiled);
        if (!rc) rc = bj_sync(ctx);
        if (rc) return bail(rc);
    }
    {   // the points the quotient is evaluated on here (prove_impl: Qe, I0) and 1 / (x - 1) on them, for the L_1 term
        const size_t Qe = (n * s->q) / s->sh.world;
        if (Qe) {
            if ((rc = bj::ensure_twiddles(ctx, s->log_n + s->log_L, false))) return bail(rc);
            if (hipMalloc((void **)&s->d_inv_xm1, Qe * 8) != hipSuccess)
                return bail(bj::fail(ctx, BJ_ERR_OOM, "bj_setup_create: device allocation failed"));
            bj::launch_inv_x_minus_one(ctx->tw_fwd.p, Qe, (size_t)s->c0 * n, s->d_inv_xm1, ctx->stream);
            if (hipGetLastError() != hipSuccess) return bail(bj::fail(ctx, BJ_ERR_HIP, "bj_setup_create: launch failed"));
        }
    }
    if (hipMalloc((void **)&s->d_tree, bj_merkle_tree_digests(s->Nl, s->cap_l) * 32) != hipSuccess)
        return bail(bj::fail(ctx, BJ_ERR_OOM, "bj_setup_create: tree allocation failed"));
    rc = bj_merkle_tree_build(ctx, s->d_lde, s->Ls, n_cols, s->Nl, s->cap_l, s->d_tree);
    s->cap.resize(4 * s->cap_size);
    if (!rc) rc = bj::gather_cap(ctx, s->sh, s->d_tree, s->Nl, s->cap_size, s->cap.data());
    if (rc) return bail(rc);
    if (lean && s->sh.world == 1) {   // the tree and the cap stand: from here on nothing but a proof wants the LDE, and a lean proof rebuilds what it reads
        if ((rc = bj_sync(ctx))) return bail(rc);
        (void)hipFree(s->d_lde);
        s->d_lde = nullptr;
        s->lean = true;
    }
    *out = s;
    return BJ_OK;
}

extern "C" {

int bj_setup_shape(const bj_setup *s, unsigned *log_n, unsigned *num_vars, unsigned *num_witness_cols, unsigned *num_public_inputs) {
    if (s && num_public_inputs) *num_public_inputs = (unsigned)s->pub_cols.size();
    if (!s) return BJ_ERR_INVALID_ARG;
    if (log_n) *log_n = s->log_n;
    if (num_vars) *num_vars = s->V;
    if (num_witness_cols) *num_witness_cols = s->Wc;
    return BJ_OK;
}

int bj_setup_cap(const bj_setup *s, uint64_t *h_cap) {
    if (!s || !h_cap) return BJ_ERR_INVALID_ARG;
    std::memcpy(h_cap, s->cap.data(), s->cap.size() * 8);
    return BJ_OK;
}

int bj_setup_device_bytes(const bj_setup *s, size_t *bytes) {
    if (!s || !bytes) return BJ_ERR_INVALID_ARG;
    const size_t n = (size_t)1 << s->log_n;
    const unsigned n_cols = s->layout.widths[bj::ORACLE_SETUP];
    size_t b = 0;
    if (s->d_nat) b += (size_t)n_cols * n * 8;
    if (s->d_mono) b += (size_t)n_cols * n * 8;
    if (s->d_lde) b += (size_t)n_cols * s->Ls * 8;
    if (s->d_tree) b += bj_merkle_tree_digests(s->Nl, s->cap_l) * 32;
    if (s->d_non_res) b += (size_t)s->V * 8;
    if (s->d_inv_xm1) b += (n * s->q) / s->sh.world * 8;
    if (s->d_placement) b += (size_t)s->V * n * 4;
    if (s->d_wit_placement) b += (size_t)s->Wc * n * 4;
    *bytes = b;
    return BJ_OK;
}

}  // extern "C"
