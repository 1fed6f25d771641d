// Internal: the context object behind the opaque `bj_ctx` of include/boojum_hip.h, shared by the C-ABI translation
// units (abi.hip, fri_prover.hip, ...).  Its memory, the workspace of the proof in flight, the probes and the environment
// switches are defined in ctx.hip.
#pragma once
#include "../../include/boojum_hip.h"
#include "arena_bump.h"
#include "async_admission.h"
#include "gl.h"
#include "kernels.h"

#include <hip/hip_runtime.h>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#define BJ_MAX_KERNEL_PROBES 12

namespace bj {
struct Pipeline;        // prove_async.hip: the two lanes of bj_prove_async
// A grow-only device allocation of a context: the six parts a proof is admitted by (async_admission.h) are one each.
struct DevBuf {
    gl::u64 *p = nullptr;
    size_t words = 0;
    size_t bytes() const { return words * sizeof(gl::u64); }
    // at least `need` words: nothing if it is that large already, else the context's stream is drained and the block is freed and
    // allocated again (the contents are lost; *grew says so).  BJ_ERR_OOM / BJ_ERR_HIP with the buffer left empty.
    int ensure(bj_ctx *ctx, size_t need, bool *grew = nullptr);
    hipError_t drop();   // frees and zeroes; the caller has drained whatever may still use the block
};
// The words of the context's small block (bj_ctx::d_small).  Nothing reads or writes SHIFTS any more, but for its first word,
// which is the flag of the witness gather (VALUES_BAD); the offsets behind it stay where they have always been.
struct SmallBlock {
    static constexpr size_t SHIFTS = 0;                            // 64 words
    static constexpr size_t VALUES_BAD = SHIFTS;                   // witness_gather_kernel: a cell named a value beyond all_values
    static constexpr size_t ROUND_SCALES = 64;                     // 64 cosets x 32 rounds (launch_round_scales)
    static constexpr size_t GATHER = ROUND_SCALES + 64 * 32;       // what a collective gathers before it goes to the host
    static constexpr size_t GATHER_WORDS = 4096;                   // evaluate_at sends from the first half into the second
    static constexpr size_t GATHER_HALF = GATHER + GATHER_WORDS / 2;
    static constexpr size_t FRONT_TABLE = GATHER + GATHER_WORDS;   // BJ_FRONT_TABLE_WORDS (kernels.h)
    static constexpr size_t WORDS = FRONT_TABLE + BJ_FRONT_TABLE_WORDS;
};
constexpr size_t RING_BYTES = (size_t)1 << 20, RING_MAX_BLOCK = (size_t)128 << 10;   // the pinned ring, and the largest block that goes through it
}

struct bj_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // twiddle caches (bit-reversed tables; a table for 2^k holds 2^(k-1) words and serves every smaller size as a prefix)
    bj::DevBuf tw_fwd, tw_inv;
    bj::DevBuf tw_inv_scaled22;   // tw_inv[j] / 2^22, j < 2^21: the last round of a 2^22-point inverse transform into the tiled layout
    gl::u64 *d_small = nullptr;   // bj::SmallBlock
    bj::DevBuf d_ptrs;            // the column pointers of bj_merkle_tree_build_ptrs
    bj::DevBuf d_scratch;         // big scratch for out-of-place steps
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> events;   // every event ensure_event has created on this context, destroyed with it
    // bump-allocated workspace reused across proofs (hipMalloc/hipFree of multi-GB buffers per proof is slow and
    // synchronising); grown on demand, reset at the start of every bj_prove_dev
    bj::DevBuf arena;
    // A proof whose buffers outgrow the reservation does not fail: further blocks come out of overflow slabs (hipMalloc in the
    // middle of a proof — slow, once), the proof reports its high-water mark (bj_proof_workspace_bytes) and the next reservation
    // on this context is at least that large.  The reservation is the total of the proof's plan and every buffer is taken from
    // that plan, so only an allowance that was no upper bound can lead here; the suite asserts that no proof needed a slab.
    bj::ArenaBump bump;                  // where the next block goes (arena_bump.h)
    std::vector<gl::u64 *> slab_base;    // the device blocks of bump.slabs
    size_t arena_learned = 0;            // largest high-water mark seen on this context
    int hasher = BJ_HASHER_POSEIDON2;   // tree hasher of the bj_merkle_tree_* calls (bj_ctx_set_tree_hasher / bj_prove)
    bool in_proof = false;       // bj_prove_dev is running: temporaries come out of the arena instead of hipMalloc
    const bj::WorkspacePlan *ws_plan = nullptr;   // of the proof in flight (it owns the plan), and the entry TmpBuf::take expects next
    size_t ws_next = 0;
    // pinned staging ring for the small host->device blocks between kernels (challenges, pointer tables, query indices):
    // a copy out of pageable memory costs a blocking staging pass plus a stream synchronisation, ~35 us of idle GPU each
    unsigned char *h_ring = nullptr;
    size_t ring_off = 0, ring_inflight = 0;
    // bj_prove (host witness): device staging of the witness columns, kept across proofs, and a copy stream with one event
    // per column group so that the PCIe transfer of group k+1 runs under the iNTT / LDE of group k
    bj::DevBuf wit_stage;
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_ev[64] = {};
    // collectives of the sharded proof in flight: an event pair around each (created on first use, reused), summed into
    // bj_proof_comm_stats when the proof has drained — what a scaling run needs to tell waiting-for-peers from computing
    hipEvent_t comm_ev[48][2] = {};
    unsigned comm_n = 0;          // pairs recorded by the proof in flight
    size_t comm_bytes = 0;        // bytes received by this rank in them
    float comm_host_ms = 0;       // synchronous host-callback transport: wall time inside the callbacks
    // per-kernel probes of the proof in flight (bj_proof_kernel_stats): an event pair on the launch stream around the first
    // launch of each named kernel, with the algorithmic bytes of that launch — no synchronisation added
    struct KernelProbe {
        const char *name = nullptr;
        double bytes = 0;
        hipEvent_t ev[2] = {nullptr, nullptr};
        bool closed = false;      // the closing event was recorded in THIS proof (an unclosed probe still holds the previous proof's)
    } probes[BJ_MAX_KERNEL_PROBES];
    unsigned probe_n = 0;
    bj::Pipeline *pipe = nullptr;   // bj_prove_async: created on first use, destroyed with the context
    // a lane of bj_prove_async sets it for one proof that was admitted with a lean workspace (async_admission.h); wins over
    // BJ_PROOF_LEAN.  -1: the environment decides; 1: the witness and stage-2 oracles keep no evaluations
    int lean_override = -1;
    // bj_verify and bj_verify_batch keep one each, for bj_verify_kernel_ms and bj_verify_batch_ms: of the last call, events
    // (created on first use) before / after its uploads and after each of its two kernels, and the wall time of its host phase
    struct VerifyTiming {
        hipEvent_t ev[4] = {};
        int state = 0;        // the last call: 0 none (or refused, or bj_verify ended on the host), 1 the batch ended in its host phase, 2 launched its kernels
        float host_ms = 0;    // bj_verify_batch only
    } verify_timing, verify_batch_timing;
};

namespace bj {
// first launch of `name` inside a proof: records the opening event and returns the probe's index (-1: not in a proof, name
// already probed in this proof, or table full — the caller just launches); probe_end records the closing event
int probe_begin(bj_ctx *ctx, const char *name, double algorithmic_bytes);
void probe_end(bj_ctx *ctx, int idx);
int fail(bj_ctx *ctx, int code, const char *fmt, ...);   // ctx == nullptr (host-only calls): the message goes to the calling thread's slot
// setup.hip: what bj_setup_create refuses about a circuit description and a proof config (no device work); `who` starts the messages
// *gates: the resolved gate list (gate_list.h)
struct GateList;
int circuit_check(bj_ctx *ctx, const char *who, const bj_circuit *c, const bj_proof_config *cfg, bool has_tables, const bj_comm *comm,
                  GateList *gates);
int bind(bj_ctx *ctx);
// host block -> device, ordered on ctx->stream like a kernel launch; returns without waiting (h_src may be reused at once)
int h2d_async(bj_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int ensure_twiddles(bj_ctx *ctx, unsigned log_n, bool inverse);
inline unsigned twiddles_log(const bj_ctx *ctx, bool inverse) {   // the table serves up to 2^this points (0: none yet)
    const DevBuf &t = inverse ? ctx->tw_inv : ctx->tw_fwd;
    return t.p ? twiddle_log(t.bytes()) : 0;
}
inline int ensure_scratch(bj_ctx *ctx, size_t elems) { return ctx->d_scratch.ensure(ctx, elems); }
inline gl::u64 *round_scales(bj_ctx *ctx) { return ctx->d_small + SmallBlock::ROUND_SCALES; }
inline gl::u64 *gather_area(bj_ctx *ctx) { return ctx->d_small + SmallBlock::GATHER; }
inline gl::u64 *gather_half(bj_ctx *ctx) { return ctx->d_small + SmallBlock::GATHER_HALF; }
inline gl::u64 *front_table(bj_ctx *ctx) { return ctx->d_small + SmallBlock::FRONT_TABLE; }
inline unsigned *values_bad_flag(bj_ctx *ctx) { return reinterpret_cast<unsigned *>(ctx->d_small + SmallBlock::VALUES_BAD); }
int ensure_ring(bj_ctx *ctx);                                                          // the pinned ring exists
int ensure_event(bj_ctx *ctx, hipEvent_t &e, unsigned flags = hipEventDefault);   // e exists (created once, with `flags`)
std::string &thread_error();   // message of the last failed call that has no context, per host thread
// The one enumeration of what a context holds for proofs: the buffer behind each LanePart (async_admission.h says which of them
// bj_ctx_release_workspace gives back).  The arena's part includes its overflow slabs.
DevBuf &ctx_part(bj_ctx *ctx, unsigned part);
void ctx_drop_all(bj_ctx *ctx);      // bj_ctx_destroy: every part, kept or not, and the events
unsigned setup_world(const bj_setup *s);         // ranks of the proof a setup belongs to (1: single device)
// mode 1: whole witness first, then as on a resident witness; mode 2: groups transferred and transformed as they land, hashed once
int prove_host_copy_first(bj_ctx *ctx, const bj_setup *S, const uint64_t *h_variables, const uint64_t *h_multiplicities,
                          const uint64_t *h_public_values, bj_proof **out, int mode);
void pipeline_destroy(bj_ctx *ctx);              // waits for the asynchronous proofs in flight, ends the lanes
int pipeline_release_workspace(bj_ctx *ctx);    // bj_ctx_release_workspace on every idle lane
// Admission of bj_prove_async (async_admission.h).  ctx_held: what the context holds now.  ctx_reserve: grows every part that is
// smaller than `want` (free and allocate; the tables are filled on the context's stream), so that a proof of that footprint
// allocates nothing; the context must be idle.  ctx_release_own_workspace: bj_ctx_release_workspace without the lanes.
// async_footprints (prover.hip): what a lane wants for a bj_prove of `setup`, its oracles resident and lean.
void ctx_held(const bj_ctx *ctx, LaneBytes *out);
int ctx_reserve(bj_ctx *ctx, const LaneBytes &want);
int ctx_release_own_workspace(bj_ctx *ctx);
int async_footprints(bj_ctx *ctx, const bj_setup *setup, LaneBytes *resident, LaneBytes *lean, bool values = false, size_t n_values = 0);
// prover.hip, bj_prove_values[_async]: the refusals both share (before anything is queued), and the proof itself on a context
// that passed them (no_absorb: a lane whose sibling is proving hashes the leaves once at the end)
int values_check(bj_ctx *ctx, const char *who, const bj_setup *S, const uint64_t *h_values, size_t n_values, const uint32_t *h_multiplicities,
                 size_t n_multiplicities);
int prove_values_staged(bj_ctx *ctx, const bj_setup *S, const uint64_t *h_values, size_t n_values, const uint32_t *h_multiplicities,
                        size_t n_multiplicities, bj_proof **out, bool no_absorb);
inline int stage_witness_elems(bj_ctx *ctx, size_t need) { return ctx->wit_stage.ensure(ctx, need); }   // kept for the next proof
int ensure_scaled22(bj_ctx *ctx);                    // tw_inv_scaled22 exists (tw_inv must reach 2^22)
int arena_reset(bj_ctx *ctx, size_t need_elems);     // a new proof: nothing taken, no slabs, at least need_elems words
gl::u64 *arena_alloc(bj_ctx *ctx, size_t elems);   // nullptr if the reservation was too small
// A block of device memory for the scope that holds it: out of the arena inside a proof (no hipMalloc / hipFree, no implicit
// synchronisation; the arena is a bump allocator and gives nothing back before the next proof), hipMalloc'ed and freed otherwise.
struct TmpBuf {
    gl::u64 *p = nullptr;
    bool from_arena = false;
    bool drain = false;          // a hipMalloc'ed block is freed after the stream has drained (the stand-alone operators)
    bj_ctx *ctx = nullptr;
    TmpBuf() = default;
    explicit TmpBuf(bool drain_before_free) : drain(drain_before_free) {}
    TmpBuf(const TmpBuf &) = delete;
    TmpBuf &operator=(const TmpBuf &) = delete;
    ~TmpBuf();
    int alloc(bj_ctx *c, size_t words);   // a temporary of the callee's own: inside a proof, covered by an allowance of the plan
    // a named buffer of the proof in flight: `id` (a WsId) must be the next exact entry of its plan and `words`, unless 0, that
    // entry's size — anything else is an internal error and nothing is allocated.  No proof in flight: alloc(words)
    int take(bj_ctx *c, unsigned id, size_t words = 0);
    gl::u64 *release() {   // the caller keeps the block (bj_fri lists its hipMalloc'ed ones)
        gl::u64 *q = p;
        p = nullptr;
        return q;
    }
};
int workspace_all_taken(bj_ctx *ctx);   // the proof in flight has taken every exact entry of its plan, or an internal error
int lde_cosets_strided(bj_ctx *ctx, const gl::u64 *d_mono, size_t in_col_stride, gl::u64 *d_out, size_t out_col_stride,
                       unsigned log_n, unsigned n_cols, unsigned log_lde, unsigned coset_begin, unsigned coset_count,
                       bool tiled_in = false);
bool mono_tiled(unsigned log_n);   // the monomial layout of bj_prove for this trace length (abi.hip)
int intt_to_tiled(bj_ctx *ctx, const gl::u64 *d_in, size_t in_col_stride, gl::u64 *d_out, size_t out_col_stride, unsigned log_n,
                  unsigned n_cols);
// setup_placement.hip: sigma from the variable placement.  The workspace lives in the context's scratch (valid until the next
// ensure_scratch): u32 key / cell-number double buffers of the sort, its temporary storage, the non-residues, a flag word and
// `staging_elems` words for the caller's uploads.  keys[0] takes the placement as u32 (PLACEMENT_NONE = placeholder).
constexpr uint32_t PLACEMENT_NONE = 0xFFFFFFFFu;
struct PlacementWorkspace {
    size_t cells = 0, sort_bytes = 0;
    uint32_t *keys[2] = {}, *vals[2] = {};
    gl::u64 *sort_tmp = nullptr, *non_res = nullptr, *staging = nullptr;
    unsigned *bad = nullptr;
};
int placement_workspace(bj_ctx *ctx, unsigned num_vars, unsigned log_n, size_t staging_elems, PlacementWorkspace *w);
// copy-hint cells [cols][n] (bit 63 = placeholder, low 48 bits = index) -> u32; an index above 2^32 - 2 raises the flag word
int placement_narrow(bj_ctx *ctx, const PlacementWorkspace &w, const gl::u64 *d_hint, size_t in_stride, unsigned cols, unsigned log_n,
                     uint32_t *d_out);
int placement_check(bj_ctx *ctx, const PlacementWorkspace &w);   // synchronises; BJ_ERR_UNSUPPORTED if the flag was raised
int sigmas_from_keys(bj_ctx *ctx, const PlacementWorkspace &w, unsigned num_vars, unsigned log_n, const gl::u64 *h_non_residues,
                     gl::u64 *d_sigmas, size_t sig_stride);      // sorts keys[0] (destroyed) and scatters
// openings_abi.hip: the DEEP stage on column lists (opening_args.h); one argument block of L.words() words per call
int combine_monomials(bj_ctx *ctx, const ColumnList &L, size_t n, uint64_t *d_out0, uint64_t *d_out1);
int deep_accumulate_multi(bj_ctx *ctx, const ColumnList &L, unsigned log_n, unsigned log_lde, size_t N_local, size_t I0,
                          uint64_t *d_dst_c0, uint64_t *d_dst_c1, int accumulate);
// setup.hip: bj_setup_create[_sharded] with the sigma columns either from the host or written on the device by `fill_sigmas`
// ([num_vars][n] at d_sigmas, called once the setup's buffers exist); a placement handed over is freed with the setup
int setup_create_impl(bj_ctx *ctx, const bj_circuit *c, const uint64_t *h_sigmas, const std::function<int(bj_setup *, gl::u64 *)> &fill_sigmas,
                      const uint64_t *h_constants, const uint64_t *h_tables, const bj_proof_config *cfg, const bj_comm *comm, bj_setup **out,
                      bool lean = false);   // lean: drop the LDE once the tree stands (single device only; the callers pass env().setup_lean)
void setup_adopt_placement(bj_setup *s, uint32_t *d_placement);   // [num_vars][n] u32, hipMalloc'ed
const uint32_t *setup_placement(const bj_setup *s);               // nullptr unless created from a placement
void setup_adopt_witness_placement(bj_setup *s, uint32_t *d_placement);   // [num_witness_cols][n] u32, hipMalloc'ed; replaces one held
int setup_read_public_placement(bj_ctx *ctx, bj_setup *s);       // fills bj_setup::pub_place from the placements the setup holds
// lookup_multiplicities.hip: the multiplicity column [n] counted from raw columns (the arguments of bj_lookup_multiplicities) or
// from a setup's replicated natural-order columns and the variables.  In the context's scratch, on its stream; synchronises.
// A looked-up tuple that is in no table row: BJ_ERR_INVALID_ARG, the message starts with `who` and names the first such lookup.
int lookup_multiplicities(bj_ctx *ctx, const char *who, const gl::u64 *d_lvars, size_t var_stride, const gl::u64 *d_table_id,
                          const gl::u64 *d_tables, size_t table_stride, unsigned reps, unsigned width, unsigned log_n, gl::u64 *d_out);
int setup_lookup_multiplicities(bj_ctx *ctx, const char *who, const bj_setup *S, const gl::u64 *d_variables, gl::u64 *d_out);
// dumps.hip: WitnessVec + copy-hint dumps -> [num_vars + num_witness_cols][n] cells, [n] multiplicities (device) and the public
// input values (host), handed to `use` and freed when it returns; variables_hint may be NULL for a setup that holds its placement
int witness_from_dumps(bj_ctx *ctx, const char *who, const bj_setup *setup, const void *witness_vec, size_t witness_vec_len,
                       const void *variables_hint, size_t variables_hint_len, const void *witness_hint, size_t witness_hint_len,
                       const std::function<int(const uint64_t *d_cells, const uint64_t *d_mult, const uint64_t *h_public)> &use);
inline bool is_pow2(size_t x) { return x && !(x & (x - 1)); }
inline unsigned log2_exact(size_t x) {
    unsigned r = 0;
    while (((size_t)1 << r) < x) r++;
    return r;
}
}  // namespace bj

#define BJ_HIP(ctx, call)                                                                                       \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess)                                                                                   \
            return bj::fail(ctx, e_ == hipErrorOutOfMemory ? BJ_ERR_OOM : BJ_ERR_HIP, "%s failed: %s", #call,   \
                            hipGetErrorString(e_));                                                             \
    } while (0)

#define BJ_CHECK_LAUNCH(ctx)                                                                                    \
    do {                                                                                                        \
        hipError_t e_ = hipGetLastError();                                                                      \
        if (e_ != hipSuccess)                                                                                   \
            return bj::fail(ctx, BJ_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e_));                \
    } while (0)
