// The internals of a context (ctx.h): what it holds on the device and how that grows and goes away, the workspace of the proof
// in flight, the pinned ring, the lazily created events, the kernel probes and the environment switches.  The entry points that
// use them are in abi.hip and its neighbours.
#include "ctx.h"
#include "workspace_plan.h"

#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using gl::u64;

namespace bj {

std::string &thread_error() {   // bj_last_error(NULL) reads it
    static thread_local std::string e;
    return e;
}

int fail(bj_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else thread_error() = buf;
    return code;
}

int bind(bj_ctx *ctx) {
    if (!ctx) return BJ_ERR_INVALID_ARG;
    BJ_HIP(ctx, hipSetDevice(ctx->device));
    return BJ_OK;
}

int DevBuf::ensure(bj_ctx *ctx, size_t need, bool *grew) {
    if (need <= words) return BJ_OK;
    if (p) {
        BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        BJ_HIP(ctx, drop());
    }
    BJ_HIP(ctx, hipMalloc((void **)&p, need * sizeof(u64)));
    words = need;
    if (grew) *grew = true;
    return BJ_OK;
}
hipError_t DevBuf::drop() {
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr;
    words = 0;
    return e;
}

int ensure_twiddles(bj_ctx *ctx, unsigned log_n, bool inverse) {
    DevBuf &tab = inverse ? ctx->tw_inv : ctx->tw_fwd;
    if (log_n == 0) log_n = 1;
    bool grew = false;
    if (int rc = tab.ensure(ctx, twiddle_bytes(log_n) / sizeof(u64), &grew)) return rc;
    if (!grew) return BJ_OK;
    bj::launch_twiddles(tab.p, log_n, inverse, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

int ensure_scaled22(bj_ctx *ctx) {   // a table for 2^22 is a prefix of every larger one: built once per context, whatever tw_inv grows to
    if (ctx->tw_inv_scaled22.p) return BJ_OK;
    const size_t n = (size_t)1 << 22;
    if (ctx->tw_inv.words < n / 2) return fail(ctx, BJ_ERR_HIP, "internal error: the scaled twiddle table before the inverse twiddles of 2^22");
    if (int rc = ctx->tw_inv_scaled22.ensure(ctx, n / 2)) return rc;
    bj::launch_scale_table(ctx->tw_inv.p, ctx->tw_inv_scaled22.p, n / 2, gl::inv(gl::canon((u64)n % gl::P)), ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

static int arena_drop_slabs(bj_ctx *ctx) {
    if (ctx->slab_base.empty()) return BJ_OK;
    BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (u64 *p : ctx->slab_base) (void)hipFree(p);
    ctx->slab_base.clear();
    ctx->bump.drop_slabs();
    return BJ_OK;
}
int arena_reset(bj_ctx *ctx, size_t need_elems) {
    ctx->bump.reset();
    if (int rc = arena_drop_slabs(ctx)) return rc;
    const int rc = ctx->arena.ensure(ctx, need_elems);
    ctx->bump.arena_words = ctx->arena.words;
    return rc;
}

u64 *arena_alloc(bj_ctx *ctx, size_t elems) {
    ArenaBump &b = ctx->bump;
    const size_t slab_off = b.slab_off, high_water = b.high_water;
    const ArenaBump::Place at = b.place(elems, ctx->in_proof);
    if (at.where == ArenaBump::ARENA) return ctx->arena.p + at.offset;
    if (at.where == ArenaBump::LAST_SLAB) return ctx->slab_base.back() + at.offset;
    if (at.where == ArenaBump::NOTHING) return nullptr;
    u64 *p = nullptr;   // the reservation was too small: an overflow slab
    if (hipMalloc((void **)&p, at.slab_words * sizeof(u64)) != hipSuccess) {
        b.slabs.pop_back();   // as if it had not been asked
        b.slab_off = slab_off, b.high_water = high_water;
        return nullptr;
    }
    ctx->slab_base.push_back(p);
    return p;
}

DevBuf &ctx_part(bj_ctx *ctx, unsigned part) {
    switch (part) {
        case LANE_STAGING: return ctx->wit_stage;
        case LANE_SCRATCH: return ctx->d_scratch;
        case LANE_TW_FWD: return ctx->tw_fwd;
        case LANE_TW_INV: return ctx->tw_inv;
        case LANE_TW_SCALED22: return ctx->tw_inv_scaled22;
        default: return ctx->arena;   // LANE_ARENA
    }
}
static size_t ctx_part_bytes(const bj_ctx *ctx, unsigned part) {
    return ctx_part(const_cast<bj_ctx *>(ctx), part).bytes() + (part == LANE_ARENA ? ctx->bump.slab_words() * sizeof(u64) : 0);
}

void ctx_held(const bj_ctx *ctx, LaneBytes *out) {
    for (unsigned part = 0; part < LANE_N_PARTS; part++) out->part[part] = ctx_part_bytes(ctx, part);
}

int ctx_reserve(bj_ctx *ctx, const LaneBytes &want) {
    if (int rc = bind(ctx)) return rc;
    if (ctx->in_proof) return fail(ctx, BJ_ERR_INVALID_ARG, "internal error: a workspace reserved under a running proof");
    for (unsigned part = 0; part < LANE_N_PARTS; part++) {
        const size_t bytes = want.part[part], words = bytes / sizeof(u64);
        int rc = BJ_OK;
        if (part == LANE_ARENA)
            rc = arena_reset(ctx, words > ctx->arena_learned ? words : ctx->arena_learned);
        else if (part == LANE_TW_FWD || part == LANE_TW_INV)
            rc = bytes ? ensure_twiddles(ctx, twiddle_log(bytes), part == LANE_TW_INV) : BJ_OK;   // a table is filled as it grows
        else if (part == LANE_TW_SCALED22)
            rc = bytes ? ensure_scaled22(ctx) : BJ_OK;
        else
            rc = ctx_part(ctx, part).ensure(ctx, words);
        if (rc) return rc;
    }
    // the small blocks a proof would otherwise create on first use: the pinned ring of the host -> device blocks, the copy stream
    if (int rc = ensure_ring(ctx)) return rc;
    if (!ctx->copy_stream) BJ_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    return BJ_OK;
}

int ctx_release_own_workspace(bj_ctx *ctx) {
    BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->copy_stream) BJ_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    if (int rc = arena_drop_slabs(ctx)) return rc;
    for (unsigned part = 0; part < LANE_N_PARTS; part++)
        if (LANE_RELEASED[part]) BJ_HIP(ctx, ctx_part(ctx, part).drop());
    ctx->bump = ArenaBump();
    ctx->arena_learned = 0;
    return BJ_OK;
}

void ctx_drop_all(bj_ctx *ctx) {
    (void)arena_drop_slabs(ctx);
    for (unsigned part = 0; part < LANE_N_PARTS; part++) (void)ctx_part(ctx, part).drop();
    (void)ctx->d_ptrs.drop();
    for (hipEvent_t e : ctx->events) (void)hipEventDestroy(e);
    ctx->events.clear();
}

int ensure_ring(bj_ctx *ctx) {
    if (!ctx->h_ring) BJ_HIP(ctx, hipHostMalloc((void **)&ctx->h_ring, RING_BYTES, hipHostMallocDefault));
    return BJ_OK;
}

int ensure_event(bj_ctx *ctx, hipEvent_t &e, unsigned flags) {
    if (e) return BJ_OK;
    BJ_HIP(ctx, hipEventCreateWithFlags(&e, flags));
    ctx->events.push_back(e);
    return BJ_OK;
}

int TmpBuf::alloc(bj_ctx *c, size_t words) {
    ctx = c;
    from_arena = false;
    if (c->in_proof && (p = arena_alloc(c, words))) {
        from_arena = true;
        return BJ_OK;
    }
    if (hipMalloc((void **)&p, words ? words * 8 : 8) != hipSuccess) {
        p = nullptr;
        return fail(c, BJ_ERR_OOM, "out of device memory (%zu MiB)", words * 8 >> 20);
    }
    return BJ_OK;
}
int TmpBuf::take(bj_ctx *c, unsigned id, size_t words) {
    const WorkspacePlan *plan = c->ws_plan;
    if (!plan) return alloc(c, words);
    while (c->ws_next < plan->entries.size() && !plan->entries[c->ws_next].exact) c->ws_next++;
    if (c->ws_next == plan->entries.size())
        return fail(c, BJ_ERR_HIP, "bj_prove: internal error: the workspace plan ends before %s", ws_name(id));
    const WorkspaceEntry &e = plan->entries[c->ws_next];
    if (e.id != id) return fail(c, BJ_ERR_HIP, "bj_prove: internal error: the workspace plan holds %s where the proof takes %s", ws_name(e.id), ws_name(id));
    if (words && words != e.words)
        return fail(c, BJ_ERR_HIP, "bj_prove: internal error: %s is planned with %zu words and taken with %zu", ws_name(id), e.words, words);
    c->ws_next++;
    ctx = c;
    if (!(p = arena_alloc(c, e.words))) return fail(c, BJ_ERR_OOM, "workspace reservation too small for %zu MiB", e.words * 8 >> 20);
    from_arena = true;   // never freed: a planned buffer may outlive the scope that took it
    return BJ_OK;
}
TmpBuf::~TmpBuf() {
    if (!p || from_arena) return;
    if (drain) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(p);
}
int workspace_all_taken(bj_ctx *ctx) {
    const WorkspacePlan *plan = ctx->ws_plan;
    for (size_t i = ctx->ws_next; plan && i < plan->entries.size(); i++)
        if (plan->entries[i].exact)
            return fail(ctx, BJ_ERR_HIP, "bj_prove: internal error: the proof ends without taking %s of its workspace plan", ws_name(plan->entries[i].id));
    return BJ_OK;
}

int h2d_async(bj_ctx *ctx, void *d_dst, const void *h_src, size_t bytes) {
    if (int rc = bind(ctx)) return rc;
    if (!bytes) return BJ_OK;
    if (!d_dst || !h_src) return fail(ctx, BJ_ERR_INVALID_ARG, "h2d_async: null pointer");
    if (bytes > RING_MAX_BLOCK) return bj_memcpy_h2d(ctx, d_dst, h_src, bytes);
    if (int rc = ensure_ring(ctx)) return rc;
    const size_t slot = (bytes + 63) & ~(size_t)63;
    if (ctx->ring_off + slot > RING_BYTES) {   // wrap: the skipped tail counts as in flight, or a reset at a mid-ring offset
        ctx->ring_inflight += RING_BYTES - ctx->ring_off;   // would let the next lap overwrite copies still queued
        ctx->ring_off = 0;
    }
    if (ctx->ring_inflight + slot > RING_BYTES) {   // the ring wrapped onto copies that may not have run yet
        BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->ring_inflight = 0;
    }
    std::memcpy(ctx->h_ring + ctx->ring_off, h_src, bytes);
    BJ_HIP(ctx, hipMemcpyAsync(d_dst, ctx->h_ring + ctx->ring_off, bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->ring_off += slot;
    ctx->ring_inflight += slot;
    return BJ_OK;
}

int probe_begin(bj_ctx *ctx, const char *name, double algorithmic_bytes) {
    if (!ctx->in_proof || ctx->probe_n >= BJ_MAX_KERNEL_PROBES) return -1;
    for (unsigned i = 0; i < ctx->probe_n; i++)
        if (!strcmp(ctx->probes[i].name, name)) return -1;
    auto &p = ctx->probes[ctx->probe_n];
    if (ensure_event(ctx, p.ev[0]) || ensure_event(ctx, p.ev[1])) return -1;
    p.name = name;
    p.bytes = algorithmic_bytes;
    p.closed = false;
    if (hipEventRecord(p.ev[0], ctx->stream) != hipSuccess) return -1;
    return (int)ctx->probe_n++;
}
void probe_end(bj_ctx *ctx, int idx) {
    if (idx >= 0) ctx->probes[idx].closed = hipEventRecord(ctx->probes[idx].ev[1], ctx->stream) == hipSuccess;
}

namespace {
EnvConfig g_env;
std::once_flag g_env_once;
void load_env() {
    EnvConfig e;
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    auto str = [](const char *name) { const char *v = getenv(name); return std::string(v ? v : ""); };
    e.ntt_two_pass = str("BJ_NTT_TWO_PASS").rfind("0", 0) != 0;
    e.mono_tiled = str("BJ_MONO_TILED").rfind("0", 0) != 0;
    if (set("BJ_ASYNC_MODE")) e.async_mode = atoi(getenv("BJ_ASYNC_MODE"));
    e.async_stagger = str("BJ_ASYNC_STAGGER").rfind("0", 0) != 0;
    e.async_debug = set("BJ_ASYNC_DEBUG");
    if (set("BJ_HBM_BUDGET_BYTES")) e.hbm_budget_bytes = (size_t)strtoull(getenv("BJ_HBM_BUDGET_BYTES"), nullptr, 10);
    e.peer_debug = set("BJ_PEER_DEBUG");
    if (set("BJ_PEER_TEST_FAIL_RANK")) e.peer_test_fail_rank = atoi(getenv("BJ_PEER_TEST_FAIL_RANK"));
    e.gate_no_aot = set("BJ_GATE_NO_AOT");
    e.gate_no_fuse = set("BJ_GATE_NO_FUSE");
    e.gate_no_jit = set("BJ_GATE_NO_JIT");
    e.gates_windowed = str("BJ_GATES_WINDOWED").rfind("0", 0) != 0;
    e.prove_no_absorb = set("BJ_PROVE_NO_ABSORB");
    e.setup_lean = set("BJ_SETUP_LEAN") && str("BJ_SETUP_LEAN").rfind("0", 0) != 0;
    e.proof_lean = set("BJ_PROOF_LEAN") && str("BJ_PROOF_LEAN").rfind("0", 0) != 0;
    e.prove_uniform_groups = set("BJ_PROVE_UNIFORM_GROUPS");
    e.copy_perm_wide_k = set("BJ_COPY_PERM_WIDE_K");
    if (set("BJ_PROVE_H2D_GROUP")) {
        const unsigned v = (unsigned)strtoul(getenv("BJ_PROVE_H2D_GROUP"), nullptr, 10);
        e.prove_h2d_group = v ? v : 8u;
    }
    if (set("BJ_NODES_LANEPAR_MAX")) e.nodes_lanepar_max = (size_t)strtoull(getenv("BJ_NODES_LANEPAR_MAX"), nullptr, 10);
    if (set("BJ_VERIFY_THREADS")) {
        const long v = strtol(getenv("BJ_VERIFY_THREADS"), nullptr, 10);
        e.verify_threads = v < 1 ? 1u : v > 16 ? 16u : (unsigned)v;
    }
    e.jit_cache_dir = str("BJ_GATE_JIT_CACHE");
    e.rccl_lib = str("BJ_RCCL_LIB");
    g_env = e;
}
}  // namespace
const EnvConfig &env() {
    std::call_once(g_env_once, load_env);
    return g_env;
}
void env_reload() {
    (void)env();
    load_env();
}
}  // namespace bj
