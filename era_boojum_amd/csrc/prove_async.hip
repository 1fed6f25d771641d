// bj_prove_async / bj_proof_wait: two proofs in flight on ONE device from ONE host thread (include/boojum_hip.h).
//
// The call site replaced is a host loop over witnesses around prove_cpu_basic (src/cs/implementations/prover.rs:153-168,
// convenience.rs:119-196).  A proof ends in a latency-bound tail — ~100 lane-parallel node layers, the FRI tail oracles, ~15
// transcript round trips between host and device — during which most of the chip idles, and it starts with a PCIe transfer
// during which the CUs only transform the columns that have landed.  Neither can be filled from inside the proof (the transcript
// serialises it); the next proof's head can fill both.  A context therefore owns two LANES: each a private sub-context (its own
// non-blocking HIP stream, copy stream, workspace arena, witness staging, twiddle tables, staging ring) driven by its own worker
// thread.  bj_prove_async hands the witness to the next lane in turn and returns; the worker runs the ordinary bj_prove on the
// lane's sub-context.  Nothing is shared between the lanes but the (read-only) setup, so every proof is the bytes bj_prove gives.
// At most two proofs are in flight: a third submission waits for the lane it is due on.
//
// Memory.  A lane is a full context, so two of them beside the parent's own workspace are three proofs' worth of HBM.  Every
// submission is therefore ADMITTED first (async_admission.h), on the submitting thread: the device's free bytes, capped by
// BJ_HBM_BUDGET_BYTES, against what the proof's lane wants (the workspace plan of the proof, the witness staging, scratch and
// tables).  First rung that fits: the lane it is due on with a resident workspace; that lane with a lean workspace (the same bytes,
// BJ_PROOF_LEAN for this one proof); behind the other lane; the same once the idle parent has released its workspace; refused with
// BJ_ERR_OOM before a ticket exists.  The lane's whole footprint is reserved at admission, while the lane is idle, so a proof on a
// lane allocates and frees nothing while its sibling runs, and an out-of-memory is the status of bj_prove_async itself.
//
// Tickets.  Every live ticket is in a process-wide registry; bj_proof_wait and bj_proof_poll look the pointer up before they
// read it, so a ticket that was waited for, was never issued or whose context is gone is BJ_ERR_INVALID_ARG, not a read of freed
// memory.  Destroying the context frees the proofs and tickets nobody waited for.
#include "ctx.h"
#include "../../include/boojum_hip_diag.h"
#include "async_admission.h"

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <unordered_set>
#include <vector>

struct bj_ticket {
    bj_ctx *parent = nullptr;
    unsigned lane = 0;
    bool lean = false;             // admitted with a lean workspace: the lane proves with lean_override set
    const bj_setup *setup = nullptr;
    const uint64_t *h_variables = nullptr, *h_multiplicities = nullptr;
    // bj_prove_values_async: the proof is bj_prove_values' (h_variables and h_multiplicities above stay null)
    bool from_values = false;
    const uint64_t *h_values = nullptr;
    const uint32_t *h_counters = nullptr;
    size_t n_values = 0, n_counters = 0;
    std::vector<uint64_t> public_values;
    bool has_public = false;
    // result (written by the lane's worker under the lane's mutex)
    bool done = false;
    int rc = BJ_OK;
    bj_proof *proof = nullptr;
    std::string err;
};

namespace bj {

// the tickets bj_prove_async has handed out and nobody has waited for yet
static std::mutex g_tickets_m;
static std::unordered_set<const bj_ticket *> g_tickets;

struct Lane {
    bj_ctx *sub = nullptr;
    LaneBytes held;                // what sub holds, read on the submitting thread while the lane is idle
    hipStream_t stream = nullptr;
    std::thread worker;
    std::mutex m;
    std::condition_variable cv;
    bj_ticket *job = nullptr;      // submitted, not finished
    bool quit = false;
    Lane *sibling = nullptr;
    // when the proof in flight started, how long the last one took, and for which setup (for the stagger below)
    std::chrono::steady_clock::time_point started;
    double last_ms = 0;
    const bj_setup *running = nullptr, *last_setup = nullptr;

    bool busy() {
        std::lock_guard<std::mutex> lk(m);
        return job != nullptr;
    }
    // Two lanes that prove the same circuit take the same time, so whatever offset they start with stays: started together they stay in
    // phase — both hash at once, both sit in their latency-bound tails at once — and the second proof in flight fills nothing.  A lane
    // that is about to start within a quarter period of its sibling's start (same setup, period known from the last proof) therefore
    // waits until half a period after it; the device is busy with the sibling meanwhile, and from then on the lanes alternate.
    void stagger(const bj_setup *setup) {
        if (!sibling || !bj::env().async_stagger) return;
        double wait_ms = 0;
        {
            std::lock_guard<std::mutex> lk(sibling->m);
            const double period = sibling->last_setup == setup && sibling->last_ms > 0 ? sibling->last_ms : (last_setup == setup ? last_ms : 0);
            if (sibling->job && sibling->running == setup && period > 0) {
                const double off = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - sibling->started).count();
                if (off < 0.25 * period) wait_ms = 0.5 * period - off;
            }
        }
        if (wait_ms > 0) std::this_thread::sleep_for(std::chrono::duration<double, std::milli>(wait_ms));
    }

    void run() {
        for (;;) {
            bj_ticket *t;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return quit || (job && !job->done); });
                if (quit) return;
                t = job;
            }
            // What a lane does while its sibling proves, by witness size (measured, tools/async_small.py; BJ_ASYNC_MODE overrides):
            //   below 1 GiB (<= 2^20 rows of the bench geometry): bj_prove as is — the group-wise transfer hides behind the lane's own
            //   transforms — with the lanes STAGGERED half a period apart: 2^16 / 2^18 / 2^20 rows 1.10 / 1.18 / 1.09 x the serial rate
            //   (0.91 x at 2^20 when both lanes start together);
            //   from 1 GiB on: the whole witness first (55 ms of PCIe at 2^22 rows, under the sibling's kernels — which also sets the
            //   lanes apart), then the proof as on a resident witness: one leaf kernel instead of group-wise absorption; 1.03 x serial.
            unsigned v = 0, w = 0, ln = 0;
            (void)bj_setup_shape(t->setup, &ln, &v, &w, nullptr);
            const size_t witness_bytes = ((size_t)(v + w + 1) << ln) * 8;
            int mode = bj::env().async_mode;
            if (mode < 0) mode = witness_bytes >= ((size_t)1 << 30) ? 1 : 0;
            const auto t_pick = std::chrono::steady_clock::now();
            if (mode == 0) stagger(t->setup);
            {
                std::lock_guard<std::mutex> lk(m);
                started = std::chrono::steady_clock::now();
                running = t->setup;
            }
            sub->lean_override = t->lean ? 1 : -1;
            bj_proof *p = nullptr;
            const uint64_t *pub = t->has_public ? t->public_values.data() : nullptr;
            const bool overlapped = sibling && sibling->busy() && mode != 0;
            // from values there is no transfer to put first: a lane whose sibling proves gathers and transforms in groups and hashes once
            const int rc = t->from_values ? prove_values_staged(sub, t->setup, t->h_values, t->n_values, t->h_counters, t->n_counters, &p, overlapped)
                           : overlapped   ? prove_host_copy_first(sub, t->setup, t->h_variables, t->h_multiplicities, pub, &p, mode)
                                          : bj_prove(sub, t->setup, t->h_variables, t->h_multiplicities, pub, &p);
            sub->lean_override = -1;
            if (bj::env().async_debug)
                fprintf(stderr, "[lane %p] mode %d overlapped %d: picked up, ran %.1f ms (stagger %.1f ms)\n", (void *)this, mode, (int)overlapped,
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - started).count(),
                        std::chrono::duration<double, std::milli>(started - t_pick).count());
            {
                std::lock_guard<std::mutex> lk(m);
                last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - started).count();
                last_setup = t->setup;
                running = nullptr;
                t->rc = rc;
                t->proof = p;
                if (rc) t->err = sub->err;
                t->done = true;
                job = nullptr;
            }
            cv.notify_all();
        }
    }
};

struct Pipeline {
    Lane lanes[2];
    unsigned next = 0;
};

static int lane_start(bj_ctx *ctx, Lane &L) {
    if (int rc = bj_ctx_create(ctx->device, &L.sub)) return fail(ctx, rc, "bj_prove_async: creating a lane's context failed");
    if (hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking) != hipSuccess) {
        bj_ctx_destroy(L.sub);
        L.sub = nullptr;
        return fail(ctx, BJ_ERR_HIP, "bj_prove_async: creating a lane's stream failed");
    }
    L.sub->stream = L.stream;
    L.sub->hasher = ctx->hasher;
    L.worker = std::thread([&L] { L.run(); });
    return BJ_OK;
}

void pipeline_destroy(bj_ctx *ctx) {
    Pipeline *P = ctx->pipe;
    if (!P) return;
    for (Lane &L : P->lanes) {      // first every worker ends (nothing of a lane may go while a sibling still proves) ...
        if (!L.sub) continue;
        {
            std::unique_lock<std::mutex> lk(L.m);
            L.cv.wait(lk, [&] { return L.job == nullptr; });   // a proof in flight finishes first
            L.quit = true;
        }
        L.cv.notify_all();
        if (L.worker.joinable()) L.worker.join();
    }
    {   // ... then the tickets nobody waited for, with their proofs: a later wait or poll finds them in no registry
        std::lock_guard<std::mutex> lk(g_tickets_m);
        for (auto it = g_tickets.begin(); it != g_tickets.end();) {
            bj_ticket *t = const_cast<bj_ticket *>(*it);
            if (t->parent != ctx) {
                ++it;
                continue;
            }
            if (t->proof) bj_proof_destroy(t->proof);
            delete t;
            it = g_tickets.erase(it);
        }
    }
    for (Lane &L : P->lanes) {      // ... then the contexts go
        if (L.sub) bj_ctx_destroy(L.sub);
        if (L.stream) (void)hipStreamDestroy(L.stream);
    }
    delete P;
    ctx->pipe = nullptr;
}

int pipeline_release_workspace(bj_ctx *ctx) {
    Pipeline *P = ctx->pipe;
    if (!P) return BJ_OK;
    for (Lane &L : P->lanes) {
        if (!L.sub) continue;
        std::unique_lock<std::mutex> lk(L.m);
        if (L.job) return fail(ctx, BJ_ERR_INVALID_ARG, "bj_ctx_release_workspace: an asynchronous proof is running");
        if (int rc = bj_ctx_release_workspace(L.sub)) return fail(ctx, rc, "%s", L.sub->err.c_str());
    }
    return BJ_OK;
}

// Admission of one submission, on the submitting thread (async_admission.h): decides, starts the lane where it does not exist,
// waits for it where it is busy and has to grow, and reserves the lane's whole footprint.  A lane that cannot be started or
// reserved although the decision said it would fit (another process took the bytes) sends the submission down the ladder, so to
// the lane that exists.  BJ_ERR_OOM with both byte counts in the message where nothing fits.
static int admit_and_reserve(bj_ctx *ctx, const bj_setup *setup, bool values, size_t n_values, AdmissionDecision *out) {
    Pipeline *P = ctx->pipe;
    AdmissionInput in;
    if (int rc = async_footprints(ctx, setup, &in.resident, &in.lean, values, n_values)) return rc;
    in.due = P->next;
    in.parent_idle = !ctx->in_proof;
    for (unsigned first = TWO_LANES_RESIDENT;;) {
        ctx_held(ctx, &in.parent);
        for (unsigned i = 0; i < 2; i++) {
            Lane &L = P->lanes[i];
            in.created[i] = L.sub != nullptr;
            in.idle[i] = !in.created[i] || !L.busy();
            if (in.created[i] && in.idle[i]) ctx_held(L.sub, &L.held);   // a busy lane holds what it held when it was given its proof
            in.held[i] = in.created[i] ? L.held : LaneBytes();
        }
        size_t device_total = 0;
        BJ_HIP(ctx, hipMemGetInfo(&in.device_free, &device_total));
        in.budget = env().hbm_budget_bytes;
        const AdmissionDecision d = admit(in, first);
        if (env().async_debug)
            fprintf(stderr, "[async %p] admission: %s on lane %u%s, reserves %zu bytes of %zu available (budget %zu, held %zu)\n", (void *)ctx,
                    admission_name(d.rung), d.lane, d.lean ? " (lean)" : "", d.reserve_bytes, d.available, in.budget, in.held_total());
        if (d.rung == REFUSE)
            return fail(ctx, BJ_ERR_OOM, "bj_prove_async: the smallest plan (one lane, lean workspace) needs %zu more bytes, %zu bytes are available%s",
                        d.reserve_bytes, d.available, in.budget ? " under BJ_HBM_BUDGET_BYTES" : "");
        if (d.release_parent)
            if (int rc = ctx_release_own_workspace(ctx)) return rc;
        Lane &L = P->lanes[d.lane];
        int rc = L.sub ? BJ_OK : lane_start(ctx, L);
        if (!rc) {
            {
                std::unique_lock<std::mutex> lk(L.m);
                L.cv.wait(lk, [&] { return L.job == nullptr; });   // the lane's workspace is its proof's until the proof is done
            }
            if ((rc = ctx_reserve(L.sub, d.want))) fail(ctx, rc, "%s", L.sub->err.c_str());
            ctx_held(L.sub, &L.held);
        }
        if (!rc) {
            *out = d;
            return BJ_OK;
        }
        if (rc != BJ_ERR_OOM && rc != BJ_ERR_HIP) return rc;
        first = d.rung + 1;   // the next rung down, with what is held now
    }
}

}  // namespace bj

extern "C" {

// The part of a submission both entry points share: admission (no ticket exists before it: an out-of-memory is the call's own
// status), then the ticket `fill` completes goes to the lane admission chose.
static int submit(bj_ctx *ctx, const bj_setup *setup, bool values, size_t n_values, const std::function<void(bj_ticket *)> &fill, bj_ticket **out) {
    if (!ctx->pipe) {
        ctx->pipe = new bj::Pipeline();
        ctx->pipe->lanes[0].sibling = &ctx->pipe->lanes[1];
        ctx->pipe->lanes[1].sibling = &ctx->pipe->lanes[0];
    }
    bj::Pipeline *P = ctx->pipe;
    bj::Lane *L = nullptr;
    bj::AdmissionDecision d;
    if (int rc = bj::admit_and_reserve(ctx, setup, values, n_values, &d)) return rc;
    L = &P->lanes[d.lane];
    bj_ticket *t = new bj_ticket();
    t->parent = ctx;
    t->lane = d.lane;
    t->lean = d.lean;
    t->setup = setup;
    fill(t);
    {
        std::lock_guard<std::mutex> lk(bj::g_tickets_m);
        bj::g_tickets.insert(t);
    }
    {
        std::unique_lock<std::mutex> lk(L->m);
        L->cv.wait(lk, [&] { return L->job == nullptr; });   // at most two in flight (admission has waited for a lane it had to grow)
        L->job = t;
    }
    L->cv.notify_all();
    P->next = d.lane ^ 1;
    *out = t;
    return BJ_OK;
}

int bj_prove_async(bj_ctx *ctx, const bj_setup *setup, const uint64_t *h_variables, const uint64_t *h_multiplicities,
                   const uint64_t *h_public_values, bj_ticket **out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove_async: null out pointer");
    *out = nullptr;
    if (!setup || !h_variables) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove_async: null argument");
    unsigned n_pub = 0;
    if (int rc = bj_setup_shape(setup, nullptr, nullptr, nullptr, &n_pub)) return bj::fail(ctx, rc, "bj_prove_async: bad setup");
    if (bj::setup_world(setup) != 1)
        return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_prove_async: single-device setups only (the ranks of a sharded proof are concurrent already)");
    if (n_pub && !h_public_values) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove_async: public input values required");
    return submit(ctx, setup, false, 0, [&](bj_ticket *t) {
        t->h_variables = h_variables;
        t->h_multiplicities = h_multiplicities;
        if (n_pub) {
            t->public_values.assign(h_public_values, h_public_values + n_pub);   // the caller's array may go away; the witness may not
            t->has_public = true;
        }
    }, out);
}

int bj_prove_values_async(bj_ctx *ctx, const bj_setup *setup, const uint64_t *h_values, size_t n_values, const uint32_t *h_multiplicities,
                          size_t n_multiplicities, bj_ticket **out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove_values_async: null out pointer");
    *out = nullptr;
    if (int rc = bj::values_check(ctx, "bj_prove_values_async", setup, h_values, n_values, h_multiplicities, n_multiplicities)) return rc;
    return submit(ctx, setup, true, n_values, [&](bj_ticket *t) {
        t->from_values = true;
        t->h_values = h_values, t->n_values = n_values;
        t->h_counters = h_multiplicities, t->n_counters = n_multiplicities;
    }, out);
}

// A ticket that is in the registry is taken out of it by the one wait that gets it: the pointer of a ticket that was waited for,
// was never issued or went with its context is refused before anything is read through it.
int bj_proof_wait(bj_ticket *t, bj_proof **out) {
    if (out) *out = nullptr;
    if (!t) return BJ_ERR_INVALID_ARG;
    {
        std::lock_guard<std::mutex> lk(bj::g_tickets_m);
        if (!bj::g_tickets.erase(t))
            return bj::fail(nullptr, BJ_ERR_INVALID_ARG, "bj_proof_wait: no live ticket (waited for already, never issued, or its context was destroyed)");
    }
    bj_ctx *ctx = t->parent;
    bj::Lane &L = ctx->pipe->lanes[t->lane];
    {
        std::unique_lock<std::mutex> lk(L.m);
        L.cv.wait(lk, [&] { return t->done; });
    }
    const int rc = t->rc;
    if (rc) ctx->err = t->err;
    if (out)
        *out = t->proof;
    else if (t->proof)
        bj_proof_destroy(t->proof);
    delete t;
    return rc;
}

int bj_proof_poll(const bj_ticket *t) {
    if (!t) return BJ_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> reg(bj::g_tickets_m);   // held while the ticket is read: no wait frees it meanwhile
    if (!bj::g_tickets.count(t))
        return bj::fail(nullptr, BJ_ERR_INVALID_ARG, "bj_proof_poll: no live ticket (waited for already, never issued, or its context was destroyed)");
    bj::Lane &L = t->parent->pipe->lanes[t->lane];
    std::lock_guard<std::mutex> lk(L.m);
    return t->done ? 1 : 0;
}

}  // extern "C"
