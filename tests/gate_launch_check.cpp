// Stand-alone check of csrc/gate_launch.h and csrc/term_io.h (tests/test_gate_launch_host.py builds it host-only with the address
// and undefined-behaviour sanitizers): the host functions that turn a bj::GateShape and the launch descriptors into kernel
// arguments, against values written out by hand.  Nothing here touches a device: the pointers are host arrays used as addresses.
#include "gate_launch.h"

#include <cstdio>
#include <initializer_list>

using bj::u64;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static bj::GateShape shape(int kind, std::initializer_list<int> path, unsigned reps, unsigned var_stride, unsigned const_stride, unsigned num_terms,
                           unsigned first_term, unsigned wit_stride = 0) {
    bj::GateShape G;
    G.kind = kind;
    for (int b : path) G.path[G.path_len++] = (unsigned char)b;
    G.reps = reps; G.var_stride = var_stride; G.const_stride = const_stride; G.wit_stride = wit_stride; G.num_terms = num_terms;
    G.first_term = first_term;
    return G;
}

int main() {
    static u64 vars[64], consts[64], wits[8], alphas[256], out0[4], out1[4], terms[16];

    // ---- Cols::at ----
    const bj::Cols v{vars, 5}, c{consts, 7};
    CHECK(v.at(0).p == vars && v.at(0).stride == 5);
    CHECK(v.at(3).p == vars + 15 && v.at(3).stride == 5);
    CHECK(v.at(3).at(2).p == vars + 25);
    CHECK(c.at(9).p == consts + 63 && c.at(9).stride == 7);

    // ---- prog_args ----
    bj::DevProgram P;
    bj::DevRelation rel[3];
    u64 values[2];
    P.d_rel = rel; P.d_values = values; P.n_rel = 3; P.n_writes = 2; P.reads_witness = true;
    const bj::GateShape G = shape(BJ_GATE_PROGRAM, {0, 1, 1}, 26, 5, 2, 2, 11, 3);
    const bj::GateCols cols{v, c, wits};
    {   // quotient mode
        const bj::gpdev::ProgArgs a = bj::prog_args(P, G, cols, bj::TermSink{alphas, 1000, out0, out1}, nullptr);
        CHECK(a.vars == vars && a.var_stride == 5 && a.consts == consts && a.const_stride == 7);
        CHECK(a.wits == wits && a.rep_wit_stride == 3);   // the witness columns lie at var_stride: there is no stride of their own
        CHECK(a.rel == rel && a.values == values && a.n_rel == 3 && a.n_writes == 2);
        CHECK(a.path_len == 3);
        const unsigned char want[8] = {0, 1, 1, 0, 0, 0, 0, 0};   // padded to 8
        for (int b = 0; b < 8; b++) CHECK(a.path[b] == want[b]);
        CHECK(a.reps == 26 && a.rep_var_stride == 5 && a.rep_const_stride == 2);
        CHECK(a.alphas == alphas + 2 * 11);   // the category's first power + 2 * first_term
        CHECK(a.Q == 1000 && a.out0 == out0 && a.out1 == out1 && a.terms == nullptr);
    }
    {   // A program that reads no witness column is given none, whatever the circuit has.  The fused launch of the generated bodies
        // (launch_gate_aot_fused) takes only entries with alpha powers, no term buffer and NO witness pointer, and
        // launch_gate_programs fills its entries with the circuit's columns: they must pass on a circuit with witness columns.
        bj::DevProgram F = P;
        F.reads_witness = false;
        const bj::gpdev::ProgArgs a = bj::prog_args(F, G, cols, bj::TermSink{alphas, 1000, out0, out1}, nullptr);
        CHECK(cols.wits != nullptr && a.wits == nullptr && a.rep_wit_stride == 0);
        CHECK(a.alphas != nullptr && a.terms == nullptr && a.rep_var_stride != 0 && a.reps != 0);
        CHECK(a.vars == vars && a.consts == consts && a.alphas == alphas + 2 * 11 && a.Q == 1000);
    }
    {   // stand-alone term mode: null alphas stay null, whatever first_term says
        const bj::gpdev::ProgArgs a = bj::prog_args(P, G, bj::GateCols{v, c, nullptr}, bj::TermSink{nullptr, 8, nullptr, nullptr}, terms);
        CHECK(a.alphas == nullptr && a.terms == terms && a.Q == 8 && a.out0 == nullptr && a.out1 == nullptr && a.wits == nullptr);
    }
    {   // a path of 8 is copied whole; bytes of the shape behind path_len are not
        bj::GateShape H = shape(BJ_GATE_PROGRAM, {1, 1, 1, 1, 1, 1, 1, 1}, 1, 1, 0, 1, 0);
        bj::gpdev::ProgArgs a = bj::prog_args(P, H, cols, bj::TermSink{alphas, 1, out0, out1}, nullptr);
        for (int b = 0; b < 8; b++) CHECK(a.path[b] == 1);
        CHECK(a.alphas == alphas);
        H.path_len = 2;
        a = bj::prog_args(P, H, cols, bj::TermSink{alphas, 1, out0, out1}, nullptr);
        for (int b = 0; b < 8; b++) CHECK(a.path[b] == (b < 2 ? 1 : 0));
    }

    // ---- TermSink::powers: the one null rule ----
    CHECK((bj::TermSink{alphas, 1, out0, out1}.powers(0) == alphas) && (bj::TermSink{alphas, 1, out0, out1}.powers(7) == alphas + 14));
    CHECK((bj::TermSink{nullptr, 1, out0, out1}.powers(7) == nullptr));

    // ---- path_bits agrees with GateShape::path ----
    for (unsigned len = 0; len <= 8; len++)
        for (unsigned bits = 0; bits < (1u << len); bits++) {
            bj::GateShape H;
            H.path_len = len;
            for (unsigned b = 0; b < 8; b++) H.path[b] = b < len ? (bits >> b) & 1 : 1;   // entries behind the path do not count
            CHECK(bj::path_bits(H) == bits);
        }

    // ---- gate_windows: the SHA-256 circuit's gates (60 general-purpose columns) ----
    const bj::GateShape sha[4] = {shape(BJ_GATE_CONSTANT_ALLOCATOR, {0, 0, 1}, 4, 1, 1, 1, 0), shape(BJ_GATE_FMA_NO_CONSTANT, {1}, 15, 4, 0, 1, 4),
                                  shape(BJ_GATE_REDUCTION4, {0, 1}, 12, 5, 0, 1, 19), shape(BJ_GATE_NOP, {0, 0, 0}, 1, 0, 0, 0, 31)};
    {
        bj::GateWindows gw;
        CHECK(bj::gate_windows(sha, 4, &gw));
        CHECK(gw.n_windows == 3 && gw.n_vars == 60);   // 15 x 4 = 12 x 5 = 60 columns in windows of 20
        CHECK(!gw.present[0] && gw.present[bj::K_ALLOC] && gw.present[bj::K_FMA] && gw.present[bj::K_RED4]);
        CHECK(gw.aoff[bj::K_ALLOC] == 0 && gw.aoff[bj::K_FMA] == 4 && gw.aoff[bj::K_RED4] == 19);
        CHECK(gw.reps[bj::K_ALLOC] == 4 && gw.reps[bj::K_FMA] == 15 && gw.reps[bj::K_RED4] == 12);
        CHECK(gw.const_stride[bj::K_ALLOC] == 1 && gw.const_stride[bj::K_FMA] == 0 && gw.const_stride[bj::K_RED4] == 0);
        CHECK(gw.path_len[bj::K_ALLOC] == 3 && gw.path_len[bj::K_FMA] == 1 && gw.path_len[bj::K_RED4] == 2);
        CHECK(gw.path[bj::K_ALLOC][0] == 0 && gw.path[bj::K_ALLOC][1] == 0 && gw.path[bj::K_ALLOC][2] == 1);
        CHECK(gw.path[bj::K_FMA][0] == 1 && gw.path[bj::K_RED4][0] == 0 && gw.path[bj::K_RED4][1] == 1);
        // a kind with a kernel of its own is passed over; one window for a lone allocator; no hand-written gate at all is refused
        const bj::GateShape mixed[2] = {shape(BJ_GATE_PROGRAM, {1, 1}, 3, 9, 0, 2, 0), shape(BJ_GATE_CONSTANT_ALLOCATOR, {0}, 7, 1, 1, 1, 6)};
        CHECK(bj::gate_windows(mixed, 2, &gw) && gw.n_windows == 1 && gw.n_vars == 7 && gw.aoff[bj::K_ALLOC] == 6 && !gw.present[bj::K_FMA]);
        CHECK(!bj::gate_windows(mixed, 1, &gw));
        CHECK(!bj::gate_windows(sha + 3, 1, &gw));
    }
    {   // each refusal
        bj::GateWindows gw;
        auto refused = [&](unsigned at, const bj::GateShape &with) {
            bj::GateShape list[5] = {sha[0], sha[1], sha[2], sha[3], sha[3]};
            list[at] = with;
            return !bj::gate_windows(list, 5, &gw);
        };
        CHECK(!refused(4, sha[3]));                                                            // the list itself passes
        CHECK(refused(4, shape(BJ_GATE_FMA_NO_CONSTANT, {1, 1}, 2, 4, 0, 1, 31)));             // a kind that appears twice
        CHECK(refused(1, shape(BJ_GATE_FMA_NO_CONSTANT, {1}, 15, 5, 0, 1, 4)));                // a non-principal var_stride
        CHECK(refused(0, shape(BJ_GATE_CONSTANT_ALLOCATOR, {0, 0, 1}, 4, 2, 1, 1, 0)));
        CHECK(refused(2, shape(BJ_GATE_REDUCTION4, {0, 1}, 12, 5, 0, 2, 19)));                 // num_terms != 1
        CHECK(refused(1, shape(BJ_GATE_FMA_NO_CONSTANT, {1}, 15, 4, 2, 1, 4)));                // shared constants with a const_stride
        CHECK(refused(2, shape(BJ_GATE_REDUCTION4, {0, 1}, 12, 5, 4, 1, 19)));
        CHECK(refused(2, shape(BJ_GATE_REDUCTION4, {0, 1, 0, 1, 0, 1, 0}, 12, 5, 0, 1, 19)));  // a path longer than 6
        CHECK(!refused(2, shape(BJ_GATE_REDUCTION4, {0, 1, 0, 1, 0, 1}, 12, 5, 0, 1, 19)));
    }

    // ---- gate_set: list order, every field ----
    {
        const bj::GateSet gs = bj::gate_set(sha, 4);
        CHECK(gs.n_gates == 4);
        CHECK(gs.g[1].kind == BJ_GATE_FMA_NO_CONSTANT && gs.g[1].path_len == 1 && gs.g[1].reps == 15 && gs.g[1].var_stride == 4 &&
              gs.g[1].const_stride == 0 && gs.g[1].num_terms == 1 && gs.g[1].path[0] == 1 && gs.g[1].path[1] == 0);
        CHECK(gs.g[0].const_stride == 1 && gs.g[0].path[2] == 1 && gs.g[2].var_stride == 5 && gs.g[3].kind == BJ_GATE_NOP && gs.g[3].num_terms == 0);
    }

    if (failures) return 1;
    std::printf("gate launch arguments == expected\n");
    return 0;
}
