// The layout of a proof, defined once: which columns each of the four base oracles holds, which polynomials are opened where and
// in which order, and where each of them sits inside a query's words and inside the serialised proof.  The prover, the verifier,
// the setup, the satisfiability check and the multiplicity count read the values made here; none of them lays a column, an
// opening or a section out again.  Plain C++17 over include/boojum_hip.h: a host program can use it (tests/proof_layout_check.cpp).
#pragma once
#include "../../include/boojum_hip.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace bj {

// What a setup and a verification key share about a circuit and its proof config: bj_setup and bj_vk derive from it.
struct CircuitShape {
    unsigned log_n = 0, V = 0, num_gp_vars = 0, nC = 0, q = 0;
    unsigned Wc = 0;               // non-copiable witness columns (behind the V variable columns in the witness oracle)
    unsigned lookup_w = 0, lookup_reps = 0;
    unsigned lookup_cps = 0;       // variable columns of a sub-argument (specialized_columns_per_subargument, cs/mod.rs:300-312)
    bool tid_var = false;          // UseSpecializedColumnsWithTableIdAsVariable: the table id is the last of lookup_cps = lookup_w + 1
    unsigned table_id_col = 0;     // the constant column that holds the table id (0 when tid_var)
    unsigned log_fri = 0, cap_size = 0;
};

// LookupParameters::UseSpecializedColumnsWithTableIdAsVariable (cs/mod.rs:237-241): table_ids_column_idxes is empty (setup.rs:970-971)
// and a sub-argument owns width + 1 variable columns, the last one the table id (lookup_argument_in_ext.rs:354-366, 949-1000)
inline CircuitShape circuit_shape(const bj_circuit *c, const bj_proof_config *cfg) {
    CircuitShape s;
    s.log_n = c->log_n; s.V = c->num_vars; s.num_gp_vars = c->num_gp_vars; s.Wc = c->num_witness_cols; s.nC = c->num_constant_cols;
    s.q = c->quotient_degree;
    s.lookup_w = c->lookup_width; s.lookup_reps = c->lookup_reps;
    s.tid_var = c->lookup_reps && c->table_id_col == BJ_TABLE_ID_AS_VARIABLE;
    s.table_id_col = s.tid_var ? 0 : c->table_id_col;
    s.lookup_cps = c->lookup_width + (s.tid_var ? 1u : 0u);
    while (s.log_fri < 31 && (1u << s.log_fri) < cfg->fri_lde_factor) s.log_fri++;
    s.cap_size = cfg->cap_size;
    return s;
}

enum : unsigned { ORACLE_WITNESS = 0, ORACLE_STAGE2 = 1, ORACLE_QUOTIENT = 2, ORACLE_SETUP = 3, NO_COLUMN = 0xFFFFFFFFu };
// One opened polynomial: a base-field column (col1 == NO_COLUMN) or the two adjacent columns of an F_p^2 polynomial.
struct Opened {
    unsigned oracle, col0, col1;
};

// The opening sets in the order the DEEP challenge powers are handed out (prover.rs:1803-2067, verifier.rs:2233-2290): everything
// at z, z(x) at z * omega, the lookup sums at 0, then the public inputs of every distinct row at omega^row.  value[i]: which
// value of the set's kind polys[i] takes — of values_at_z, values_at_z_omega, values_at_0, or of the public inputs.
enum : unsigned { OPEN_AT_Z = 0, OPEN_AT_Z_OMEGA = 1, OPEN_AT_ZERO = 2, OPEN_AT_ROW = 3 };
struct OpeningSet {
    unsigned point, row;   // row: OPEN_AT_ROW only
    std::vector<Opened> polys;
    std::vector<unsigned> value;
};

struct ProofLayout {
    CircuitShape s;
    bool has_lookup = false;
    unsigned n_chunks = 0, n_partials = 0, n_lookup_terms = 0, nz = 0;
    unsigned widths[4] = {};   // leaf widths: witness, stage 2, quotient, setup

    // column numbers inside an oracle; the caller multiplies by its own stride.  Witness: variables || witness || multiplicities
    // (prover.rs:317-347)
    unsigned var(unsigned i) const { return i; }
    unsigned wit(unsigned i) const { return s.V + i; }
    unsigned lookup_var(unsigned sub, unsigned j) const { return s.num_gp_vars + sub * s.lookup_cps + j; }
    unsigned multiplicity() const { return s.V + s.Wc; }
    // stage 2: z || partial products || A_i || B, each the first column of an F_p^2 pair
    unsigned z() const { return 0; }
    unsigned partial(unsigned j) const { return 2 + 2 * j; }
    unsigned lookup_a(unsigned i) const { return 2 + 2 * n_partials + 2 * i; }
    unsigned lookup_b() const { return lookup_a(s.lookup_reps); }
    // quotient: chunk j of c0 and of c1 side by side (prover.rs:1445-1467)
    unsigned chunk(unsigned j) const { return 2 * j; }
    // setup: sigma || constants || tables (polynomial_storage.rs:667-676)
    unsigned sigma(unsigned i) const { return i; }
    unsigned constant(unsigned i) const { return s.V + i; }
    unsigned table_id() const { return constant(s.table_id_col); }
    unsigned table(unsigned j) const { return s.V + s.nC + j; }

    // the polynomials opened at z, in opening order (prover.rs:1550-1683, verifier.rs:1150-1206), and where each kind starts in
    // that list.  Without lookups at_mult = at_a = at_b = at_table = at_chunk.
    std::vector<Opened> opened;
    unsigned at_var = 0, at_wit = 0, at_const = 0, at_sigma = 0, at_z = 0, at_partial = 0, at_mult = 0, at_a = 0, at_b = 0, at_table = 0,
             at_chunk = 0;

    std::vector<OpeningSet> opening_sets(const unsigned *pub_cols, const unsigned *pub_rows, size_t n_pub) const;
};

inline ProofLayout proof_layout(const CircuitShape &s) {
    ProofLayout L;
    L.s = s;
    L.has_lookup = s.lookup_reps > 0;
    L.n_chunks = s.q ? (s.V + s.q - 1) / s.q : 0;
    L.n_partials = L.n_chunks ? L.n_chunks - 1 : 0;
    L.n_lookup_terms = L.has_lookup ? s.lookup_reps + 1 : 0;
    const unsigned n_tables = L.has_lookup ? s.lookup_w + 1 : 0;
    L.widths[ORACLE_WITNESS] = s.V + s.Wc + (L.has_lookup ? 1u : 0u);
    L.widths[ORACLE_STAGE2] = 2 * (1 + L.n_partials + L.n_lookup_terms);
    L.widths[ORACLE_QUOTIENT] = 2 * s.q;
    L.widths[ORACLE_SETUP] = s.V + s.nC + n_tables;
    auto base = [&L](unsigned oracle, unsigned col) { L.opened.push_back({oracle, col, NO_COLUMN}); };
    auto ext = [&L](unsigned oracle, unsigned col) { L.opened.push_back({oracle, col, col + 1}); };
    auto here = [&L]() { return (unsigned)L.opened.size(); };
    L.at_var = here();
    for (unsigned i = 0; i < s.V; i++) base(ORACLE_WITNESS, L.var(i));
    L.at_wit = here();
    for (unsigned i = 0; i < s.Wc; i++) base(ORACLE_WITNESS, L.wit(i));
    L.at_const = here();
    for (unsigned i = 0; i < s.nC; i++) base(ORACLE_SETUP, L.constant(i));
    L.at_sigma = here();
    for (unsigned i = 0; i < s.V; i++) base(ORACLE_SETUP, L.sigma(i));
    L.at_z = here();
    ext(ORACLE_STAGE2, L.z());
    L.at_partial = here();
    for (unsigned j = 0; j < L.n_partials; j++) ext(ORACLE_STAGE2, L.partial(j));
    L.at_mult = here();
    if (L.has_lookup) base(ORACLE_WITNESS, L.multiplicity());
    L.at_a = here();
    for (unsigned i = 0; i < s.lookup_reps; i++) ext(ORACLE_STAGE2, L.lookup_a(i));
    L.at_b = here();
    if (L.has_lookup) ext(ORACLE_STAGE2, L.lookup_b());
    L.at_table = here();
    for (unsigned j = 0; j < n_tables; j++) base(ORACLE_SETUP, L.table(j));
    L.at_chunk = here();
    for (unsigned j = 0; j < s.q; j++) ext(ORACLE_QUOTIENT, L.chunk(j));
    L.nz = here();
    return L;
}

// pub_cols / pub_rows: the circuit's public-input locations.  Inputs of one row share a set; the sets come in the order their
// rows first appear, the inputs inside a set in the order they were given.
inline std::vector<OpeningSet> ProofLayout::opening_sets(const unsigned *pub_cols, const unsigned *pub_rows, size_t n_pub) const {
    std::vector<OpeningSet> sets;
    sets.push_back({OPEN_AT_Z, 0, opened, {}});
    for (unsigned i = 0; i < nz; i++) sets.back().value.push_back(i);
    sets.push_back({OPEN_AT_Z_OMEGA, 0, {opened[at_z]}, {0}});
    if (has_lookup) {
        sets.push_back({OPEN_AT_ZERO, 0, {}, {}});
        for (unsigned i = 0; i < n_lookup_terms; i++) {   // the A_i, then B: adjacent in the opened list
            sets.back().polys.push_back(opened[at_a + i]);
            sets.back().value.push_back(i);
        }
    }
    const size_t first_pub = sets.size();
    for (size_t i = 0; i < n_pub; i++) {
        size_t pos = first_pub;
        while (pos < sets.size() && sets[pos].row != pub_rows[i]) pos++;
        if (pos == sets.size()) sets.push_back({OPEN_AT_ROW, pub_rows[i], {}, {}});
        sets[pos].polys.push_back({ORACLE_WITNESS, var(pub_cols[i]), NO_COLUMN});
        sets[pos].value.push_back((unsigned)i);
    }
    return sets;
}

// The 19 words a serialised proof starts with.  fill() writes them all; matches() compares what the key and the schedule fix,
// which leaves N_QUERIES (the caller's rule: a verifier may take fewer) and POW_CHALLENGE (the proof's own).
struct ProofHeader {
    enum : unsigned { MAGIC, VERSION, N_PUBLIC, CAP_SIZE, N_AT_Z, N_AT_Z_OMEGA, N_AT_ZERO, N_FRI_ORACLES, FINAL_DEGREE, N_QUERIES, WIDTH_WITNESS,
                      WIDTH_STAGE2, WIDTH_QUOTIENT, WIDTH_SETUP, DEPTH, LOG_N, FRI_LDE, POW_BITS, POW_CHALLENGE, WORDS };
    static constexpr uint64_t MAGIC_BJPF = 0x424A5046ULL, VERSION_2 = 2;
    uint64_t w[WORDS] = {};
    void fill(const ProofLayout &L, size_t n_pub, size_t sched_len, size_t final_degree, size_t n_queries, unsigned depth, unsigned pow_bits,
              uint64_t pow_challenge) {
        const uint64_t words[WORDS] = {MAGIC_BJPF, VERSION_2, n_pub, L.s.cap_size, L.nz, 1, L.n_lookup_terms, sched_len, final_degree, n_queries,
                                       L.widths[0], L.widths[1], L.widths[2], L.widths[3], depth, L.s.log_n, (uint64_t)1 << L.s.log_fri, pow_bits,
                                       pow_challenge};
        for (unsigned i = 0; i < WORDS; i++) w[i] = words[i];
    }
    bool matches(const uint64_t *W) const {
        for (unsigned i = 0; i < WORDS; i++)
            if (i != N_QUERIES && i != POW_CHALLENGE && W[i] != w[i]) return false;
        return true;
    }
};

// Where the sections of a serialised proof start (words from the start of the buffer; layout: proof_format.py), and the words of
// one query: the index, then leaf and Merkle path of the four base oracles, then leaf and path of every FRI oracle.
struct SerialLayout {
    bool ok = false;       // false: the domain is smaller than the cap, or a schedule no prover emits (steps of 1..3, no layer below the cap)
    unsigned depth = 0;    // path length of the base oracles
    unsigned fri_depth[32] = {}, total_folds = 0;
    size_t header = 0, schedule = 0, public_inputs = 0, witness_cap = 0, stage2_cap = 0, quotient_cap = 0, values_at_z = 0, values_at_z_omega = 0,
           values_at_0 = 0, fri_caps = 0, final_c0 = 0, final_c1 = 0, queries = 0, total = 0;
    size_t query_words = 0;
    uint32_t leaf_off[4] = {}, path_off[4] = {}, fri_leaf_off[32] = {}, fri_path_off[32] = {};   // inside one query
};

inline SerialLayout serial_layout(const ProofLayout &L, const uint32_t *sched, size_t sched_len, size_t final_degree, size_t n_queries,
                                  size_t n_pub) {
    SerialLayout S;
    const unsigned log_full = L.s.log_n + L.s.log_fri;
    const size_t cap = L.s.cap_size;
    if (log_full > 32 || sched_len > 32 || !cap || ((size_t)1 << log_full) < cap) return S;
    auto log2_of = [](size_t x) {
        unsigned r = 0;
        while (((size_t)1 << r) < x) r++;
        return r;
    };
    S.depth = log2_of(((size_t)1 << log_full) / cap);
    uint32_t o = 1;   // word 0 of a query: its index
    for (int k = 0; k < 4; k++) {
        S.leaf_off[k] = o;
        S.path_off[k] = o += L.widths[k];
        o += S.depth * 4;
    }
    size_t leaves = (size_t)1 << log_full;
    for (size_t l = 0; l < sched_len; l++) {
        const unsigned k = sched[l];
        if (k < 1 || k > 3 || (leaves >> k) < cap) return S;
        leaves >>= k;
        S.fri_depth[l] = log2_of(leaves / cap);
        S.total_folds += k;
        S.fri_leaf_off[l] = o;
        S.fri_path_off[l] = o += 2u << k;
        o += S.fri_depth[l] * 4;
    }
    S.query_words = o;
    size_t at = 0;
    auto section = [&at](size_t words) {
        const size_t start = at;
        at += words;
        return start;
    };
    S.header = section(ProofHeader::WORDS);
    S.schedule = section(sched_len);
    S.public_inputs = section(n_pub);
    S.witness_cap = section(cap * 4);
    S.stage2_cap = section(cap * 4);
    S.quotient_cap = section(cap * 4);
    S.values_at_z = section(2 * (size_t)L.nz);
    S.values_at_z_omega = section(2);
    S.values_at_0 = section(2 * (size_t)L.n_lookup_terms);
    S.fri_caps = section(sched_len * cap * 4);
    S.final_c0 = section(final_degree);
    S.final_c1 = section(final_degree);
    S.queries = section(n_queries * S.query_words);
    S.total = at;
    S.ok = true;
    return S;
}

}  // namespace bj
