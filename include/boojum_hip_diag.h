/* boojum_hip_diag.h — diagnostics beside the C ABI of include/boojum_hip.h, exported by the same libboojum_hip.so.
 *
 * boojum_hip.h is the drop-in boundary: its entry points and structs are counted and pinned by the test suite, and every one
 * of them replaces an interface of the reference.  What a host uses only while it debugs a circuit or a witness generator, and
 * what the reference has no counterpart for, is declared here instead; it needs nothing but the types of boojum_hip.h, changes
 * no layout of them and comes within the same BJ_ABI_VERSION.  So is an entry point added beside the pinned set that needs none of
 * its structs changed: bj_prove_values / bj_prove_values_async / bj_setup_set_witness_placement, at the end of this file.
 * tools/gen_py_abi.py and tools/gen_rust_bindings.py generate era_boojum_amd/_abi_diag.py and rust/boojum_hip_diag_sys.rs from
 * this header as they generate _abi.py and boojum_hip_sys.rs from the other. */
#ifndef BOOJUM_HIP_DIAG_H
#define BOOJUM_HIP_DIAG_H

#include "boojum_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bj_list_unsatisfied: EVERY failure that bj_check_satisfied's rule finds, not the first one — check_if_satisfied
 * (src/cs/implementations/satisfiability_test.rs:15-353) stops at its first panic, and a witness generator's bug usually breaks a
 * family of cells whose shape is the diagnosis.  One bj_unsat_entry per failure, fields as in bj_unsat_report:
 *   kinds 1, 2: one entry per non-zero term (a row can contribute many), `value` the term's canonical value;
 *   kind 3: one entry per (row, sub-argument) whose tuple is in no table row;
 *   kind 4: one entry per class whose multiplicity sum is not its count, `value` / `expected` as in the report.
 * The list is in the order above carried through to the end: all of kind 1 by (row, repetition, term), then all of kind 2 by (row,
 * gate, repetition, term), then all of kind 3 by (row, sub-argument), then all of kind 4 by smallest table row of the class.
 * h_entries (host memory) receives the first min(capacity, total) entries of that order and *n_entries that number; capacity == 0
 * with h_entries == NULL is a pure count.  totals[k], k = 1..4, is the exact number of entries of kind k in the whole trace, not
 * the number written, and totals[0] their sum.  totals[3] and totals[4] equal bj_unsat_report.failures[3] and [4]; totals[1] and
 * totals[2] count TERMS where failures[1] and failures[2] count rows.  If there is any entry and capacity >= 1, entry 0 carries
 * the seven fields of bj_check_satisfied's report on the same input; a satisfied witness gives *n_entries == 0 and all totals 0.
 * Which rows are looked at rests on the same pass under the same fixed weights as bj_check_satisfied, with the same caveat (a
 * witness built against the weights is not covered).  What is written is exact: every term of every flagged row is evaluated
 * again on its own with unit weight, so totals[1] and totals[2] are exact over the rows the combination flags, and kinds 3 and 4
 * involve no randomness.  The cost is one pass over the n rows plus the terms on the flagged rows, in chunks of rows that fit the
 * context's scratch; the scratch also holds min(capacity, the most entries n rows can have) entries.
 * Everything else as for bj_check_satisfied (arguments, values canonical or not, nothing modified, the context's stream and
 * scratch, synchronises, sharded setups, not while a proof runs, a proof made afterwards is byte for byte the proof made before,
 * the same limits with the same wording).  BJ_OK whenever the listing ran; BJ_ERR_INVALID_ARG for a null n_entries or totals, or a
 * null h_entries with capacity != 0. */
typedef struct bj_unsat_entry {
    uint32_t kind;        /* bj_unsat_kind, never BJ_SAT */
    uint32_t gate;        /* as in bj_unsat_report */
    uint32_t repetition;
    uint32_t term;
    uint64_t row;
    uint64_t value;
    uint64_t expected;
} bj_unsat_entry;
int bj_list_unsatisfied(bj_ctx *ctx, const bj_setup *setup, const uint64_t *d_variables, const uint64_t *d_multiplicities,
                        bj_unsat_entry *h_entries, size_t capacity, size_t *n_entries, uint64_t totals[5]);
int bj_list_unsatisfied_from_dumps(bj_ctx *ctx, const bj_setup *setup, const void *witness_vec, size_t witness_vec_len,
                                   const void *variables_hint, size_t variables_hint_len, const void *witness_hint,
                                   size_t witness_hint_len, bj_unsat_entry *h_entries, size_t capacity, size_t *n_entries,
                                   uint64_t totals[5]);

/* ---- proofs from a WitnessVec's values (beside the pinned set of boojum_hip.h; no struct of it changes, ABI version 6) ----
 * What a reference host holds per proof (prove_from_witness_vec_and_precomputations, convenience.rs:160): a WitnessVec
 * (witness.rs:29-71) as plain arrays, not [column][n] witness columns.  h_values: all_values [n_values].  h_multiplicities: the
 * u32 counters, concatenated per table as the reference keeps them [n_multiplicities <= n], zero-extended to the trace on the
 * device; NULL / 0 with lookups: counted on the device as for bj_prove.  Public input values are the cells at the setup's public
 * input locations and are read from h_values through the placement: none are passed (a public input on a placeholder cell has
 * value 0).
 * The setup must hold the variables' placement (bj_setup_create_from_placement) and, if the circuit has non-copiable witness
 * columns, the witness placement (bj_setup_set_witness_placement): otherwise BJ_ERR_INVALID_ARG, the message naming what is
 * missing.  Single device only: a sharded setup is BJ_ERR_UNSUPPORTED.  all_values crosses PCIe once (n_values * 8 bytes instead
 * of the materialised columns), every column group is gathered on the device (witness_set_from_witness_vec, witness.rs:386-443)
 * straight into the witness staging and transformed, extended and hashed as a group of bj_prove's host witness is.  The proof is
 * byte for byte bj_prove's on the columns materialised from the same placement and values.  A cell that names a value at or
 * beyond n_values refuses the proof — BJ_ERR_INVALID_ARG, "a cell names a variable beyond all_values" — before the witness cap
 * enters the transcript.  Memory: the values and the counters wait in the context's witness staging behind the multiplicity
 * column (n_values * 8 + n * 4 bytes more than for bj_prove); nothing is allocated per proof once the context has seen the size.
 * bj_prove_values_async: tickets, bj_proof_wait / bj_proof_poll, lifetimes (h_values and h_multiplicities stay valid and
 * unchanged until bj_proof_wait returns), error reporting and admission are those of bj_prove_async, the footprint being that of
 * a host-witness proof plus the bytes above; the refusals above and BJ_ERR_OOM come from the submission, never from bj_proof_wait.
 * bj_prove_from_dumps with a NULL variables hint and no witness hint is bj_prove_values on the arrays inside the dump. */
int bj_prove_values(bj_ctx *ctx, const bj_setup *setup, const uint64_t *h_values, size_t n_values, const uint32_t *h_multiplicities,
                    size_t n_multiplicities, bj_proof **out);
int bj_prove_values_async(bj_ctx *ctx, const bj_setup *setup, const uint64_t *h_values, size_t n_values, const uint32_t *h_multiplicities,
                          size_t n_multiplicities, bj_ticket **out);
/* DenseWitnessCopyHint dump (hints/mod.rs:17-21; circuit->num_witness_cols columns of n cells) -> the resident u32 placement of
 * the non-copiable witness columns of a single-device setup: same narrowing and limits as the variables' placement, 4 bytes per
 * cell, counted by bj_setup_device_bytes.  Setting it again replaces the one held; not while a proof of the setup runs.
 * Synchronises the context's stream. */
int bj_setup_set_witness_placement(bj_ctx *ctx, bj_setup *setup, const void *witness_hint, size_t witness_hint_len);

/* Test door of the kernel behind bj_prove_values (witness_gather_kernel, csrc/witness_values.hip) on caller-given device arrays:
 * d_cells[i] = d_values[d_placement[i]] for the cols * 2^log_n cells of a u32 placement [cols][n]; 0xFFFFFFFF (a placeholder)
 * gives 0, an index at or beyond n_values gives 0 and sets *bad (host memory) to non-zero.  The pointers need only their types'
 * alignment.  On the context's stream; synchronises.  bj_witness_gather_sweep_cells: the cells one sweep of the launcher's grid
 * covers on this device (a larger count takes the grid-stride loop round again); 0 for a context that cannot be bound. */
int bj_witness_gather(bj_ctx *ctx, const uint32_t *d_placement, unsigned cols, unsigned log_n, const uint64_t *d_values, size_t n_values,
                      uint64_t *d_cells, unsigned *bad);
size_t bj_witness_gather_sweep_cells(bj_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* BOOJUM_HIP_DIAG_H */
