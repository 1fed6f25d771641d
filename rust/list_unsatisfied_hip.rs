//! `HipSetup::list_unsatisfied`: the sibling of `check_satisfied_hip` (prove_hip.rs) that returns every failure instead of the
//! first.  A child module of prove_hip.rs, over the generated declarations of include/boojum_hip_diag.h
//! (`boojum_hip_diag_sys.rs`, tools/gen_rust_bindings.py).
use super::diag_sys::*;
use super::{HipCtx, HipSetup};

impl HipSetup {
    /// Every place where a witness fails the circuit, not the first one (`bj_list_unsatisfied`; `check_satisfied_hip` and
    /// the reference's `check_if_satisfied`, satisfiability_test.rs:15-353, stop at the first): the first
    /// `min(capacity, total)` entries in the order documented in include/boojum_hip_diag.h — kind 1 by (row, repetition, term), kind 2
    /// by (row, gate, repetition, term), kind 3 by (row, sub-argument), kind 4 by table row — and the totals per kind over the
    /// whole trace (`totals[0]` their sum; kinds 1 and 2 count terms).  `d_variables` / `d_multiplicities`: the device pointers
    /// `bj_prove_dev` takes (`d_multiplicities` null only without lookups); nothing is modified.  `capacity == 0` only counts.
    pub fn list_unsatisfied(&self, ctx: &HipCtx, d_variables: *const u64, d_multiplicities: *const u64, capacity: usize) -> (Vec<bj_unsat_entry>, [u64; 5]) {
        let empty = bj_unsat_entry { kind: 0, gate: 0, repetition: 0, term: 0, row: 0, value: 0, expected: 0 };
        let mut entries = vec![empty; capacity];
        let (mut n_entries, mut totals) = (0usize, [0u64; 5]);
        let h_entries = if capacity == 0 { std::ptr::null_mut() } else { entries.as_mut_ptr() };
        ctx.check(unsafe { bj_list_unsatisfied(ctx.raw, self.raw, d_variables, d_multiplicities, h_entries, capacity, &mut n_entries, totals.as_mut_ptr()) });
        entries.truncate(n_entries);
        (entries, totals)
    }
}
