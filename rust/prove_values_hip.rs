//! `prove_hip_from_values`: the proof from what `prove_from_witness_vec_and_precomputations` (convenience.rs:160) holds per proof.
//! A child module of prove_hip.rs, over the generated declarations of include/boojum_hip_diag.h (`boojum_hip_diag_sys.rs`,
//! tools/gen_rust_bindings.py): `bj_prove_values` stands there, beside the pinned entry points of boojum_hip.h.
use super::diag_sys::bj_prove_values;
use super::sys::{bj_proof_destroy, bj_proof_serialize, bj_proof_size_u64};
use super::{proof_from_bjpf, HipCtx, HipSetup, F};
use crate::cs::implementations::proof::Proof;
use crate::cs::implementations::prover::ProofConfig;
use crate::cs::oracle::TreeHasher;
use crate::field::FieldExtension;

/// No serialisation and no hint per call: `all_values` and the u32 multiplicity counters of the `WitnessVec` go to `bj_prove_values`
/// as they lie in memory (`F` is `repr(transparent)` over `u64`).  The setup must have been made by `bj_setup_create_from_placement`
/// (and `bj_setup_set_witness_placement` where the circuit has non-copiable witness columns); the public inputs are read through
/// the placement.
pub fn prove_hip_from_values<H: TreeHasher<F>, EXT: FieldExtension<2, BaseField = F>>(
    ctx: &HipCtx,
    setup: &HipSetup,
    witness_vec: &crate::cs::implementations::witness::WitnessVec<F>,
    proof_config: ProofConfig,
) -> Proof<F, H, EXT> {
    let mut proof = std::ptr::null_mut();
    ctx.check(unsafe {
        bj_prove_values(
            ctx.raw,
            setup.raw,
            witness_vec.all_values.as_ptr() as *const u64,
            witness_vec.all_values.len(),
            witness_vec.multiplicities.as_ptr(),
            witness_vec.multiplicities.len(),
            &mut proof,
        )
    });
    let mut words = vec![0u64; unsafe { bj_proof_size_u64(proof) }];
    ctx.check(unsafe { bj_proof_serialize(proof, words.as_mut_ptr()) });
    unsafe { bj_proof_destroy(proof) };
    proof_from_bjpf::<H, EXT>(&words, proof_config)
}
