"""ctypes binding of include/boojum_hip.h.  Device buffers are plain integer addresses (e.g. ``tensor.data_ptr()``)."""
import contextlib
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _abi
from . import _abi_diag

_HERE = os.path.dirname(os.path.abspath(__file__))
P = (1 << 64) - (1 << 32) + 1
u64p = C.POINTER(C.c_uint64)

# era_boojum_amd/_abi.py is generated from include/boojum_hip.h (tools/gen_py_abi.py): every symbol the header declares as
# name -> (restype, argtypes), its structs, callback types, enumerators and defines.  The names below are the binding's own.
_SIGNATURES = _abi.SIGNATURES
ABI_VERSION = _abi.BJ_ABI_VERSION
RCCL_UNIQUE_ID_BYTES = _abi.BJ_RCCL_UNIQUE_ID_BYTES
DeepSet = _abi.bj_deep_set                 # one opening set of bj_deep_quotient_accumulate_sets
_GateDesc, _Circuit, _ProofConfig = _abi.bj_gate_desc, _abi.bj_circuit, _abi.bj_proof_config
_Comm, _ALL_GATHER_FN, _ALL_GATHER_STREAM_FN = _abi.bj_comm, _abi.bj_comm_all_gather, _abi.bj_comm_all_gather_stream
_HOST_EXCHANGE_FN = _abi.bj_host_exchange_fn
_VerifyReport, _UnsatReport, _CopyReport = _abi.bj_verify_report, _abi.bj_unsat_report, _abi.bj_copy_report
_UnsatEntry = _abi_diag.bj_unsat_entry      # include/boojum_hip_diag.h: diagnostics beside the ABI, generated like _abi.py


class BoojumHipError(RuntimeError):
    pass


def lib_path():
    # BOOJUM_HIP_LIB lets tuning experiments point at an alternative build of the SAME library (never a fallback)
    return os.environ.get("BOOJUM_HIP_LIB") or os.path.join(_HERE, "libboojum_hip.so")


def exported_symbols():
    return sorted(_SIGNATURES)


_lib = None


def load_library():
    """dlopen libboojum_hip.so; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise BoojumHipError("%s is missing: run `python -m era_boojum_amd.build` (hipcc, gfx950). "
                                 "There is no CPU fallback." % path)
        lib = C.CDLL(path)
        for name, (res, args) in list(_SIGNATURES.items()) + list(_abi_diag.SIGNATURES.items()):
            fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        if lib.bj_abi_version() != ABI_VERSION:     # a library built from another header than the one _abi.py was generated from
            raise BoojumHipError("%s has ABI version %d, this binding was generated for %d: rebuild (python -m era_boojum_amd.build)"
                                 % (path, lib.bj_abi_version(), ABI_VERSION))
        _lib = lib
    return _lib


def _np_ptr(a):
    assert isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One per GPU: wraps bj_ctx (device, stream, twiddle cache, scratch)."""

    def __init__(self, device=0, stream=None):
        self._lib = load_library()
        self.device = int(device)
        h = C.c_void_p()
        rc = self._lib.bj_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise BoojumHipError("bj_ctx_create(device=%d) failed: %s" % (device, self._lib.bj_status_string(rc).decode()))
        self._h = h
        if stream is not None:
            self.set_stream(stream)

    def gate_program_eval(self, program, d_vars, var_stride, d_consts, const_stride, reps, rep_var_stride, rep_const_stride,
                          n_points, d_terms):
        """bj_gate_program_eval: raw terms of a seam-S3 gate program at n_points points."""
        self._check(self._lib.bj_gate_program_eval(self._h, C.byref(program.struct), C.c_void_p(d_vars), var_stride,
                                                   C.c_void_p(d_consts) if d_consts else None, const_stride, reps, rep_var_stride,
                                                   rep_const_stride, n_points, C.c_void_p(d_terms)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bj_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise BoojumHipError("%s: %s" % (self._lib.bj_status_string(rc).decode(),
                                             self._lib.bj_last_error(self._h).decode()))

    # -- plumbing
    def set_tree_hasher(self, hasher):
        """BJ_HASHER_POSEIDON2 (default), BJ_HASHER_BLAKE2S, BJ_HASHER_KECCAK256 or BJ_HASHER_POSEIDON (v1): hasher of the
        merkle_tree_* / fri calls on this context."""
        self._check(self._lib.bj_ctx_set_tree_hasher(self._h, int(hasher)))

    def set_stream(self, stream_handle):
        self._check(self._lib.bj_ctx_set_stream(self._h, C.c_void_p(stream_handle)))

    def sync(self):
        self._check(self._lib.bj_sync(self._h))

    def release_workspace(self):
        """Give the proof workspace (arena, NTT scratch, host-witness staging) back to the device allocator."""
        self._check(self._lib.bj_ctx_release_workspace(self._h))

    def lean_proofs(self, on=True):
        """Context manager: the proofs started inside it are lean (binding.lean_proofs; a process-wide switch)."""
        return lean_proofs(self._lib, on)

    def malloc(self, nbytes):
        p = C.c_void_p()
        self._check(self._lib.bj_malloc(self._h, nbytes, C.byref(p)))
        return p.value

    def free(self, dptr):
        self._check(self._lib.bj_free(self._h, C.c_void_p(dptr)))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        self._check(self._lib.bj_memcpy_h2d(self._h, C.c_void_p(dptr), _np_ptr(arr), arr.nbytes))

    def d2h(self, dptr, shape):
        out = np.empty(shape, dtype=np.uint64)
        self._check(self._lib.bj_memcpy_d2h(self._h, _np_ptr(out), C.c_void_p(dptr), out.nbytes))
        return out

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        d = self.malloc(arr.nbytes)
        self.h2d(d, arr)
        return d

    def witness_gather(self, d_placement, cols, log_n, d_values, n_values, d_cells):
        """bj_witness_gather (boojum_hip_diag.h), the kernel behind prove_values on device arrays: d_cells[i] =
        d_values[d_placement[i]] over a u32 placement [cols][n].  Returns True if a cell named a value at or beyond n_values."""
        bad = C.c_uint(0)
        self._check(self._lib.bj_witness_gather(self._h, C.c_void_p(d_placement), cols, log_n, C.c_void_p(d_values), n_values,
                                                C.c_void_p(d_cells), C.byref(bad)))
        return bool(bad.value)

    def witness_gather_sweep_cells(self):
        """bj_witness_gather_sweep_cells: the cells one sweep of the gather's grid covers on this device."""
        return int(self._lib.bj_witness_gather_sweep_cells(self._h))

    def timer_start(self):
        self._check(self._lib.bj_timer_start(self._h))

    def timer_stop_ms(self):
        ms = C.c_float()
        self._check(self._lib.bj_timer_stop_ms(self._h, C.byref(ms)))
        return ms.value

    # -- NTT family (device pointers)
    def ntt_forward_batch(self, d_in, d_out, log_n, n_cols, col_stride=None, coset=1):
        col_stride = (1 << log_n) if col_stride is None else col_stride
        self._check(self._lib.bj_ntt_forward_batch(self._h, d_in, d_out, log_n, n_cols, col_stride, coset))

    def intt_batch(self, d_in, d_out, log_n, n_cols, col_stride=None, coset=1):
        col_stride = (1 << log_n) if col_stride is None else col_stride
        self._check(self._lib.bj_intt_batch(self._h, d_in, d_out, log_n, n_cols, col_stride, coset))

    def lde_batch(self, d_mono, d_out, log_n, n_cols, log_lde, col_stride=None):
        col_stride = (1 << log_n) if col_stride is None else col_stride
        self._check(self._lib.bj_lde_batch(self._h, d_mono, col_stride, d_out, log_n, n_cols, log_lde))

    def lde_cosets_batch(self, d_mono, d_out, log_n, n_cols, log_lde, coset_begin, coset_count, col_stride=None):
        col_stride = (1 << log_n) if col_stride is None else col_stride
        self._check(self._lib.bj_lde_cosets_batch(self._h, d_mono, col_stride, d_out, log_n, n_cols, log_lde,
                                                  coset_begin, coset_count))

    def monomials_tiled(self, log_n):
        """True when bj_prove keeps the monomials of 2^log_n-row traces in the tiled layout (include/boojum_hip.h)."""
        return bool(self._lib.bj_monomials_tiled(log_n))

    def intt_batch_tiled(self, d_in, d_out, log_n, n_cols, col_stride=None):
        col_stride = (1 << log_n) if col_stride is None else col_stride
        self._check(self._lib.bj_intt_batch_tiled(self._h, d_in, d_out, log_n, n_cols, col_stride))

    def lde_cosets_batch_tiled(self, d_mono, d_out, log_n, n_cols, log_lde, coset_begin, coset_count, col_stride=None):
        col_stride = (1 << log_n) if col_stride is None else col_stride
        self._check(self._lib.bj_lde_cosets_batch_tiled(self._h, d_mono, col_stride, d_out, log_n, n_cols, log_lde,
                                                        coset_begin, coset_count))

    def tiled_permute_batch(self, d_in, d_out, log_n, n_cols, to_tiled, col_stride=None):
        col_stride = (1 << log_n) if col_stride is None else col_stride
        self._check(self._lib.bj_tiled_permute_batch(self._h, d_in, d_out, log_n, n_cols, col_stride, 1 if to_tiled else 0))

    def trace_to_lde_batch(self, d_cols, d_out, log_n, n_cols, log_lde, col_stride=None):
        col_stride = (1 << log_n) if col_stride is None else col_stride
        self._check(self._lib.bj_trace_to_lde_batch(self._h, d_cols, col_stride, d_out, log_n, n_cols, log_lde))

    def bitreverse_batch(self, d_in, d_out, log_n, n_cols, col_stride=None):
        col_stride = (1 << log_n) if col_stride is None else col_stride
        self._check(self._lib.bj_bitreverse_batch(self._h, d_in, d_out, log_n, n_cols, col_stride))

    def canonicalize(self, d, n):
        self._check(self._lib.bj_canonicalize(self._h, d, n))

    # -- seam S2: second round and quotient terms on device columns (pointers are device addresses, challenges (c0, c1) tuples)
    @staticmethod
    def _e2(x):
        return np.array([int(x[0]), int(x[1])], dtype=np.uint64)

    def copy_perm_stage2(self, d_vars, var_stride, d_sigmas, sig_stride, non_residues, num_vars, chunk, log_n, beta, gamma, d_z,
                         d_partials):
        nr = np.ascontiguousarray(non_residues, dtype=np.uint64)
        self._check(self._lib.bj_copy_perm_stage2(self._h, d_vars, var_stride, d_sigmas, sig_stride, _np_ptr(nr), num_vars, chunk,
                                                  log_n, _np_ptr(self._e2(beta)), _np_ptr(self._e2(gamma)), d_z, d_partials))

    def sigmas_from_placement(self, d_placement, num_vars, log_n, non_residues, d_sigmas, place_stride=None, sig_stride=None):
        """bj_sigmas_from_placement: d_placement [num_vars][n] copy-hint cells (bit 63 = placeholder) -> d_sigmas [num_vars][n]."""
        nr = np.array([int(k) for k in non_residues], dtype=np.uint64)
        n = 1 << log_n
        self._check(self._lib.bj_sigmas_from_placement(self._h, d_placement, place_stride or n, num_vars, log_n, _np_ptr(nr), d_sigmas,
                                                       sig_stride or n))

    def sigma_cells(self, d_sigmas, num_vars, log_n, non_residues, d_cells, sig_stride=None, cell_stride=None):
        """bj_sigma_cells, the inverse of sigmas_from_placement: d_sigmas [num_vars][n] u64 -> d_cells [num_vars][n] u32, the cell
        j * n + r each word k_j * omega^r names, 0xFFFFFFFF for a word in no coset.  Returns (first_invalid, num_invalid):
        the smallest key row * num_vars + column of such a word (None when there is none) and their number."""
        n = 1 << log_n
        nr = np.ascontiguousarray(non_residues[:num_vars], dtype=np.uint64)
        first, count = C.c_uint64(), C.c_uint64()
        self._check(self._lib.bj_sigma_cells(self._h, d_sigmas, sig_stride or n, num_vars, log_n, _np_ptr(nr), d_cells, cell_stride or n,
                                             C.byref(first), C.byref(count)))
        return (None if first.value == NO_CELL_KEY else int(first.value)), int(count.value)

    def lookup_polys(self, d_lvars, var_stride, d_table_id, d_tables, table_stride, d_mult, reps, width, log_n, beta, gamma, d_A, d_B):
        self._check(self._lib.bj_lookup_polys(self._h, d_lvars, var_stride, d_table_id, d_tables, table_stride, d_mult, reps, width,
                                              log_n, _np_ptr(self._e2(beta)), _np_ptr(self._e2(gamma)), d_A, d_B))

    def lookup_multiplicities(self, d_lvars, var_stride, d_table_id, d_tables, table_stride, reps, width, log_n, d_mult):
        """bj_lookup_multiplicities: the multiplicity column [n] counted from raw columns (those of lookup_polys) into d_mult."""
        self._check(self._lib.bj_lookup_multiplicities(self._h, d_lvars, var_stride, d_table_id, d_tables, table_stride, reps, width,
                                                       log_n, d_mult))

    def quotient_gates(self, d_vars, var_stride, num_gp_vars, d_consts, const_stride, num_constant_cols, gates, alphas, num_points,
                       d_out0, d_out1):
        descs = gate_desc_array(gates)
        al = np.ascontiguousarray(np.array(alphas, dtype=np.uint64).reshape(-1))
        self._check(self._lib.bj_quotient_gates(self._h, d_vars, var_stride, num_gp_vars, d_consts, const_stride, num_constant_cols,
                                                C.cast(descs, C.c_void_p), len(gates), _np_ptr(al) if al.size else None,
                                                num_points, d_out0, d_out1))

    def quotient_lookup(self, d_lvars, var_stride, d_table_id, d_tables, table_stride, d_mult, d_A, d_B, s2_stride, reps, width,
                        beta, gamma, alphas, num_points, d_out0, d_out1):
        al = np.ascontiguousarray(np.array(alphas, dtype=np.uint64).reshape(-1))
        self._check(self._lib.bj_quotient_lookup(self._h, d_lvars, var_stride, d_table_id, d_tables, table_stride, d_mult, d_A, d_B,
                                                 s2_stride, reps, width, _np_ptr(self._e2(beta)), _np_ptr(self._e2(gamma)),
                                                 _np_ptr(al), num_points, d_out0, d_out1))

    def quotient_copy_perm(self, d_vars, var_stride, d_sigmas, sig_stride, d_stage2, s2_stride, non_residues, num_vars, chunk, log_n,
                           log_lde, beta, gamma, alphas, num_points, first_point, d_out0, d_out1):
        nr = np.ascontiguousarray(non_residues, dtype=np.uint64)
        al = np.ascontiguousarray(np.array(alphas, dtype=np.uint64).reshape(-1))
        self._check(self._lib.bj_quotient_copy_perm(self._h, d_vars, var_stride, d_sigmas, sig_stride, d_stage2, s2_stride,
                                                    _np_ptr(nr), num_vars, chunk, log_n, log_lde, _np_ptr(self._e2(beta)),
                                                    _np_ptr(self._e2(gamma)), _np_ptr(al), num_points, first_point, d_out0, d_out1))

    def combine_residues(self, d_residues, world, residue_len, num_cols, moduli, d_out):
        """bj_combine_residues: [world][num_cols][E] residues T mod (x^E - a_i) -> [num_cols][world * E] coefficients of T."""
        a = np.ascontiguousarray(np.array([int(v) for v in moduli], dtype=np.uint64))
        self._check(self._lib.bj_combine_residues(self._h, d_residues, world, residue_len, num_cols, _np_ptr(a), d_out))

    # every BJ_FIELD_* operator of the header under its name in lower case ("add", ..., "w16_butterfly"), in header order
    FIELD_OPS = {{"acc160x2_e2": "acc_ext2"}.get(name, name): value for name, value in
                 ((k[len("BJ_FIELD_"):].lower(), v) for k, v in vars(_abi).items() if k.startswith("BJ_FIELD_"))}
    # operator -> (parts of n words in d_a, in d_b (0: unused), in d_out); every other operator is (1, 1, 1) or unary (1, 0, 1)
    FIELD_OP_PARTS = {"ext2_mul": (2, 2, 2), "ext2_mul_lazy": (2, 2, 2), "butterfly": (2, 1, 2), "addsub": (2, 0, 2), "acc160": (3, 2, 1),
                      "acc_ext2": (2, 2, 2), "w16_butterfly": (2, 1, 2), "ext2_inverse": (2, 0, 2), "ext2_inverse_chain": (2, 0, 2)}

    def field_op(self, op, a, b=None):
        """bj_field_op_batch on host arrays (uploads, runs, downloads): elementwise Goldilocks / F_p^2 operators.  An operand of
        several parts is [parts][n] (or flat); the result has the operand's shape, for acc160 (three parts in, one out) it is [n]."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        pa, pb, po = self.FIELD_OP_PARTS.get(op, (1, 1, 1))
        n = a.size // pa
        if a.size != n * pa:
            raise ValueError("field_op %s: the first operand holds %d parts of n words" % (op, pa))
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.uint64)
            if pb and b.size != n * pb:     # the kernel reads pb parts of n words: a short operand would be read past its end
                raise ValueError("field_op %s: the second operand holds %d parts of %d words" % (op, pb, n))
        da = self.upload(a)
        db = self.upload(b) if b is not None else None
        do = self.malloc(a.nbytes)
        try:
            self._check(self._lib.bj_field_op_batch(self._h, self.FIELD_OPS[op], C.c_void_p(da), C.c_void_p(db) if db else None,
                                                    C.c_void_p(do), n))
            return self.d2h(do, a.shape if po == pa else (n,))
        finally:
            for p in (da, db, do):
                if p:
                    self.free(p)

    # -- host convenience
    def ntt_forward_host(self, arr, coset=1):
        a = np.ascontiguousarray(arr, dtype=np.uint64).copy()
        a2 = a.reshape(-1, a.shape[-1])
        self._check(self._lib.bj_ntt_forward_host(self._h, _np_ptr(a2), a2.shape[1].bit_length() - 1, a2.shape[0], coset))
        return a

    def intt_host(self, arr, coset=1):
        a = np.ascontiguousarray(arr, dtype=np.uint64).copy()
        a2 = a.reshape(-1, a.shape[-1])
        self._check(self._lib.bj_intt_host(self._h, _np_ptr(a2), a2.shape[1].bit_length() - 1, a2.shape[0], coset))
        return a

    # -- Merkle
    def merkle_tree_digests(self, num_leaves, cap_size):
        return self._lib.bj_merkle_tree_digests(num_leaves, cap_size)

    def merkle_tree_build(self, d_cols, col_stride, n_cols, num_leaves, cap_size, d_tree):
        self._check(self._lib.bj_merkle_tree_build(self._h, d_cols, col_stride, n_cols, num_leaves, cap_size, d_tree))

    def merkle_tree_build_ptrs(self, col_ptrs, num_leaves, cap_size, d_tree):
        arr = (C.c_void_p * len(col_ptrs))(*col_ptrs)
        self._check(self._lib.bj_merkle_tree_build_ptrs(self._h, arr, len(col_ptrs), num_leaves, cap_size, d_tree))

    def merkle_tree_build_chunked(self, d_c0, d_c1, length, log_elems_per_leaf, cap_size, d_tree):
        self._check(self._lib.bj_merkle_tree_build_chunked(self._h, d_c0, d_c1, length, log_elems_per_leaf, cap_size, d_tree))

    def merkle_tree_nodes(self, d_tree, num_leaves, cap_size):
        self._check(self._lib.bj_merkle_tree_nodes(self._h, d_tree, num_leaves, cap_size))

    def merkle_tree_cap(self, d_tree, num_leaves, cap_size):
        cap = np.empty((cap_size, 4), dtype=np.uint64)
        self._check(self._lib.bj_merkle_tree_cap(self._h, d_tree, num_leaves, cap_size, _np_ptr(cap)))
        return cap

    def merkle_tree_proof(self, d_tree, num_leaves, cap_size, idx):
        depth = (num_leaves // cap_size).bit_length() - 1
        leaf = np.empty(4, dtype=np.uint64)
        path = np.empty((max(depth, 1), 4), dtype=np.uint64)
        self._check(self._lib.bj_merkle_tree_proof(self._h, d_tree, num_leaves, cap_size, idx, _np_ptr(leaf), _np_ptr(path)))
        return leaf, path[:depth]

    def poseidon2_permute(self, d_states, n_states):
        self._check(self._lib.bj_poseidon2_permute(self._h, d_states, n_states))

    def poseidon_permute(self, d_states, n_states):
        """The Poseidon (v1) permutation (BJ_HASHER_POSEIDON / BJ_TRANSCRIPT_POSEIDON) on n_states 12-word device states."""
        self._check(self._lib.bj_poseidon_permute(self._h, d_states, n_states))

    # -- FRI
    def fri_fold(self, d_c0, d_c1, length, d_o0, d_o1, log_full, coset_inv, ch):
        self._check(self._lib.bj_fri_fold(self._h, d_c0, d_c1, length, d_o0, d_o1, log_full, coset_inv, ch[0], ch[1]))

    # -- openings
    def barycentric_weights(self, log_n, coset, at, d_w0, d_w1):
        a = np.array(at, dtype=np.uint64)
        self._check(self._lib.bj_barycentric_weights(self._h, log_n, coset, _np_ptr(a), d_w0, d_w1))

    def barycentric_eval_batch(self, col_ptrs, log_n, d_w0, d_w1):
        arr = (C.c_void_p * len(col_ptrs))(*col_ptrs)
        out = np.empty((len(col_ptrs), 2), dtype=np.uint64)
        self._check(self._lib.bj_barycentric_eval_batch(self._h, arr, len(col_ptrs), log_n, d_w0, d_w1, _np_ptr(out)))
        return out

    def deep_quotient_accumulate(self, sources, values, challenges, at, log_n, log_lde, d_dst0, d_dst1, accumulate=True):
        """sources: list of (d_c0, d_c1_or_None) device pointers of LDE columns."""
        k = len(sources)
        p0 = (C.c_void_p * k)(*[a for a, _ in sources])
        p1 = (C.c_void_p * k)(*[b for _, b in sources])
        v = np.ascontiguousarray(np.array(values, dtype=np.uint64).reshape(-1))
        ch = np.ascontiguousarray(np.array(challenges, dtype=np.uint64).reshape(-1))
        a = np.array(at, dtype=np.uint64)
        self._check(self._lib.bj_deep_quotient_accumulate(self._h, p0, p1, k, _np_ptr(v), _np_ptr(ch), _np_ptr(a), log_n,
                                                          log_lde, d_dst0, d_dst1, int(bool(accumulate))))

    @staticmethod
    def _deep_args(sources, values, challenges, at):
        k = len(sources)
        p0 = (C.c_void_p * k)(*[a for a, _ in sources])
        p1 = (C.c_void_p * k)(*[b for _, b in sources])
        v = np.ascontiguousarray(np.array(values, dtype=np.uint64).reshape(-1))
        ch = np.ascontiguousarray(np.array(challenges, dtype=np.uint64).reshape(-1))
        return p0, p1, k, v, ch, np.array(at, dtype=np.uint64)

    def deep_quotient_accumulate_range(self, sources, values, challenges, at, log_n, log_lde, first, count, d_dst0, d_dst1,
                                       accumulate=True):
        """The same on the LDE indices [first, first + count): every pointer addresses the `count` entries of that range."""
        p0, p1, k, v, ch, a = self._deep_args(sources, values, challenges, at)
        self._check(self._lib.bj_deep_quotient_accumulate_range(self._h, p0, p1, k, _np_ptr(v), _np_ptr(ch), _np_ptr(a), log_n,
                                                                log_lde, first, count, d_dst0, d_dst1, int(bool(accumulate))))

    def deep_quotient_accumulate_sets(self, sets, log_n, log_lde, first, count, d_dst0, d_dst1, accumulate=True):
        """sets: list of (sources, values, challenges, at), each as in deep_quotient_accumulate; one pass for all of them."""
        keep = [self._deep_args(*s) for s in sets]
        arr = (DeepSet * max(len(sets), 1))()
        for t, (p0, p1, k, v, ch, a) in enumerate(keep):
            arr[t] = DeepSet(p0, p1, k, v.ctypes.data_as(u64p), ch.ctypes.data_as(u64p), a.ctypes.data_as(u64p))
        self._check(self._lib.bj_deep_quotient_accumulate_sets(self._h, C.cast(arr, C.c_void_p), len(sets), log_n, log_lde, first,
                                                               count, d_dst0, d_dst1, int(bool(accumulate))))

    def linear_combination(self, sources, challenges, n, d_out0, d_out1):
        """out = sum_k ch_k * src_k over n entries; sources: list of (d_c0, d_c1_or_None) device pointers."""
        k = len(sources)
        p0 = (C.c_void_p * k)(*[a for a, _ in sources])
        p1 = (C.c_void_p * k)(*[b for _, b in sources])
        ch = np.ascontiguousarray(np.array(challenges, dtype=np.uint64).reshape(-1))
        self._check(self._lib.bj_linear_combination(self._h, p0, p1, k, _np_ptr(ch), n, d_out0, d_out1))

    def eval_monomials_at(self, d_mono, col_stride, n_cols, log_n, log_lde, d_idx, n_idx, d_out, tiled=False, first_leaf=0):
        """bj_eval_monomials_at: d_out[j][c] = the polynomial of column c at the point of leaf first_leaf + d_idx[j] of the
        2^(log_n + log_lde) LDE domain (d_idx: n_idx u64 on the device), from natural-order or tiled monomials."""
        self._check(self._lib.bj_eval_monomials_at(self._h, d_mono, col_stride, n_cols, log_n, log_lde, 1 if tiled else 0, first_leaf,
                                                   d_idx, n_idx, d_out))

    def merkle_leaves_absorb(self, d_cols, col_stride, n_cols, num_leaves, d_capacity, d_digests, first, last):
        """bj_merkle_leaves_absorb: one group of columns into the leaf sponges of the context's algebraic tree hasher; the capacity
        words travel through d_capacity ([4][num_leaves]) between groups, the last group writes d_digests ([num_leaves][4])."""
        self._check(self._lib.bj_merkle_leaves_absorb(self._h, d_cols, col_stride, n_cols, num_leaves, d_capacity, d_digests,
                                                      1 if first else 0, 1 if last else 0))

    def pow_search(self, pow_runner, seed5, pow_bits, base, count):
        """bj_pow_search: the smallest nonce of [base, base + count) that the runner (BJ_POW_*) accepts for the five seed words at
        pow_bits, or 2^64 - 1 when the window holds none."""
        seed = np.ascontiguousarray(seed5, dtype=np.uint64)
        if seed.size != 5:
            raise ValueError("pow_search: the seed is five words")
        out = C.c_uint64()
        self._check(self._lib.bj_pow_search(self._h, int(pow_runner), _np_ptr(seed), pow_bits, base, count, C.byref(out)))
        return int(out.value)

    def fri_fold_step(self, d_c0, d_c1, length, k, d_o0, d_o1, log_full, coset_inv, ch):
        self._check(self._lib.bj_fri_fold_step(self._h, d_c0, d_c1, length, k, d_o0, d_o1, log_full, coset_inv, ch[0], ch[1]))

    def fri_prove(self, d_c0, d_c1, log_n, log_lde, schedule, cap_size, transcript):
        """do_fri on the device; returns a FriProof handle (oracles stay in HBM)."""
        sched = (C.c_uint32 * len(schedule))(*schedule)
        h = C.c_void_p()
        self._check(self._lib.bj_fri_prove(self._h, d_c0, d_c1, log_n, log_lde, sched, len(schedule), cap_size,
                                           transcript._h, C.byref(h)))
        return FriProof(self, h, cap_size, list(schedule))


class Transcript:
    """Host-side Poseidon2 Fiat–Shamir transcript of the product (bj_transcript_*); needs no GPU."""

    def __init__(self, kind=_abi.BJ_TRANSCRIPT_POSEIDON2):
        """kind: BJ_TRANSCRIPT_POSEIDON2 (the default) or BJ_TRANSCRIPT_POSEIDON (Poseidon v1)."""
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.bj_transcript_create(int(kind), C.byref(h))
        if rc != 0:
            raise BoojumHipError("bj_transcript_create failed: %d" % rc)
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.bj_transcript_destroy(self._h)
            self._h = None

    def absorb(self, els):
        a = np.ascontiguousarray(np.asarray(els, dtype=np.uint64)).reshape(-1)
        if a.size:
            rc = self._lib.bj_transcript_absorb(self._h, _np_ptr(a), a.size)
            if rc != 0:
                raise BoojumHipError("bj_transcript_absorb failed: %d" % rc)

    def absorb_cap(self, cap):
        a = np.ascontiguousarray(np.asarray(cap, dtype=np.uint64)).reshape(-1)
        if a.size:
            rc = self._lib.bj_transcript_absorb_cap(self._h, _np_ptr(a), a.size)
            if rc != 0:
                raise BoojumHipError("bj_transcript_absorb_cap failed: %d" % rc)

    def challenge(self):
        out = C.c_uint64()
        rc = self._lib.bj_transcript_challenge(self._h, C.byref(out))
        if rc != 0:
            raise BoojumHipError("bj_transcript_challenge failed: %d" % rc)
        return out.value

    def challenge_ext(self):
        return (self.challenge(), self.challenge())

    def query_index(self, log_n, log_lde):
        out = C.c_uint64()
        rc = self._lib.bj_transcript_query_index(self._h, log_n, log_lde, C.byref(out))
        if rc != 0:
            raise BoojumHipError("bj_transcript_query_index failed: %d" % rc)
        return out.value


def fri_schedule(security_bits, cap_size, pow_bits, rate_log2, initial_degree_log2):
    """compute_fri_schedule (prover.rs:2281-2372) through the C ABI: (new_pow_bits, num_queries, schedule, final_degree)."""
    lib = load_library()
    sched = (C.c_uint32 * 32)()
    new_pow, nq, ln, fd = C.c_uint32(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    rc = lib.bj_fri_schedule(security_bits, cap_size, pow_bits, rate_log2, initial_degree_log2, C.byref(new_pow),
                             C.byref(nq), sched, C.byref(ln), C.byref(fd))
    if rc != 0:
        raise BoojumHipError("bj_fri_schedule failed: %d" % rc)
    return new_pow.value, nq.value, [int(sched[i]) for i in range(ln.value)], fd.value


class FriProof:
    def __init__(self, ctx, handle, cap_size, schedule):
        self._ctx, self._h, self.cap_size, self.schedule = ctx, handle, cap_size, schedule
        self._lib = ctx._lib

    def close(self):
        if self._h:
            self._lib.bj_fri_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_oracles(self):
        return self._lib.bj_fri_num_oracles(self._h)

    @property
    def final_degree(self):
        return self._lib.bj_fri_final_degree(self._h)

    def cap(self, i):
        out = np.empty((self.cap_size, 4), dtype=np.uint64)
        self._ctx._check(self._lib.bj_fri_cap(self._h, i, _np_ptr(out)))
        return out

    def challenge(self, i):
        out = np.empty(2, dtype=np.uint64)
        self._ctx._check(self._lib.bj_fri_challenge(self._h, i, _np_ptr(out)))
        return (int(out[0]), int(out[1]))

    def final_monomials(self):
        fd = self.final_degree
        c0, c1 = np.empty(fd, dtype=np.uint64), np.empty(fd, dtype=np.uint64)
        self._ctx._check(self._lib.bj_fri_final_monomials(self._h, _np_ptr(c0), _np_ptr(c1)))
        return c0, c1

    def query(self, oracle, index, oracle_len):
        e = 1 << self.schedule[oracle]
        leaf = np.empty(2 * e, dtype=np.uint64)
        depth = ((oracle_len >> self.schedule[oracle]) // self.cap_size).bit_length() - 1
        path = np.empty((max(depth, 1), 4), dtype=np.uint64)
        self._ctx._check(self._lib.bj_fri_query(self._ctx._h, self._h, oracle, index, _np_ptr(leaf), _np_ptr(path)))
        return leaf, path[:depth]


def gate_desc_array(gates):
    """bj_gate_desc[] for gates with the attributes of synthetic.Gate (kind, path, reps, var_stride, const_stride, num_terms); an
    op-list gate (BJ_GATE_PROGRAM) points at its program, which the caller keeps alive for the call."""
    arr = (_GateDesc * len(gates))()
    for i, g in enumerate(gates):
        arr[i].kind, arr[i].path_len = int(g.kind), len(g.path)
        for b, bit in enumerate(g.path):
            arr[i].path[b] = 1 if bit else 0
        arr[i].num_repetitions, arr[i].var_stride, arr[i].const_stride = int(g.reps), int(g.var_stride), int(g.const_stride)
        arr[i].num_terms, arr[i].program = int(g.num_terms), None
        if int(g.kind) == _abi.BJ_GATE_PROGRAM and getattr(g, "program", None) is not None:
            arr[i].program = C.pointer(g.program.struct)
    return arr


STAGE_NAMES = ["witness_lde_and_tree", "second_stage", "quotient_work_and_lde", "openings_at_z",
               "batched_fri_opening_computation", "fri", "queries"]


def rccl_unique_id():
    """bj_rccl_unique_id: 128 opaque bytes made by rank 0 and handed to every rank of the proof."""
    buf = C.create_string_buffer(RCCL_UNIQUE_ID_BYTES)
    rc = load_library().bj_rccl_unique_id(buf)
    if rc != 0:
        raise BoojumHipError("bj_rccl_unique_id failed: %s" % load_library().bj_status_string(rc).decode())
    return buf.raw


class RcclComm:
    """The in-library transport (bj_comm_rccl_create): ncclAllGather on the context's stream, directly on the prover's buffers.
    `unique_id` = the 128 bytes of rccl_unique_id() from rank 0 (ship them with any channel, e.g. torch.distributed's
    broadcast_object_list).  Collective: every rank of the proof constructs it."""

    def __init__(self, ctx, unique_id, rank, world):
        self._ctx, self._lib = ctx, ctx._lib
        self.rank, self.world = rank, world
        self.struct = _Comm()
        ctx._check(self._lib.bj_comm_rccl_create(ctx._h, C.c_char_p(unique_id), rank, world, C.byref(self.struct)))

    @property
    def calls(self):
        return self._stats()[0]

    @property
    def bytes(self):
        return self._stats()[1]

    def _stats(self):
        a, b = C.c_size_t(), C.c_size_t()
        self._lib.bj_comm_rccl_stats(C.byref(self.struct), C.byref(a), C.byref(b))
        return a.value, b.value

    def all_gather(self, d_send, d_recv, nbytes, stream=None):
        """One all-gather through the transport's own entry (bj_comm.all_gather_stream when `stream` is given, the blocking
        bj_comm.all_gather otherwise): what the sharded prover calls, exposed for self-tests."""
        if stream is not None:
            rc = self.struct.all_gather_stream(self.struct.user, C.c_void_p(d_send), C.c_void_p(d_recv), nbytes, C.c_void_p(stream))
        else:
            rc = self.struct.all_gather(self.struct.user, C.c_void_p(d_send), C.c_void_p(d_recv), nbytes)
        if rc != 0:
            raise BoojumHipError("RcclComm.all_gather failed (%d)" % rc)

    def close(self):
        if self.struct.user:
            self._lib.bj_comm_rccl_destroy(C.byref(self.struct))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReplayComm:
    """The recorded-peer transport (bj_comm_replay_create): one rank of a `world`-rank proof alone on its GPU, every all-gather
    answered by a device copy of what that collective gathered in a real run.  `recorded` = [(device pointer, bytes)] in call
    order: n_setup buffers for the setup's collectives, then the buffers of one proof (used cyclically)."""

    def __init__(self, ctx, rank, world, recorded, n_setup=0, verify=False, keepalive=None, capture=None):
        """keepalive: whatever owns the recorded device buffers (e.g. the list of torch tensors) — held for the life of the comm.
        capture = (device pointer, capacity in bytes): the first collective past the recorded ones is not served; this rank's
        contribution is copied there and the call fails, ending the proof (bj_comm_replay_capture); `captured` then says how many
        bytes were taken."""
        self._ctx, self._lib = ctx, ctx._lib
        self.rank, self.world = rank, world
        self._keep = keepalive
        self._ptrs = (C.c_void_p * max(1, len(recorded)))(*[p for p, _ in recorded])
        self._sizes = (C.c_size_t * max(1, len(recorded)))(*[b for _, b in recorded])
        self.struct = _Comm()
        ctx._check(self._lib.bj_comm_replay_create(ctx._h, rank, world, self._ptrs, self._sizes, n_setup, len(recorded) - n_setup,
                                                   1 if verify else 0, C.byref(self.struct)))
        if capture is not None:
            ctx._check(self._lib.bj_comm_replay_capture(C.byref(self.struct), C.c_void_p(capture[0]), capture[1]))

    @property
    def captured(self):
        b = C.c_size_t()
        self._lib.bj_comm_replay_captured(C.byref(self.struct), C.byref(b))
        return int(b.value)

    def stats(self):
        a, b, m = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._lib.bj_comm_replay_stats(C.byref(self.struct), C.byref(a), C.byref(b), C.byref(m))
        return a.value, b.value, m.value

    calls = property(lambda self: self.stats()[0])
    bytes = property(lambda self: self.stats()[1])
    mismatches = property(lambda self: self.stats()[2])

    def close(self):
        if self.struct.user:
            self._lib.bj_comm_replay_destroy(C.byref(self.struct))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ThreadGroup:
    """`world` ranks of ONE sharded proof as threads of this process, all on one GPU (each with its own Context = its own stream
    and arena): the all-gather is a rendezvous of the threads and device-to-device copies.  Functionally the sharded prover as
    it runs over RCCL (the ranks time-slice the GPU, so its timing means nothing); with record=True rank 0 keeps a copy of
    every gathered buffer — what ReplayComm then serves to one rank running alone (bench.py --replay-world)."""

    def __init__(self, world, record=False):
        import threading
        self.world, self.record = world, record
        self._barrier = threading.Barrier(world)
        self._posted = [None] * world
        self.recorded = []            # [(torch uint8 tensor)] in call order (rank 0's view)
        self.marks = []               # len(recorded) at the moments mark() was called
        self.error = None

    def mark(self):
        self.marks.append(len(self.recorded))

    def comm(self, ctx, rank):
        return _ThreadComm(self, ctx, rank)


class _ThreadComm:
    def __init__(self, group, ctx, rank):
        self._g, self._ctx, self.rank, self.world = group, ctx, rank, group.world
        self.calls, self.bytes = 0, 0
        self._fn = _ALL_GATHER_FN(self._all_gather)
        self.struct = _Comm(rank, group.world, self._fn, None, _ALL_GATHER_STREAM_FN())

    def _all_gather(self, _user, d_send, d_recv, nbytes):
        g = self._g
        try:
            g._posted[self.rank] = (d_send, nbytes)
            g._barrier.wait()                   # every rank's stream is idle here (the library's contract for this entry)
            ctx, lib = self._ctx, self._ctx._lib
            for r in range(self.world):
                src, nb = g._posted[r]
                if nb != nbytes:
                    raise BoojumHipError("ranks disagree on the size of a collective (%d vs %d bytes)" % (nb, nbytes))
                ctx._check(lib.bj_memcpy_d2d(ctx._h, C.c_void_p(d_recv + r * nbytes), C.c_void_p(src), nbytes))
            if g.record and self.rank == 0:
                import torch
                t = torch.empty(nbytes * self.world, dtype=torch.uint8, device=torch.device("cuda", ctx.device))
                ctx._check(lib.bj_memcpy_d2d(ctx._h, C.c_void_p(t.data_ptr()), C.c_void_p(d_recv), nbytes * self.world))
                g.recorded.append(t)
            g._barrier.wait()                   # nobody overwrites its send buffer before every peer has read it
            self.calls += 1
            self.bytes += nbytes * self.world
            return 0
        except Exception as e:                  # an exception must not unwind through the C frames
            import traceback
            traceback.print_exc()
            g.error = e
            try:
                g._barrier.abort()
            except Exception:
                pass
            return 1


class TorchComm:
    """bj_comm over torch.distributed: the all-gather the sharded prover asks the host for.

    The library hands over raw device pointers; they are copied (device to device) through torch-owned staging tensors
    so that the collective itself is torch.distributed's: backend nccl (= RCCL over xGMI) runs on the staging tensors
    directly, backend gloo (CPU tests, or several ranks sharing one GPU) bounces through host memory."""

    def __init__(self, ctx, group=None):
        import torch
        import torch.distributed as dist
        self._ctx, self._torch, self._dist, self._group = ctx, torch, dist, group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self._device = torch.device("cuda", ctx.device)
        self._on_device = dist.get_backend(group) == "nccl"
        self._send = self._recv = None
        self.calls, self.bytes = 0, 0
        self._fn = _ALL_GATHER_FN(self._all_gather)        # keep the trampoline alive
        self.struct = _Comm(self.rank, self.world, self._fn, None, _ALL_GATHER_STREAM_FN())

    def _staging(self, nbytes):
        t = self._torch
        if self._send is None or self._send.numel() < nbytes:
            self._send = t.empty(nbytes, dtype=t.uint8, device=self._device)
            self._recv = t.empty(nbytes * self.world, dtype=t.uint8, device=self._device)
        return self._send[:nbytes], self._recv[:nbytes * self.world]

    def _all_gather(self, _user, d_send, d_recv, nbytes):
        try:
            ctx, lib = self._ctx, self._ctx._lib
            send, recv = self._staging(nbytes)
            ctx._check(lib.bj_memcpy_d2d(ctx._h, C.c_void_p(send.data_ptr()), C.c_void_p(d_send), nbytes))
            if self._on_device:
                self._dist.all_gather_into_tensor(recv, send, group=self._group)
                self._torch.cuda.synchronize(self._device)
            else:
                h_send = send.cpu()
                h_recv = self._torch.empty(nbytes * self.world, dtype=self._torch.uint8)
                self._dist.all_gather_into_tensor(h_recv, h_send, group=self._group)
                recv.copy_(h_recv)
                self._torch.cuda.synchronize(self._device)
            ctx._check(lib.bj_memcpy_d2d(ctx._h, C.c_void_p(d_recv), C.c_void_p(recv.data_ptr()), nbytes * self.world))
            self.calls += 1
            self.bytes += nbytes * self.world
            return 0
        except Exception as e:  # an exception must not unwind through the C frames
            import traceback
            traceback.print_exc()
            self.error = e
            return 1


class PeerComm:
    """bj_comm_peer_create: full-mesh peer copies for the bulk exchanges of a sharded proof (every rank writes its contribution
    straight into every peer's receive buffer, mapped through HIP IPC), everything smaller through `base` (a TorchComm or RcclComm).
    The control channel — a blocking all-gather of a few host bytes — is torch.distributed on `ctrl_group` (default: the default
    group): host tensors over gloo, tiny device tensors over nccl.  Every rank of the proof constructs it."""

    def __init__(self, ctx, base, ctrl_group=None, bulk_threshold_bytes=1 << 20):
        import torch
        import torch.distributed as dist
        self._ctx, self._lib, self._base = ctx, ctx._lib, base
        self._torch, self._dist = torch, dist
        self.rank, self.world = base.rank, base.world
        # the control channel rides on the process group the host already has (no second rendezvous that could fail on its own):
        # host tensors over gloo, tiny device tensors over nccl (= RCCL)
        self._ctrl = ctrl_group
        self._on_device = dist.get_backend(ctrl_group) == "nccl"
        self._device = torch.device("cuda", ctx.device)
        self.error = None
        self._fn = _HOST_EXCHANGE_FN(self._exchange)             # keep the trampoline alive
        self.struct = _Comm()
        ctx._check(self._lib.bj_comm_peer_create(ctx._h, C.byref(base.struct), self._fn, None, bulk_threshold_bytes, C.byref(self.struct)))

    def _exchange(self, _user, h_send, h_recv, nbytes):
        try:
            t = self._torch
            send = t.frombuffer((C.c_ubyte * nbytes).from_address(h_send), dtype=t.uint8).clone()
            if self._on_device:
                d_send = send.to(self._device)
                d_recv = t.empty(nbytes * self.world, dtype=t.uint8, device=self._device)
                self._dist.all_gather_into_tensor(d_recv, d_send, group=self._ctrl)
                recv = d_recv.cpu()
            else:
                recv = t.empty(nbytes * self.world, dtype=t.uint8)
                self._dist.all_gather_into_tensor(recv, send, group=self._ctrl)
            C.memmove(h_recv, recv.data_ptr(), nbytes * self.world)
            return 0
        except Exception as e:  # an exception must not unwind through the C frames
            import traceback
            traceback.print_exc()
            self.error = e
            return 1

    def stats(self):
        a, b, c, d = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._lib.bj_comm_peer_stats(C.byref(self.struct), C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return {"bulk_calls": a.value, "bulk_bytes_received": b.value, "small_calls": c.value, "fallbacks": d.value}

    @property
    def calls(self):
        s = self.stats()
        return s["bulk_calls"] + s["small_calls"]

    @property
    def bytes(self):
        return self.stats()["bulk_bytes_received"] + getattr(self._base, "bytes", 0)

    def close(self):
        if self.struct.user:
            self._lib.bj_comm_peer_destroy(C.byref(self.struct))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def circuit_struct(c, from_dump=False):
    """bj_circuit for a circuit of era_boojum_amd.synthetic.Circuit shape, and the ctypes objects it points into (keep them alive
    for the call).  from_dump: paths, constant-column count, table-id column, quotient degree and non-residues are left to
    bj_setup_create_from_dump."""
    gates = (_GateDesc * len(c.gates))()
    for i, g in enumerate(c.gates):
        gates[i].kind = g.kind
        gates[i].path_len = 0 if from_dump else len(g.path)
        for b, bit in enumerate([] if from_dump else list(g.path)[:8]):
            gates[i].path[b] = 1 if bit else 0
        gates[i].num_repetitions, gates[i].var_stride, gates[i].const_stride, gates[i].num_terms = \
            g.reps, g.var_stride, g.const_stride, g.num_terms
        gates[i].wit_stride = getattr(g, "wit_stride", 0)
        prog = getattr(g, "program", None)       # seam S3: evaluate this gate from its op list (gate_program.py)
        if prog is not None and g.kind != _abi.BJ_GATE_POSEIDON_FLATTENED:     # whose program serves the host-side checks only
            gates[i].kind = _abi.BJ_GATE_PROGRAM
            gates[i].program = C.pointer(prog.struct)
    spec_list = list(getattr(c, "specialized_gates", []) or [])
    spec = (_GateDesc * max(1, len(spec_list)))()
    for i, g in enumerate(spec_list):                # gates over specialized columns: op lists, no selector
        spec[i].kind, spec[i].path_len = _abi.BJ_GATE_PROGRAM, 0
        spec[i].num_repetitions, spec[i].var_stride, spec[i].const_stride, spec[i].num_terms = g.reps, g.var_stride, g.const_stride, g.num_terms
        spec[i].program = C.pointer(g.program.struct)
    nr = np.array(c.non_residues, dtype=np.uint64)
    cols = (C.c_uint * max(1, len(c.public_inputs)))(*[p[0] for p in c.public_inputs])
    rows = (C.c_uint * max(1, len(c.public_inputs)))(*[p[1] for p in c.public_inputs])
    cc = _Circuit(c.log_n, c.num_vars, c.num_gp_vars, int(getattr(c, "num_witness_cols", 0)), 0 if from_dump else c.num_constant_cols,
                  c.lookup_width, c.lookup_reps, 0 if from_dump else c.table_id_col, 0 if from_dump else c.quotient_degree, len(c.gates), gates,
                  None if from_dump else nr.ctypes.data_as(C.POINTER(C.c_uint64)), len(c.public_inputs),
                  cols, rows, len(spec_list), spec if spec_list else None)
    return cc, (gates, spec, nr, cols, rows)


def proof_config_struct(fri_lde_factor, cap_size, security_level, pow_bits, transcript="poseidon2", tree_hasher=None, pow_runner="blake2s"):
    """bj_proof_config; tree_hasher None pairs the transcript with its usual hasher (Transcript::CompatibleCap = TreeHasher::Output)."""
    transcript_kind = TRANSCRIPT_KINDS[transcript]
    if tree_hasher is None:
        tree_hasher = transcript if transcript in ("blake2s", "keccak256") else "poseidon2"
    return _ProofConfig(fri_lde_factor, cap_size, security_level, pow_bits, transcript_kind, HASHER_KINDS[tree_hasher], POW_KINDS[pow_runner])


TRANSCRIPT_KINDS = {"poseidon2": _abi.BJ_TRANSCRIPT_POSEIDON2, "poseidon": _abi.BJ_TRANSCRIPT_POSEIDON,
                    "blake2s": _abi.BJ_TRANSCRIPT_BLAKE2S, "keccak256": _abi.BJ_TRANSCRIPT_KECCAK256}
HASHER_KINDS = {"poseidon2": _abi.BJ_HASHER_POSEIDON2, "blake2s": _abi.BJ_HASHER_BLAKE2S, "keccak256": _abi.BJ_HASHER_KECCAK256,
                "poseidon": _abi.BJ_HASHER_POSEIDON}
POW_KINDS = {"blake2s": _abi.BJ_POW_BLAKE2S256, "keccak256": _abi.BJ_POW_KECCAK256}

(VERIFY_OK, VERIFY_SHAPE, VERIFY_LOOKUP_SUM, VERIFY_QUOTIENT, VERIFY_POW, VERIFY_MERKLE, VERIFY_FRI_VALUE, VERIFY_FRI_MERKLE, VERIFY_FINAL) = (
    _abi.BJ_VERIFY_OK, _abi.BJ_VERIFY_SHAPE, _abi.BJ_VERIFY_LOOKUP_SUM, _abi.BJ_VERIFY_QUOTIENT, _abi.BJ_VERIFY_POW, _abi.BJ_VERIFY_MERKLE,
    _abi.BJ_VERIFY_FRI_VALUE, _abi.BJ_VERIFY_FRI_MERKLE, _abi.BJ_VERIFY_FINAL)     # bj_verify_stage
VERIFY_STAGE_NAMES = ["ok", "shape", "lookup_sum", "quotient", "pow", "merkle", "fri_value", "fri_merkle", "final"]
VERIFY_PARTIAL_QUERIES = _abi.BJ_VERIFY_PARTIAL_QUERIES


@dataclass
class VerifyReport:
    """bj_verify_report: true when the proof is valid under the key; otherwise the first failing check."""
    stage: int = VERIFY_OK
    query: int = 0
    oracle: int = 0
    queries_checked: int = 0

    def __bool__(self):
        return self.stage == VERIFY_OK

    def __str__(self):
        if self.stage == VERIFY_OK:
            return "valid (%d queries)" % self.queries_checked
        return "invalid: %s (query %d, oracle %d)" % (VERIFY_STAGE_NAMES[self.stage], self.query, self.oracle)


class Verifier:
    """A verification key (bj_vk) and bj_verify.  Making the key needs no device: Verifier(circuit, cap, config) with config a dict
    of the keyword arguments of `proof_config_struct`; ProverSetup.verifier() takes the same key out of a setup."""

    def __init__(self, circuit=None, cap=None, config=None, _handle=None, _lib=None):
        self._lib = _lib or load_library()
        if _handle is not None:
            self._h = _handle
            return
        cc, keep = circuit_struct(circuit)
        cfg = proof_config_struct(**config)
        cap = np.ascontiguousarray(cap, dtype=np.uint64).reshape(-1)
        if cap.size != 4 * int(cfg.cap_size):
            raise BoojumHipError("bj_vk_create: the setup cap has %d words, cap_size %d needs %d" % (cap.size, cfg.cap_size, 4 * cfg.cap_size))
        h = C.c_void_p()
        rc = self._lib.bj_vk_create(C.byref(cc), _np_ptr(cap), C.byref(cfg), C.byref(h))
        del keep
        if rc != 0:
            raise BoojumHipError("%s (%d): %s" % (self._lib.bj_status_string(rc).decode(), rc, self._lib.bj_last_error(None).decode()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bj_vk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def verify(self, ctx, buf, partial=False):
        """bj_verify on the serialised proof words: a VerifyReport (true when valid).  partial: the buffer carries only the first
        k > 0 query openings (BJ_VERIFY_PARTIAL_QUERIES)."""
        a = np.ascontiguousarray(buf, dtype=np.uint64).reshape(-1)
        if a.size == 0:
            a = np.zeros(1, dtype=np.uint64)
            n = 0
        else:
            n = a.size
        r = _VerifyReport()
        ctx._check(self._lib.bj_verify(ctx._h, self._h, _np_ptr(a), n, VERIFY_PARTIAL_QUERIES if partial else 0, C.byref(r)))
        return VerifyReport(int(r.stage), int(r.query), int(r.oracle), int(r.queries_checked))

    def verify_batch(self, ctx, proofs, partial_queries=False):
        """bj_verify_batch: the proofs of `proofs` (serialised words each; None or an empty buffer is a proof of no words) under this
        key in one call; a list with the VerifyReport bj_verify would give each of them."""
        bufs = [np.zeros(0, dtype=np.uint64) if p is None else np.ascontiguousarray(p, dtype=np.uint64).reshape(-1) for p in proofs]
        n = len(bufs)
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        sizes = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        reports = (_VerifyReport * max(n, 1))()
        ctx._check(self._lib.bj_verify_batch(ctx._h, self._h, ptrs, sizes, n, VERIFY_PARTIAL_QUERIES if partial_queries else 0, reports))
        return [VerifyReport(int(r.stage), int(r.query), int(r.oracle), int(r.queries_checked)) for r in reports[:n]]

    def batch_ms(self, ctx):
        """Of the last verify_batch on ctx: (host wall ms, upload ms, openings kernel ms, DEEP + FRI kernel ms)."""
        v = [C.c_float() for _ in range(4)]
        ctx._check(self._lib.bj_verify_batch_ms(ctx._h, *[C.byref(x) for x in v]))
        return tuple(float(x.value) for x in v)

    def kernel_ms(self, ctx):
        """HIP-event durations (openings, DEEP + FRI) of the two kernels of the last verify on ctx."""
        a, b = C.c_float(), C.c_float()
        ctx._check(self._lib.bj_verify_kernel_ms(ctx._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)


SAT, UNSAT_GATE, UNSAT_SPECIALIZED_GATE, UNSAT_LOOKUP, UNSAT_MULTIPLICITY = (
    _abi.BJ_SAT, _abi.BJ_UNSAT_GATE, _abi.BJ_UNSAT_SPECIALIZED_GATE, _abi.BJ_UNSAT_LOOKUP, _abi.BJ_UNSAT_MULTIPLICITY)     # bj_unsat_kind


@dataclass
class SatisfiabilityReport:
    """bj_unsat_report: the first failure of a witness (order: include/boojum_hip.h) and the number of failures per kind.
    True when the witness satisfies the circuit; str() is worded like the panic of the reference's check_if_satisfied."""
    kind: int = SAT
    gate: int = 0
    repetition: int = 0
    term: int = 0
    row: int = 0
    value: int = 0
    expected: int = 0
    failures: tuple = (0, 0, 0, 0, 0)
    gate_name: str = ""

    def __bool__(self):
        return self.kind == SAT

    def __str__(self):
        if self.kind == SAT:
            return "Satisfied"
        if self.kind in (UNSAT_GATE, UNSAT_SPECIALIZED_GATE):
            return "Unsatisfied at row %d with value %d for term number %d for subinstance number %d of gate %s" % (
                self.row, self.value, self.term, self.repetition, self.gate_name or "#%d" % self.gate)
        if self.kind == UNSAT_LOOKUP:
            return "Unsatisfied at row %d: the tuple of lookup sub-argument %d is in no table row" % (self.row, self.gate)
        return "Unsatisfied at table row %d: multiplicities sum to %d, %d lookups" % (self.row, self.expected, self.value)


@dataclass(frozen=True)
class UnsatEntry:
    """bj_unsat_entry: one failure of a witness (bj_list_unsatisfied); the fields mean what they mean in SatisfiabilityReport."""
    kind: int
    gate: int
    repetition: int
    term: int
    row: int
    value: int
    expected: int

    def fields(self):
        return (self.kind, self.gate, self.repetition, self.term, self.row, self.value, self.expected)


COPY_OK, COPY_SIGMA_INVALID, COPY_SIGMA_NOT_PERMUTATION, COPY_VALUE_MISMATCH = (
    _abi.BJ_COPY_OK, _abi.BJ_COPY_SIGMA_INVALID, _abi.BJ_COPY_SIGMA_NOT_PERMUTATION, _abi.BJ_COPY_VALUE_MISMATCH)     # bj_copy_kind
NO_CELL = 0xFFFFFFFF                # bj_sigma_cells: a word in no coset; bj_copy_report.variable: no placement index
NO_CELL_KEY = (1 << 64) - 1         # bj_sigma_cells: *first_invalid when every word is valid


@dataclass
class CopyReport:
    """bj_copy_report: the first cell that breaks a copy constraint (categories and order: include/boojum_hip.h) and the number of
    failures per kind.  True when sigma is a permutation of the cells and every cell holds the value of the cell its sigma names."""
    kind: int = COPY_OK
    column: int = 0
    row: int = 0
    partner_column: int = 0
    partner_row: int = 0
    value: int = 0
    partner_value: int = 0
    variable: int = NO_CELL
    failures: tuple = (0, 0, 0, 0)

    def __bool__(self):
        return self.kind == COPY_OK

    def __str__(self):
        if self.kind == COPY_OK:
            return "Copy constraints hold"
        if self.kind == COPY_SIGMA_INVALID:
            return "sigma at column %d row %d names no cell" % (self.column, self.row)
        if self.kind == COPY_SIGMA_NOT_PERMUTATION:
            return "sigma is no permutation: column %d row %d names column %d row %d, and so does another cell" % (
                self.column, self.row, self.partner_column, self.partner_row)
        return "column %d row %d holds %d, the cell its sigma names (column %d row %d) holds %d%s" % (
            self.column, self.row, self.value, self.partner_column, self.partner_row, self.partner_value,
            "" if self.variable == NO_CELL else " (variable %d)" % self.variable)


class _Ticket:
    """A proof in flight (bj_ticket) + the host arrays it reads + the setup and the context its lane works on: while the ticket
    lives, neither is collected under the lane's worker.  `handle` is None once it was waited for."""

    def __init__(self, handle, keep, setup=None, ctx=None):
        self.handle, self.keep, self.setup, self.ctx = handle, keep, setup, ctx


@contextlib.contextmanager
def _setup_lean_switch(lib, on):
    """BJ_SETUP_LEAN set (and read by the library) for the calls inside, then whatever the environment held before, read again.
    `on` false: nothing is touched, the library keeps what it last read."""
    if not on:
        yield
        return
    before = os.environ.get("BJ_SETUP_LEAN")
    os.environ["BJ_SETUP_LEAN"] = "1"
    lib.bj_env_reload()
    try:
        yield
    finally:
        if before is None:
            os.environ.pop("BJ_SETUP_LEAN", None)
        else:
            os.environ["BJ_SETUP_LEAN"] = before
        lib.bj_env_reload()


@contextlib.contextmanager
def lean_proofs(lib, on=True):
    """Proofs started inside keep no LDE of their witness and stage-2 oracles (BJ_PROOF_LEAN, include/boojum_hip.h at bj_prove_dev):
    the same bytes out of a workspace smaller by (nW + nS2) * (L - 1) * n words.  The switch is the process's, not a context's:
    BJ_PROOF_LEAN is set to "1" (`on` false: to "0") and read by the library for the calls inside, then whatever the environment
    held before comes back and is read again.  Like bj_env_reload it must not run beside another call into the library."""
    before = os.environ.get("BJ_PROOF_LEAN")
    os.environ["BJ_PROOF_LEAN"] = "1" if on else "0"
    lib.bj_env_reload()
    try:
        yield
    finally:
        if before is None:
            os.environ.pop("BJ_PROOF_LEAN", None)
        else:
            os.environ["BJ_PROOF_LEAN"] = before
        lib.bj_env_reload()


class ProverSetup:
    """Device-resident setup for a circuit of era_boojum_amd.synthetic.Circuit shape (bj_setup_create).

    With `comm` (a TorchComm) the LDE cosets of every column are split across the ranks of the process group and
    `prove` / `prove_dev` become collective: every rank passes the same witness and gets the same proof
    (bj_setup_create_sharded)."""

    def __init__(self, ctx, circuit, fri_lde_factor=8, cap_size=16, security_level=100, pow_bits=0, comm=None,
                 transcript="poseidon2", setup_base_dump=None, pow_runner="blake2s", tree_hasher=None, variables_hint_dump=None, lean=False):
        """lean: the setup keeps its monomials and its tree and drops the LDE of its columns once the tree stands (BJ_SETUP_LEAN,
        DESIGN.md §3): `n_cols * L * n * 8` bytes less in HBM, the same cap and byte-identical proofs, each proof paying one coset
        transform of the setup columns per quotient coset and an evaluation per queried leaf.  The switch is set for the creation
        only and the value the environment held is put back, also when the creation raises; not thread-safe (bj_env_reload), so
        never while a proof runs.  Single GPU only: refused together with `comm`.
        pow_runner: "blake2s" | "keccak256" — the PoWRunner (pow.rs), independent of the transcript as in the reference.
        tree_hasher: None pairs the transcript with its usual hasher (Poseidon2 trees for "poseidon2" / "poseidon", the same byte
        hash for "blake2s" / "keccak256"); "poseidon2" | "poseidon" | "blake2s" | "keccak256" picks one (BJ_HASHER_*), e.g.
        "poseidon" with transcript="poseidon" for GoldilocksPoseidonSponge trees + GoldilocksPoisedonTranscript.
        setup_base_dump: the bytes of the reference's `SetupBaseStorage::write_into_buffer` (bj_setup_create_from_dump): the
        columns, constant-column count, table-id column, selector paths, quotient degree and non-residues then come from the
        dump / are computed by the library, and `circuit` only has to carry the geometry and the gate list.
        variables_hint_dump: the bytes of `DenseVariablesCopyHint` (bj_setup_create_from_placement): `circuit.sigmas` is not read,
        the copy-permutation polynomials are built on the device from the placement, which stays resident so that
        `prove_from_dumps(witness_vec_dump, None)` works.  See `from_placement`."""
        self._ctx, self._lib, self.circuit = ctx, ctx._lib, circuit
        self._comm = comm
        self._lean = bool(lean)
        if lean and comm is not None:
            raise BoojumHipError("a lean setup is single-GPU: a shard already holds only its own cosets of the LDE")
        with _setup_lean_switch(self._lib, self._lean):
            self._create(ctx, circuit, fri_lde_factor, cap_size, security_level, pow_bits, comm, transcript, setup_base_dump, pow_runner,
                         tree_hasher, variables_hint_dump)

    def _create(self, ctx, circuit, fri_lde_factor, cap_size, security_level, pow_bits, comm, transcript, setup_base_dump, pow_runner,
                tree_hasher, variables_hint_dump):
        self.fri_lde_factor, self.cap_size, self.security_level, self.pow_bits = fri_lde_factor, cap_size, security_level, pow_bits
        c = circuit
        from_dump = setup_base_dump is not None
        cc, self._keep = circuit_struct(c, from_dump)
        self.num_witness_cols = int(getattr(c, "num_witness_cols", 0))
        self.transcript, self.tree_hasher, self.pow_runner = transcript, tree_hasher, pow_runner
        cfg = proof_config_struct(fri_lde_factor, cap_size, security_level, pow_bits, transcript, tree_hasher, pow_runner)
        self.transcript_kind, self.hasher_kind = int(cfg.transcript), int(cfg.tree_hasher)
        con = np.ascontiguousarray(c.constants, dtype=np.uint64)
        tab = np.ascontiguousarray(c.tables, dtype=np.uint64)
        h = C.c_void_p()
        if variables_hint_dump is not None:
            if comm is not None or from_dump:
                raise BoojumHipError("a setup from a placement is single-GPU and takes its columns from the circuit, not from a dump")
            blob = bytes(variables_hint_dump)
            ctx._check(self._lib.bj_setup_create_from_placement(ctx._h, C.byref(cc), blob, len(blob), _np_ptr(con),
                                                                _np_ptr(tab) if c.lookup_reps else None, C.byref(cfg), C.byref(h)))
            self._h = h
            return
        sig = np.ascontiguousarray(c.sigmas, dtype=np.uint64)
        if from_dump:
            if comm is not None:
                raise BoojumHipError("a setup from a dump is single-GPU")
            blob = bytes(setup_base_dump)
            ctx._check(self._lib.bj_setup_create_from_dump(ctx._h, C.byref(cc), blob, len(blob), C.byref(cfg), C.byref(h)))
            self._h = h
            return
        if comm is None:
            ctx._check(self._lib.bj_setup_create(ctx._h, C.byref(cc), _np_ptr(sig), _np_ptr(con), _np_ptr(tab) if c.lookup_reps else None,
                                                 C.byref(cfg), C.byref(h)))
        else:   # bj_setup_create_sharded does not look at BJ_SETUP_LEAN
            ctx._check(self._lib.bj_setup_create_sharded(ctx._h, C.byref(cc), _np_ptr(sig), _np_ptr(con),
                                                         _np_ptr(tab) if c.lookup_reps else None, C.byref(cfg), C.byref(comm.struct), C.byref(h)))
        self._h = h

    @property
    def lean(self):
        """True for a setup created with lean=True.  (One created with lean=False while BJ_SETUP_LEAN was set by other means is lean
        as well: `device_bytes` tells.)"""
        return self._lean

    @classmethod
    def from_placement(cls, ctx, circuit, var_ids, *args, **kwargs):
        """Setup from the variable placement instead of `circuit.sigmas`: var_ids [num_vars][n] integers, negative = empty cell
        (what `DenseVariablesCopyHint` encodes).  Other arguments as for the constructor."""
        from . import memcopy_format
        return cls(ctx, circuit, *args, variables_hint_dump=memcopy_format.write_variables_hint(var_ids), **kwargs)

    def device_bytes(self):
        """HBM held by this setup (its shard when sharded): bj_setup_device_bytes."""
        b = C.c_size_t()
        self._ctx._check(self._lib.bj_setup_device_bytes(self._h, C.byref(b)))
        return int(b.value)

    def set_comm(self, comm):
        """bj_setup_set_comm: another transport for the same shard (same rank / world)."""
        self._ctx._check(self._lib.bj_setup_set_comm(self._h, C.byref(comm.struct)))
        self._comm = comm

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bj_setup_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def cap(self):
        out = np.empty((self.cap_size, 4), dtype=np.uint64)
        self._ctx._check(self._lib.bj_setup_cap(self._h, _np_ptr(out)))
        return out

    def config(self):
        """The proof config as the keyword arguments of `proof_config_struct` / the `config` of `Verifier`."""
        return dict(fri_lde_factor=self.fri_lde_factor, cap_size=self.cap_size, security_level=self.security_level, pow_bits=self.pow_bits,
                    transcript=self.transcript, tree_hasher=self.tree_hasher, pow_runner=self.pow_runner)

    def verifier(self):
        """The verification key of this setup (bj_vk_from_setup)."""
        h = C.c_void_p()
        self._ctx._check(self._lib.bj_vk_from_setup(self._h, C.byref(h)))
        return Verifier(_handle=h, _lib=self._lib)

    def verify(self, buf, partial=False):
        """bj_verify of serialised proof words under this setup's key: a VerifyReport."""
        vk = self.verifier()
        try:
            return vk.verify(self._ctx, buf, partial)
        finally:
            vk.close()

    def prove_verified(self, vk, variables=None, multiplicities=None, public_values=None, count_multiplicities=False):
        """Service-side convenience, and the binding of bj_verify_proof: bj_prove, then the check of the handle it returned under
        the key `vk` (a Verifier), before the proof is serialised — what a proving service does with every proof it ships.
        Arguments as for `prove`.  Returns (serialised proof, VerifyReport); the proof is returned whatever the verdict."""
        c = self.circuit
        v, m, pv = self._host_witness(variables, multiplicities, public_values)
        h = C.c_void_p()
        self._ctx._check(self._lib.bj_prove(self._ctx._h, self._h, _np_ptr(v), _np_ptr(m) if c.lookup_reps and not count_multiplicities else None, _np_ptr(pv), C.byref(h)))
        r = _VerifyReport()
        rc = self._lib.bj_verify_proof(self._ctx._h, vk._h, h, C.byref(r))
        buf, _ = self._finish(h)
        self._ctx._check(rc)
        return buf, VerifyReport(int(r.stage), int(r.query), int(r.oracle), int(r.queries_checked))

    def _finish(self, h):
        n = self._lib.bj_proof_size_u64(h)
        buf = np.empty(n, dtype=np.uint64)
        self._ctx._check(self._lib.bj_proof_serialize(h, _np_ptr(buf)))
        ms = (C.c_float * 8)()
        self._lib.bj_proof_stage_ms(h, ms)
        cms, calls, recv = C.c_float(), C.c_size_t(), C.c_size_t()
        self._lib.bj_proof_comm_stats(h, C.byref(cms), C.byref(calls), C.byref(recv))
        self.last_comm = {"ms_in_collectives": float(cms.value), "calls": int(calls.value), "bytes_received": int(recv.value)}
        self.last_kernels = {}        # name -> (ms, algorithmic bytes) of the first launch of each probed kernel in this proof
        name, kms, kb, k = C.c_char_p(), C.c_float(), C.c_double(), 0
        while self._lib.bj_proof_kernel_stats(h, k, C.byref(name), C.byref(kms), C.byref(kb)) == 0:
            self.last_kernels[name.value.decode()] = (float(kms.value), float(kb.value))
            k += 1
        res, hw, slabs = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._lib.bj_proof_workspace_bytes(h, C.byref(res), C.byref(hw), C.byref(slabs))
        self.last_workspace = {"reserved_bytes": int(res.value), "high_water_bytes": int(hw.value), "overflow_slabs": int(slabs.value)}
        self._lib.bj_proof_destroy(h)
        if slabs.value and not os.environ.get("BJ_ALLOW_WORKSPACE_OVERFLOW"):
            # the proof is right, but an allowance of its workspace plan (csrc/workspace_plan.h) was no upper bound for this geometry:
            # every proof the test suite makes passes through here
            raise BoojumHipError("the proof needed %d overflow slab(s): reserved %d bytes, high-water mark %d bytes"
                                 % (slabs.value, res.value, hw.value))
        stages = dict(zip(STAGE_NAMES, [float(x) for x in ms][:7]))
        stages["witness_tree_leaf_kernel"] = float(ms[7])
        return buf, stages

    def _host_witness(self, variables, multiplicities, public_values):
        """The host arrays bj_prove / bj_prove_async take (variables with the witness columns behind them, multiplicities, public
        values); every argument defaults to the circuit's own."""
        c = self.circuit
        v = np.ascontiguousarray(c.variables if variables is None else variables, dtype=np.uint64)
        if self.num_witness_cols and v.shape[0] == c.num_vars:     # the non-copiable witness columns travel behind the variables
            v = np.ascontiguousarray(np.concatenate([v, c.witness], axis=0))
        m = np.ascontiguousarray(c.multiplicities if multiplicities is None else multiplicities, dtype=np.uint64)
        pv = np.array([p[2] for p in c.public_inputs] if public_values is None else public_values, dtype=np.uint64)
        if pv.size == 0:
            pv = np.zeros(1, dtype=np.uint64)
        return v, m, pv

    def prove(self, variables=None, multiplicities=None, public_values=None, count_multiplicities=False):
        """Host-memory entry point (bj_prove): returns (serialised proof u64 array, per-stage ms).  count_multiplicities: no column
        is handed over (NULL), the prover counts it on the device."""
        c = self.circuit
        v, m, pv = self._host_witness(variables, multiplicities, public_values)
        h = C.c_void_p()
        self._ctx._check(self._lib.bj_prove(self._ctx._h, self._h, _np_ptr(v), _np_ptr(m) if c.lookup_reps and not count_multiplicities else None,
                                            _np_ptr(pv), C.byref(h)))
        return self._finish(h)

    def prove_async(self, variables=None, multiplicities=None, public_values=None, count_multiplicities=False):
        """bj_prove_async: queues the proof on one of the context's two lanes and returns a ticket for `wait`.  Arrays passed in
        are used in place when they are contiguous uint64 (e.g. views of pinned tensors) and kept alive by the ticket.
        count_multiplicities: as for `prove`."""
        c = self.circuit
        v, m, pv = self._host_witness(variables, multiplicities, public_values)
        t = C.c_void_p()
        self._ctx._check(self._lib.bj_prove_async(self._ctx._h, self._h, _np_ptr(v), _np_ptr(m) if c.lookup_reps and not count_multiplicities else None,
                                                  _np_ptr(pv), C.byref(t)))
        return _Ticket(t, (v, m), self, self._ctx)

    def set_witness_placement(self, wit_ids):
        """bj_setup_set_witness_placement: wit_ids [num_witness_cols][n] integers, negative = empty cell (what `DenseWitnessCopyHint`
        encodes; same layout as the variables' hint).  With it `prove_values` works on a circuit with non-copiable witness columns."""
        from . import memcopy_format
        blob = memcopy_format.write_variables_hint(wit_ids)
        self._ctx._check(self._lib.bj_setup_set_witness_placement(self._ctx._h, self._h, blob, len(blob)))

    @staticmethod
    def _values_arrays(all_values, multiplicities):
        v = np.ascontiguousarray(all_values, dtype=np.uint64)
        m = None if multiplicities is None else np.ascontiguousarray(multiplicities, dtype=np.uint32)
        return v, m

    def prove_values(self, all_values, multiplicities=None):
        """bj_prove_values: the proof from a WitnessVec's `all_values` and its u32 multiplicity counters (None: counted on the
        device) on a setup made by `from_placement`; the public inputs are read through the placement.  Returns like `prove`."""
        v, m = self._values_arrays(all_values, multiplicities)
        h = C.c_void_p()
        self._ctx._check(self._lib.bj_prove_values(self._ctx._h, self._h, _np_ptr(v) if v.size else None, v.size,
                                                   m.ctypes.data_as(C.c_void_p) if m is not None else None, m.size if m is not None else 0, C.byref(h)))
        return self._finish(h)

    def prove_values_async(self, all_values, multiplicities=None):
        """bj_prove_values_async: `prove_values` queued on one of the context's two lanes; returns a ticket for `wait`.  The
        arrays are used in place when they are contiguous (uint64 / uint32) and kept alive by the ticket."""
        v, m = self._values_arrays(all_values, multiplicities)
        t = C.c_void_p()
        self._ctx._check(self._lib.bj_prove_values_async(self._ctx._h, self._h, _np_ptr(v) if v.size else None, v.size,
                                                         m.ctypes.data_as(C.c_void_p) if m is not None else None, m.size if m is not None else 0, C.byref(t)))
        return _Ticket(t, (v, m), self, self._ctx)

    def done(self, ticket):
        """bj_proof_poll: True when `wait` would not block."""
        if ticket.handle is None:
            raise BoojumHipError("this ticket was waited for already")
        rc = self._lib.bj_proof_poll(ticket.handle)
        if rc < 0:
            raise BoojumHipError("bj_proof_poll: %s: no live ticket (its context was destroyed)" % self._lib.bj_status_string(rc).decode())
        return bool(rc)

    def wait(self, ticket):
        """bj_proof_wait: blocks until the ticket's proof is complete; returns (serialised proof, per-stage ms) like `prove`."""
        if ticket.handle is None:
            raise BoojumHipError("this ticket was waited for already: a ticket is waited for exactly once")
        h = C.c_void_p()
        t, ticket.handle = ticket.handle, None
        rc = self._lib.bj_proof_wait(t, C.byref(h))
        ticket.keep = ticket.setup = ticket.ctx = None
        if rc != 0 and not self._ctx._h:   # the context was closed with the proof in flight: the library has freed proof and ticket
            raise BoojumHipError("%s: the context was closed before the ticket was waited for" % self._lib.bj_status_string(rc).decode())
        self._ctx._check(rc)
        return self._finish(h)

    def prove_from_dumps(self, witness_vec_dump, variables_hint_dump, witness_hint_dump=None):
        """bj_prove_from_dumps: the reference's `WitnessVec` and `DenseVariablesCopyHint` (+ `DenseWitnessCopyHint`) bytes in, the
        proof out.  variables_hint_dump may be None on a setup made from a placement, which holds the hint itself."""
        w = bytes(witness_vec_dump)
        v = bytes(variables_hint_dump) if variables_hint_dump is not None else None
        x = bytes(witness_hint_dump) if witness_hint_dump is not None else None
        h = C.c_void_p()
        self._ctx._check(self._lib.bj_prove_from_dumps(self._ctx._h, self._h, w, len(w), v, len(v) if v else 0, x, len(x) if x else 0, C.byref(h)))
        return self._finish(h)

    def _report(self, r):
        c, name = self.circuit, ""
        if r.kind == UNSAT_GATE:
            name = c.gates[r.gate].name
        elif r.kind == UNSAT_SPECIALIZED_GATE:
            name = c.specialized_gates[r.gate].name
        return SatisfiabilityReport(int(r.kind), int(r.gate), int(r.repetition), int(r.term), int(r.row), int(r.value), int(r.expected),
                                    tuple(int(x) for x in r.failures), name)

    def check_satisfied_dev(self, d_variables, d_multiplicities):
        """bj_check_satisfied on a witness already in HBM ([num_vars + num_witness_cols][n], multiplicities [n] or None)."""
        r = _UnsatReport()
        self._ctx._check(self._lib.bj_check_satisfied(self._ctx._h, self._h, d_variables, d_multiplicities, C.byref(r)))
        return self._report(r)

    def check_satisfied(self, variables=None, multiplicities=None):
        """Where the witness fails the circuit (bj_check_satisfied): a SatisfiabilityReport, true when it does not.  Arrays default
        to the circuit's own and are uploaded for the call."""
        c = self.circuit
        v = np.ascontiguousarray(c.variables if variables is None else variables, dtype=np.uint64)
        if self.num_witness_cols and v.shape[0] == c.num_vars:
            v = np.ascontiguousarray(np.concatenate([v, c.witness], axis=0))
        d_v = self._ctx.upload(v)
        d_m = None
        try:
            if c.lookup_reps:
                d_m = self._ctx.upload(np.ascontiguousarray(c.multiplicities if multiplicities is None else multiplicities, dtype=np.uint64))
            return self.check_satisfied_dev(d_v, d_m)
        finally:
            self._ctx.free(d_v)
            if d_m is not None:
                self._ctx.free(d_m)

    def check_satisfied_from_dumps(self, witness_vec_dump, variables_hint_dump, witness_hint_dump=None):
        """bj_check_satisfied_from_dumps: the arguments of prove_from_dumps, the report of check_satisfied."""
        w = bytes(witness_vec_dump)
        v = bytes(variables_hint_dump) if variables_hint_dump is not None else None
        x = bytes(witness_hint_dump) if witness_hint_dump is not None else None
        r = _UnsatReport()
        self._ctx._check(self._lib.bj_check_satisfied_from_dumps(self._ctx._h, self._h, w, len(w), v, len(v) if v else 0, x, len(x) if x else 0,
                                                                 C.byref(r)))
        return self._report(r)

    @staticmethod
    def _entries(buf, n):
        return [UnsatEntry(int(e.kind), int(e.gate), int(e.repetition), int(e.term), int(e.row), int(e.value), int(e.expected)) for e in (buf[:n] if n else [])]

    def list_unsatisfied_dev(self, d_variables, d_multiplicities, capacity=1024):
        """bj_list_unsatisfied on a witness already in HBM: (the first min(capacity, total) UnsatEntry records in the order of
        include/boojum_hip.h, the five totals — [k] entries of kind k in the whole trace, [0] their sum)."""
        buf = (_UnsatEntry * capacity)() if capacity else None
        n, totals = C.c_size_t(0), (C.c_uint64 * 5)()
        self._ctx._check(self._lib.bj_list_unsatisfied(self._ctx._h, self._h, d_variables, d_multiplicities, buf, capacity, C.byref(n), totals))
        return self._entries(buf, n.value), tuple(int(x) for x in totals)

    def list_unsatisfied(self, variables=None, multiplicities=None, capacity=1024):
        """Every place where the witness fails the circuit (bj_list_unsatisfied), not the first one: (entries, totals) as
        list_unsatisfied_dev returns them.  Arrays default to the circuit's own and are uploaded for the call."""
        c = self.circuit
        v = np.ascontiguousarray(c.variables if variables is None else variables, dtype=np.uint64)
        if self.num_witness_cols and v.shape[0] == c.num_vars:
            v = np.ascontiguousarray(np.concatenate([v, c.witness], axis=0))
        d_v = self._ctx.upload(v)
        d_m = None
        try:
            if c.lookup_reps:
                d_m = self._ctx.upload(np.ascontiguousarray(c.multiplicities if multiplicities is None else multiplicities, dtype=np.uint64))
            return self.list_unsatisfied_dev(d_v, d_m, capacity)
        finally:
            self._ctx.free(d_v)
            if d_m is not None:
                self._ctx.free(d_m)

    def list_unsatisfied_from_dumps(self, witness_vec_dump, variables_hint_dump, witness_hint_dump=None, capacity=1024):
        """bj_list_unsatisfied_from_dumps: the arguments of prove_from_dumps, the result of list_unsatisfied."""
        w = bytes(witness_vec_dump)
        v = bytes(variables_hint_dump) if variables_hint_dump is not None else None
        x = bytes(witness_hint_dump) if witness_hint_dump is not None else None
        buf = (_UnsatEntry * capacity)() if capacity else None
        n, totals = C.c_size_t(0), (C.c_uint64 * 5)()
        self._ctx._check(self._lib.bj_list_unsatisfied_from_dumps(self._ctx._h, self._h, w, len(w), v, len(v) if v else 0, x, len(x) if x else 0,
                                                                  buf, capacity, C.byref(n), totals))
        return self._entries(buf, n.value), tuple(int(x) for x in totals)

    def check_copy_constraints(self, d_variables):
        """bj_check_copy_constraints on a witness in HBM (the pointer prove_dev takes): a CopyReport, true when every copy
        constraint holds.  bj_check_satisfied does not look at them, and bj_prove refuses such a witness without naming a cell."""
        r = _CopyReport()
        self._ctx._check(self._lib.bj_check_copy_constraints(self._ctx._h, self._h, d_variables, C.byref(r)))
        return CopyReport(int(r.kind), int(r.column), int(r.row), int(r.partner_column), int(r.partner_row), int(r.value),
                          int(r.partner_value), int(r.variable), tuple(int(x) for x in r.failures))

    def count_multiplicities_dev(self, d_variables, d_multiplicities):
        """bj_setup_lookup_multiplicities on a witness already in HBM: writes the column [n] at d_multiplicities."""
        self._ctx._check(self._lib.bj_setup_lookup_multiplicities(self._ctx._h, self._h, d_variables, d_multiplicities))

    def count_multiplicities(self, variables=None):
        """The multiplicity column [1, n] of the witness, counted on the device (bj_setup_lookup_multiplicities): per class of equal
        table rows the number of looked-up tuples equal to it, on the class's smallest row.  `variables` defaults to the circuit's
        own and is uploaded for the call.  Raises, naming the first (row, sub-argument), if a looked-up tuple is in no table row."""
        c = self.circuit
        v = np.ascontiguousarray(c.variables if variables is None else variables, dtype=np.uint64)
        d_v, d_m = self._ctx.upload(v), self._ctx.malloc(8 * c.n)
        try:
            self.count_multiplicities_dev(d_v, d_m)
            return self._ctx.d2h(d_m, (1, c.n))
        finally:
            self._ctx.free(d_v)
            self._ctx.free(d_m)

    def prove_dev(self, d_variables, d_multiplicities, public_values=None, count_multiplicities=False):
        """Witness already in HBM (bj_prove_dev).  count_multiplicities: d_multiplicities is ignored and NULL handed over, the
        prover counts the column on the device."""
        if count_multiplicities:
            d_multiplicities = None
        c = self.circuit
        pv = np.array([p[2] for p in c.public_inputs] if public_values is None else public_values, dtype=np.uint64)
        if pv.size == 0:
            pv = np.zeros(1, dtype=np.uint64)
        h = C.c_void_p()
        self._ctx._check(self._lib.bj_prove_dev(self._ctx._h, self._h, d_variables, d_multiplicities, _np_ptr(pv), C.byref(h)))
        return self._finish(h)
