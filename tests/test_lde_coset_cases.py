"""The oracle's LDE at 16, 32 and 64 cosets, without a GPU: what tests/test_gpu_lde_cosets.py compares the kernels with rests on the
definition of transform_monomials_to_lde (utils.rs:311-403), not only on the oracle's own C code.  Coset c of a 2^log_lde-fold extension
is the transform on the shift 7 * omega_(n L)^bitrev(c, log_lde); entry i of it is the polynomial at that shift times
omega_n^bitrev(i, log_n)."""
import numpy as np
import pytest

import oracle as O

P = O.P
LOG_N = 6


def _mono():
    rng = np.random.default_rng(640)
    n = 1 << LOG_N
    canon = rng.integers(0, P, size=n, dtype=np.uint64)
    top = np.full(n, P - 1, dtype=np.uint64)
    weak = (np.uint64(P) + rng.integers(0, 2**32 - 1, size=n, dtype=np.uint64)).astype(np.uint64)      # p .. 2^64 - 1
    return np.stack([canon, top, weak])


@pytest.mark.parametrize("log_lde", [4, 5, 6])
def test_every_coset_of_a_wide_lde_is_the_transform_on_its_shift(log_lde):
    mono = _mono()
    lde = O.lde_batch(mono, log_lde, threads=2)
    shifts = O.lde_coset_shifts(LOG_N, log_lde)
    assert lde.shape == (3, 1 << log_lde, 1 << LOG_N) and shifts.shape == (1 << log_lde,)
    w = O.omega(LOG_N + log_lde)
    for c in range(1 << log_lde):
        assert int(shifts[c]) == 7 * pow(w, O.bitrev(c, log_lde), P) % P
        assert np.array_equal(lde[:, c, :], O.fft_batch(mono, int(shifts[c])))
    assert len({int(s) for s in shifts}) == 1 << log_lde
    assert int(lde.max()) < P                                                # canonical residues out, whatever went in


@pytest.mark.parametrize("log_lde", [4, 5, 6])
def test_wide_lde_entries_are_horner_values_at_the_defined_points(log_lde):
    """Four entries of every coset of every column, in Python integers: the first, the last and two in between."""
    mono = _mono()
    n = 1 << LOG_N
    lde = O.lde_batch(mono, log_lde)
    w_big, w_n = O.omega(LOG_N + log_lde), O.omega(LOG_N)
    rng = np.random.default_rng(641 + log_lde)
    for c in range(1 << log_lde):
        shift = 7 * pow(w_big, O.bitrev(c, log_lde), P) % P
        for i in [0, n - 1] + [int(v) for v in rng.integers(1, n - 1, size=2)]:
            x = shift * pow(w_n, O.bitrev(i, LOG_N), P) % P
            for col in range(3):
                acc = 0
                for coeff in mono[col][::-1]:
                    acc = (acc * x + int(coeff)) % P
                assert int(lde[col, c, i]) == acc, (col, c, i)
