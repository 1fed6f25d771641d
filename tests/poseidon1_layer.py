"""Test-side hashing layer for the Poseidon (v1) tree hasher, GoldilocksPoseidonSponge<AbsorptionModeOverwrite>
(sponge.rs:345-357): the overwrite sponge of the Poseidon2 hasher (rate 8, zero-padded tail, no length tag, node = L || R || 0,
digest = state[0..4]) around the permutation of poseidon_goldilocks_naive.rs.

It plugs into oracle/prover.py and oracle/verifier.py where they pick their hashing module (`oracle.prover.hashing_layer`,
patched by the tests): the trees are this layer's, the transcript and the query indexer are the algebraic ones of the oracle
(oracle.Transcript of either kind, oracle.QueryIndexer), and do_fri / merkle_cap / merkle_proof are oracle.blake.ByteHashLayer's.

`SpongeLayer(permute_many)` takes a permutation of many states at once, (B, 12) uint64 -> (B, 12) canonical:
  * poseidon1_many_c / poseidon2_many_c: one oracle C call per state (oracle.poseidon_permutation / poseidon2_permutation);
  * poseidon1_many_np: the v1 permutation lane-wise in numpy (checked against the C one by tests/test_poseidon1_layer.py),
    for trees too large for per-state calls (batches under 256 states still go through the C calls).
"""
import numpy as np

import oracle as O
from oracle import blake as OB

P = O.P
_P = np.uint64(P)
_EPS = np.uint64(0xFFFFFFFF)
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
EXPS = [0, 0, 1, 0, 3, 5, 1, 8, 12, 3, 16, 10]


def _canon(a):
    a = np.asarray(a, dtype=np.uint64)
    return np.where(a >= _P, a - _P, a)


def poseidon1_many_c(states):
    s = np.asarray(states, dtype=np.uint64).reshape(-1, 12)
    return np.stack([O.poseidon_permutation(x) for x in s]) if s.shape[0] else s.copy()


def poseidon2_many_c(states):
    s = np.asarray(states, dtype=np.uint64).reshape(-1, 12)
    return np.stack([O.poseidon2_permutation(x) for x in s]) if s.shape[0] else s.copy()


# ---- numpy Goldilocks arithmetic on canonical words (lane-wise)
def _add(a, b):
    with np.errstate(over="ignore"):
        s = a + b
        s = np.where(s < a, s + _EPS, s)           # wrap: 2^64 == EPS; the wrapped sum is < p, no second carry
    return np.where(s >= _P, s - _P, s)


def _mul(a, b):
    with np.errstate(over="ignore"):
        a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
        p00 = a0 * b0
        mid = a0 * b1 + (p00 >> _S32)
        mid2 = a1 * b0 + (mid & _M32)
        lo = (mid2 << _S32) | (p00 & _M32)
        hi = a1 * b1 + (mid >> _S32) + (mid2 >> _S32)
        hh, hl = hi >> _S32, hi & _M32
        t0 = lo - hh                                  # lo + hl * 2^64 + hh * 2^96 == lo + hl * EPS - hh
        t0 = np.where(lo < hh, t0 - _EPS, t0)
        t1 = hl * _EPS
        r = t0 + t1
        r = np.where(r < t1, r + _EPS, r)
    return np.where(r >= _P, r - _P, r)


def _pow7(x):
    x2 = _mul(x, x)
    x3 = _mul(x2, x)
    x4 = _mul(x2, x2)
    return _mul(x4, x3)


_RC = None


def poseidon1_many_np(states):
    """The v1 permutation on B states at once: every round + RC, x^7 on all / on word 0, MDS 2^EXPS[(col - row) mod 12]."""
    global _RC
    if np.asarray(states).size < 12 * 256:      # a few states (verifier paths): per-state C calls are faster than numpy's overhead
        return poseidon1_many_c(states)
    if _RC is None:
        _RC = np.array(O.poseidon_round_constants(), dtype=np.uint64)           # (30, 12), canonical
    s = _canon(np.asarray(states, dtype=np.uint64).reshape(-1, 12)).T.copy()   # (12, B)
    for r in range(30):
        s = _add(s, _RC[r][:, None])
        if r < 4 or r >= 26:
            s = _pow7(s)
        else:
            s[0] = _pow7(s[0])
        lo, hi = s & _M32, s >> _S32
        out = np.empty_like(s)
        with np.errstate(over="ignore"):
            for row in range(12):
                A = np.zeros(s.shape[1], dtype=np.uint64)
                B = np.zeros(s.shape[1], dtype=np.uint64)
                for col in range(12):
                    e = np.uint64(EXPS[(col - row) % 12])
                    A += lo[col] << e                  # < 2^49 summed
                    B += hi[col] << e
                T = A + (B >> _S32) * _EPS             # A + B * 2^32 == A + hi32(B) * EPS + lo32(B) * 2^32, T < 2^50
                out[row] = _add(_canon(T), _canon((B & _M32) << _S32))
        s = out
    return s.T.copy()


class SpongeLayer(OB.ByteHashLayer):
    """merkle_* / Transcript / QueryIndexer / do_fri of the overwrite sponge (rate 8, capacity 4) around `permute_many`."""

    def __init__(self, permute_many):
        super().__init__(None, None, kind=1)
        self.permute_many = permute_many
        self.Transcript = O.Transcript          # algebraic transcript: kind 1 Poseidon2, kind 2 Poseidon (v1)
        self.QueryIndexer = O.QueryIndexer

    def _sponge(self, rows):
        rows = _canon(np.atleast_2d(np.asarray(rows, dtype=np.uint64)))
        b, n = rows.shape
        st = np.zeros((b, 12), dtype=np.uint64)
        for i in range(0, n, 8):
            blk = rows[:, i:i + 8]
            st[:, :8] = 0
            st[:, :blk.shape[1]] = blk
            st = self.permute_many(st)
        return st[:, :4].copy()

    # ---- tree hasher (oracle/mod.rs:114-176)
    def hash_leaf(self, els):
        return self._sponge(np.asarray(els, dtype=np.uint64).reshape(1, -1))[0]

    def hash_node(self, l, r):
        st = np.zeros((1, 12), dtype=np.uint64)
        st[0, :4], st[0, 4:8] = _canon(np.asarray(l).reshape(4)), _canon(np.asarray(r).reshape(4))
        return self.permute_many(st)[0, :4].copy()

    def _leaves(self, rows):
        return self._sponge(rows)

    def _nodes(self, leaf_hashes, cap_size):
        layers = [np.asarray(leaf_hashes, dtype=np.uint64)]
        while layers[-1].shape[0] > cap_size:
            pairs = layers[-1].reshape(-1, 8)
            st = np.zeros((pairs.shape[0], 12), dtype=np.uint64)
            st[:, :8] = pairs
            layers.append(self.permute_many(st)[:, :4].copy())
        return np.concatenate(layers, axis=0)


def poseidon1_layer(numpy_permutation=True):
    return SpongeLayer(poseidon1_many_np if numpy_permutation else poseidon1_many_c)


def poseidon2_layer():
    return SpongeLayer(poseidon2_many_c)
