"""The Blake2s oracle's chunked trees (oracle/blake.py) at the leaf sizes the GPU's chunked trees are compared with: leaf 0 is
hashlib.blake2s of the concatenated canonical little-endian bytes of the two sources' chunks."""
import hashlib

import numpy as np

from oracle import blake as B

P = 2**64 - 2**32 + 1


def test_chunked_leaf_is_hashlib_of_the_concatenated_canonical_bytes():
    rng = np.random.default_rng(6)
    for log_e in (0, 3, 4, 5, 6):
        E, n = 1 << log_e, 2048
        c0, c1 = (rng.integers(0, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True) for _ in range(2))
        c0[0], c1[E - 1] = np.uint64(P), np.uint64(2**64 - 1)          # words >= p inside leaf 0
        tree = B.merkle_construct_chunked([c0, c1], E, 4)
        assert tree.shape == (2 * (n >> log_e) - 4, 4)
        msg = b"".join((int(w) % P).to_bytes(8, "little") for w in list(c0[:E]) + list(c1[:E]))
        assert tree[0].astype("<u8").tobytes() == hashlib.blake2s(msg).digest(), log_e
        assert tree[n >> log_e].astype("<u8").tobytes() == hashlib.blake2s(tree[0].astype("<u8").tobytes() + tree[1].astype("<u8").tobytes()).digest()
