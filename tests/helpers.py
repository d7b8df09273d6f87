"""Shared test helpers: vector generation through the ORACLE (checker side)."""
import hashlib
import os
import random

import numpy as np

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493


def b2b(m, n=32):
    return hashlib.blake2b(m, digest_size=n).digest()


def arr(list_of_bytes, width):
    return np.frombuffer(b"".join(list_of_bytes), dtype=np.uint8).reshape(-1, width).copy()


def rng(seed):
    return random.Random(seed)


def rbytes(r, n):
    return bytes(r.getrandbits(8) for _ in range(n))


def corrupt(b: bytes, k: int) -> bytes:
    """consensus-testlib Test/Util/Corruption.hs:29-35: increment byte k mod len."""
    b = bytearray(b)
    i = k % len(b)
    b[i] = (b[i] + 1) & 0xFF
    return bytes(b)


def _context_under(env):
    """a context opened with env set (the schedule's knobs are read when a context opens)"""
    import praos_hip
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return praos_hip.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
