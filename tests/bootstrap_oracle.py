"""Host oracle of mts_bootstrap_sums (include/mts.h): the counter hash of common.h in numpy uint64 (the mirror tests/test_gpu_dropout.py
uses for the dropout masks), the multiply-shift draw, and the sums added one document after the other -- never np.sum, which adds
pairwise.  It is the project's own rule; there is nothing upstream to record."""
import numpy as np


def hash32(seed, idx):
    """mts_hash32(seed, idx) for an array of uint64 counters -> uint64 array holding the 32-bit values"""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(32)


def draws(seed, n, S):
    """int64 [S, n]: index j of resample s is (hash32(seed, s * n + j) * n) >> 32"""
    ctr = np.arange(S, dtype=np.uint64)[:, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :]
    return ((hash32(seed, ctr) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)            # < 2^32 * 2^20: no overflow


def sums(values, seed, S):
    """float64 [M, S]: values [M, n] (or [n]) summed over every resample's draws in draw order, starting from 0"""
    v = np.asarray(values, dtype=np.float64)
    v = v.reshape(1, -1) if v.ndim == 1 else v
    idx = draws(seed, v.shape[1], S)
    acc = np.zeros((v.shape[0], S), dtype=np.float64)
    for j in range(v.shape[1]):
        acc = acc + v[:, idx[:, j]]
    return acc
