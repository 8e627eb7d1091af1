"""The dropout mask of csrc/dropout.h restated in numpy (helper of tests/test_dropout_cpu.py and tests/test_gpu_dropout.py).

    keep(seed, offset, a, b, c)  <=>  hash32(seed, offset, a, b, c) >= thr,      thr = floor(p 2^32)

The GPU tests pin this restatement to the device function bit for bit (ops.dropout_mask_attn / ops.dropout_mask_rows), so the
statistical checks of the CPU tests are checks of the device function."""
import numpy as np

M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
M1, M2, M3, M4 = 0x9E3779B1, 0x85EBCA77, 0xCC9E2D51, 0x1B873593


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, offset, a):
    """(k0, k1) of the wave-uniform arguments: Python integers, exact"""
    z = _mix64(_mix64(_mix64(int(seed) & M64) ^ (int(offset) & M64)) ^ int(a))
    return z & M32, z >> 32


def hash32(seed, offset, a, b, c):
    """uint32 array over the broadcast of the integer arrays ``b`` and ``c`` (uint64 arithmetic masked to 32 bits after every step)"""
    k0, k1 = key(seed, offset, a)
    b = np.asarray(b, dtype=np.uint64)
    c = np.asarray(c, dtype=np.uint64)
    m = np.uint64(M32)
    x = ((b + np.uint64(k0)) & m) * np.uint64(M1) & m
    x = x ^ (x >> np.uint64(16))
    y = (b * np.uint64(M2) + np.uint64(k1)) & m
    h = ((x + c) & m) * np.uint64(M3) & m
    h = h ^ (h >> np.uint64(15))
    h = ((h + y) & m) * np.uint64(M4) & m
    return h.astype(np.uint32)


def thr(p):
    return int(float(p) * 4294967296.0)


def mask_attn(p, seed, offset, H, n_total):
    """uint8 [H, n_total, n_total]: 1 = kept; (a, b, c) = (head, packed query row, packed key row)"""
    r = np.arange(n_total)
    return np.stack([hash32(seed, offset, h, r[:, None], r[None, :]) >= np.uint32(thr(p)) for h in range(H)]).astype(np.uint8)


def mask_rows(p, seed, offset, n, C):
    """uint8 [n, C]: 1 = kept; (a, b, c) = (0, row, column)"""
    return (hash32(seed, offset, 0, np.arange(n)[:, None], np.arange(C)[None, :]) >= np.uint32(thr(p))).astype(np.uint8)
