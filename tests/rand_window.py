"""Windows of the libc rand() stream chosen by the draws they lead to (TEST INFRASTRUCTURE).

glibc's rand() is x_j = x_{j-31} + x_{j-3} (mod 2^32), rand() = x_j >> 1 (oracle_bind.glibc_window, mchip_generators.hip).  The recurrence
runs backwards as well, x_{j-31} = x_j - x_{j-3}, so any 31 consecutive words fix the whole stream: `window_placing` puts
chosen draws at draw P..P+30 (the low bit of each word is free) and steps back to the 31 words behind draw 0, the form
mchip_simulate_genotypes, mchip_mstep_from_rand_partition and `ref_time --bootstrap` take.  `draws` runs a window forwards."""
import functools

import numpy as np

LAG = 31
RAND_MAX = (1 << 31) - 1


def window_placing(draws, pos, low_bits=0, fill_seed=0):
    """The window (31 uint32 words behind draw 0, oldest first) of the stream whose draws pos, pos+1, ... are `draws` (at most
    31 values in [0, RAND_MAX]).  Draws of the 31-word block not given are seeded random values; `low_bits` (scalar or one
    per draw) is the free low bit of each word."""
    return np.array(_window(tuple(int(v) for v in draws), int(pos), tuple(np.broadcast_to(low_bits, (len(draws),)).tolist()),
                            int(fill_seed)), dtype=np.uint32)


@functools.lru_cache(maxsize=256)
def _window(draws, pos, low_bits, fill_seed):
    assert 0 < len(draws) <= LAG and pos >= 0 and all(0 <= v <= RAND_MAX for v in draws)
    words = np.random.default_rng(fill_seed).integers(0, 1 << 32, LAG, dtype=np.uint64).astype(np.uint32)
    words[:len(draws)] = (np.array(draws, dtype=np.uint64) << np.uint64(1) | np.array(low_bits, dtype=np.uint64) & np.uint64(1)).astype(np.uint32)
    # x[e] holds x_{e-31}: x_{-31} .. x_{pos+30}; x[low:] is known
    x = np.zeros(pos + 2 * LAG, dtype=np.uint32)
    low = pos + LAG
    x[low:] = words
    with np.errstate(over="ignore"):
        while low > 0:
            # x_{j-31} = x_j - x_{j-3} for the 28 indices j whose x_{j-3} is known and whose x_{j-31} is not
            j = np.arange(max(low + 3, LAG), low + LAG)
            x[j - LAG] = x[j] - x[j - 3]
            low = int(j[0]) - LAG
    return x[:LAG].tolist()


def draws(window, n):
    """rand() n times from the 31-word window (a plain loop: n is at most a few times 10^5 in tests)"""
    x = [int(w) for w in window]
    out = np.empty(n, dtype=np.int64)
    for t in range(n):
        v = (x[t] + x[t + 28]) & 0xFFFFFFFF
        x.append(v)
        out[t] = v >> 1
    return out
