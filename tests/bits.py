"""Comparing results bit for bit: the bytes of an array, equality of doubles as bit patterns with NaN in the same places, the
distance of two doubles in units in the last place, and the byte form the features' digests hash (each digest keeps its own layout
of such pieces)."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same_bits(a, b):
    """equal as bit patterns where neither is NaN, NaN in the same places"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def ulp_distance(a, b):
    """units in the last place between two finite doubles of the same sign"""
    x, y = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    return abs(int(x) - int(y))


def canonical_bytes(a):
    """the bytes of a float64 array with one NaN pattern: the positions count, not the payload"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.float64("nan"), a).tobytes()
