"""The summation order of the one-wavefront-per-segment kernels (csrc/kernels_segments.hip.h), restated in numpy: lane l
of 64 adds the entries l, l + 64, l + 128, ... of the segment one after the other, starting from 0.0; the 64 partial sums
are then folded by the butterfly a[l] = a[l] + a[l ^ o] for o = 32, 16, 8, 4, 2, 1.  Every operation is one IEEE float64
addition, so the result has the kernel's bits."""
import numpy as np

LANES = 64


def wave_sum(v, keep=None):
    """The sum of the float64 values v of one segment in that order.  ``keep`` (boolean, like v): an entry that is not
    kept is skipped by the lane it falls to; it still takes its place in the walk."""
    v = np.asarray(v, dtype=np.float64)
    keep = np.ones(v.shape, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    a = np.zeros(LANES)
    for lane in range(LANES):
        for x in v[lane::LANES][keep[lane::LANES]]:
            a[lane] = a[lane] + x
    idx = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[idx ^ o]
    assert (a == a[0]).all()                               # every lane ends with the same value
    return a[0]


def sequential_sum(v):
    """v[0] + v[1] + ... from the left"""
    s = np.float64(0.0)
    for x in np.asarray(v, dtype=np.float64):
        s = s + x
    return s
