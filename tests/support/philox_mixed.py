"""NumPy restatement of `k_generate_mixed` (csrc/kernels_acq.hip), in the style of oracle/philox.py, whose Philox words it uses:
element E = (first_row + row) * d + k of stream `seed` has u = `_unit_words(E, seed)`; a column with L = levels[k] > 0 levels is
discrete -- index = min(floor(u L), L - 1), x = lo + index * ((hi - lo) / (L - 1)) (lo for L = 1) -- and a column with
levels[k] = 0 is real, x = lo + (hi - lo) * u.  Every product and sum is rounded separately, as in the kernel (fp contraction off)."""
import numpy as np

from oracle import philox


def mixed_box(lo, hi, levels, M, seed, first_row=0):
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    L = np.asarray(levels, dtype=np.float64)
    d = len(lo)
    E = np.arange(first_row * d, (first_row + M) * d, dtype=np.uint64)
    u = philox._unit_words(E, seed)
    k = (E % np.uint64(d)).astype(np.int64)
    width = hi[k] - lo[k]
    Lk = L[k]
    index = np.minimum(np.floor(u * Lk), Lk - 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        step = np.where(Lk > 1.0, width / (Lk - 1.0), 0.0)
    x = np.where(Lk > 0.0, lo[k] + index * step, lo[k] + width * u)
    return x.reshape(M, d)


def level_indices(levels, M, seed, first_row=0):
    """The level index of every element (columns with levels[k] = 0 get -1)."""
    L = np.asarray(levels, dtype=np.float64)
    d = len(L)
    E = np.arange(first_row * d, (first_row + M) * d, dtype=np.uint64)
    u = philox._unit_words(E, seed)
    Lk = L[(E % np.uint64(d)).astype(np.int64)]
    return np.where(Lk > 0, np.minimum(np.floor(u * Lk), Lk - 1.0), -1.0).astype(np.int64).reshape(M, d)
