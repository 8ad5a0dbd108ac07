"""The two edges of a ranked tail (k winners of one criterion over the stored values), shared by the GPU tests of the entries that
return ranks: more ranks than candidates, and a tie decided across the boundary of a partial second workgroup of 256 rows."""
import numpy as np


def pin_ranked_tail(upload, sweep, Xs):
    """`upload(X)` makes X the candidates; `sweep(k)` returns (best (k,), idx (k,), values (M,)) of one criterion over them.
    (a) M = 5, k = 8: ranks 0 .. 4 are the stable sort of the five values, ranks 5 .. 7 are (-inf, -1).
    (b) M = 257 with the maximum in rows 255 and 256 alone -- the last row of the first workgroup and the only row of the second:
        the lower index wins, at rank 0 for k = 1 and at ranks 0 and 1 for k = 2."""
    upload(Xs[:5])
    b, i, v = sweep(8)
    order = sorted(range(5), key=lambda j: (-v[j], j))
    assert list(i[:5]) == order and np.array_equal(b[:5], v[order])
    assert list(i[5:]) == [-1, -1, -1] and np.all(np.isneginf(b[5:]))
    X = np.array(Xs[:257], dtype=float)
    assert X.shape[0] == 257
    upload(X)
    v = sweep(1)[2]
    top, low = X[int(np.argmax(v))].copy(), X[int(np.argmin(v))].copy()
    X[int(np.argmax(v))] = low  # the maximum leaves its row ...
    X[255] = X[256] = top  # ... and stands in the two rows around the workgroup boundary
    upload(X)
    b1, i1, v1 = sweep(1)
    assert v1[255] == v1[256] == v1.max() and int(np.sum(v1 == v1.max())) == 2
    assert i1[0] == 255 and b1[0] == v1[255]
    b2, i2, _ = sweep(2)
    assert list(i2) == [255, 256] and b2[0] == v1[255] and b2[1] == v1[256]
