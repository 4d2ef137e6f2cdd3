"""Shared by the packed-row tests: a numpy restatement of the packed row format
(csrc/pack_rows.hpp) and source tables that hold its edge cases."""
import numpy as np

D, WORDS, HDR, SLOTS = 128, 96, 8, 88
DENSE_BIT = np.uint32(1 << 31)
NNZ_CASES = (0, 1, 87, 88, 89, 128)


def numpy_pack(x):
    """packed uint32 [n, 96] of fp32 [n, 128]: mask[4], pre (4 bytes), nnz | dense << 31, two
    zero words, then the non-zero 32-bit patterns in column order (none for a dense row)."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    n = bits.shape[0]
    p = np.zeros((n, WORDS), dtype=np.uint32)
    for r in range(n):
        nz = bits[r] != 0
        for w in range(4):
            word = 0
            for b in np.nonzero(nz[32 * w:32 * w + 32])[0]:
                word |= 1 << int(b)
            p[r, w] = word
            p[r, 4] |= np.uint32(int(nz[:32 * w].sum()) << (8 * w))
        nnz = int(nz.sum())
        p[r, 5] = nnz
        if nnz > SLOTS:
            p[r, 5] |= DENSE_BIT
        else:
            p[r, HDR:HDR + nnz] = bits[r][nz]
    return p


def numpy_unpack(p, x_dense):
    out = np.zeros((p.shape[0], D), dtype=np.uint32)
    for r in range(p.shape[0]):
        if p[r, 5] & DENSE_BIT:
            out[r] = np.ascontiguousarray(x_dense[r], dtype=np.float32).view(np.uint32)
            continue
        q = 0
        for c in range(D):
            if (int(p[r, c >> 5]) >> (c & 31)) & 1:
                out[r, c] = p[r, HDR + q]
                q += 1
    return out.view(np.float32)


def row_with_nnz(rng, nnz):
    """One fp32 row with exactly `nnz` non-zero bit patterns at random columns."""
    x = np.zeros(D, dtype=np.float32)
    cols = rng.permutation(D)[:nnz]
    v = rng.standard_normal(nnz).astype(np.float32)
    v[v == 0] = 1.0
    x[cols] = v
    return x


def edge_rows(rng):
    """Rows with nnz 0, 1, 87, 88, 89 and 128, then rows holding -0.0, NaN (with a payload)
    and a denormal: all three are non-zero bit patterns and must survive bit for bit."""
    rows = [row_with_nnz(rng, k) for k in NNZ_CASES]
    special = np.array([0x80000000, 0x7FC01234, 0x00000001, 0xFFFFFFFF], dtype=np.uint32)
    for k in (3, 88):
        x = row_with_nnz(rng, k).view(np.uint32)
        nz = np.nonzero(x)[0]
        x[nz[:3]] = special[:3]
        rows.append(x.view(np.float32))
    x = np.zeros(D, dtype=np.uint32)
    x[[0, 31, 32, 127]] = special  # the ends of the mask words
    rows.append(x.view(np.float32))
    return np.stack(rows)


def relu_table(rng, n, p_zero=0.5):
    """[n, 128] with each entry zero with probability p_zero (a post-ReLU table)."""
    x = rng.standard_normal((n, D)).astype(np.float32)
    x[rng.random((n, D)) < p_zero] = 0.0
    return x


def source_table(rng, n):
    """A ReLU-like table of n >= 64 rows with the edge rows sprinkled through it, and dense
    rows next to sparse ones so both meet in one gather step."""
    x = relu_table(rng, n)
    e = edge_rows(rng)
    at = rng.permutation(n)[:len(e)]
    x[at] = e
    for r in range(5, n, 7):  # every 7th row dense: nnz 89..128
        x[r] = row_with_nnz(rng, int(rng.integers(89, 129)))
    return x
