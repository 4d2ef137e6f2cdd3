"""Inputs shared by tests/test_recommend_cpu.py and tests/test_gpu_recommend.py: the CPU file
checks, with the algorithm restated in torch, that these very tables keep every row's
candidate count under the cap the GPU tests run with (they assert overflow_rows == 0)."""
import numpy as np

EPS = 2.0 ** -7 + 2.0 ** -11   # |bf16 approximate score - score| (csrc/recommend.hip)
N_USERS, N_ITEMS = 130, 5000
SAMPLE, CAND_CAP = 1024, 1024
DIMS = (16, 64, 128)
WIDE_D = 160  # dpad > 128: the scoring kernel's other form
KINDS = ("normal", "relu")
KS = (1, 10, 64)
KIND_IDS = {"normal": 0, "relu": 1, "lowrank": 2, "midpoint": 3}


def tables(kind, d, n_users=N_USERS, n_items=N_ITEMS, seed=0):
    """(h_user, h_item) fp32: 'normal', 'relu' (ReLU'd normal), 'lowrank' (rank-4 product,
    ReLU'd), 'midpoint' (every entry halfway between two neighbouring bf16 values)."""
    rng = np.random.default_rng([seed, d, KIND_IDS[kind]])
    if kind in ("normal", "relu"):
        hu = rng.standard_normal((n_users, d))
        hi = rng.standard_normal((n_items, d))
    elif kind == "lowrank":
        basis = rng.standard_normal((4, d))
        hu = rng.standard_normal((n_users, 4)) @ basis
        hi = rng.standard_normal((n_items, 4)) @ basis
    elif kind == "midpoint":
        def mid(shape):  # (1 + (2 j + 1) 2^-8) 2^e, signed: 8 bits of significand after the 1
            j = rng.integers(0, 128, shape)
            e = rng.integers(-3, 4, shape)
            sgn = rng.choice([-1.0, 1.0], shape)
            return sgn * (1.0 + (2 * j + 1) * 2.0 ** -8) * 2.0 ** e
        hu, hi = mid((n_users, d)), mid((n_items, d))
    else:
        raise KeyError(kind)
    if kind in ("relu", "lowrank"):
        hu, hi = np.maximum(hu, 0), np.maximum(hi, 0)
    return hu.astype(np.float32), hi.astype(np.float32)


def exclusions(n_users=N_USERS, n_items=N_ITEMS, lo=0, hi=60, seed=1):
    """Per user `lo`..`hi` distinct random items, unsorted -> (indptr int64, indices int32)."""
    rng = np.random.default_rng(seed)
    lists = [rng.choice(n_items, int(rng.integers(lo, hi + 1)), replace=False)
             for _ in range(n_users)]
    return csr(lists)


def csr(lists):
    indptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=indptr[1:])
    flat = np.concatenate([np.asarray(x, np.int32) for x in lists] + [np.zeros(0, np.int32)])
    return indptr, flat.astype(np.int32)


def ranked(scores, indptr, indices, k, rows=None):
    """The definition: per row the k best columns by (score desc, column asc) among those
    not in the row's user's exclusion list, padded with (-1, -inf) -> (idx, vals)."""
    n_rows, n_cols = scores.shape
    idx = np.full((n_rows, k), -1, np.int64)
    vals = np.full((n_rows, k), -np.inf, scores.dtype)
    for r in range(n_rows):
        u = r if rows is None else int(rows[r])
        cols = np.arange(n_cols)
        if indptr is not None:
            cols = np.setdiff1d(cols, indices[indptr[u]:indptr[u + 1]])
        order = cols[np.lexsort((cols, -scores[r, cols]))][:k]
        idx[r, :order.size] = order
        vals[r, :order.size] = scores[r, order]
    return idx, vals
