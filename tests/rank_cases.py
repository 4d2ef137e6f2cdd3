"""The definition, pair sets and metrics shared by tests/test_rank_cases_cpu.py and
tests/test_gpu_rank.py (gnnrec.recs.rank_items / ranks_to_metrics), restated in
numpy from a score matrix.  Tables, exclusions and the fp64 cosine are recommend_cases'.

    rank(u, g) = 1 + #{v not in exclude(u), v != g : s(u,v) > s(u,g) or (s(u,v) == s(u,g), v < g)}
    rank(u, g) = 0 where g is in exclude(u)

The base shape is recommend_cases' 130 users x 5000 items (5000 = 4 * 1024 + 7 * 128 + 8: a
partial 1024-item partial, a partial 128-item step and an 8-of-32 subtile) at d in DIMS (160
takes the dpad > 128 staging), all four kinds, eight pairs per user."""
import numpy as np

import recommend_cases as rc

DIMS = (16, 64, 128, 160)
KINDS = rc.KINDS
CAND_CAP = 1024
PAIRS_PER_USER = 8
COS_TOL = 1e-5      # sddmm_cos against the fp64 cosine (the project's tolerance for the head)
KS = (1, 10, 50)


def eps(d):
    """rank_eps restated: (4 dpad + 32) 2^-24, dpad = d rounded up to a multiple of 8."""
    return (4.0 * ((d + 7) // 8 * 8) + 32.0) * 2.0 ** -24


def ranks(S, users, items, indptr=None, indices=None):
    """The definition, from score rows S [n_users, n_items] -> int64 [P]."""
    n = S.shape[1]
    ids = np.arange(n)
    out = np.zeros(len(users), np.int64)
    for p, (u, g) in enumerate(zip(np.asarray(users).tolist(), np.asarray(items).tolist())):
        row = S[u]
        t = row[g]
        ahead = (row > t) | ((row == t) & (ids < g))
        if indptr is not None:
            ex = np.unique(indices[indptr[u]:indptr[u + 1]])
            if (ex == g).any():
                continue                                  # excluded: rank 0
            ahead[ex[(ex >= 0) & (ex < n)]] = False
        out[p] = 1 + int(ahead.sum())
    return out


def pairs(S, excl, k=10):
    """Eight pairs per user from the user's ranking of S with the exclusions applied: five
    positions of its top-k list (user u takes positions (5 u + j) % k, so two neighbouring
    users cover every position 1..k), its worst-ranked item, an excluded item (the first of
    its list; item (37 u) % n_items where the list is empty), and pair 0 again.
    -> (users, items) int64 [8 n_users]."""
    indptr, indices = excl
    n_users, n_items = S.shape
    idx, _ = rc.ranked(S, indptr, indices, k)
    us, gs = [], []
    for u in range(n_users):
        ex = indices[indptr[u]:indptr[u + 1]]
        cols = np.setdiff1d(np.arange(n_items), ex)
        worst = cols[np.lexsort((cols, -S[u, cols]))][-1]
        mine = [idx[u][(5 * u + j) % k] for j in range(5)]
        mine += [worst, ex[0] if ex.size else (37 * u) % n_items, mine[0]]
        us += [u] * PAIRS_PER_USER
        gs += [int(g) for g in mine]
    return np.asarray(us, np.int64), np.asarray(gs, np.int64)


def metrics(rank, users, ks):
    """ranks_to_metrics restated with Python floats."""
    rank, users = np.asarray(rank).tolist(), np.asarray(users).tolist()
    nan = float("nan")
    P = len(rank)
    ranked = [r for r in rank if r > 0]
    out = {"unranked": P - len(ranked),
           "mrr": sum(1.0 / r for r in ranked) / len(ranked) if ranked else nan,
           "mean_rank": sum(ranked) / len(ranked) if ranked else nan}
    per_user = {}
    for u, r in zip(users, rank):
        per_user.setdefault(u, set())
        if r > 0:
            per_user[u].add(r)            # a rank names one item: distinct ranks = distinct items
    for k in ks:
        out[f"recall@{k}"] = sum(1 for r in rank if 1 <= r <= k) / P if P else nan
        out[f"hit_rate@{k}"] = (sum(1 for s in per_user.values() if any(r <= k for r in s)) /
                                len(per_user)) if per_user else nan
        nd = []
        for s in per_user.values():
            if not s:
                continue
            dcg = sum(1.0 / np.log2(1.0 + r) for r in sorted(s) if r <= k)
            idcg = sum(1.0 / np.log2(1.0 + j) for j in range(1, min(k, len(s)) + 1))
            nd.append(dcg / idcg)
        out[f"ndcg@{k}"] = sum(nd) / len(nd) if nd else nan
    return out


def band_counts(C, users, items, d):
    """Items whose fp64 cosine lies within 2 (eps(d) + COS_TOL) of the pair's, per pair: an
    upper bound on what the count pass can put into the pair's band (|a - c| and |t - c| are
    each within eps + COS_TOL)."""
    w = 2.0 * (eps(d) + COS_TOL)
    t = C[users, items][:, None]
    return (np.abs(C[users] - t) <= w).sum(1)
