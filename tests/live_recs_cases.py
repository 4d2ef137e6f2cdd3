"""Inputs shared by tests/test_live_recs_cpu.py and tests/test_gpu_live_recs.py, and the rule
of gnnrec.recs.update_recommendations restated with numpy on the host.  TEST
INFRASTRUCTURE: nothing here touches the device or the product's code.

A case is a pair of user / item tables before a refresh, the item and user rows the refresh
rewrote, the tables after it, and every user's exclusion row.  The CPU file checks on these
very tables that the rule settles only rows whose merged list is the exhaustive ranking's,
and that the share of rows it cannot settle stays under half the cap the GPU test asserts
for the same tables.

The rule, per clean user u with cached list L_u (k entries by (score desc, id asc), or
fewer: padded) and kappa = the key of its last real entry:
  K_u = the dirty eligible items with approximate score a(u, v) >= s_last - 2 EPS
  M_u = the k best of (L_u minus dirty items) | K_u, cached scores for the list's entries,
        refreshed scores for K_u
  settled  <=>  L_u was padded, or |M_u| = k and its k-th key is not worse than kappa
"""
import numpy as np

import recommend_cases as rc

EPS = rc.EPS
N_USERS, N_ITEMS = 300, 700   # three 128-row user tiles (the last partial), six item tiles
EXCLUDED = 5                  # random excluded items per user
SIGMA = 0.05                  # the small perturbation: new row = old + SIGMA * N(0, 1)
SEED = 0                      # the committed seed of every case
# (d, k, dirty items, dirty users): the three lane-group widths and the smallest width, the
# list lengths, dirty counts of one, a twentieth of the items and one across an item tile
GRID = (
    (4, 1, 1, 0), (4, 5, 35, 1), (4, 10, 129, 40),
    (64, 5, 35, 0), (64, 1, 129, 1), (64, 64, 1, 40),
    (128, 10, 35, 40), (128, 64, 129, 0), (128, 5, 1, 1),
    (256, 64, 35, 1), (256, 10, 129, 40), (256, 1, 35, 0),
)
SMALL = 35                    # 5 % of the items: the "small perturbation" case
UNSETTLED_CPU, UNSETTLED_GPU = 0.05, 0.10   # caps on the unsettled share of the clean rows
# A row's settle decision compares the merged list's k-th score with the old last score.  The
# device ranks fp32 cosines, the restatement float64 ones; an fp32 cosine of d <= 256 columns is
# within d 2^-23 <= 2^-15 of the float64 one, so the two can decide a row differently only
# where the two scores lie within 2 * 2^-15 of each other: rule() counts those rows as
# undecided, and the device may hand back that many more rows than the restatement, no more.
DECIDE_TOL = 2.0 ** -14


def tables(d, n_users=N_USERS, n_items=N_ITEMS, seed=SEED):
    rng = np.random.default_rng([seed, d, n_users, n_items])
    return (rng.standard_normal((n_users, d)).astype(np.float32),
            rng.standard_normal((n_items, d)).astype(np.float32))


def exclusions(n_users=N_USERS, n_items=N_ITEMS, per_user=EXCLUDED, seed=SEED):
    return rc.exclusions(n_users, n_items, min(per_user, n_items), min(per_user, n_items),
                         seed=seed + 1)


def pick(n, count, seed):
    """`count` distinct ids of [0, n), ascending int64."""
    return np.sort(np.random.default_rng(seed).permutation(n)[:count]).astype(np.int64)


def marks(n, ids):
    m = np.zeros(n, np.int32)
    m[ids] = 1
    return m


def perturbed(table, ids, seed, sigma=SIGMA):
    """The table with rows `ids` moved by sigma * N(0, 1)."""
    out = table.copy()
    rng = np.random.default_rng([seed, table.shape[1], len(ids)])
    out[ids] = (table[ids] + sigma * rng.standard_normal((len(ids), table.shape[1]))
                ).astype(np.float32)
    return out


def grid_case(d, k, n_di, n_du, seed=SEED):
    """-> dict(hu0, hi0, hu1, hi1, excl, du, di): the small perturbation of n_di item rows
    and n_du user rows."""
    hu0, hi0 = tables(d, seed=seed)
    di = pick(N_ITEMS, n_di, [seed, 1, d, k])
    du = pick(N_USERS, n_du, [seed, 2, d, k])
    return dict(hu0=hu0, hi0=hi0, hu1=perturbed(hu0, du, seed + 7), hi1=perturbed(hi0, di, seed + 8),
                excl=exclusions(seed=seed), du=du, di=di)


# ---------------------------------------------------------------- the rule, restated
def approx(hu, hi):
    """a(u, v): rows normalised in fp32, rounded to bf16, multiplied with fp32 accumulation
    (the restatement `_approx` of tests/test_recommend_cpu.py, on rc.unit_bf16)."""
    return rc.unit_bf16(hu) @ rc.unit_bf16(hi).T


def refreshed_scores(s0, hu1, hi1, du, di):
    """The score matrix after the refresh: only the rows of dirty users and the columns of
    dirty items are recomputed, so a clean pair keeps its bits (fact 1)."""
    s1 = s0.copy()
    if len(di):
        s1[:, di] = rc.cosine64(hu1, hi1[di])
    if len(du):
        s1[du, :] = rc.cosine64(hu1[du], hi1)
    return s1


def rule(s0, s1, a1, excl, k, du, di):
    """The merge of every CLEAN user, restated.  s0 / s1: scores before / after, a1: the
    approximate scores after.  -> (idx, vals [n_users, k] of the rule's lists, settled bool
    [n_users], kept: per user the set K_u, undecided bool [n_users]: the settle test compared
    two different items' scores less than DECIDE_TOL apart); rows of dirty users are left
    (-1, -inf), False."""
    n_users, n_items = s0.shape
    indptr, indices = excl
    dirty = np.zeros(n_items, bool)
    dirty[di] = True
    idx0, vals0 = rc.ranked(s0, indptr, indices, k)
    idx = np.full((n_users, k), -1, np.int64)
    vals = np.full((n_users, k), -np.inf, s0.dtype)
    settled = np.zeros(n_users, bool)
    undecided = np.zeros(n_users, bool)
    kept = [set() for _ in range(n_users)]
    clean = np.setdiff1d(np.arange(n_users), du)
    for u in clean:
        real = idx0[u] >= 0
        L, Ls = idx0[u][real], vals0[u][real]
        padded = L.size < k
        s_last = Ls[-1] if L.size else -np.inf
        elig = np.ones(n_items, bool)
        elig[[c for c in indices[indptr[u]:indptr[u + 1]] if 0 <= c < n_items]] = False
        K = np.nonzero(dirty & elig & (a1[u] >= np.float32(s_last) - np.float32(2 * EPS)))[0]
        kept[u] = set(K.tolist())
        stay = ~dirty[L]
        ids = np.concatenate([L[stay], K])
        sc = np.concatenate([Ls[stay], s1[u, K]])
        order = np.lexsort((ids, -sc))[:k]
        m = order.size
        idx[u, :m], vals[u, :m] = ids[order], sc[order]
        if padded:
            settled[u] = True
        elif m == k:
            kth = (sc[order[-1]], ids[order[-1]])
            kappa = (Ls[-1], L[-1])
            worse = kth[0] < kappa[0] or (kth[0] == kappa[0] and kth[1] > kappa[1])
            settled[u] = not worse
            undecided[u] = kth[1] != kappa[1] and abs(kth[0] - kappa[0]) < DECIDE_TOL
    return idx, vals, settled, kept, undecided
