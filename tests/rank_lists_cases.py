"""Held-out LISTS and host restatements shared by tests/test_rank_lists_cpu.py and
tests/test_gpu_rank_lists.py (gnnrec.recs.rank_lists / list_pairs).  Tables,
exclusions, heads, the definition and the pair sets are recommend_cases', recommend_mlp_cases',
rank_cases' and rank_mlp_cases'; this file adds the grouping of pairs into per-user lists, the
list generator of the kernel tests, and numpy restatements of list_pairs and of the row plan."""
import numpy as np

import rank_cases as rk
import recommend_cases as rc

BUDGET = 16          # kDenseListSlots of csrc/heads.hip: list entries per row of the count pass
LONG = 200           # entries of the one long list: 13 rows of the plan, the last one half full
COUNT_ROWS = (1, 63, 64, 65, 130)     # users; 64 = kDenseUsers (the plan's rows are more)
COUNT_ITEMS = (1, 31, 32, 33, 1023, 1024, 1025, 5000)   # tile (32) and chunk (1024) edges
LENGTHS = (0, 1, 2, BUDGET - 1, BUDGET, BUDGET + 1)
PLAN_LENGTHS = (0, 1, BUDGET - 1, BUDGET, BUDGET + 1, 5 * BUDGET)
EMPTY_USER, SINGLE_USER, LONG_USER = 3, 5, 7     # grouped(): users with 0, 1 and LONG entries
BATCHES = (1, 7, 130)
# Share of the saturated head's list entries with an item tied exactly below AND above them.
# Reasoning, not measurement: 99.7 % of that head's scores are 1.0f, so an entry at a random id
# is tied on both sides; item 0 and the last item never are.  Lists of the six LENGTHS hold
# 51 entries per six lists, at most 9 of them forced to item 0 / the last item: 0.82 expected,
# the long list only raises it.  0.6 leaves room for the draw of the lengths.
TIED_BOTH_SIDES_MIN = 0.6


def list_pairs(user_rows, indptr, indices):
    """recs.list_pairs restated: the served users' lists concatenated in user_rows order, each
    in CSR order -> (users, items) int64."""
    indptr = np.asarray(indptr)
    if user_rows is None:
        user_rows = np.arange(indptr.size - 1)
    us, gs = [], []
    for u in np.asarray(user_rows).tolist():
        seg = np.asarray(indices[indptr[u]:indptr[u + 1]], np.int64)
        us += [u] * seg.size
        gs += seg.tolist()
    return np.asarray(us, np.int64), np.asarray(gs, np.int64)


def row_plan(lens, budget=BUDGET):
    """recs._list_row_plan restated with a Python loop: a list of n entries takes ceil(n /
    budget) rows of consecutive slots -> (owner int64 [R], lptr int64 [R + 1])."""
    owner, lptr, at = [], [0], 0
    for i, n in enumerate(np.asarray(lens).tolist()):
        for k in range(0, n, budget):
            owner.append(i)
            lptr.append(at + min(n, k + budget))
        at += n
    return np.asarray(owner, np.int64), np.asarray(lptr, np.int64)


def kernel_lists(n_users, n_items, seed=0):
    """One list per user for the kernel tests, lengths drawn from LENGTHS and user
    (n_users - 1) // 2 given LONG entries.  As far as its length allows a list holds the last
    item (entry 0), item 0 (entry 1) and a duplicate (its last entry copies entry 0 — two
    entries, or from four on a random earlier one); a list of two is (last, 0) for even users
    and a duplicated random id for odd ones.  The rest are random ids.  -> (indptr, indices)."""
    rng = np.random.default_rng([seed, 17, n_users, n_items])
    lens = rng.choice(LENGTHS, n_users)
    lens[(n_users - 1) // 2] = LONG
    lists = []
    for u, n in enumerate(lens.tolist()):
        x = rng.integers(0, n_items, n)
        if n >= 1:
            x[0] = n_items - 1
        if n >= 2:
            x[1] = 0
        if n == 2 and u % 2:
            x[:] = rng.integers(0, n_items)
        if n >= 3:
            x[-1] = x[0] if n == 3 else x[rng.integers(2, n - 1)]
        lists.append(x)
    return rc.csr(lists)


def regroup(us, gs, n_users=rc.N_USERS):
    """Pairs -> per-user lists, each in pair order."""
    lists = [[] for _ in range(n_users)]
    for u, g in zip(np.asarray(us).tolist(), np.asarray(gs).tolist()):
        lists[u].append(g)
    return lists


def grouped(us, gs, n_items, n_users=rc.N_USERS, seed=0):
    """rank_cases.pairs' eight pairs per user regrouped into per-user lists (pair order kept:
    the lists are unsorted and repeat their first item), then EMPTY_USER's list emptied,
    SINGLE_USER's cut to one entry and LONG_USER's filled up to LONG entries with random ids
    (repeats among them).  -> (indptr int64, indices int32)."""
    rng = np.random.default_rng([seed, 23, n_items])
    lists = regroup(us, gs, n_users)
    assert all(len(x) == rk.PAIRS_PER_USER for x in lists)
    lists[EMPTY_USER] = []
    lists[SINGLE_USER] = lists[SINGLE_USER][:1]
    more = rng.integers(0, n_items, LONG - len(lists[LONG_USER]))
    more[-1] = more[0]
    lists[LONG_USER] = lists[LONG_USER] + more.tolist()
    return rc.csr(lists)
