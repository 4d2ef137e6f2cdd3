"""Inputs and host restatements shared by tests/test_rank_mlp_cpu.py and
tests/test_gpu_rank_mlp.py (gnnrec.recs.rank_items(head=...)).  Tables and
exclusions are recommend_cases', heads recommend_mlp_cases', the definition and the pair sets
rank_cases'.  The CPU file shows on the host what the GPU tests lean on for these very inputs:
that the saturated head's pairs have exact ties on both sides of the held-out id, and that the
popularity vector below produces exact ties of the rating."""
import numpy as np

import recommend_cases as rc

COUNT_ROWS = (1, 7, 63, 64, 65, 130)     # one group; 64 = kDenseUsers; 65 and 130 = two and three
COUNT_ITEMS = (1, 31, 32, 33, 1023, 1024, 1025, 5000)   # tile (32) and chunk (1024) edges
POP_WEIGHTS = (0.0, 0.5)
POP_LEVELS = 8
SATURATED_D = 16
# host: at least this share of the saturated pairs has an item tied exactly with the held-out
# one below its id AND one above it (the list positions 2..10, the excluded items; not a
# list's first entry, nor the worst-ranked item, whose score is its own)
TIED_BOTH_SIDES_MIN = 0.6


def popularity(n_items=rc.N_ITEMS, seed=0):
    """fp32 [n_items] with POP_LEVELS distinct values j / POP_LEVELS: many repeats, every
    value and every product with POP_WEIGHTS exact in fp32."""
    rng = np.random.default_rng([seed, 91, n_items])
    return (rng.integers(0, POP_LEVELS, n_items) / POP_LEVELS).astype(np.float32)


def ratings32(S, Z, p):
    """rating.hpp restated in numpy fp32: expf(S) / Z + p, each operation rounded once.
    (numpy's fp32 exp need not be the device's expf bit for bit: for host checks of tie
    STRUCTURE only, never a reference for device values.)"""
    E = np.exp(S.astype(np.float32))
    return (E / Z.astype(np.float32)[:, None]).astype(np.float32) + p.astype(np.float32)[None, :]


def tied_both_sides(S, users, items):
    """Per pair: is some v < g and some v' > g with S[u, v] == S[u, g] == S[u, v']."""
    out = np.zeros(len(users), bool)
    for i, (u, g) in enumerate(zip(np.asarray(users).tolist(), np.asarray(items).tolist())):
        same = np.nonzero(S[u] == S[u, g])[0]
        out[i] = (same < g).any() and (same > g).any()
    return out
