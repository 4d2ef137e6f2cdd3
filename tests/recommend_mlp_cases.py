"""Heads and host restatements shared by tests/test_recommend_mlp_cpu.py and
tests/test_gpu_recommend_mlp.py (the many-user top-k for the MLP head).  Tables, exclusions
and ranked() come from tests/recommend_cases.py; the CPU file checks on the host what the GPU
tests lean on for these very inputs: that no row's candidate count comes near the cap they
run with, and that the saturated head really saturates."""
import numpy as np
import torch

import recommend_cases as rc

KINDS = ("normal", "relu", "lowrank")
DIMS = rc.DIMS
KS = rc.KS
USER_GROUP = 64   # kDenseUsers of csrc/heads.hip: users scored per staged item tile
STORE_USERS = (1, 7, 130, USER_GROUP - 1, USER_GROUP + 1)
STORE_ITEMS = (1, 31, 32, 33, 255, 257, 5000)
FILTER_CAPS = (1, 64, 4096)
SATURATED_SCALE = 16.0  # host: 99.7 % of the 130 x 5000 scores are 1.0f, at least 4720 per row


def head(d):
    """PredictingLayer(d) under torch.manual_seed(0), in eval()."""
    from gnnrec.nn import PredictingLayer
    torch.manual_seed(0)
    return PredictingLayer(d).eval()


def saturated_head(d):
    """The same head with a non-negative output layer, times SATURATED_SCALE: the hidden-2
    activations are ReLU'd, so every pre-sigmoid value is large and positive and most scores
    are exactly 1.0f."""
    pl = head(d)
    with torch.no_grad():
        pl.output.weight.copy_(pl.output.weight.abs() * SATURATED_SCALE)
        pl.output.bias.copy_(pl.output.bias.abs() * SATURATED_SCALE)
    return pl


def host_scores(pl, hu, hi, chunk=8):
    """The head restated in torch on the CPU, fp32: sigmoid(w3 . relu(W2 relu(P + Q) + b2)
    + b3) with P = hu W1a^T + b1, Q = hi W1b^T -> [n_users, n_items] numpy."""
    d = hu.shape[1]
    with torch.no_grad():
        W1 = pl.hidden_1.weight
        P = torch.from_numpy(hu) @ W1[:, :d].T + pl.hidden_1.bias
        Q = torch.from_numpy(hi) @ W1[:, d:].T
        out = []
        for u0 in range(0, P.shape[0], chunk):
            a = torch.relu(P[u0:u0 + chunk, None, :] + Q[None, :, :])
            b = torch.relu(a @ pl.hidden_2.weight.T + pl.hidden_2.bias)
            out.append(torch.sigmoid(b @ pl.output.weight.reshape(-1) + pl.output.bias))
    return torch.cat(out).numpy()


def filter_counts(S, indptr, indices, k, sample):
    """recommend(head=...)'s filter on a score matrix: tau = the k-th best non-excluded
    score of the item prefix (-inf when fewer than k are eligible there), the count of
    items with score >= tau per row."""
    m = min(sample, S.shape[1])
    counts = np.zeros(S.shape[0], np.int64)
    for r in range(S.shape[0]):
        pre = S[r, :m].copy()
        ex = indices[indptr[r]:indptr[r + 1]]
        pre[ex[ex < m]] = -np.inf
        tau = np.sort(pre)[::-1][k - 1] if m >= k else -np.inf
        counts[r] = (S[r] >= tau).sum()
    return counts
