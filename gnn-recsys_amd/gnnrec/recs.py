"""Recommendation scoring + top-k — drop-ins for reference
src/metrics.py (`create_ground_truth` :9-17, `create_already_bought` :20-28,
`get_recs` :31-78, `recs_to_metrics` :81-107, `get_metrics_at_k` :110-134),
consumed by main_inference.py:153-166.

The reference loops over users in Python: repeat the user embedding once per
item, cosine (or the MLP head) against every item, copy to the host, argsort,
filter already-bought items, keep k.  Here a batch of users is scored against
every item in one fp32 MFMA GEMM of L2-normalised embeddings (gnnrec_gemm_f32),
or by the re-associated MLP head (gnnrec_edge_mlp_dense_store_f32: every pair
without id arrays, the bits of gnnrec_edge_mlp_f32), and
gnnrec_topk_rows_f32 selects the k best non-bought items per user on the
device.  Only the [users, k] result leaves the GPU.

`recommend` / `recommend_for_graph` / `recs_to_metrics_device` serve many users (the
reference's `--user_ids all`) on device tensors: the same ranking for the cosine head, bit
for bit, from a bf16 MFMA prefilter and an fp32 rescoring of the few items it cannot rule
out, with no score matrix.  With `head=` (a PredictingLayer) they rank by
the MLP head's score instead, exactly and again without a score matrix.

`rank_items` / `rank_for_graph` / `ranks_to_metrics` evaluate: the exact position of every
held-out item in the cosine head's exhaustive ranking, from one fp32 MFMA pass over the items
whose epilogue counts instead of storing; with `head=` the position in the MLP
head's ranking (and with `popularity=` in its popularity-weighted one), from a counting
epilogue on the dense MLP kernel that compares the final fp32 value.
`rank_lists` / `rank_lists_for_graph` / `list_pairs` take held-out LISTS, one per user, and give
the same ranks with each user scored once for the MLP head.
"""
from __future__ import annotations

import contextlib
import math
import time
from collections import defaultdict

import numpy as np
import torch

from . import _lib, ops


def create_ground_truth(users, items):
    """{user: [items actually bought]} (reference src/metrics.py:9-17)."""
    d = defaultdict(list)
    for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist()):
        d[u].append(i)
    return d


def create_already_bought(g, bought_eids, etype='buys'):
    """{user: [items already bought]} from the bought edges (src/metrics.py:20-28)."""
    users, items = g.find_edges(bought_eids, etype=etype)
    return create_ground_truth(torch.as_tensor(users).cpu().numpy(),
                               torch.as_tensor(items).cpu().numpy())


def topk_rows(scores: torch.Tensor, k: int, exclude_indptr=None, exclude_indices=None):
    """Per row: k best columns by (score desc, column asc), excluded columns skipped
    -> (vals, idx), padded with (-inf, -1) where a row has fewer than k eligible columns.
    A -inf score is a score: its column is returned, in column order after every finite
    one (callers that mask to -inf rewrite those indices themselves).  exclude_indptr is a
    contiguous int64 [n_rows + 1] over exclude_indices (int64 column ids, any order,
    duplicates and ids outside [0, n_cols) allowed).  No NaN."""
    n_rows, n_cols = scores.shape
    vals = torch.empty((n_rows, k), dtype=torch.float32, device=scores.device)
    idx = torch.empty((n_rows, k), dtype=torch.int64, device=scores.device)
    _lib.torch_ops().topk_rows(scores, k, exclude_indptr, exclude_indices, vals, idx)
    return vals, idx


def _normalize_rows(x: torch.Tensor) -> torch.Tensor:
    """x / ||x|| per row (zero rows stay zero) — the fused GEMM with an identity weight
    and its L2-norm epilogue (exact: x·I adds only zero products)."""
    eye = torch.eye(x.shape[1], dtype=torch.float32, device=x.device)
    return ops.gemm(x.contiguous(), eye, l2norm=True)


def get_recs(g, h, model, embed_dim, k, user_ids, already_bought_dict,
             remove_already_bought=True, cuda=True, device=None, pred: str = 'cos',
             use_popularity: bool = False, weight_popularity=1, batch_size: int = 1024):
    """Top-k recommendations for every user in user_ids: {user: np.ndarray[k]}."""
    if pred not in ('cos', 'nn'):
        raise KeyError(f'Prediction function {pred} not recognized.')
    dev = h['item'].device
    items = h['item'].contiguous()
    n_items = items.shape[0]
    user_ids = [int(u) for u in user_ids]
    if pred == 'cos':
        items_hat = _normalize_rows(items)
    else:
        layer = model.pred_fn.layer_nn
        W1 = layer.hidden_1.weight
        Q = ops.gemm(items, W1[:, embed_dim:])                     # item half of hidden_1
    pop = None
    if use_popularity:
        pop = g.ndata['popularity']['item'].reshape(-1).to(dev).float() * weight_popularity
    if pred == 'nn':
        batch_size = max(1, min(batch_size, (1 << 26) // max(1, n_items)))
    recs = {}
    for b0 in range(0, len(user_ids), batch_size):
        ub = user_ids[b0:b0 + batch_size]
        users = h['user'][torch.tensor(ub, device=dev)].contiguous()
        if pred == 'cos':
            scores = ops.gemm(_normalize_rows(users), items_hat)   # [B, n_items] cosine
        else:
            P = ops.gemm(users, W1[:, :embed_dim], bias=layer.hidden_1.bias)
            # every pair without id arrays; the values are bitwise ops.edge_mlp's
            scores = ops.edge_mlp_dense_store(P, Q, layer.hidden_2.weight, layer.hidden_2.bias,
                                              layer.output.weight.reshape(-1), layer.output.bias)
        if pop is not None:  # softmax over items, plus weighted popularity (metrics.py:69-72)
            scores = torch.softmax(scores, dim=1) + pop
        ex_ptr = ex_idx = None
        if remove_already_bought:
            lists = [already_bought_dict.get(u, []) for u in ub]
            ip = np.zeros(len(lists) + 1, np.int64)
            np.cumsum([len(x) for x in lists], out=ip[1:])
            flat = np.fromiter((i for x in lists for i in x), dtype=np.int64, count=int(ip[-1]))
            ex_ptr = torch.from_numpy(ip).to(dev)
            ex_idx = torch.from_numpy(flat).to(dev) if flat.size else torch.zeros(1, dtype=torch.int64, device=dev)
        _, top = topk_rows(scores, k, ex_ptr, ex_idx)
        top = top.cpu().numpy()
        for r, u in enumerate(ub):
            row = top[r]
            recs[u] = row[row >= 0]
    return recs


# ---- exact top-k behind a bf16 MFMA prefilter (csrc/recommend.hip) ----------
# |a - score| <= REC_EPS for the approximate score a (bf16 operands, fp32 accumulation) of
# two normalised rows with d <= REC_MAX_D; the derivation is in csrc/recommend.hip and
# DESIGN.md §16.  The library holds the constant it filters with; this one is for callers.
REC_EPS = 2.0 ** -7 + 2.0 ** -11
REC_MAX_D = 2048
REC_MAX_CAP = 4096
# |Ra - R| <= REC_RATING_BAND / Z_u + REC_RATING_SLACK max(p) for the rating R = expf(score) /
# Z_u + p_v and its approximation Ra from the bf16 score (csrc/recommend.hip, THE RATING BAND;
# DESIGN.md §19): e^(1 + eps) ((e^eps - 1) + 2^-20) and 2^-22, the library's constants.
REC_RATING_BAND = math.exp(1.0 + REC_EPS) * (math.expm1(REC_EPS) + 2.0 ** -20)
REC_RATING_SLACK = 2.0 ** -22


def _to_ratings(sc, c0, rating):
    """A chunk of exhaustive score rows to ratings in place; rating = (Z over the rows or
    None, p): without Z the denominators are summed from the score rows themselves."""
    Z, p = rating
    Zc = ops.exp_rowsum(sc) if Z is None else Z[c0:c0 + sc.shape[0]].contiguous()
    ops.rating_rows_(sc, Zc, p)


def _rows_exact(scorer, k, rows, exclude, vals, idx, out_pos, Z=None):
    """The fallback, always exact: every item scored in fp32 by the scorer's head for the
    user rows `rows` (int64 device tensor), in chunks of 2^26 / n_items rows, excluded items
    masked to -inf, topk_rows; results into vals/idx at rows `out_pos`.  With a popularity
    the score rows become R = expf(score) / Z + p first (Z [len(rows)]; None: summed from the
    rows, g = the score)."""
    n_items = scorer.h_item.shape[0]
    if rows.numel() == 0:
        return
    if n_items == 0:
        vals[out_pos] = float('-inf')
        idx[out_pos] = -1
        return
    step = max(1, (1 << 26) // n_items)
    for c0 in range(0, rows.numel(), step):
        r = rows[c0:c0 + step].contiguous()
        sc = scorer.score_rows(r)
        if scorer.p is not None:
            _to_ratings(sc, c0, (Z, scorer.p))
        if exclude is not None:
            ops.mask_excluded(sc, r, exclude[0], exclude[1])
        v, i = topk_rows(sc, k)
        i = torch.where(v == float('-inf'), torch.full_like(i, -1), i)  # masked or past the end
        pos = out_pos[c0:c0 + step]
        vals[pos] = v
        idx[pos] = i


# ---- the scorers: what _recommend and _rows_exact need of a head, and nothing else ----------
#   fast_ok                     does the fast path (and the denominator kernel) exist here
#   prepare(m, pop_sample)      once per call on the fast path: the item table the filter
#                               reads and the rows of the threshold sample; sets col_ids
#   batch(rows) -> st           per-batch state, st[1] the rows' Z (None without popularity)
#   sample_scores(st)           scores (ratings) of the sample columns [B, sample]
#   keep(st, tau, counts, cap)  one pass over all items -> the kept candidates
#   rank(st, kept, counts, rows, k, ex0, ex1, vals, idx)
#   score_rows(r)               exhaustive fp32 score rows [len(r), n_items]
#   denominators_of(rows)       with popularity: Z of a batch of rows
# Each is built once per call from (h_user, h_item[, head]) and p (popularity * weight, or
# None); whether it scores or rates is the scorer's business: p is a property of the input.
class _Scorer:
    col_ids = None      # item id per sample column (int32); None: the columns are a prefix

    def _take_sample(self, table, m, pop_sample):
        """self.sample = the threshold sample's rows of `table`: the prefix [0, m) as a view,
        or with popularity the prefix and the popular items, gathered (both once per call)."""
        if self.p is None:
            self.sample = table[:m]
            return
        self.col_ids = _popular_sample(self.p, m, pop_sample)
        cols = self.col_ids.to(torch.int64)
        self.p_col = self.p[cols].contiguous()
        self.sample = table[cols].contiguous()


class _CosHead(_Scorer):
    """The cosine head behind the bf16 MFMA prefilter (rating: §19)."""

    def __init__(self, h_user, h_item, p=None):
        d = h_item.shape[1]
        self.h_user, self.h_item, self.p = h_user, h_item, p
        self.fast_ok = d % 4 == 0 and 4 <= d <= REC_MAX_D    # the widths of the MFMA kernels
        if p is not None and self.fast_ok and h_item.shape[0]:
            self.items_f32 = ops.normalize_rows_f32(h_item)      # converted once per call

    def prepare(self, m, pop_sample):
        self.items_bf = ops.normalize_rows_bf16(self.h_item)     # converted once per call
        self._take_sample(self.items_bf, m, pop_sample)
        if self.p is not None:
            self.pmax = self.p.max().reshape(1)

    def denominators_of(self, rows):
        return ops.cos_denominators(ops.normalize_rows_f32(self.h_user, rows), self.items_f32)

    def batch(self, rows):
        Zb = None if self.p is None else self.denominators_of(rows)
        return ops.normalize_rows_bf16(self.h_user, rows), Zb

    def sample_scores(self, st):
        if self.p is None:
            return ops.score_bf16_store(st[0], self.sample)
        return ops.score_bf16_store_rating(st[0], self.sample, st[1], self.p_col)

    def keep(self, st, tau, counts, cand_cap):
        users_bf, Zb = st
        cand = torch.empty((tau.numel(), cand_cap), dtype=torch.int32, device=tau.device)
        if self.p is None:    # the kernel itself subtracts 2 REC_EPS
            ops.score_bf16_filter(users_bf, self.items_bf, tau, counts, cand)
        else:
            thr = ops.rating_thresholds(tau, Zb, self.pmax)   # tau - 2 delta_u, once per batch
            ops.score_bf16_filter_rating(users_bf, self.items_bf, Zb, self.p, thr, counts, cand)
        return cand

    def rank(self, st, cand, counts, rows, k, ex0, ex1, vals, idx):
        if self.p is None:
            ops.topk_candidates(counts, cand, rows, self.h_user, self.h_item, k, ex0, ex1, vals,
                                idx)
        else:
            ops.topk_candidates_rating(counts, cand, rows, self.h_user, self.h_item, st[1],
                                       self.p, k, ex0, ex1, vals, idx)

    def score_rows(self, r):
        if not hasattr(self, '_all_items'):     # once per call: _rows_exact runs at most once
            self._all_items = torch.arange(self.h_item.shape[0], device=self.h_item.device)
            self._grouped = ops.cos_grouped_ok(self.h_user, self.h_item)
        G, n_items = r.numel(), self.h_item.shape[0]
        dst = self._all_items.repeat(G)
        if self._grouped:
            _, sc = ops.sddmm_cos_grouped(r, None, n_items, dst, self.h_user, self.h_item)
        else:
            sc = ops.sddmm_cos(r.repeat_interleave(n_items), dst, self.h_user, self.h_item)
        return sc.view(G, n_items)


class _MlpHead(_Scorer):
    """A PredictingLayer re-associated for scoring a user batch against every item:
    Q = h_item W1b^T once, P = h_user[rows] W1a^T + b1 per batch, the rest of the head in
    ops.edge_mlp_dense_store / _filter (each score bitwise ops.edge_mlp's for the pair).
    The filter compares the final fp32 score (or rating): no band."""
    fast_ok = True

    def __init__(self, head, h_user, h_item, p=None):
        d = h_item.shape[1]
        W1 = head.hidden_1.weight
        if tuple(W1.shape) != (128, 2 * d):
            raise ValueError(f'head.hidden_1 must be [128, {2 * d}] for d = {d}, got '
                             f'{tuple(W1.shape)}')
        for t in (W1, head.hidden_2.weight, head.output.weight):
            ops._dev(t, 'head weights', torch.float32)
        self.h_user, self.h_item, self.p = h_user, h_item, p
        self.W1a, self.b1 = W1[:, :d], head.hidden_1.bias
        self.tail = (head.hidden_2.weight.detach().contiguous(),
                     head.hidden_2.bias.detach().contiguous(),
                     head.output.weight.detach().reshape(-1).contiguous(),
                     head.output.bias.detach().contiguous())
        self.Q = ops.gemm(h_item, W1[:, d:]) if h_item.shape[0] else \
            torch.empty((0, 128), dtype=torch.float32, device=h_item.device)

    def P(self, rows):
        return ops.gemm(self.h_user[rows].contiguous(), self.W1a, bias=self.b1)

    def store(self, P, n=None):
        return ops.edge_mlp_dense_store(P, self.Q if n is None else self.Q[:n], *self.tail)

    def filter(self, P, tau, counts, cand_items, cand_scores):
        ops.edge_mlp_dense_filter(P, self.Q, *self.tail, tau, counts, cand_items, cand_scores)

    # the rating forms (popularity): Z over all items, R of a sample table, the R filter
    def denominators(self, P):
        return ops.edge_mlp_dense_denominators(P, self.Q, *self.tail)

    def store_rating(self, P, Q_cols, Z, p_col):
        return ops.edge_mlp_dense_store_rating(P, Q_cols, *self.tail, Z, p_col)

    def filter_rating(self, P, Z, p, tau, counts, cand_items, cand_scores):
        ops.edge_mlp_dense_filter_rating(P, self.Q, *self.tail, Z, p, tau, counts, cand_items,
                                         cand_scores)

    # the scorer interface, on the members above
    def prepare(self, m, pop_sample):
        self._take_sample(self.Q, m, pop_sample)

    def denominators_of(self, rows):
        return self.denominators(self.P(rows))

    def batch(self, rows):
        P = self.P(rows)
        return P, None if self.p is None else self.denominators(P)

    def sample_scores(self, st):
        if self.p is None:
            return ops.edge_mlp_dense_store(st[0], self.sample, *self.tail)
        return self.store_rating(st[0], self.sample, st[1], self.p_col)

    def keep(self, st, tau, counts, cand_cap):
        P, Zb = st
        cand = torch.empty((tau.numel(), cand_cap), dtype=torch.int32, device=tau.device)
        cand_sc = torch.empty((tau.numel(), cand_cap), dtype=torch.float32, device=tau.device)
        if self.p is None:
            self.filter(P, tau, counts, cand, cand_sc)
        else:
            self.filter_rating(P, Zb, self.p, tau, counts, cand, cand_sc)
        return cand, cand_sc

    def rank(self, st, kept, counts, rows, k, ex0, ex1, vals, idx):
        ops.topk_scored_candidates(counts, *kept, k, rows, ex0, ex1, vals, idx)

    def score_rows(self, r):
        return self.store(self.P(r))


def _popularity_vector(popularity, weight_popularity, n_items):
    """p = popularity * weight as fp32 [n_items] (one fp32 multiply per item, once per call)."""
    if not isinstance(popularity, torch.Tensor):
        raise ValueError('popularity must be a fp32 device tensor')
    ops._dev(popularity, 'popularity', torch.float32)
    if popularity.dim() > 2 or (popularity.dim() == 2 and popularity.shape[1] != 1) or \
            popularity.numel() != n_items:
        raise ValueError(f'popularity must be [n_items] or [n_items, 1] with n_items = '
                         f'{n_items}, got {tuple(popularity.shape)}')
    return (popularity.reshape(-1) * float(weight_popularity)).contiguous()


def _popular_sample(p, m, pop_sample):
    """The threshold sample's item ids, ascending (int32): the prefix [0, m) and the
    pop_sample items of largest p outside it, ties by id."""
    n, dev = p.numel(), p.device
    ids = torch.arange(m, device=dev)
    extra = min(int(pop_sample), n - m)
    if extra > 0:
        order = torch.sort(p[m:], descending=True, stable=True).indices[:extra] + m
        ids = torch.cat((ids, torch.sort(order).values))
    return ids.to(torch.int32)


def _recommend(scorer, k, user_rows, exclude, batch_size, m, cand_cap, pop_sample, stats, vals,
               idx):
    """recommend()'s one driver, for either head and with or without popularity: per batch the
    sample columns scored, the row's excluded items masked, the k-th best value taken as tau,
    one filter pass over all items, the kept candidates ranked; after the last batch one
    readback, and the overflowed rows redone exhaustively."""
    dev = vals.device
    U, n_items = user_rows.numel(), scorer.h_item.shape[0]
    ex0, ex1 = (None, None) if exclude is None else exclude
    # the rows' denominators, kept for the exhaustive path (which sums them from its score
    # rows where the denominator kernel does not exist: Z None)
    Z = None
    if scorer.p is not None and scorer.fast_ok:
        Z = torch.empty(U, dtype=torch.float32, device=dev)
    if not (scorer.fast_ok and k <= cand_cap // 4 and U > 0 and n_items > 0):
        if Z is not None and n_items > 0:
            for b0 in range(0, U, batch_size):
                Z[b0:b0 + batch_size] = scorer.denominators_of(user_rows[b0:b0 + batch_size])
        _rows_exact(scorer, k, user_rows, exclude, vals, idx, torch.arange(U, device=dev), Z)
        return
    stats['fast_path'] = True
    scorer.prepare(m, pop_sample)
    if scorer.col_ids is not None:
        stats['pop_sample'] = int(scorer.col_ids.numel()) - m
    counts = torch.zeros(U, dtype=torch.int32, device=dev)
    for b0 in range(0, U, batch_size):
        rows = user_rows[b0:b0 + batch_size]
        cut = slice(b0, b0 + rows.numel())
        st = scorer.batch(rows)
        s = scorer.sample_scores(st)
        if Z is not None:
            Z[cut] = st[1]
        if exclude is not None and scorer.col_ids is None:
            ops.mask_excluded(s, rows, ex0, ex1)
        elif exclude is not None:
            ops.mask_excluded_mapped(s, scorer.col_ids, rows, ex0, ex1)
        tau = topk_rows(s, k)[0][:, k - 1].contiguous()  # -inf: fewer than k eligible there
        del s
        kept = scorer.keep(st, tau, counts[cut], cand_cap)
        scorer.rank(st, kept, counts[cut], rows, k, ex0, ex1, vals[cut], idx[cut])
    cnt = counts.cpu().numpy()                       # the call's one readback
    over = np.nonzero(cnt > cand_cap)[0]
    if over.size:
        pos = torch.from_numpy(over).to(dev)
        _rows_exact(scorer, k, user_rows[pos], exclude, vals, idx, pos,
                    None if Z is None else Z[pos])
    stats.update(candidates_mean=float(cnt.mean()), candidates_max=int(cnt.max()),
                 overflow_rows=int(over.size))


def recommend(h_user, h_item, k, user_rows=None, exclude=None, *, batch_size=8192,
              sample=65536, cand_cap=1024, return_stats=False, head=None, popularity=None,
              weight_popularity=1.0, pop_sample=4096):
    """The k best items per user by (cosine desc, item id asc), excluded items removed —
    the lists of an exhaustive fp32 ranking, bit for bit — on device tensors and without a
    score matrix.

    h_user [n_users, d], h_item [n_items, d]: fp32 device tables (raw embeddings; the cosine
    divides by max(norm, 1e-12) as CosinePrediction does).  user_rows: int64 device tensor of
    rows of h_user to serve (None: all of them, in order; repeats allowed).  exclude:
    (indptr int64 [n_users + 1], indices int32) over h_user's rows, unsorted rows allowed —
    the graph's g.in_csr('bought-by')[:2] — or None.
    -> (idx int64 [U, k], vals fp32 [U, k]) [, stats]; rows with fewer than k eligible items
    are padded with (-1, -inf).  vals are the values of ops.sddmm_cos for the pairs.

    Per batch of `batch_size` users: both tables normalised and rounded to bf16, approximate
    scores (bf16 MFMA, fp32 accumulation) of the item prefix [0, min(sample, n_items)) stored
    and their k-th best non-excluded value taken as tau; one pass over all items keeps the
    items with approximate score >= tau - 2 REC_EPS (a superset of the exact top k: |approx -
    exact| <= REC_EPS), at most `cand_cap` per user; those are rescored in fp32 and ranked.
    Rows that kept more than cand_cap items (and the whole call when k > cand_cap / 4,
    d > REC_MAX_D or d % 4 != 0) are recomputed exhaustively with sddmm_cos + topk_rows, so
    the result never depends on the filter.  The bound REC_EPS is derived for rows whose norm
    lies in fp32's normal range and away from the 1e-12 guard (or is exactly zero).  The host reads the device once per call (the
    per-row candidate counts, after the last batch).

    Non-finite embeddings are outside the contract: a NaN or inf score has no place in the
    ranking, and the filter's comparison drops it silently.

    head: None ranks by the cosine, as above.  A PredictingLayer (model.pred_fn.layer_nn,
    the reference's 128 / 32 hidden sizes, hidden_1 [128, 2 d]) ranks by the MLP head's score
    instead; vals are then the values of ops.edge_mlp for the pairs, and everything else —
    the (score desc, item id asc) order, user_rows, exclude, the padding, the stats, the one
    readback — is the same.  Q = h_item W1b^T is formed once per call; per batch
    P = h_user[rows] W1a^T + b1, the head's scores of the item prefix are stored (no id
    arrays) and their k-th best non-excluded value taken as tau; one pass over all items
    keeps the (item, score) pairs with score >= tau, at most cand_cap per user, and those are
    ranked.  There is no band: the filter compares the final fp32 score, at least k eligible
    items of the prefix score >= tau, so every member of the exhaustive top k (and every tie
    at the k-th value) is kept.  Rows that kept more than cand_cap items — a saturated head,
    whose scores are 1.0f for many items, does that — and the whole call when
    k > cand_cap / 4 are recomputed exhaustively (dense scores of the rows over all items in
    chunks of 2^26 / n_items rows, topk_rows).  Non-finite scores are outside the contract,
    as for the cosine.

    popularity: None ranks by the score, as above (that code path is untouched).  A fp32
    device tensor [n_items] or [n_items, 1] (the reference's g.ndata['popularity']['item'])
    ranks by the reference's use_popularity rating instead (src/metrics.py:69-72), for either
    head, still exactly and without a score matrix:
        R(u, v) = expf(score(u, v)) / Z_u + popularity[v] * weight_popularity,
    Z_u the sum of expf over ALL items (excluded ones too: the reference removes bought items
    after the softmax), each operation rounded once in fp32; vals are the R values.  Z_u is
    bitwise the same for a user whatever the batch size, the order of user_rows or the run: a
    fixed-order reduction (for the cosine head on the fp32 MFMA over the fp32-normalised
    tables, for the MLP head a denominator pass of the dense kernel).  The threshold sample is
    the item prefix plus the `pop_sample` items of largest popularity * weight outside it
    (ties by id) — with the reference's weights the best ratings are the popular items', and a
    tau taken from a prefix without them keeps every popular item for every row.  The cosine
    filter keeps the items with Ra >= tau - 2 delta_u, Ra the rating of the bf16 score and
    delta_u = REC_RATING_BAND / Z_u + REC_RATING_SLACK max(p) the bound on |Ra - R|; the MLP
    filter compares the final R, without a band.  Overflowed rows, k > cand_cap / 4 and (for
    the cosine head) d % 4 != 0 or d > REC_MAX_D take the exhaustive path: score rows, the
    same R of the same Z, topk_rows (for those widths Z is summed from the score rows).

    stats (return_stats=True): candidates_mean, candidates_max (kept items per row, counted
    past the cap), overflow_rows, sample, cand_cap, fast_path; with popularity also
    pop_sample (the items added to the sample)."""
    ops._dev(h_user, 'h_user', torch.float32)
    ops._dev(h_item, 'h_item', torch.float32)
    if h_user.dim() != 2 or h_item.dim() != 2 or h_user.shape[1] != h_item.shape[1]:
        raise ValueError(f'h_user / h_item must be 2-D with one feature size, got '
                         f'{tuple(h_user.shape)} and {tuple(h_item.shape)}')
    k, batch_size, sample, cand_cap = int(k), int(batch_size), int(sample), int(cand_cap)
    if k < 1 or batch_size < 1 or sample < 1 or not 1 <= cand_cap <= REC_MAX_CAP:
        raise ValueError(f'recommend: k, batch_size and sample must be >= 1 and cand_cap in '
                         f'[1, {REC_MAX_CAP}]')
    dev = h_item.device
    h_user, h_item = h_user.contiguous(), h_item.contiguous()
    n_items, p = h_item.shape[0], None
    if popularity is not None:   # refused before any launch
        if int(pop_sample) < 0:
            raise ValueError('recommend: pop_sample must be >= 0')
        p = _popularity_vector(popularity, weight_popularity, n_items)
    if user_rows is None:
        user_rows = torch.arange(h_user.shape[0], device=dev)
    ops._dev(user_rows, 'user_rows', torch.int64)
    user_rows = user_rows.reshape(-1).contiguous()
    if exclude is not None:
        ex_ptr, ex_idx = exclude
        ops._dev(ex_ptr, 'exclude indptr', torch.int64)
        ops._dev(ex_idx, 'exclude indices', torch.int32)
        if ex_ptr.numel() != h_user.shape[0] + 1:
            raise ValueError(f'exclude indptr must have n_users + 1 = {h_user.shape[0] + 1} '
                             f'entries, got {ex_ptr.numel()}')
        exclude = (ex_ptr.contiguous(), ex_idx.contiguous())
    U = user_rows.numel()
    vals = torch.empty((U, k), dtype=torch.float32, device=dev)
    idx = torch.empty((U, k), dtype=torch.int64, device=dev)
    m = min(sample, n_items)
    stats = {'candidates_mean': 0.0, 'candidates_max': 0, 'overflow_rows': 0, 'sample': m,
             'cand_cap': cand_cap, 'fast_path': False}
    if p is not None:
        stats['pop_sample'] = 0
    scorer = _CosHead(h_user, h_item, p) if head is None else _MlpHead(head, h_user, h_item, p)
    _recommend(scorer, k, user_rows, exclude, batch_size, m, cand_cap, pop_sample, stats, vals,
               idx)
    return (idx, vals, stats) if return_stats else (idx, vals)


def recommend_for_graph(g, h, k, user_ids=None, etype='bought-by', use_popularity=False,
                        weight_popularity=1, **kw):
    """recommend() for the users of a graph, the items each has an `etype` edge from
    removed: the exclusion lists are the graph's own dst-major CSR of
    ('item', etype, 'user') (indptr over users, int32 item ids), already on the device.
    h: {'user': ..., 'item': ...} embeddings; user_ids: ids to serve (None: every user).
    use_popularity: rank by softmax + weight_popularity * g.ndata['popularity']['item'], the
    reference's get_recs(use_popularity=True) (recommend's popularity=)."""
    dev = h['item'].device
    if use_popularity:
        try:
            pop = g.ndata['popularity']['item']
        except (KeyError, AttributeError, TypeError) as exc:
            raise KeyError("recommend_for_graph(use_popularity=True): the graph has no "
                           "ndata['popularity']['item']") from exc
        kw = dict(kw, popularity=torch.as_tensor(pop).to(dev).float(),
                  weight_popularity=weight_popularity)
    ex_ptr, ex_idx = g.in_csr(etype)[:2]
    exclude = (ex_ptr.to(dev), ex_idx.to(dev))
    if user_ids is not None:
        user_ids = torch.as_tensor(user_ids, dtype=torch.int64, device=dev)
    return recommend(h['user'], h['item'], k, user_ids, exclude, **kw)


# ---- exact rank of held-out items among all items (csrc/rank.hip) -----------
def rank_eps(d):
    """|a - score| <= rank_eps(d) for the fp32 MFMA dot a of the two fp32-normalised rows
    (ops.normalize_rows_f32) and score = ops.sddmm_cos: (4 dpad + 32) 2^-24 with dpad = d rounded
    up to a multiple of 8 — 3.2e-5 at d = 128, 4.9e-4 at d = 2048.  Derived in csrc/rank.hip
    and DESIGN.md §23 for rows whose norm lies in fp32's normal range and away from the 1e-12
    guard (or is exactly zero), as REC_EPS is.  The library holds the value it compares with
    (ops.rank_eps); this one is for callers."""
    return (4.0 * ((int(d) + 7) // 8 * 8) + 32.0) * 2.0 ** -24


def _distinct_exclusions(exclude, served, n_served, total, n_items):
    """The exclusion rows of the served users only (served: bool [n_users], n_served of them,
    their rows `total` entries long — both read with the id check), each row's ids ascending
    and an id's repeats replaced by -1 (a multigraph's rows hold duplicates; an excluded item is
    subtracted once) -> (indptr over ALL users, the other rows empty; indices int32).  One sort
    of the served rows' entries, once per call; no host read."""
    ex_ptr, ex_idx = exclude
    dev, n_users = ex_idx.device, served.numel()
    su = torch.sort(served.to(torch.int8), descending=True, stable=True).indices[:n_served]
    deg = (ex_ptr[1:] - ex_ptr[:-1])[su]                       # su ascends: rows stay in order
    ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(torch.zeros(n_users, dtype=torch.int64, device=dev)
                           .index_put_((su,), deg), 0)
    if total == 0:      # every served row is empty: one unread entry, so the list has an address
        return ptr, torch.full((1,), -1, dtype=torch.int32, device=dev)
    row = torch.repeat_interleave(torch.arange(n_served, device=dev), deg, output_size=total)
    src = ex_ptr[su][row] + (torch.arange(total, device=dev) - ptr[su][row])
    ids = ex_idx[src].to(torch.int64)
    ids = torch.where((ids < 0) | (ids > n_items), torch.full_like(ids, n_items), ids)
    key = torch.sort(row * (int(n_items) + 1) + ids).values
    ids = (key % (int(n_items) + 1)).to(torch.int32)
    ids[1:][key[1:] == key[:-1]] = -1
    ids[ids >= n_items] = -1                                    # ids past the table: no item
    return ptr, ids.contiguous()


def _ranks_exact(scorer, users, items, vals, exclude, rank, out_pos, Z=None):
    """The definition on exhaustive score rows, for the pairs (users, items) with threshold
    vals, in chunks of 2^26 / n_items rows: ranks into rank[out_pos].  Where the scorer has a
    popularity (scorer.p) the rows become ratings first, as in _rows_exact (Z [len(users)];
    None: summed from the rows), and vals are the pairs' ratings."""
    n_items = scorer.h_item.shape[0]
    if users.numel() == 0:
        return
    ids = torch.arange(n_items, device=users.device)
    step = max(1, (1 << 26) // n_items)
    for c0 in range(0, users.numel(), step):
        u = users[c0:c0 + step].contiguous()
        g = items[c0:c0 + step].unsqueeze(1)
        t = vals[c0:c0 + step].unsqueeze(1)
        sc = scorer.score_rows(u)
        if scorer.p is not None:
            _to_ratings(sc, c0, (Z, scorer.p))
        ahead = (sc > t) | ((sc == t) & (ids < g))       # v = g itself: equal score, not below
        r = None
        if exclude is not None:
            mark = torch.zeros_like(sc)
            ops.mask_excluded(mark, u, exclude[0], exclude[1])
            bought = mark == float('-inf')
            ahead &= ~bought
            r = bought.gather(1, g).squeeze(1)
        out = 1 + ahead.sum(1)
        if r is not None:
            out = torch.where(r, torch.zeros_like(out), out)
        rank[out_pos[c0:c0 + step]] = out


def _rank_rows_mlp(scorer, P, Z, row_user, lptr, row, items, exclude, rank, vals):
    """One batch of the MLP head's full-ranking evaluation (scorer: a _MlpHead whose Q is
    formed).  P [R, 128]: the rows' P rows; Z [R]: their denominators, or None without a
    popularity; row_user [R]: the rows' users; lptr [R + 1]: row r's entries are the slots
    [lptr[r], lptr[r + 1]); row / items [E]: each entry's row and its held-out item; exclude: the
    distinct exclusion CSR or (None, None); rank / vals [E]: the output slices.  The entries'
    own edge_mlp scores, one count pass over all items, one resolve launch.  No host read:
    there is nothing to overflow."""
    s = ops.edge_mlp(row, items, P, scorer.Q, *scorer.tail)
    gid = items.to(torch.int32)
    if Z is None:
        ahead = ops.edge_mlp_dense_count_lists(P, scorer.Q, *scorer.tail, lptr, s, gid)
    else:
        ahead = ops.edge_mlp_dense_count_lists_rating(P, scorer.Q, *scorer.tail, Z, scorer.p,
                                                      lptr, s, gid)
    ops.rank_resolve_mlp_lists(row_user, lptr, s, gid, ahead, scorer.h_user.shape[0], P,
                               scorer.Q, *scorer.tail, *exclude, Z, scorer.p, rank, vals)


def rank_items(h_user, h_item, users, items, exclude=None, *, batch_size=8192, cand_cap=1024,
               return_stats=False, head=None, popularity=None, weight_popularity=1.0):
    """The exact position of item items[p] in recommend()'s exhaustive ranking for user
    users[p], for every pair p, without a score matrix.

        rank(u, g) = 1 + #{v not in exclude(u), v != g : s(u,v) > s(u,g) or
                                                          (s(u,v) == s(u,g) and v < g)}
        rank(u, g) = 0 where g is in exclude(u)   (the reference drops bought items)

    with s = ops.sddmm_cos's value, the score recommend ranks by.  h_user [n_users, d], h_item
    [n_items, d]: fp32 device tables.  users / items: int64 device tensors [P], repeats allowed;
    an id out of range raises before any kernel of the pass is launched (one read: the four
    id extremes and the size of the served users' exclusion rows).  exclude: recommend's
    (indptr int64 [n_users + 1], indices int32); rows may be unsorted and hold an id more than once (a multigraph's bought-by CSR) — an excluded item
    counts once: the served users' rows are sorted and their repeats struck once per call.
    -> (rank int64 [P], vals fp32 [P]) [, stats]; vals are sddmm_cos's values for the pairs.

    Per batch of `batch_size` pairs: the pairs' user rows and (once per call) the item table
    normalised in fp32, then one fp32 MFMA pass over all items (ops.rank_count) whose epilogue
    compares each dot a with the row's threshold t = vals[p]: a > t + eps is provably ahead and
    counted, a < t - eps provably behind, anything between joins the row's band list (at most
    cand_cap ids); ops.rank_resolve rescores the band and the user's excluded items with the
    exact cosine and forms 1 + ahead + band_ahead - excluded_ahead.  eps = rank_eps(d) bounds
    |a - s|.  Rows whose band holds more than cand_cap items (many items tied with the held-out
    one) and the whole call when d % 4 != 0 or d > REC_MAX_D are redone from exhaustive score
    rows in chunks of 2^26 / n_items rows, so the result never depends on the pass.  Apart
    from the id check the host reads the device once (the band counts, after the last batch).
    Non-finite embeddings are outside the contract, as for recommend.

    stats (return_stats=True): band_mean, band_max (band items per row, counted past the cap),
    overflow_rows, fast_path, eps, cand_cap.

    head: None ranks by the cosine, as above (that code path is untouched).  A PredictingLayer
    (model.pred_fn.layer_nn, validated as for recommend) ranks by the MLP head's score instead:
    s = ops.edge_mlp's value, vals those values bit for bit, the definition, the exclusions
    and the repeats as above.  Q = h_item W1b^T is formed once per call; per
    batch of pairs P = h_user[users] W1a^T + b1, the pairs' own scores (ops.edge_mlp), one pass
    of the dense MLP kernel over all items whose epilogue counts the items exactly ahead
    (ops.edge_mlp_dense_count_lists, each pair a row with one entry: rank_lists' kernels, which
    share a row among a user's entries), and ops.rank_resolve_mlp_lists, which rescores the
    user's excluded items with the same bits and subtracts those exactly ahead.  The pass
    compares the final fp32 score — the very value the ranking is defined on — so there is no
    error bound, no band, no overflow and no exhaustive redo: cand_cap is accepted and unused,
    the stats are fast_path True, band_mean 0.0, band_max 0, overflow_rows 0, eps 0.0, and the
    id check is the call's only host read.

    popularity (with head=): a fp32 device tensor [n_items] or [n_items, 1], as for recommend.
    The ranking is by R(u, v) = expf(s(u, v)) / Z_u + popularity[v] * weight_popularity, Z_u
    recommend's denominator (the MLP head's denominator pass: the same bits for a user in any
    batch), so a user's R values are the bits recommend(head=, popularity=) returns; vals are
    the pairs' R.  The count pass and the resolve form every R, the pair's own included, with
    the one function of csrc/rating.hpp.
    popularity without head= raises NotImplementedError before anything is launched: the
    cosine count pass classifies by |a - s| <= eps, and in rating space that needs a proved
    band for expf(a) / Z_u + p_v against the rating of the exact cosine — the analogue of
    REC_RATING_BAND for the fp32 MFMA dot — which has not been derived.  It is not
    approximated."""
    if popularity is not None and head is None:
        raise NotImplementedError(
            'rank_items: popularity= needs head= (the cosine head has no proved band in rating '
            'space for its count pass; DESIGN.md §24)')
    ops._dev(h_user, 'h_user', torch.float32)
    ops._dev(h_item, 'h_item', torch.float32)
    if h_user.dim() != 2 or h_item.dim() != 2 or h_user.shape[1] != h_item.shape[1]:
        raise ValueError(f'h_user / h_item must be 2-D with one feature size, got '
                         f'{tuple(h_user.shape)} and {tuple(h_item.shape)}')
    batch_size, cand_cap = int(batch_size), int(cand_cap)
    if batch_size < 1 or not 1 <= cand_cap <= REC_MAX_CAP:
        raise ValueError(f'rank_items: batch_size must be >= 1 and cand_cap in '
                         f'[1, {REC_MAX_CAP}]')
    ops._dev(users, 'users', torch.int64)
    ops._dev(items, 'items', torch.int64)
    users, items = users.reshape(-1).contiguous(), items.reshape(-1).contiguous()
    if users.numel() != items.numel():
        raise ValueError(f'rank_items: {users.numel()} users for {items.numel()} items')
    (n_users, d), n_items = h_user.shape, h_item.shape[0]
    if exclude is not None:
        ex_ptr, ex_idx = exclude
        ops._dev(ex_ptr, 'exclude indptr', torch.int64)
        ops._dev(ex_idx, 'exclude indices', torch.int32)
        if ex_ptr.numel() != n_users + 1:
            raise ValueError(f'exclude indptr must have n_users + 1 = {n_users + 1} entries, '
                             f'got {ex_ptr.numel()}')
        exclude = (ex_ptr.contiguous(), ex_idx.contiguous())
    dev = h_item.device
    h_user, h_item = h_user.contiguous(), h_item.contiguous()
    P = users.numel()
    fast = d % 4 == 0 and 4 <= d <= REC_MAX_D
    stats = {'band_mean': 0.0, 'band_max': 0, 'overflow_rows': 0, 'fast_path': False,
             'eps': rank_eps(d) if head is None else 0.0, 'cand_cap': cand_cap}
    rank = torch.empty(P, dtype=torch.int64, device=dev)
    if P == 0:
        vals = torch.empty(0, dtype=torch.float32, device=dev)
        return (rank, vals, stats) if return_stats else (rank, vals)
    if n_users == 0 or n_items == 0:
        raise ValueError(f'rank_items: ids out of range ({P} pairs for {n_users} users and '
                         f'{n_items} items)')
    check = [users.min(), users.max(), items.min(), items.max()]
    if exclude is not None:     # what the exclusion sort needs to size itself: the same read
        served = torch.zeros(n_users, dtype=torch.bool, device=dev)
        served[users.clamp(0, n_users - 1)] = True
        deg = exclude[0][1:] - exclude[0][:-1]
        check += [served.sum(), (deg * served).sum()]
    lo_u, hi_u, lo_i, hi_i, *sizes = torch.stack(check).tolist()
    if lo_u < 0 or hi_u >= n_users or lo_i < 0 or hi_i >= n_items:
        raise ValueError(f'rank_items: ids out of range (users in [{lo_u}, {hi_u}] of '
                         f'{n_users}, items in [{lo_i}, {hi_i}] of {n_items})')
    if head is not None:    # the MLP head: exact in one pass, nothing to read back
        p = None if popularity is None else \
            _popularity_vector(popularity, weight_popularity, n_items)
        scorer = _MlpHead(head, h_user, h_item, p)           # Q formed once per call
        ex = (None, None) if exclude is None else \
            _distinct_exclusions(exclude, served, *sizes, n_items)
        vals = torch.empty(P, dtype=torch.float32, device=dev)
        rows = torch.arange(min(batch_size, P) + 1, device=dev)     # a pair is a one-slot row
        for b0 in range(0, P, batch_size):
            ub = users[b0:b0 + batch_size]
            n = ub.numel()
            cut = slice(b0, b0 + n)
            Pb = scorer.P(ub)
            # recommend's Z_u: the same bits in any batch
            Z = None if p is None else scorer.denominators(Pb)
            _rank_rows_mlp(scorer, Pb, Z, ub, rows[:n + 1], rows[:n], items[cut], ex, rank[cut],
                           vals[cut])
        stats['fast_path'] = True
        return (rank, vals, stats) if return_stats else (rank, vals)
    vals = ops.sddmm_cos(users, items, h_user, h_item)
    scorer = _CosHead(h_user, h_item)
    if not fast:
        _ranks_exact(scorer, users, items, vals, exclude, rank, torch.arange(P, device=dev))
        return (rank, vals, stats) if return_stats else (rank, vals)
    stats['fast_path'] = True
    items_f32 = ops.normalize_rows_f32(h_item)               # converted once per call
    ex0, ex1 = (None, None) if exclude is None else \
        _distinct_exclusions(exclude, served, *sizes, n_items)
    band_counts = torch.zeros(P, dtype=torch.int32, device=dev)
    band = torch.empty((min(batch_size, P), cand_cap), dtype=torch.int32, device=dev)
    for b0 in range(0, P, batch_size):
        ub = users[b0:b0 + batch_size]
        cut = slice(b0, b0 + ub.numel())
        bnd, t = band[:ub.numel()], vals[cut]
        ahead = ops.rank_count(ops.normalize_rows_f32(h_user, ub), items_f32, t,
                               band_counts[cut], bnd)
        ops.rank_resolve(ub, items[cut], t, ahead, band_counts[cut], bnd, h_user, h_item, ex0,
                         ex1, rank[cut])
    cnt = band_counts.cpu().numpy()                          # the call's one readback
    over = np.nonzero(cnt > cand_cap)[0]
    if over.size:
        pos = torch.from_numpy(over).to(dev)
        _ranks_exact(scorer, users[pos], items[pos], vals[pos], exclude, rank, pos)
    stats.update(band_mean=float(cnt.mean()), band_max=int(cnt.max()),
                 overflow_rows=int(over.size))
    return (rank, vals, stats) if return_stats else (rank, vals)


def rank_for_graph(g, h, ground_truth, etype='bought-by', use_popularity=False,
                   weight_popularity=1, **kw):
    """rank_items() for the held-out pairs ground_truth = (users, items) (as get_metrics_at_k
    takes them) of a graph, the items each user has an `etype` edge from excluded: the lists
    are the graph's own dst-major CSR of ('item', etype, 'user'), as in recommend_for_graph.
    h: {'user': ..., 'item': ...} embeddings.  head= (in kw) ranks by the MLP head;
    use_popularity ranks by softmax + weight_popularity * g.ndata['popularity']['item']
    (rank_items' popularity=: the MLP head only)."""
    dev = h['item'].device
    if use_popularity:
        if kw.get('head') is None:      # rank_items' refusal, before the graph is touched
            raise NotImplementedError(
                'rank_for_graph: use_popularity=True needs head= (rank_items: popularity= needs '
                'head=; DESIGN.md §24)')
        try:
            pop = g.ndata['popularity']['item']
        except (KeyError, AttributeError, TypeError) as exc:
            raise KeyError("rank_for_graph(use_popularity=True): the graph has no "
                           "ndata['popularity']['item']") from exc
        kw = dict(kw, popularity=torch.as_tensor(pop).to(dev).float(),
                  weight_popularity=weight_popularity)
    users, items = ground_truth
    users = torch.as_tensor(users, dtype=torch.int64, device=dev)
    items = torch.as_tensor(items, dtype=torch.int64, device=dev)
    ex_ptr, ex_idx = g.in_csr(etype)[:2]
    return rank_items(h['user'], h['item'], users, items, (ex_ptr.to(dev), ex_idx.to(dev)), **kw)


# ---- the list-shaped entry: one scored row per user (csrc/heads.hip) --------
def _ptr(lens):
    """[0, lens[0], lens[0] + lens[1], ...]: int64 [len + 1]."""
    ptr = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=lens.device)
    ptr[1:] = torch.cumsum(lens, 0)
    return ptr


def _expand_lists(user_rows, gt_indptr, gt_indices, lens, n_pairs=None):
    """The served lists as pairs (lens: their lengths; n_pairs: their sum where the caller has
    read it, else read here) -> (users, items, owner: the entry's position in user_rows)."""
    dev = user_rows.device
    eptr = _ptr(lens)
    if n_pairs is None:
        n_pairs = int(eptr[-1])
    owner = torch.repeat_interleave(torch.arange(user_rows.numel(), device=dev), lens,
                                    output_size=n_pairs)
    pos = gt_indptr[user_rows][owner] + (torch.arange(n_pairs, device=dev) - eptr[owner])
    return user_rows[owner], gt_indices[pos].to(torch.int64), owner


def list_pairs(user_rows, gt_indptr, gt_indices):
    """The held-out lists of the users `user_rows` (int64, any order; None: every user) of the
    ground-truth CSR (gt_indptr int64 [n_users + 1], gt_indices) as pairs, the lists
    concatenated in user_rows order and each in CSR order -> (users int64 [E], items int64
    [E]): the order of rank_lists' results, and what ranks_to_metrics takes beside its ranks.
    Plain torch on the tensors' own device; one host read (the extremes of user_rows and E)."""
    gt_indptr, gt_indices = gt_indptr.reshape(-1), gt_indices.reshape(-1)
    n_users = gt_indptr.numel() - 1
    if user_rows is None:
        user_rows = torch.arange(n_users, device=gt_indptr.device)
    user_rows = user_rows.reshape(-1)
    if user_rows.numel() == 0:
        none = torch.empty(0, dtype=torch.int64, device=gt_indptr.device)
        return none, none.clone()
    uc = user_rows.clamp(0, max(n_users - 1, 0))
    lens = (gt_indptr[uc + 1] - gt_indptr[uc]).clamp(min=0)
    lo, hi, E = torch.stack([user_rows.min(), user_rows.max(), lens.sum()]).tolist()
    if lo < 0 or hi >= n_users:
        raise ValueError(f'list_pairs: user ids out of range of {n_users} users')
    return _expand_lists(user_rows, gt_indptr, gt_indices, lens, E)[:2]


def _list_row_plan(lens, budget, n_rows=None):
    """The rows of the list count pass for lists of `lens` entries (int64 [U]) whose slots lie
    back to back in list order: a list takes ceil(len / budget) rows of at most `budget`
    consecutive slots, an empty list none -> (owner int64 [R]: the row's list, lptr int64
    [R + 1]: row r's slots are [lptr[r], lptr[r + 1])).  n_rows: R where the caller has read it
    (sum of ceil(lens / budget)), else read here.  Torch ops only, on any device."""
    dev = lens.device
    rows_per = (lens + (budget - 1)) // budget
    rptr, eptr = _ptr(rows_per), _ptr(lens)
    if n_rows is None:
        n_rows = int(rptr[-1])
    owner = torch.repeat_interleave(torch.arange(lens.numel(), device=dev), rows_per,
                                    output_size=n_rows)
    lptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    lptr[:n_rows] = eptr[owner] + (torch.arange(n_rows, device=dev) - rptr[owner]) * budget
    lptr[n_rows] = eptr[-1]      # a row ends where the next begins: the lists lie back to back
    return owner, lptr


def _lists_check(user_rows, gt_indptr, gt_indices, n_users, n_items, extra=()):
    """rank_lists' id check, one host read: the id extremes of user_rows and of the served
    lists, the distinct users among user_rows and the served entries, then whatever `extra`
    (a function of (lens, served) returning device scalars / vectors) adds to the same read
    -> (lens, served, n_pairs, extra's values as ints).  Raises ValueError on an id out of
    range or a repeated user.  Torch ops only, on any device."""
    dev = gt_indptr.device
    U, nnz = user_rows.numel(), gt_indices.numel()
    uc = user_rows.clamp(0, max(n_users - 1, 0))
    served = torch.zeros(n_users, dtype=torch.bool, device=dev)
    served[uc] = True
    lens = (gt_indptr[uc + 1] - gt_indptr[uc]).clamp(min=0)
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    if nnz:     # the entries of the served lists, wherever they lie in the CSR
        row = torch.searchsorted(gt_indptr[1:].contiguous(), torch.arange(nnz, device=dev),
                                 right=True).clamp(max=n_users - 1)
        ids = gt_indices.to(torch.int64) * served[row]      # 0, a valid id, elsewhere
        lo_i, hi_i = ids.min(), ids.max()
    else:
        lo_i = hi_i = zero
    head = [user_rows.min(), user_rows.max(), served.sum(), lens.sum(), lo_i, hi_i,
            gt_indptr[0], gt_indptr[-1], (gt_indptr[1:] < gt_indptr[:-1]).sum()]
    more = [t.reshape(-1).to(torch.int64) for t in (extra(lens, served) if extra else ())]
    got = torch.cat([torch.stack(head).to(torch.int64)] + more).tolist()   # the one read
    lo_u, hi_u, n_distinct, n_pairs, lo_i, hi_i, p0, p1, n_desc = got[:len(head)]
    if p0 != 0 or p1 != nnz or n_desc:
        raise ValueError(f'rank_lists: gt_indptr is not the indptr of {nnz} entries')
    if lo_u < 0 or hi_u >= n_users or (n_pairs and (lo_i < 0 or hi_i >= n_items)):
        raise ValueError(f'rank_lists: ids out of range (users in [{lo_u}, {hi_u}] of {n_users}, '
                         f'items of the served lists in [{lo_i}, {hi_i}] of {n_items})')
    if n_distinct != U:
        raise ValueError(f'rank_lists: user_rows holds a repeated user ({U} rows, {n_distinct} '
                         f'distinct)')
    return lens, served, n_pairs, got[len(head):]


def _rank_lists(h_user, h_item, user_rows, gt_indptr, gt_indices, exclude, head, popularity,
                weight_popularity, batch_size, cand_cap):
    """rank_lists -> (rank, vals, stats, users, items)."""
    if popularity is not None and head is None:
        raise NotImplementedError(
            'rank_lists: popularity= needs head= (rank_items: the cosine head has no proved band '
            'in rating space for its count pass; DESIGN.md §24)')
    if h_user.dim() != 2 or h_item.dim() != 2 or h_user.shape[1] != h_item.shape[1]:
        raise ValueError(f'h_user / h_item must be 2-D with one feature size, got '
                         f'{tuple(h_user.shape)} and {tuple(h_item.shape)}')
    (n_users, d), n_items = h_user.shape, h_item.shape[0]
    if gt_indptr.dtype != torch.int64 or gt_indptr.numel() != n_users + 1:
        raise ValueError(f'rank_lists: gt_indptr must be int64 [n_users + 1 = {n_users + 1}], got '
                         f'{gt_indptr.dtype} {tuple(gt_indptr.shape)}')
    if gt_indices.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'rank_lists: gt_indices must be int32 or int64, got {gt_indices.dtype}')
    batch_size, cand_cap = int(batch_size), int(cand_cap)
    if batch_size < 1 or not 1 <= cand_cap <= REC_MAX_CAP:
        raise ValueError(f'rank_lists: batch_size must be >= 1 and cand_cap in '
                         f'[1, {REC_MAX_CAP}]')
    ops._dev(h_user, 'h_user', torch.float32)
    ops._dev(h_item, 'h_item', torch.float32)
    ops._dev(gt_indptr, 'gt_indptr', torch.int64)
    ops._dev(gt_indices, 'gt_indices')
    dev = h_item.device
    if user_rows is None:
        user_rows = torch.arange(n_users, device=dev)
    ops._dev(user_rows, 'user_rows', torch.int64)
    user_rows = user_rows.reshape(-1).contiguous()
    gt_indptr, gt_indices = gt_indptr.reshape(-1).contiguous(), gt_indices.reshape(-1).contiguous()
    if exclude is not None:
        ex_ptr, ex_idx = exclude
        ops._dev(ex_ptr, 'exclude indptr', torch.int64)
        ops._dev(ex_idx, 'exclude indices', torch.int32)
        if ex_ptr.numel() != n_users + 1:
            raise ValueError(f'exclude indptr must have n_users + 1 = {n_users + 1} entries, '
                             f'got {ex_ptr.numel()}')
        exclude = (ex_ptr.contiguous(), ex_idx.contiguous())
    p = None if popularity is None else _popularity_vector(popularity, weight_popularity, n_items)
    U = user_rows.numel()
    mlp = head is not None
    stats = {'band_mean': 0.0, 'band_max': 0, 'overflow_rows': 0, 'fast_path': mlp,
             'eps': 0.0 if mlp else rank_eps(d), 'cand_cap': cand_cap}
    none = torch.empty(0, dtype=torch.int64, device=dev)
    empty = (none, torch.empty(0, dtype=torch.float32, device=dev), stats, none, none)
    if mlp:
        stats.update(rows=0, pairs=0)
    if U == 0:
        return empty
    if n_users == 0:
        raise ValueError(f'rank_lists: ids out of range ({U} user rows for no users)')
    budget = ops.rank_list_slots() if mlp else 1
    starts = torch.arange(0, U + batch_size, batch_size, device=dev).clamp(max=U)

    def sizes(lens, served):
        out = []
        if mlp:     # the batches' first slots and rows, the last one's end
            out += [_ptr(lens)[starts], _ptr((lens + (budget - 1)) // budget)[starts]]
            if exclude is not None:     # what the exclusion sort needs to size itself
                deg = exclude[0][1:] - exclude[0][:-1]
                out += [served.sum(), (deg * served).sum()]
        return out

    lens, served, E, more = _lists_check(user_rows, gt_indptr, gt_indices, n_users, n_items, sizes)
    if E == 0:
        return empty
    pairs = _expand_lists(user_rows, gt_indptr, gt_indices, lens, E)
    if not mlp:     # the cosine head: rank_items on the expanded pairs, as it is
        rank, vals, stats = rank_items(h_user, h_item, pairs[0], pairs[1], exclude,
                                       batch_size=batch_size, cand_cap=cand_cap,
                                       return_stats=True)
        return rank, vals, stats, pairs[0], pairs[1]
    nb = starts.numel()
    cuts = list(zip(more[:nb], more[nb:2 * nb]))
    h_user, h_item = h_user.contiguous(), h_item.contiguous()
    scorer = _MlpHead(head, h_user, h_item, p)               # Q formed once per call
    ex = (None, None) if exclude is None else \
        _distinct_exclusions(exclude, served, *more[2 * nb:], n_items)
    plan = _list_row_plan(lens, budget, cuts[-1][1])
    rank = torch.empty(E, dtype=torch.int64, device=dev)
    vals = torch.empty(E, dtype=torch.float32, device=dev)
    items, (row_owner, lptr) = pairs[1], plan
    for i, u0 in enumerate(range(0, U, batch_size)):    # per batch of users: one P row each
        (e0, r0), (e1, r1) = cuts[i], cuts[i + 1]
        if e1 == e0:
            continue
        ub = user_rows[u0:u0 + batch_size]
        Pu = scorer.P(ub)
        ro = row_owner[r0:r1] - u0                      # a long list's rows repeat the P row
        lp = (lptr[r0:r1 + 1] - e0).contiguous()
        row = torch.repeat_interleave(torch.arange(r1 - r0, device=dev), lp[1:] - lp[:-1],
                                      output_size=e1 - e0)
        Z = None if p is None else scorer.denominators(Pu)[ro].contiguous()   # recommend's Z_u
        _rank_rows_mlp(scorer, Pu[ro], Z, ub[ro].contiguous(), lp, row, items[e0:e1], ex,
                       rank[e0:e1], vals[e0:e1])
    stats.update(rows=cuts[-1][1], pairs=E)
    return rank, vals, stats, pairs[0], pairs[1]


def rank_lists(h_user, h_item, user_rows, gt_indptr, gt_indices, exclude=None, *, head=None,
               popularity=None, weight_popularity=1.0, batch_size=8192, cand_cap=1024,
               return_stats=False):
    """rank_items for held-out LISTS: the exact position of every item of the served users'
    ground-truth lists — the set the reference's create_ground_truth builds, one item list per
    user — with each distinct user scored once per batch for the MLP head.

    (gt_indptr int64 [n_users + 1], gt_indices int32 or int64): the ground-truth CSR over all
    users, the pair recs_to_metrics_device takes; lists may be empty and unsorted, and an item
    listed twice gets its rank twice.  user_rows: int64 device tensor of DISTINCT users in any
    order (None: every user).  exclude, head, popularity, weight_popularity, cand_cap: as for
    rank_items.  -> (rank int64 [E], vals fp32 [E]) [, stats]; entry e is entry e of
    list_pairs(user_rows, gt_indptr, gt_indices), and

        rank_lists(...) == rank_items(h_user, h_item, *list_pairs(...), exclude, ...)

    ranks equal, vals bit for bit, for every head and popularity setting rank_items accepts:
    its definition, tie rule, exclusion semantics and vals carry over.  A repeated user or an
    id out of range (in user_rows or a served list) raises ValueError before any kernel of the
    pass is launched.

    head=None (cosine): the lists are expanded and rank_items' cosine machinery runs on the
    pairs as it is — no new kernel and NO speed-up: the stats are rank_items', and a user with
    G items is still scored G times.  Its count pass keeps its counters in registers, which
    makes a grouped epilogue a different job; it is not done here.  popularity= without head=
    raises rank_items' NotImplementedError.

    head= a PredictingLayer: Q = h_item W1b^T once per call; per batch of at most `batch_size`
    USERS P = h_user[rows] W1a^T + b1 (one row per user), with a popularity Z_u of those rows
    (recommend's denominators: the same bits in any batch), the entries' own scores
    (ops.edge_mlp), one pass of the dense kernel over all items whose epilogue, after a user's
    32 scores of a tile are formed, loops over that user's entries and counts each against
    them (ops.edge_mlp_dense_count_lists), and one resolve launch that walks the user's
    exclusion row once for all of its entries (ops.rank_resolve_mlp_lists).  A row of the pass
    holds at most ops.rank_list_slots() entries; a longer list takes several rows that repeat
    the user's P row (the plan is built on the device; there is no cap on a list's length).
    The results do not depend on batch_size.  One host read per call (rank_lists(head=) itself:
    list_pairs and rank_lists_for_graph make reads of their own): the id check, which carries
    the id extremes of user_rows and of the served lists, the number of entries, the batches'
    slot and row offsets and the served exclusion sizes.
    Memory: a batch is batch_size USERS, and the count pass's workspace is int32
    [ceil(n_items / 1024), entries of the batch] — 256 MB at 1M items and 8,192 users with 8
    items each, as for rank_items' 65,536 pairs, but 3.2 GB with 100 items each: lower batch_size
    for long lists (the results do not change).  A served user with an empty list still gets its
    P row, and with a popularity its Z, in the batch; it takes no row of the pass.  stats: rank_items(head=)'s
    (fast_path True, band_mean 0.0, band_max 0, overflow_rows 0, eps 0.0, cand_cap accepted
    and unused) plus rows, the dense-kernel rows scored, and pairs = E."""
    rank, vals, stats, _, _ = _rank_lists(h_user, h_item, user_rows, gt_indptr, gt_indices,
                                          exclude, head, popularity, weight_popularity,
                                          batch_size, cand_cap)
    return (rank, vals, stats) if return_stats else (rank, vals)


def rank_lists_for_graph(g, h, ground_truth, etype='bought-by', use_popularity=False,
                         weight_popularity=1, **kw):
    """rank_lists() for the held-out pairs ground_truth = (users, items) of a graph, grouped
    by user on the device (ops.membership_csr: each user's list ascending by item, repeats
    kept), the distinct users among them served in ascending order and the items each has an
    `etype` edge from excluded through g.in_csr(etype), as in rank_for_graph.
    -> (rank, vals, users, items) [, stats with return_stats=True]: users / items are the
    pairs in result order (a permutation of ground_truth), what ranks_to_metrics takes.
    head= (in kw) ranks by the MLP head, one scored row per user; use_popularity as for
    rank_for_graph (the MLP head only).  Host reads: the pairs' id extremes before the CSR build
    and the number of distinct users (torch.nonzero), then rank_lists' one."""
    dev = h['item'].device
    if use_popularity:
        if kw.get('head') is None:      # rank_items' refusal, before the graph is touched
            raise NotImplementedError(
                'rank_lists_for_graph: use_popularity=True needs head= (rank_items: popularity= '
                'needs head=; DESIGN.md §24)')
        try:
            pop = g.ndata['popularity']['item']
        except (KeyError, AttributeError, TypeError) as exc:
            raise KeyError("rank_lists_for_graph(use_popularity=True): the graph has no "
                           "ndata['popularity']['item']") from exc
        kw = dict(kw, popularity=torch.as_tensor(pop).to(dev).float(),
                  weight_popularity=weight_popularity)
    return_stats = kw.pop('return_stats', False)
    users, items = ground_truth
    users = torch.as_tensor(users, dtype=torch.int64, device=dev).reshape(-1)
    items = torch.as_tensor(items, dtype=torch.int64, device=dev).reshape(-1)
    n_users, n_items = h['user'].shape[0], h['item'].shape[0]
    if users.numel() != items.numel():
        raise ValueError(f'rank_lists_for_graph: {users.numel()} users for {items.numel()} items')
    if users.numel():       # the CSR build sorts by these ids: checked before it runs
        lo_u, hi_u, lo_i, hi_i = torch.stack([users.min(), users.max(), items.min(),
                                              items.max()]).tolist()
        if lo_u < 0 or hi_u >= n_users or lo_i < 0 or hi_i >= n_items:
            raise ValueError(f'rank_lists_for_graph: ids out of range (users in [{lo_u}, {hi_u}] '
                             f'of {n_users}, items in [{lo_i}, {hi_i}] of {n_items})')
    gt_ptr, gt_idx = ops.membership_csr(items, users, n_items, n_users)
    user_rows = torch.nonzero(gt_ptr[1:] > gt_ptr[:-1]).reshape(-1)
    ex_ptr, ex_idx = g.in_csr(etype)[:2]
    kw.setdefault('head', None)
    kw.setdefault('popularity', None)
    kw.setdefault('weight_popularity', 1.0)
    kw.setdefault('batch_size', 8192)
    kw.setdefault('cand_cap', 1024)
    rank, vals, stats, us, gs = _rank_lists(h['user'], h['item'], user_rows, gt_ptr, gt_idx,
                                            (ex_ptr.to(dev), ex_idx.to(dev)), **kw)
    return (rank, vals, us, gs, stats) if return_stats else (rank, vals, us, gs)


def ranks_to_metrics(rank, users, ks=(10,)):
    """Full-ranking metrics from rank_items' ranks (0 = the item is excluded for the user) and
    the pairs' users, every sum on the device in float64 -> dict:
      unranked      pairs with rank 0
      mrr           mean of 1 / rank over the ranked pairs
      mean_rank     mean rank over the ranked pairs
      recall@k      pairs with 1 <= rank <= k / all pairs (unranked included): for the same
                    users' recommend(k) lists, recs_to_metrics_device's recall as the same ratio
      hit_rate@k    users with at least one pair of rank in [1, k] / users among the pairs
      ndcg@k        binary relevance over each user's distinct ranked items (a repeated pair
                    counts once): DCG = sum of 1 / log2(1 + rank) over ranks <= k, IDCG over the
                    first min(k, distinct ranked items) positions; the mean over the users with
                    at least one ranked item
    Ratios with an empty denominator are nan."""
    ops._dev(rank, 'rank', torch.int64)
    ops._dev(users, 'users', torch.int64)
    rank, users = rank.reshape(-1), users.reshape(-1)
    if rank.numel() != users.numel():
        raise ValueError(f'ranks_to_metrics: {rank.numel()} ranks for {users.numel()} users')
    ks = tuple(int(k) for k in ks)
    if any(k < 1 for k in ks):
        raise ValueError('ranks_to_metrics: every k must be >= 1')
    dev, P = rank.device, rank.numel()
    nan = float('nan')

    def ratio(a, b):
        return float(a) / float(b) if float(b) else nan

    ranked = rank > 0
    n_ranked = int(ranked.sum())
    rr = rank[ranked].to(torch.float64)
    out = {'unranked': P - n_ranked, 'mrr': ratio((1.0 / rr).sum(), n_ranked),
           'mean_rank': ratio(rr.sum(), n_ranked)}
    uniq, inv = torch.unique(users, return_inverse=True)
    U = uniq.numel()
    # each user's distinct ranked items: a rank names one item of a user's ranking
    span = int(rank.max()) + 1 if P else 1
    pair = torch.unique(inv[ranked] * span + rank[ranked])
    pu, pr = pair // span, pair % span
    n_dist = torch.bincount(pu, minlength=U)
    kmax = max(ks) if ks else 1
    disc = 1.0 / torch.log2(torch.arange(2, kmax + 2, device=dev, dtype=torch.float64))
    ideal = torch.cat([disc.new_zeros(1), torch.cumsum(disc, 0)])   # ideal[j]: j positions
    for k in ks:
        hit = ranked & (rank <= k)
        out[f'recall@{k}'] = ratio(hit.sum(), P)
        per_user = torch.zeros(U, dtype=torch.int64, device=dev)
        per_user.index_add_(0, inv, hit.to(torch.int64))
        out[f'hit_rate@{k}'] = ratio((per_user > 0).sum(), U)
        top = pr <= k
        dcg = torch.zeros(U, dtype=torch.float64, device=dev)
        dcg.index_add_(0, pu[top], disc[pr[top] - 1])
        has = n_dist > 0
        idcg = ideal[n_dist.clamp(max=k)]
        out[f'ndcg@{k}'] = ratio((dcg[has] / idcg[has]).sum(), int(has.sum()))
    return out


# ---- cached lists kept current after a refresh ---------------
# Largest dirty share of the item rows at which update_recommendations still runs the merge;
# above it the whole call re-ranks.  The sweep found no crossover up to its largest share: at
# 0.76 of the items (and 0.75 of the users) dirty every run of the update still beat every run
# of a full re-rank, 294 against 330 ms (profiles/live_recs_ab.md); nothing above
# that share is measured
LIVE_MAX_DIRTY_FRAC = 0.75


@contextlib.contextmanager
def _phase(phase_ms, name):
    """With a dict: the part's time between two device synchronisations, added to
    phase_ms[name] (a measurement, tools/bench_live_recs.py)."""
    if phase_ms is None:
        yield
        return
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        phase_ms[name] = phase_ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3


def no_dirty_rows(n_rows, device):
    """The final_dirty entry of a type none of whose rows changed: (zero marks, no ids)."""
    return (torch.zeros(n_rows, dtype=torch.int32, device=device),
            torch.empty(0, dtype=torch.int64, device=device))


def _dirty_entry(entry, n_rows, what):
    if entry is None:
        return None
    mark, ids = entry
    ops._dev(mark, f'{what} marks', torch.int32)
    ops._dev(ids, f'{what} ids', torch.int64)
    if mark.numel() != n_rows:
        raise ValueError(f'{what} marks must have {n_rows} entries, got {mark.numel()}')
    return mark.contiguous(), ids.reshape(-1).contiguous()


def _marked_ids(mark, count):
    """The ascending ids of the `count` non-zero entries of an int32 mark table."""
    ids = torch.empty(count, dtype=torch.int64, device=mark.device)
    if count:
        _lib.torch_ops().compact_marked(mark, ops.exclusive_scan(mark), ids)
    return ids


def update_recommendations(idx, vals, h_user, h_item, dirty_users, dirty_items, exclude=None, *,
                           batch_size=8192, max_dirty_frac=None, return_stats=False,
                           phase_ms=None, **recommend_kw):
    """The cached lists of EVERY user brought up to date, in place, after a refresh of the
    embedding tables: idx / vals [n_users, k] (row r = user r) as recommend(h_user_old,
    h_item_old, k, None, exclude_old) returned them become, bit for bit in both, what
    recommend(h_user, h_item, k, None, exclude) returns now.  Cosine head, no popularity.

    dirty_users / dirty_items: the rows the refresh rewrote, RefreshStats.final_dirty's entries
    — (mark int32 [n_rows], ids int64 ascending) device tensors, or None for every row
    (no_dirty_rows(n, device) for none); a row is dirty where its mark is non-zero, and ids
    lists exactly those rows (its length is the count the call relies on: nothing reads the
    device to check it).  Every other row of the tables, and the exclusion row
    of every user outside dirty_users, must be bitwise what the lists were computed from.

    A clean user's score against a clean item has not changed (the cosine reads the two rows
    and nothing else), so its list can only change through dirty items.  Per batch of clean
    users: the dirty items (normalised, bf16, once per call) are filtered against
    tau = the list's last score (the bf16 filter of recommend(): every dirty item scoring
    >= tau is kept), and ops.topk_update merges the kept ones into the list — dropping the
    list's own dirty entries — where the merged list is provably the exact one (DESIGN.md
    §22: the old list was padded, or k entries remain and the k-th is not worse than the old
    last entry).  The rows it cannot settle, the rows whose candidates exceed the slots, and
    the dirty users are re-ranked by one recommend(..., user_rows=...) call, so the result
    never depends on the merge.

    The whole call re-ranks (stats['full']) when either dirty entry is None, more than
    max_dirty_frac (default LIVE_MAX_DIRTY_FRAC) of the items are dirty, k > 64, or
    recommend's own fast path does not apply (d % 4 != 0, d > REC_MAX_D).  recommend_kw
    (sample, cand_cap, pop_sample) goes to recommend; head= and popularity= are refused (with
    popularity every user's denominator changes with any item; the MLP head has no merge yet).

    The host reads the device once (the size of the redo set and the count statistics, one
    transfer) apart from what the recommend call reads.  -> None, or with return_stats the
    dict: clean_rows, dirty_users, dirty_items, redo_rows (clean rows the merge handed back,
    overflowed ones included), overflow_rows (their candidates exceeded the slots),
    candidates_max (kept dirty items of a row, counted past the cap), full.  Rows left
    untouched are not counted (it would take a gather of every list's marks).

    phase_ms: for measurements only (tools/bench_live_recs.py).  With a dict, the device is
    synchronised around every part and the parts' times are added to its keys 'filter',
    'merge' and 'rerank' in ms; None (the default) synchronises nothing."""
    if recommend_kw.get('head') is not None or recommend_kw.get('popularity') is not None:
        raise ValueError('update_recommendations: the cosine head without popularity only '
                         '(head= / popularity= are refused)')
    ops._dev(h_user, 'h_user', torch.float32)
    ops._dev(h_item, 'h_item', torch.float32)
    ops._dev(idx, 'idx', torch.int64)
    ops._dev(vals, 'vals', torch.float32)
    if h_user.dim() != 2 or h_item.dim() != 2 or h_user.shape[1] != h_item.shape[1]:
        raise ValueError(f'h_user / h_item must be 2-D with one feature size, got '
                         f'{tuple(h_user.shape)} and {tuple(h_item.shape)}')
    n_users, d = h_user.shape
    n_items = h_item.shape[0]
    if idx.dim() != 2 or idx.shape[0] != n_users or idx.shape[1] < 1 or \
            vals.shape != idx.shape or not (idx.is_contiguous() and vals.is_contiguous()):
        raise ValueError(f'idx / vals must be contiguous [n_users = {n_users}, k], got '
                         f'{tuple(idx.shape)} and {tuple(vals.shape)}')
    k, batch_size = idx.shape[1], int(batch_size)
    frac = LIVE_MAX_DIRTY_FRAC if max_dirty_frac is None else float(max_dirty_frac)
    if batch_size < 1 or not 0.0 <= frac <= 1.0:
        raise ValueError('update_recommendations: batch_size must be >= 1 and max_dirty_frac '
                         'in [0, 1]')
    du = _dirty_entry(dirty_users, n_users, 'dirty_users')
    di = _dirty_entry(dirty_items, n_items, 'dirty_items')
    if exclude is not None:
        ex_ptr, ex_idx = exclude
        ops._dev(ex_ptr, 'exclude indptr', torch.int64)
        ops._dev(ex_idx, 'exclude indices', torch.int32)
        if ex_ptr.numel() != n_users + 1:
            raise ValueError(f'exclude indptr must have n_users + 1 = {n_users + 1} entries, '
                             f'got {ex_ptr.numel()}')
        exclude = (ex_ptr.contiguous(), ex_idx.contiguous())
    dev = h_item.device
    h_user, h_item = h_user.contiguous(), h_item.contiguous()
    stats = {'clean_rows': 0, 'dirty_users': n_users, 'dirty_items': n_items, 'redo_rows': 0,
             'overflow_rows': 0, 'candidates_max': 0, 'full': True}
    fast = d % 4 == 0 and 4 <= d <= REC_MAX_D and k <= ops.UPDATE_MAX_K
    if du is None or di is None or not fast or n_users == 0 or n_items == 0 or \
            di[1].numel() > frac * n_items:
        with _phase(phase_ms, 'rerank'):
            i, v = recommend(h_user, h_item, k, None, exclude, batch_size=batch_size,
                             **recommend_kw)
            idx.copy_(i)
            vals.copy_(v)
        return stats if return_stats else None
    (umark, uids), (imark, iids) = du, di
    n_du, n_di = uids.numel(), iids.numel()
    stats.update(clean_rows=n_users - n_du, dirty_users=n_du, dirty_items=n_di, full=False)
    if n_du == 0 and n_di == 0:
        return stats if return_stats else None
    ex0, ex1 = (None, None) if exclude is None else exclude
    todo = uids
    if n_di and n_du < n_users:
        cap = ops.UPDATE_SLOTS - k
        with _phase(phase_ms, 'filter'):
            clean = _marked_ids((umark == 0).to(torch.int32), n_users - n_du)
            items_bf = ops.normalize_rows_bf16(h_item, iids)     # converted once per call
            dirty_ids = iids.to(torch.int32)
        redo = torch.zeros(n_users, dtype=torch.int32, device=dev)
        counts = torch.zeros(clean.numel(), dtype=torch.int32, device=dev)
        cand = torch.empty((min(batch_size, clean.numel()), cap), dtype=torch.int32, device=dev)
        last = vals[:, k - 1]
        for b0 in range(0, clean.numel(), batch_size):
            rows = clean[b0:b0 + batch_size]
            cnt, cnd = counts[b0:b0 + rows.numel()], cand[:rows.numel()]
            with _phase(phase_ms, 'filter'):
                users_bf = ops.normalize_rows_bf16(h_user, rows)
                tau = last.index_select(0, rows)     # -inf for a padded list: keeps them all
                ops.score_bf16_filter(users_bf, items_bf, tau, cnt, cnd)
            with _phase(phase_ms, 'merge'):
                ops.topk_update(rows, idx, vals, imark, cnt, cnd, dirty_ids, h_user, h_item,
                                redo, ex0, ex1)
        n_redo, n_over, c_max = torch.stack(       # the call's one readback
            [redo.sum(), (counts > cap).sum(), counts.max()]).tolist()
        stats.update(redo_rows=n_redo, overflow_rows=n_over, candidates_max=c_max)
        if n_redo:
            todo = _marked_ids(torch.bitwise_or(redo, (umark != 0).to(torch.int32)),
                               n_redo + n_du)
    if todo.numel():
        with _phase(phase_ms, 'rerank'):
            i, v = recommend(h_user, h_item, k, todo, exclude, batch_size=batch_size,
                             **recommend_kw)
            ops.scatter_rows(idx, todo, i)
            ops.scatter_rows(vals, todo, v)
    return stats if return_stats else None


class LiveRecommendations:
    """Every user's top-k list of a graph under edits, kept equal to recommend_for_graph on the
    refreshed embeddings.

        inc = IncrementalEmbeddings(g, model)
        live = LiveRecommendations(inc, k=10)          # recommend_for_graph for every user
        inc.add_edges(u, v, etype='buys'); inc.add_edges(v, u, etype='bought-by')
        refresh_stats, update_stats = live.refresh()   # inc.refresh() + update_recommendations

    idx / vals [n_users, k] stay valid and are updated in place; they are replaced (by grown
    tensors, the new rows re-ranked as dirty users) when users were added, and by new tensors
    with every user re-ranked (stats['full']) when a type was renumbered (inc.remove_nodes;
    inc.numbering shows it): the cached lists hold item ids of the old numbering and are not
    remapped.  The items each
    user has an `etype` edge from are excluded, as in recommend_for_graph.  A refresh of `inc`
    that did not go through this object (inc.generation shows it) makes the next refresh()
    re-rank every user.  kw (batch_size, sample, cand_cap) goes to recommend; head= and
    popularity are refused.  phase_ms: for measurements only — set it to a dict and refresh()
    synchronises around its parts and adds their times ('refresh', 'filter', 'merge',
    'rerank', ms) to it."""

    def __init__(self, inc, k, etype='bought-by', max_dirty_frac=None, **kw):
        if kw.get('head') is not None or kw.get('popularity') is not None or \
                kw.get('use_popularity'):
            raise ValueError('LiveRecommendations: the cosine head without popularity only '
                             '(head= / popularity are refused)')
        self.inc, self.k, self.etype = inc, int(k), etype
        self.max_dirty_frac, self.kw = max_dirty_frac, dict(kw)
        self.phase_ms = None
        self.idx, self.vals = recommend_for_graph(inc.g, inc.h, self.k, None, etype, **self.kw)
        self._generation, self._numbering = inc.generation, inc.numbering

    def refresh(self):
        """inc.refresh(), then the lists of every user brought up to date ->
        (RefreshStats, the stats of update_recommendations)."""
        inc = self.inc
        skipped = inc.generation != self._generation   # a refresh this object did not see
        with _phase(self.phase_ms, 'refresh'):
            rstats = inc.refresh()
        h = inc.h
        dev, n_users, n_items = h['item'].device, h['user'].shape[0], h['item'].shape[0]
        if inc.numbering != self._numbering:   # a type was renumbered: no list survives
            self.idx = self.idx.new_full((n_users, self.k), -1)
            self.vals = self.vals.new_full((n_users, self.k), float('-inf'))
            skipped = True
        grown = n_users - self.idx.shape[0]
        if grown > 0:    # users were added: their rows are dirty users, re-ranked below
            self.idx = torch.cat([self.idx, self.idx.new_full((grown, self.k), -1)])
            self.vals = torch.cat([self.vals, self.vals.new_full((grown, self.k),
                                                                 float('-inf'))])
        fd = rstats.final_dirty
        du = di = None
        if not skipped:
            du = fd['user'] if 'user' in fd else no_dirty_rows(n_users, dev)
            di = fd['item'] if 'item' in fd else no_dirty_rows(n_items, dev)
        ex_ptr, ex_idx = inc.g.in_csr(self.etype)[:2]
        ustats = update_recommendations(self.idx, self.vals, h['user'], h['item'], du, di,
                                        (ex_ptr.to(dev), ex_idx.to(dev)),
                                        max_dirty_frac=self.max_dirty_frac, return_stats=True,
                                        phase_ms=self.phase_ms, **self.kw)
        self._generation, self._numbering = inc.generation, inc.numbering
        return rstats, ustats


def recs_to_metrics_device(idx, user_rows, gt_indptr, gt_indices, n_items):
    """precision / recall / coverage of recs_to_metrics (reference src/metrics.py:81-107)
    from device tensors: idx [U, k] the lists of recommend() (-1 = no item), user_rows [U]
    their users (None: row r is user r; each user once, as in the reference's dict),
    (gt_indptr int64 [n_users + 1], gt_indices) the ground-truth items per user, duplicates
    kept.  precision: recommended items found in the user's ground truth / recommended
    items; recall: ground-truth edges (with multiplicity) of the served users whose item is
    in the user's list / those edges; coverage: distinct recommended items / n_items."""
    dev = idx.device
    U, k = idx.shape
    n_users = gt_indptr.numel() - 1
    if user_rows is None:
        user_rows = torch.arange(U, device=dev)
    user_rows = user_rows.to(dev).reshape(-1)
    gt_indptr = gt_indptr.to(dev)
    gt_items = gt_indices.to(dev).to(torch.int64)
    E = gt_items.numel()
    deg = gt_indptr[1:] - gt_indptr[:-1]
    gt_users = torch.repeat_interleave(torch.arange(n_users, device=dev), deg, output_size=E)
    ok = idx >= 0
    rec_items = idx[ok]
    rec_users = user_rows.unsqueeze(1).expand(U, k)[ok]
    # precision: (item -> user) membership in the ground truth
    ip, ix = ops.membership_csr(gt_items, gt_users, n_items, n_users)
    hit = ops.has_edges(ip, ix, n_items, rec_items, rec_users)
    precision = int(hit.sum()) / int(rec_items.numel())
    # recall: ground-truth edges of the served users found in the lists
    served = torch.zeros(n_users, dtype=torch.bool, device=dev)
    served[user_rows] = True
    e_ok = served[gt_users]
    ip, ix = ops.membership_csr(rec_items, rec_users, n_items, n_users)
    found = ops.has_edges(ip, ix, n_items, gt_items[e_ok], gt_users[e_ok])
    recall = int(found.sum()) / int(e_ok.sum())
    coverage = int(torch.unique(rec_items).numel()) / n_items
    return precision, recall, coverage


def recs_to_metrics(recs, ground_truth_dict, g):
    """precision / recall / coverage (reference src/metrics.py:81-107)."""
    k_relevant = k_total = 0
    for uid, iids in recs.items():
        gt = set(ground_truth_dict[uid])
        k_total += len(iids)
        k_relevant += sum(1 for i in iids if i in gt)
    precision = k_relevant / k_total
    k_relevant = k_total = 0
    for uid, iids in recs.items():
        rec = set(np.asarray(iids).tolist())
        k_total += len(ground_truth_dict[uid])
        k_relevant += sum(1 for i in ground_truth_dict[uid] if i in rec)
    recall = k_relevant / k_total
    nb_recommended = len(set(int(i) for v in recs.values() for i in v))
    coverage = nb_recommended / g.num_nodes('item')
    return precision, recall, coverage


def get_metrics_at_k(h, g, model, embed_dim, ground_truth, bought_eids, k,
                     remove_already_bought=True, cuda=True, device=None, pred='cos',
                     use_popularity=False, weight_popularity=1):
    """reference src/metrics.py:110-134."""
    already_bought_dict = create_already_bought(g, bought_eids)
    users, items = ground_truth
    user_ids = np.unique(users).tolist()
    ground_truth_dict = create_ground_truth(users, items)
    recs = get_recs(g, h, model, embed_dim, k, user_ids, already_bought_dict,
                    remove_already_bought, cuda, device, pred, use_popularity, weight_popularity)
    return recs_to_metrics(recs, ground_truth_dict, g)


def MRR_neg_edges(model, blocks, pos_g, neg_g, etype, neg_sample_size):
    """Mean reciprocal rank of each positive edge among its negatives (reference
    src/metrics.py:137-157, marked "currently not used" there).  The reference passes
    `etype` where ConvModel.forward expects `embedding_layer` and reshapes the per-etype
    score dict directly; here the model runs with its own embedding_layer setting and the
    scores of `etype` are ranked: rank = #{neg >= pos} + 1 over the positive's
    neg_sample_size negatives (negatives grouped [E_pos, K], sampling.py:163-165)."""
    input_features = blocks[0].srcdata['features']
    with torch.no_grad():
        _, pos_score, neg_score = model(blocks, input_features, pos_g, neg_g,
                                        getattr(model, 'embedding_layer', True))
    if isinstance(pos_score, dict):
        ce = next(c for c in pos_score if etype in (c, c[1]))
        pos_score, neg_score = pos_score[ce], neg_score[ce]
    neg = neg_score.reshape(-1, neg_sample_size)
    rankings = torch.sum(neg >= pos_score.reshape(-1, 1), dim=1) + 1
    return float(np.mean(1.0 / rankings.cpu().numpy()))
