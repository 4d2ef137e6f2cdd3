"""Popularity-weighted exact top-k without a score matrix (gnnrec.recs.recommend with
popularity=) against the score-matrix path it stands beside
(get_recs(use_popularity=True): fp32 MFMA GEMM or dense MLP scores, torch.softmax, the
popularity row, topk_rows), C4 item count, random normal tables.  HIP events, warm-up, medians
of alternating runs in one process.

    python tools/bench_recommend_pop.py [--out profiles/recommend_pop_ab.json]

Popularity as the reference builds it (about 5 % of the items non-zero, Zipf counts over
their sum) at weights .01 and .1, and one dense uniform popularity at a weight that makes
both terms matter (4 / n_items).
1. one batch, cosine head: 1024 users x 1M items, d = 128, k = 10, 50 bought items per user —
   the old path's launches, the new path end to end and stage by stage, the denominator pass
   against ops.gemm of the same shape;
2. many users, cosine head: recommend() over 65536 users; candidate statistics; the lists
   against the old path's under the tie rule (a differing rank must hold ratings within 1e-5
   relative of each other);
3. the MLP head: recommend(head=, popularity=) and get_recs(pred='nn', use_popularity=True)
   over 1024 users, the denominator pass alone, 65536 users.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn-recsys_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gnnrec import ops  # noqa: E402
from gnnrec.nn import PredictingLayer  # noqa: E402
from gnnrec.recs import _MlpHead, _normalize_rows, _popular_sample, get_recs, recommend, \
    topk_rows  # noqa: E402


def timed(fns, reps):
    """Median ms per function, the functions run in turn `reps` times (alternating)."""
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ms[name].append(s.elapsed_time(e))
    return {name: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            for name, v in ms.items()}


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


class _G:
    def __init__(self, pop):
        self.ndata = {"popularity": {"item": pop}}


def tie_rule_violations(idx_new, vals_new, idx_old, vals_old, tol=1e-5):
    """Rows that differ item for item, and ranks that differ without the two ratings being
    within tol relative of each other."""
    diff = idx_new != idx_old
    a, b = vals_new.astype(np.float64), vals_old.astype(np.float64)
    far = diff & (np.abs(a - b) > tol * np.maximum(np.abs(a), np.abs(b)))
    return int(diff.any(1).sum()), int(far.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--users", type=int, default=65_536)
    ap.add_argument("--mlp-users", type=int, default=65_536)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--bought", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n_u, n_i, d, k = a.users, a.items, a.d, a.k
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    h_user = torch.randn(n_u, d, device=dev, generator=g)
    h_item = torch.randn(n_i, d, device=dev, generator=g)
    ex_ptr = torch.arange(n_u + 1, device=dev) * a.bought
    ex_idx = torch.randint(0, n_i, (n_u * a.bought,), device=dev, generator=g, dtype=torch.int32)
    exclude = (ex_ptr, ex_idx)
    rng = np.random.default_rng(0)
    nz = rng.choice(n_i, n_i // 20, replace=False)
    counts = rng.zipf(1.5, nz.size).astype(np.float64)
    sparse = np.zeros(n_i, np.float32)
    sparse[nz] = (counts / counts.sum()).astype(np.float32)
    pops = {"sparse w=.01": (torch.from_numpy(sparse).to(dev), 0.01),
            "sparse w=.1": (torch.from_numpy(sparse).to(dev), 0.1),
            "dense uniform w=4/n": (torch.rand(n_i, device=dev, generator=g), 4.0 / n_i)}
    res = {"shape": {"users": n_u, "items": n_i, "d": d, "k": k, "bought": a.bought,
                     "device": torch.cuda.get_device_name(0)}}

    # ---- 1. one 1024-user batch, cosine head
    B = 1024
    rows = torch.arange(B, device=dev)
    ex64 = ex_idx[:B * a.bought].to(torch.int64)
    items_hat = _normalize_rows(h_item)
    u_hat = _normalize_rows(h_user[:B].contiguous())
    items_f32 = ops.normalize_rows_f32(h_item)
    items_bf = ops.normalize_rows_bf16(h_item)
    pop, w = pops["sparse w=.01"]
    p = (pop * w).contiguous()
    col_ids = _popular_sample(p, min(65536, n_i), 4096)
    cols = col_ids.to(torch.int64)
    sample_bf, p_col, pmax = items_bf[cols].contiguous(), p[cols].contiguous(), p.max().reshape(1)
    st = {}

    def old_gemm():
        st["scores"] = ops.gemm(u_hat, items_hat)

    def old_softmax_pop():
        st["rated"] = torch.softmax(st["scores"], dim=1) + p

    def old_topk():
        st["old"] = topk_rows(st["rated"], k, ex_ptr[:B + 1], ex64)

    def new_norm():
        st["uf"] = ops.normalize_rows_f32(h_user, rows)
        st["ub"] = ops.normalize_rows_bf16(h_user, rows)

    def new_denominators():
        st["Z"] = ops.cos_denominators(st["uf"], items_f32)

    def new_sample():
        s = ops.score_bf16_store_rating(st["ub"], sample_bf, st["Z"], p_col)
        ops.mask_excluded_mapped(s, col_ids, rows, ex_ptr, ex_idx)
        st["tau"] = topk_rows(s, k)[0][:, k - 1].contiguous()

    def new_filter():
        st["counts"] = torch.zeros(B, dtype=torch.int32, device=dev)
        st["cand"] = torch.empty((B, 1024), dtype=torch.int32, device=dev)
        thr = ops.rating_thresholds(st["tau"], st["Z"], pmax)
        ops.score_bf16_filter_rating(st["ub"], items_bf, st["Z"], p, thr, st["counts"], st["cand"])

    def new_cand():
        ops.topk_candidates_rating(st["counts"], st["cand"], rows, h_user, h_item, st["Z"], p, k,
                                   ex_ptr, ex_idx)

    def new_call():
        st["new"] = recommend(h_user, h_item, k, rows, exclude, batch_size=B, popularity=pop,
                              weight_popularity=w)

    fns = {"old: score GEMM (fp32 MFMA)": old_gemm,
           "old: torch.softmax + popularity": old_softmax_pop,
           "old: topk_rows": old_topk,
           "new: normalise users (fp32 and bf16)": new_norm,
           "new: denominators (fp32 MFMA, nothing stored)": new_denominators,
           "new: sample pass (store-R, mask, top-k)": new_sample,
           "new: thresholds + filter pass (bf16 MFMA, Ra compared)": new_filter,
           "new: candidates (fp32 rescore, R, rank)": new_cand,
           "new: recommend(popularity=) end to end, item conversions and readback included":
               new_call,
           "new: item table conversions (once per call)":
               lambda: (ops.normalize_rows_f32(h_item), ops.normalize_rows_bf16(h_item))}
    timed(fns, 2)  # warm-up
    one = timed(fns, a.reps)
    old = sum(one[n]["ms"] for n in fns if n.startswith("old:"))
    stages = sum(one[n]["ms"] for n in fns if n.startswith("new:") and "recommend(" not in n
                 and "conversions" not in n)
    one["old path total (three launches' worth)"] = {"ms": old}
    one["new path, the five per-batch stages"] = {"ms": stages}
    one["speed-up of the per-batch stages over the old path"] = old / stages
    one["denominator pass / score GEMM"] = \
        one["new: denominators (fp32 MFMA, nothing stored)"]["ms"] / \
        one["old: score GEMM (fp32 MFMA)"]["ms"]
    one["denominator pass fp32 TFLOP/s"] = \
        2.0 * B * n_i * d / one["new: denominators (fp32 MFMA, nothing stored)"]["ms"] / 1e9
    cnt = st["counts"].cpu().numpy()
    one["candidates per row"] = {"mean": float(cnt.mean()), "max": int(cnt.max()),
                                 "overflow_rows": int((cnt > 1024).sum())}
    res["one batch of 1024 users, cosine head, sparse w=.01"] = one
    del st["scores"], st["rated"]

    # get_recs itself (host dict in, host lists out) and the lists, per popularity
    exi = ex_idx[:B * a.bought].cpu().numpy().reshape(B, a.bought)
    bought = {u: exi[u].tolist() for u in range(B)}
    h = {"user": h_user, "item": h_item}
    per_pop = {}
    for name, (pop, w) in pops.items():
        get_recs(_G(pop), h, None, d, k, list(range(B)), bought, use_popularity=True,
                 weight_popularity=w)
        t_old = [wall(lambda: get_recs(_G(pop), h, None, d, k, list(range(B)), bought,
                                       use_popularity=True, weight_popularity=w))[0]
                 for _ in range(3)]
        recommend(h_user, h_item, k, rows, exclude, batch_size=B, popularity=pop,
                  weight_popularity=w)
        t_new, out = [], None
        for _ in range(3):
            dt, out = wall(lambda: recommend(h_user, h_item, k, rows, exclude, batch_size=B,
                                             popularity=pop, weight_popularity=w,
                                             return_stats=True))
            t_new.append(dt)
        idx, vals, stats = out
        rated = torch.softmax(ops.gemm(u_hat, items_hat), dim=1) + pop * w
        ov, oi = topk_rows(rated, k, ex_ptr[:B + 1], ex64)
        del rated
        rows_diff, far = tie_rule_violations(idx.cpu().numpy(), vals.cpu().numpy(),
                                             oi.cpu().numpy(), ov.cpu().numpy())
        per_pop[name] = {"get_recs(use_popularity=True) 1024 users, wall ms (3 runs)":
                         [1e3 * t for t in t_old],
                         "recommend(popularity=) 1024 users, wall ms (3 runs)":
                         [1e3 * t for t in t_new],
                         "stats": stats, "rows differing item for item": rows_diff,
                         "ranks differing beyond the tie rule": far}
    res["1024 users, cosine head, per popularity"] = per_pop
    del items_hat, u_hat, st

    # ---- 2. many users, cosine head
    many = {}
    pop, w = pops["sparse w=.01"]
    for bs in (1024, 8192):
        recommend(h_user[:bs * 2], h_item, k, None, (ex_ptr[:bs * 2 + 1], ex_idx), batch_size=bs,
                  popularity=pop, weight_popularity=w)
        dt, out = wall(lambda: recommend(h_user, h_item, k, None, exclude, batch_size=bs,
                                         popularity=pop, weight_popularity=w, return_stats=True))
        many[f"recommend(popularity=) {n_u} users, batch_size {bs}"] = {
            "s": dt, "users_per_s": n_u / dt, "stats": out[2]}
    res["many users, cosine head, sparse w=.01"] = many

    # ---- 3. the MLP head
    torch.manual_seed(0)
    head = PredictingLayer(d).to(dev).eval()
    model = type("M", (), {})()
    model.pred_fn = type("P", (), {})()
    model.pred_fn.layer_nn = head
    mlp_res = {}
    with torch.no_grad():
        mlp = _MlpHead(head, h_user, h_item)
        P = mlp.P(rows)
        stages = timed({"denominator pass (dense kernel, nothing stored)":
                        lambda: mlp.denominators(P)}, 3)
        mlp_res.update(stages)
        recommend(h_user, h_item, k, rows, exclude, batch_size=B, head=head, popularity=pop,
                  weight_popularity=w)
        t_new = [wall(lambda: recommend(h_user, h_item, k, rows, exclude, batch_size=B, head=head,
                                        popularity=pop, weight_popularity=w,
                                        return_stats=True)) for _ in range(3)]
        mlp_res["recommend(head=, popularity=) 1024 users, wall ms (3 runs)"] = \
            [1e3 * t for t, _ in t_new]
        mlp_res["stats"] = t_new[-1][1][2]
        t_old = [wall(lambda: get_recs(_G(pop), h, model, d, k, list(range(B)), bought,
                                       pred="nn", use_popularity=True, weight_popularity=w))
                 for _ in range(2)]
        mlp_res["get_recs(pred='nn', use_popularity=True) 1024 users, wall ms (2 runs)"] = \
            [1e3 * t for t, _ in t_old]
        ref = t_old[-1][1]
        got = t_new[-1][1][0].cpu().numpy()
        mlp_res["rows whose item set differs from get_recs"] = int(sum(
            set(got[u].tolist()) != set(ref[u].tolist()) for u in range(B)))
        if a.mlp_users > B:
            n_m = min(a.mlp_users, n_u)
            dt, out = wall(lambda: recommend(h_user[:n_m], h_item, k, None,
                                             (ex_ptr[:n_m + 1], ex_idx), batch_size=8192,
                                             head=head, popularity=pop, weight_popularity=w,
                                             return_stats=True))
            mlp_res[f"recommend(head=, popularity=) {n_m} users, batch_size 8192"] = {
                "s": dt, "users_per_s": n_m / dt, "stats": out[2]}
    res["MLP head, sparse w=.01"] = mlp_res
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
