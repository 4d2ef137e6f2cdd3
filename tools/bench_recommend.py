"""Exact top-k behind the bf16 MFMA prefilter (gnnrec.recs.recommend) against the score-matrix
path it stands beside (fp32 MFMA GEMM + topk_rows, what get_recs runs per batch), C4 item
count, random normal tables.  HIP events, warm-up, medians of alternating runs in one process.

    python tools/bench_recommend.py [--out profiles/recommend_ab.json]

1. one batch: 1024 users x 1M items, d = 128, k = 10, 50 bought items per user — the old
   path's two launches, the new path end to end and stage by stage;
2. many users: recommend() over 65536 users at batch_size 1024 and 8192 (device tensors in
   and out), get_recs over 16384 users for scale, and the candidate statistics.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn-recsys_amd"))
import torch  # noqa: E402

from gnnrec import ops  # noqa: E402
from gnnrec.recs import _normalize_rows, get_recs, recommend, topk_rows  # noqa: E402


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
    return {name: statistics.median(v) for name, v in ms.items()}, \
        {name: (min(v), max(v)) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--users", type=int, default=65_536)
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
    res = {"shape": {"users": n_u, "items": n_i, "d": d, "k": k, "bought": a.bought,
                     "device": torch.cuda.get_device_name(0)}}

    # ---- 1. one 1024-user batch
    B = 1024
    rows = torch.arange(B, device=dev)
    items_hat = _normalize_rows(h_item)
    u_hat = _normalize_rows(h_user[:B].contiguous())
    items_bf = ops.normalize_rows_bf16(h_item)
    m = min(65536, n_i)
    prefix_bf = items_bf[:m]
    st = {}

    def old_gemm():
        st["scores"] = ops.gemm(u_hat, items_hat)

    def old_topk():
        topk_rows(st["scores"], k)

    def new_norm():
        st["ub"] = ops.normalize_rows_bf16(h_user, rows)

    def new_sample():
        s = ops.score_bf16_store(st["ub"], prefix_bf)
        ops.mask_excluded(s, rows, ex_ptr, ex_idx)
        st["tau"] = topk_rows(s, k)[0][:, k - 1].contiguous()

    def new_filter():
        st["counts"] = torch.zeros(B, dtype=torch.int32, device=dev)
        st["cand"] = torch.empty((B, 1024), dtype=torch.int32, device=dev)
        ops.score_bf16_filter(st["ub"], items_bf, st["tau"], st["counts"], st["cand"])

    def new_cand():
        ops.topk_candidates(st["counts"], st["cand"], rows, h_user, h_item, k, ex_ptr, ex_idx)

    def new_call():
        recommend(h_user, h_item, k, rows, exclude, batch_size=B)

    fns = {"old: score GEMM (fp32 MFMA)": old_gemm, "old: topk_rows": old_topk,
           "new: normalise users": new_norm, "new: sample pass (store, mask, top-k)": new_sample,
           "new: filter pass (bf16 MFMA)": new_filter, "new: candidates (fp32 rescore, rank)": new_cand,
           "new: recommend() end to end, item conversion and readback included": new_call,
           "new: item table conversion (once per call)": lambda: ops.normalize_rows_bf16(h_item)}
    timed(fns, 2)  # warm-up
    med, spread = timed(fns, a.reps)
    one = {name: {"ms": med[name], "min_ms": spread[name][0], "max_ms": spread[name][1]}
           for name in fns}
    old = med["old: score GEMM (fp32 MFMA)"] + med["old: topk_rows"]
    stages = sum(med[n] for n in fns if n.startswith("new:") and "recommend()" not in n
                 and "conversion" not in n)
    flop = 2.0 * B * n_i * items_bf.shape[1]
    one["old path total"] = {"ms": old}
    one["new path, the four per-batch stages"] = {"ms": stages}
    one["speed-up of the per-batch stages over the old path"] = old / stages
    one["filter pass bf16 TFLOP/s"] = flop / med["new: filter pass (bf16 MFMA)"] / 1e9
    one["old GEMM fp32 TFLOP/s"] = 2.0 * B * n_i * d / med["old: score GEMM (fp32 MFMA)"] / 1e9
    one["filter pass share of the four stages"] = med["new: filter pass (bf16 MFMA)"] / stages
    res["one batch of 1024 users"] = one
    del items_hat, u_hat, st

    # ---- 2. many users
    many = {}
    for bs in (1024, 8192):
        recommend(h_user[:bs * 2], h_item, k, None, (ex_ptr[:bs * 2 + 1], ex_idx), batch_size=bs)
        torch.cuda.synchronize()
        t = time.perf_counter()
        idx, vals, stats = recommend(h_user, h_item, k, None, exclude, batch_size=bs,
                                     return_stats=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        many[f"recommend {n_u} users, batch_size {bs}"] = {
            "s": dt, "users_per_s": n_u / dt, "stats": stats}
    n_g = min(16_384, n_u)
    exi = ex_idx[:n_g * a.bought].cpu().numpy().reshape(n_g, a.bought)
    bought = {u: exi[u].tolist() for u in range(n_g)}
    h = {"user": h_user, "item": h_item}
    get_recs(None, h, None, d, k, list(range(1024)), bought)
    torch.cuda.synchronize()
    t = time.perf_counter()
    ref = get_recs(None, h, None, d, k, list(range(n_g)), bought)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    many[f"get_recs {n_g} users (host dict in, host lists out)"] = {"s": dt, "users_per_s": n_g / dt}
    # the two paths' lists: GEMM scores and sddmm_cos scores differ in the last bits, so a
    # near-tie may swap; count rows that differ as sets
    got = idx[:n_g].cpu().numpy()
    many["rows whose item set differs from get_recs"] = int(sum(
        set(got[u].tolist()) != set(ref[u].tolist()) for u in range(n_g)))
    res["many users"] = many
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
