"""Exact full-ranking positions without a score matrix (gnnrec.recs.rank_items)
against the exact path that existed before it (exhaustive ops.sddmm_cos score rows plus the
definition on the device, recs._ranks_exact) and against the rating denominators' pass of the
same shape (ops.cos_denominators: the same MFMA loop with another epilogue).  C4 item count,
random normal tables.  HIP events, warm-up, medians of alternating runs in one process.

    python tools/bench_rank.py [--out profiles/rank_ab.json]

Two sizes, d = 128, 50 bought items per user, 8 held-out pairs per user:
  1,024 pairs and 65,536 pairs against 1M items.
Per size: rank_items end to end (its readback included) and stage by stage; the exhaustive
path on the first --exact-pairs pairs (it runs in independent chunks of 2^26 / n_items rows, so
its time is linear in the pairs: the figure for all pairs is that time scaled, and says so);
the denominators pass over the same rows.  The ranks must equal the exhaustive ones."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn-recsys_amd"))
import torch  # noqa: E402

from gnnrec import ops, recs  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1024, 65_536])
    ap.add_argument("--per-user", type=int, default=8)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--bought", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=8192)
    ap.add_argument("--exact-pairs", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n_i, d, bs = a.items, a.d, a.batch_size
    n_u = max(a.pairs) // a.per_user
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    h_user = torch.randn(n_u, d, device=dev, generator=g)
    h_item = torch.randn(n_i, d, device=dev, generator=g)
    ex_ptr = torch.arange(n_u + 1, device=dev) * a.bought
    ex_idx = torch.randint(0, n_i, (n_u * a.bought,), device=dev, generator=g, dtype=torch.int32)
    exclude = (ex_ptr, ex_idx)
    res = {"shape": {"items": n_i, "users": n_u, "d": d, "bought": a.bought,
                     "pairs_per_user": a.per_user, "batch_size": bs, "reps": a.reps,
                     "device": torch.cuda.get_device_name(0)}}
    items_f32 = ops.normalize_rows_f32(h_item)
    scorer = recs._CosHead(h_user, h_item)
    for P in a.pairs:
        users = torch.arange(P // a.per_user, device=dev).repeat_interleave(a.per_user)
        items = torch.randint(0, n_i, (P,), device=dev, generator=g)
        # one excluded item per user
        items[::a.per_user] = ex_idx[::a.bought][:P // a.per_user].long()
        n_x = min(P, a.exact_pairs)
        st = {}

        def new_call():
            st["new"] = recs.rank_items(h_user, h_item, users, items, exclude, batch_size=bs,
                                        return_stats=True)

        def thresholds():
            st["t"] = ops.sddmm_cos(users, items, h_user, h_item)

        def dedup():
            served = torch.zeros(n_u, dtype=torch.bool, device=dev)
            served[users] = True
            st["ex"] = recs._distinct_exclusions(exclude, served, P // a.per_user,
                                                 P // a.per_user * a.bought, n_i)

        def norm_users():
            st["uf"] = [ops.normalize_rows_f32(h_user, users[b:b + bs]) for b in range(0, P, bs)]

        def count():
            st["cnt"] = torch.zeros(P, dtype=torch.int32, device=dev)
            st["band"] = [torch.empty((uf.shape[0], 1024), dtype=torch.int32, device=dev)
                          for uf in st["uf"]]
            st["ahead"] = [ops.rank_count(uf, items_f32, st["t"][b:b + bs], st["cnt"][b:b + bs], bd)
                           for uf, bd, b in zip(st["uf"], st["band"], range(0, P, bs))]

        def resolve():
            st["rank"] = torch.cat([
                ops.rank_resolve(users[b:b + bs], items[b:b + bs], st["t"][b:b + bs], ah,
                                 st["cnt"][b:b + bs], bd, h_user, h_item, *st["ex"])
                for ah, bd, b in zip(st["ahead"], st["band"], range(0, P, bs))])

        def denominators():
            st["Z"] = [ops.cos_denominators(uf, items_f32) for uf in st["uf"]]

        def exhaustive():
            r = torch.empty(n_x, dtype=torch.int64, device=dev)
            recs._ranks_exact(scorer, users[:n_x], items[:n_x], st["t"][:n_x], exclude, r,
                              torch.arange(n_x, device=dev))
            st["exact"] = r

        fns = {"rank_items end to end (item conversion, exclusion sort, readbacks included)":
               new_call,
               "stage: thresholds (sddmm_cos of the pairs)": thresholds,
               "stage: the served users' exclusion rows sorted, repeats struck (once per call)":
               dedup,
               "stage: normalise the pairs' user rows (fp32)": norm_users,
               "stage: count pass (fp32 MFMA, nothing stored)": count,
               "stage: resolve (band + excluded items rescored)": resolve,
               "denominators pass of the same shape (ops.cos_denominators)": denominators,
               f"exhaustive: score_rows + the definition, first {n_x} pairs": exhaustive,
               "item table conversion (once per call)": lambda: ops.normalize_rows_f32(h_item)}
        timed(fns, 1)  # warm-up
        one = timed(fns, a.reps)
        rank, _, stats = st["new"]
        assert torch.equal(rank[:n_x], st["exact"]), "rank_items differs from the exhaustive ranks"
        assert torch.equal(rank, st["rank"]), "the staged run differs from rank_items"
        ex_ms = one[f"exhaustive: score_rows + the definition, first {n_x} pairs"]
        new_ms = one["rank_items end to end (item conversion, exclusion sort, readbacks included)"]
        one[f"exhaustive, all {P} pairs (the measured time x {P / n_x:g}: independent chunks)"] = \
            {"ms": ex_ms["ms"] * P / n_x}
        one["speed-up of rank_items over the exhaustive path"] = \
            ex_ms["ms"] * P / n_x / new_ms["ms"]
        one["slowest rank_items run / fastest exhaustive run (scaled)"] = \
            new_ms["max_ms"] / (ex_ms["min_ms"] * P / n_x)
        c = one["stage: count pass (fp32 MFMA, nothing stored)"]
        z = one["denominators pass of the same shape (ops.cos_denominators)"]
        one["count pass / denominators pass"] = c["ms"] / z["ms"]
        one["denominators pass run-to-run spread (max / min)"] = z["max_ms"] / z["min_ms"]
        one["count pass fp32 TFLOP/s"] = 2.0 * P * n_i * d / c["ms"] / 1e9
        one["stats"] = stats
        one["ranks equal to the exhaustive ones"] = f"first {n_x} pairs"
        one["unranked pairs (excluded)"] = int((rank == 0).sum())
        res[f"{P} pairs x {n_i} items"] = one
        del st
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
