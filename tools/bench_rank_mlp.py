"""Exact full-ranking positions for the MLP head without a score matrix
(gnnrec.recs.rank_items(head=...)), plain and popularity-weighted, against
  * the count pass alone (ops.edge_mlp_dense_count_lists / _lists_rating, every pair a row with
    one entry, as rank_items runs it),
  * ops.edge_mlp_dense_denominators of the same shape in the same run — the same loop over the
    items with another epilogue, the count pass's yardstick — and
  * the exact path that existed before it: exhaustive _MlpHead.score_rows chunks plus the
    definition on the device (recs._ranks_exact).
C4 item count, random normal tables and a randomly initialised head.  HIP events, warm-up,
medians of alternating runs in one process.

    python tools/bench_rank_mlp.py [--out profiles/rank_mlp_ab.json]

d = 128, 50 bought items per user, 8 held-out pairs per user; 1,024 and 65,536 pairs against 1M
items.  The exhaustive path runs on the first min(pairs, --exact-pairs) pairs of each size (it
works in independent chunks of 2^26 / n_items rows, so its time is linear in the pairs: the
figure for all pairs is that time scaled, and says so).  The ranks must equal the exhaustive
ones."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn-recsys_amd"))
import torch  # noqa: E402

from gnnrec import ops, recs  # noqa: E402
from gnnrec.nn import PredictingLayer  # noqa: E402


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
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n_i, d, bs = a.items, a.d, a.batch_size
    n_u = max(a.pairs) // a.per_user
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    torch.manual_seed(0)
    head = PredictingLayer(d).to(dev).eval()
    h_user = torch.randn(n_u, d, device=dev, generator=g)
    h_item = torch.randn(n_i, d, device=dev, generator=g)
    pop = torch.rand(n_i, device=dev, generator=g)
    ex_ptr = torch.arange(n_u + 1, device=dev) * a.bought
    ex_idx = torch.randint(0, n_i, (n_u * a.bought,), device=dev, generator=g, dtype=torch.int32)
    exclude = (ex_ptr, ex_idx)
    res = {"shape": {"items": n_i, "users": n_u, "d": d, "bought": a.bought,
                     "pairs_per_user": a.per_user, "batch_size": bs, "reps": a.reps,
                     "weight_popularity": a.weight, "device": torch.cuda.get_device_name(0)}}
    p = recs._popularity_vector(pop, a.weight, n_i)
    plain = recs._MlpHead(head, h_user, h_item)
    rated = recs._MlpHead(head, h_user, h_item, p)
    E2E = "rank_items(head=) end to end (Q, exclusion sort, id check included)"
    E2E_R = "rank_items(head=, popularity=) end to end"
    CNT, CNT_R = "count pass alone", "count pass alone, rating form"
    DEN = "denominators pass of the same shape (ops.edge_mlp_dense_denominators)"
    for P in a.pairs:
        users = torch.arange(P // a.per_user, device=dev).repeat_interleave(a.per_user)
        items = torch.randint(0, n_i, (P,), device=dev, generator=g)
        items[::a.per_user] = ex_idx[::a.bought][:P // a.per_user].long()   # one excluded item
        gid = items.to(torch.int32)
        n_x = min(P, a.exact_pairs)
        st = {}
        # the count passes' per-batch inputs, formed once outside the timed regions
        Pb = [plain.P(users[b:b + bs]) for b in range(0, P, bs)]
        sb = [ops.edge_mlp(torch.arange(pb.shape[0], device=dev), items[b:b + bs], pb, plain.Q,
                           *plain.tail) for pb, b in zip(Pb, range(0, P, bs))]
        Zb = [plain.denominators(pb) for pb in Pb]
        lptr = torch.arange(min(bs, P) + 1, device=dev)     # a pair is a one-slot row
        EX, EX_R = (f"exhaustive: score_rows + the definition, first {n_x} pairs",
                    f"exhaustive with ratings (denominators included), first {n_x} pairs")

        def e2e():
            st["new"] = recs.rank_items(h_user, h_item, users, items, exclude, batch_size=bs,
                                        return_stats=True, head=head)

        def e2e_r():
            st["new_r"] = recs.rank_items(h_user, h_item, users, items, exclude, batch_size=bs,
                                          return_stats=True, head=head, popularity=pop,
                                          weight_popularity=a.weight)

        def count():
            st["ahead"] = [ops.edge_mlp_dense_count_lists(pb, plain.Q, *plain.tail,
                                                          lptr[:pb.shape[0] + 1], s, gid[b:b + bs])
                           for pb, s, b in zip(Pb, sb, range(0, P, bs))]

        def count_r():
            st["ahead_r"] = [ops.edge_mlp_dense_count_lists_rating(pb, plain.Q, *plain.tail, z, p,
                                                                   lptr[:pb.shape[0] + 1], s,
                                                                   gid[b:b + bs])
                             for pb, s, z, b in zip(Pb, sb, Zb, range(0, P, bs))]

        def denominators():
            st["Z"] = [plain.denominators(pb) for pb in Pb]

        def exhaustive():
            r = torch.empty(n_x, dtype=torch.int64, device=dev)
            recs._ranks_exact(plain, users[:n_x], items[:n_x], st["new"][1][:n_x], exclude, r,
                              torch.arange(n_x, device=dev))
            st["exact"] = r

        def exhaustive_r():
            r = torch.empty(n_x, dtype=torch.int64, device=dev)
            Z = torch.cat([rated.denominators_of(users[b:min(b + bs, n_x)])
                           for b in range(0, n_x, bs)])
            recs._ranks_exact(rated, users[:n_x], items[:n_x], st["new_r"][1][:n_x], exclude, r,
                              torch.arange(n_x, device=dev), Z)
            st["exact_r"] = r

        fns = {E2E: e2e, E2E_R: e2e_r, CNT: count, CNT_R: count_r, DEN: denominators,
               EX: exhaustive, EX_R: exhaustive_r}
        timed(fns, 1)  # warm-up
        print(f"{P} pairs: warm-up done", file=sys.stderr, flush=True)
        one = timed(fns, a.reps)
        for key, ex_key, tag in (("new", "exact", ""), ("new_r", "exact_r", ", ratings")):
            rank, _, stats = st[key]
            assert torch.equal(rank[:n_x], st[ex_key]), f"rank_items differs from the exhaustive ranks{tag}"
            one[f"stats{tag}"] = stats
            one[f"unranked pairs (excluded){tag}"] = int((rank == 0).sum())
        scale = P / n_x
        for new, ex, tag in ((E2E, EX, ""), (E2E_R, EX_R, ", ratings")):
            one[f"exhaustive, all {P} pairs{tag} (the measured time x {scale:g}: independent "
                f"chunks)"] = {"ms": one[ex]["ms"] * scale}
            one[f"speed-up of rank_items over the exhaustive path{tag}"] = \
                one[ex]["ms"] * scale / one[new]["ms"]
            one[f"slowest rank_items run / fastest exhaustive run (scaled){tag}"] = \
                one[new]["max_ms"] / (one[ex]["min_ms"] * scale)
        z = one[DEN]
        one["count pass / denominators pass"] = one[CNT]["ms"] / z["ms"]
        one["count pass, rating form / denominators pass"] = one[CNT_R]["ms"] / z["ms"]
        one["denominators pass run-to-run spread (max / min)"] = z["max_ms"] / z["min_ms"]
        one["ranks equal to the exhaustive ones"] = f"first {n_x} pairs, both forms"
        res[f"{P} pairs x {n_i} items"] = one
        print(f"{P} pairs: done", file=sys.stderr, flush=True)
        del st, Pb, sb, Zb
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
