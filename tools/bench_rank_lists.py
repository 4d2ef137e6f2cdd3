"""Full-ranking evaluation of held-out LISTS for the MLP head, one scored row per user
(gnnrec.recs.rank_lists(head=...)), against recs.rank_items(head=...) on
recs.list_pairs of the same lists — the same kernels on the expanded pairs, every pair a row
with one entry, so the column shows what sharing a scored row saves and is no independent
check of the results — plain and popularity-weighted, both timed end to end in alternation in
one process, their results compared after every run.  Beside them the list count pass alone
(ops.edge_mlp_dense_count_lists / _lists_rating) and ops.edge_mlp_dense_denominators over the
same rows in the same run — the same loop over the items with another epilogue, so the ratio
shows what the slot loop adds to the MFMA work.

    python tools/bench_rank_lists.py [--out profiles/rank_lists_ab.md]

tools/bench_rank_mlp.py's shapes: d = 128, 1M items, 50 bought items per user, a randomly
initialised head, uniform popularity with weight 0.5.  Lists of G = 8 items (128 and 8,192
users: 1,024 and 65,536 pairs), of G = 1 (nothing to share: the cost of the slot loop alone)
and of geometric lengths with mean 8 (long lists split over several rows).  The first item of
every list is one the user bought (rank 0).  HIP events, one warm-up round, medians of --reps
rounds."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn-recsys_amd"))
import torch  # noqa: E402

from gnnrec import ops, recs  # noqa: E402
from gnnrec.nn import PredictingLayer  # noqa: E402


def timed(fns, reps, after=None):
    """Median ms per function, the functions run in turn `reps` times (alternating); `after`
    runs once per round, outside the timed regions."""
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ms[name].append(s.elapsed_time(e))
        if after:
            after()
    return {name: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            for name, v in ms.items()}


def fmt(t):
    return f"{t['ms']:,.2f} ({t['min_ms']:,.2f} – {t['max_ms']:,.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--bought", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=8192)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="+",
                    default=["8:128", "8:8192", "1:1024", "1:8192", "geo8:8192"],
                    help="G:users, G a fixed list length or geoM (geometric lengths, mean M)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n_i, d, bs = a.items, a.d, a.batch_size
    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in a.cases]
    n_u = max(u for _, u in cases)
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
    shape = {"items": n_i, "d": d, "bought": a.bought, "batch_size": bs, "reps": a.reps,
             "weight_popularity": a.weight, "list_slots": ops.rank_list_slots(),
             "device": torch.cuda.get_device_name(0)}
    p = recs._popularity_vector(pop, a.weight, n_i)
    plain = recs._MlpHead(head, h_user, h_item)
    budget = ops.rank_list_slots()
    LISTS, ITEMS = "rank_lists(head=)", "rank_items(head=) on list_pairs"
    LISTS_R, ITEMS_R = "rank_lists(head=, popularity=)", "rank_items(head=, popularity=) on list_pairs"
    CNT, CNT_R = "list count pass alone", "list count pass alone, rating form"
    DEN = "denominators pass over the same rows"
    res = {"shape": shape}
    for G, U in cases:
        if G.startswith("geo"):
            mean = float(G[3:])
            lens = torch.empty(U, device=dev).geometric_(1.0 / mean, generator=g).long()
        else:
            lens = torch.full((U,), int(G), dtype=torch.int64, device=dev)
        # the ground-truth CSR is over all users: the first U have lists, the rest none
        gt_ptr = recs._ptr(torch.cat([lens, lens.new_zeros(n_u - U)]))
        E = int(gt_ptr[-1])
        gt_idx = torch.randint(0, n_i, (E,), device=dev, generator=g)
        gt_idx[gt_ptr[:U]] = ex_idx[::a.bought][:U].long()        # one bought item per list
        rows = torch.arange(U, device=dev)
        pu, pg = recs.list_pairs(rows, gt_ptr, gt_idx)
        st = {}
        # the count pass's inputs per batch of users, formed outside the timed regions
        owner, lptr = recs._list_row_plan(lens, budget)
        inputs = []
        for u0 in range(0, U, bs):
            u1 = min(U, u0 + bs)
            e0, e1 = int(gt_ptr[u0]), int(gt_ptr[u1])
            sel = (owner >= u0) & (owner < u1)
            r0 = int((owner < u0).sum())
            ro = owner[sel] - u0
            Pb = plain.P(rows[u0:u1])
            s = ops.edge_mlp(pu[e0:e1] - u0, pg[e0:e1], Pb, plain.Q, *plain.tail)
            lp = (lptr[r0:r0 + ro.numel() + 1] - e0).contiguous()
            Pr = Pb[ro].contiguous()
            inputs.append((Pr, lp, s, pg[e0:e1].to(torch.int32), plain.denominators(Pr)))
        n_rows = sum(x[0].shape[0] for x in inputs)

        def lists():
            st["lists"] = recs.rank_lists(h_user, h_item, rows, gt_ptr, gt_idx, exclude,
                                          head=head, batch_size=bs, return_stats=True)

        def items():
            st["items"] = recs.rank_items(h_user, h_item, pu, pg, exclude, head=head,
                                          batch_size=bs, return_stats=True)

        def lists_r():
            st["lists_r"] = recs.rank_lists(h_user, h_item, rows, gt_ptr, gt_idx, exclude,
                                            head=head, popularity=pop, weight_popularity=a.weight,
                                            batch_size=bs, return_stats=True)

        def items_r():
            st["items_r"] = recs.rank_items(h_user, h_item, pu, pg, exclude, head=head,
                                            popularity=pop, weight_popularity=a.weight,
                                            batch_size=bs, return_stats=True)

        def count():
            st["ahead"] = [ops.edge_mlp_dense_count_lists(Pr, plain.Q, *plain.tail, lp, s, gid)
                           for Pr, lp, s, gid, _ in inputs]

        def count_r():
            st["ahead_r"] = [ops.edge_mlp_dense_count_lists_rating(Pr, plain.Q, *plain.tail, Z, p,
                                                                   lp, s, gid)
                             for Pr, lp, s, gid, Z in inputs]

        def denominators():
            st["Z"] = [plain.denominators(Pr) for Pr, *_ in inputs]

        def same():     # after every round: the two paths' results, ranks and value bits
            for x, y in (("lists", "items"), ("lists_r", "items_r")):
                assert torch.equal(st[x][0], st[y][0]), f"{x}: ranks differ from rank_items'"
                assert torch.equal(st[x][1].view(torch.int32), st[y][1].view(torch.int32)), \
                    f"{x}: values differ from rank_items'"

        fns = {LISTS: lists, ITEMS: items, LISTS_R: lists_r, ITEMS_R: items_r, CNT: count,
               CNT_R: count_r, DEN: denominators}
        timed(fns, 1, same)  # warm-up
        print(f"G = {G}, {U} users: warm-up done", file=sys.stderr, flush=True)
        one = timed(fns, a.reps, same)
        one["users"], one["pairs"], one["rows"] = U, E, n_rows
        one["longest list"] = int(lens.max())
        one["stats"] = st["lists"][2]
        assert st["lists"][2]["rows"] == n_rows and st["lists"][2]["pairs"] == E
        one["unranked pairs (excluded)"] = int((st["lists"][0] == 0).sum())
        for new, old, tag in ((LISTS, ITEMS, ""), (LISTS_R, ITEMS_R, ", ratings")):
            one[f"speed-up over rank_items{tag}"] = one[old]["ms"] / one[new]["ms"]
            one[f"slowest rank_lists run / fastest rank_items run{tag}"] = \
                one[new]["max_ms"] / one[old]["min_ms"]
            one[f"own spread, max / min{tag}"] = [one[new]["max_ms"] / one[new]["min_ms"],
                                                  one[old]["max_ms"] / one[old]["min_ms"]]
        z = one[DEN]
        one["list count pass / denominators pass"] = one[CNT]["ms"] / z["ms"]
        one["list count pass, rating form / denominators pass"] = one[CNT_R]["ms"] / z["ms"]
        one["denominators pass run-to-run spread (max / min)"] = z["max_ms"] / z["min_ms"]
        res[f"G = {G}, {U} users"] = one
        print(f"G = {G}, {U} users: done", file=sys.stderr, flush=True)
        del st, inputs
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        keys = [k for k in res if k != "shape"]
        rows_md = [("users / pairs / rows of the pass (longest list)",
                    lambda o: f"{o['users']:,} / {o['pairs']:,} / {o['rows']:,} "
                              f"({o['longest list']})"),
                   (f"**`{LISTS}`**", lambda o: fmt(o[LISTS])),
                   (f"`{ITEMS}`", lambda o: fmt(o[ITEMS])),
                   ("speed-up", lambda o: f"{o['speed-up over rank_items']:.2f} ×"),
                   ("slowest `rank_lists` run / fastest `rank_items` run",
                    lambda o: f"{o['slowest rank_lists run / fastest rank_items run']:.3f}"),
                   (f"**`{LISTS_R}`**", lambda o: fmt(o[LISTS_R])),
                   (f"`{ITEMS_R}`", lambda o: fmt(o[ITEMS_R])),
                   ("speed-up, ratings", lambda o: f"{o['speed-up over rank_items, ratings']:.2f} ×"),
                   ("slowest `rank_lists` run / fastest `rank_items` run, ratings",
                    lambda o: f"{o['slowest rank_lists run / fastest rank_items run, ratings']:.3f}"),
                   (CNT, lambda o: fmt(o[CNT])),
                   (CNT_R, lambda o: fmt(o[CNT_R])),
                   (DEN + " (`ops.edge_mlp_dense_denominators`)", lambda o: fmt(o[DEN])),
                   ("list count pass / denominators pass",
                    lambda o: f"{o['list count pass / denominators pass']:.3f}"),
                   ("list count pass, rating form / denominators pass",
                    lambda o: f"{o['list count pass, rating form / denominators pass']:.3f}"),
                   ("denominators pass, max / min of its own runs",
                    lambda o: f"{o['denominators pass run-to-run spread (max / min)']:.3f}")]
        notes = ""      # whatever a person wrote under "## Notes" in an earlier file is kept
        if os.path.exists(a.out):
            old = open(a.out).read()
            notes = old[old.index("## Notes"):] if "## Notes" in old else ""
        with open(a.out, "w") as f:
            f.write("# Full-ranking evaluation of held-out lists: `recs.rank_lists(head=)` against "
                    "`recs.rank_items(head=)` on the lists' pairs\n\n")
            f.write("## Measured (written by tools/bench_rank_lists.py)\n\n")
            f.write(f"{shape['device']}; {n_i:,} items, d = {d}, {a.bought} bought items per "
                    f"user, batch_size {bs}, at most {budget} list entries per row of the pass; "
                    f"ms, median (min – max) of {a.reps} alternating rounds.  `rank_items(head=)` "
                    f"runs the same kernels on the expanded pairs, every pair a row with one "
                    f"entry.  The two calls' ranks and value bits were compared after every "
                    f"round, both forms.\n\n")
            f.write("| | " + " | ".join(keys) + " |\n|---|" + "---|" * len(keys) + "\n")
            for name, get in rows_md:
                f.write(f"| {name} | " + " | ".join(get(res[k]) for k in keys) + " |\n")
            if notes:
                f.write("\n" + notes)


if __name__ == "__main__":
    main()
