"""LiveRecommendations.refresh() against what a caller had before it — a refresh of the
embeddings followed by recommend_for_graph for EVERY user — on C2- and C4-sized bipartite
graphs (buys / bought-by, d = 128, two layers behind the NodeEmbeddings, k = 10, the items a
user bought excluded): a batch of new purchases joins both relations, then

  parent   inc.refresh() + recs.recommend_for_graph(g, inc.h, k): every list from nothing;
  live     live.refresh(): the same refresh, then only the lists a dirty row can change are
           touched (a bf16 filter of the clean users against the dirty items, the
           merge kernel, a re-rank of the dirty users and of the rows the merge hands back).

Two IncrementalEmbeddings objects share the graph (the second is told the batch's
destinations with mark()), so both arms refresh the same edit in the same call.  Every run
takes a NEW batch; median of `--runs` runs of each arm, alternating which goes first, a device
synchronisation around every run, one warm-up batch of every size first.  After every run the
live lists are compared with the parent arm's, torch.equal on idx and vals, and the run fails
when they differ.  Per batch size: the dirty rows, the rows handed back (redo) and overflowed,
and the split of the live arm (one more batch with a synchronisation around every part:
refresh / filter pass / merge kernel / re-rank).

--sweep: the same with the merge never falling back (max_dirty_frac = 1): the batch sizes are
chosen to give the wanted dirty item shares, and the default of recs.LIVE_MAX_DIRTY_FRAC is
the largest measured share at which every run of the live arm beat every run of the parent's.

    python tools/bench_live_recs.py [--users 1000000 --items 100000 --edges 50000000]
        [--batches 10,1000,0.01] [--sweep 20,100,600,1400,2000,2800] [--md profiles/live_recs_ab.md]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn-recsys_amd"))
import torch  # noqa: E402

from gnnrec import nn as gnn  # noqa: E402
from gnnrec import ops, recs  # noqa: E402
from gnnrec.graph import HeteroGraph  # noqa: E402
from gnnrec.inference import IncrementalEmbeddings  # noqa: E402

BUYS, BOUGHT = ("user", "buys", "item"), ("item", "bought-by", "user")


def timed(fn):
    gc.collect()
    gc.disable()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    gc.enable()
    return dt, out


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
            "max": round(max(v), 3), "runs": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=50_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=str, default="10,1000,0.01",
                    help="edge counts (integers) or shares of --edges (floats)")
    ap.add_argument("--sweep", type=str, default=None,
                    help="batch sizes of the max_dirty_frac sweep (instead of --batches)")
    ap.add_argument("--max-dirty-frac", type=float, default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--md", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    U, I, E, d, k = a.users, a.items, a.edges, a.dim, a.k
    u, i = ops.synth_edges(11, 0, E, U, I, dev, None)
    u, i = u.long(), i.long()
    g = HeteroGraph({BUYS: (u, i), BOUGHT: (i, u)}, {"user": U, "item": I}, device=dev)
    del u, i
    gen = torch.Generator(device=dev).manual_seed(1)
    g.ndata["features"] = {nt: torch.randn((n, d), device=dev, generator=gen)
                           for nt, n in (("user", U), ("item", I))}
    torch.manual_seed(0)
    model = gnn.ConvModel(g, 3, {"user": d, "item": d, "hidden": d, "out": d}, True, 0.0, "mean",
                          "cos", "sum", True).to(dev).eval()
    for ce in (BUYS, BOUGHT):  # what add_edges keeps merged from here on
        g.in_csr(ce)
        g.out_csr(ce)
    sweep = a.sweep is not None
    spec = a.sweep if sweep else a.batches
    sizes = [int(float(b) * E) if "." in b else int(b) for b in spec.split(",")]
    graph = {"users": U, "items": I, "edges_per_direction": E, "d": d, "k": k}
    frac = 1.0 if sweep else a.max_dirty_frac
    with torch.no_grad():
        # (the sweep: the refresh itself never falls back either, so that the dirty sets stay
        # lists above its own threshold and the merge is what is measured)
        inc = IncrementalEmbeddings(g, model, max_dirty_frac=frac if sweep else None)  # live arm
        par = IncrementalEmbeddings(g, model)       # the parent arm's, told the edits by mark()
        live = recs.LiveRecommendations(inc, k, max_dirty_frac=frac)
    print(f"# graph, tables and lists ready: {U:,} users x {I:,} items", file=sys.stderr, flush=True)
    batch_no = [0]

    def edit(n):
        batch_no[0] += 1
        nu, ni = ops.synth_edges(100 + batch_no[0], 0, n, U, I, dev, None)
        nu, ni = nu.long(), ni.long()
        inc.add_edges(nu, ni, etype=BUYS)
        inc.add_edges(ni, nu, etype=BOUGHT)
        par.mark("item", ni)   # the graph is edited already: name the destinations
        par.mark("user", nu)

    def parent_arm():
        par.refresh()
        return recs.recommend_for_graph(g, par.h, k)

    def same(lists):
        return torch.equal(live.idx, lists[0]) and torch.equal(live.vals, lists[1])

    rows_out = []
    with torch.no_grad():
        for n in sizes:
            edit(n)  # warm-up of this batch size, and the first equality check
            live.refresh()
            ok = same(parent_arm())
            times = {"live": [], "parent": []}
            us = None
            for r in range(a.runs):
                edit(n)
                lists = None
                for arm in (("live", "parent") if r % 2 == 0 else ("parent", "live")):
                    if arm == "live":
                        dt, (_rs, us) = timed(live.refresh)
                    else:
                        dt, lists = timed(parent_arm)
                    times[arm].append(dt)
                ok &= same(lists)
                del lists
            # the split: one more batch with a synchronisation around every part
            edit(n)
            live.phase_ms = {}
            _rs, us_split = live.refresh()
            phases, live.phase_ms = {p: round(v, 3) for p, v in live.phase_ms.items()}, None
            ok &= same(parent_arm())
            if not ok:
                raise SystemExit(f"batch {n}: the live lists differ from recommend_for_graph")
            row = {"graph": graph, "batch": n, "lists_equal": True,
                   "live_ms": summary(times["live"]), "parent_ms": summary(times["parent"]),
                   "live_beats_parent_in_every_run": max(times["live"]) < min(times["parent"]),
                   "speedup_of_medians": round(statistics.median(times["parent"]) /
                                               statistics.median(times["live"]), 3),
                   "update": us, "dirty_item_share": round(us["dirty_items"] / I, 4),
                   "dirty_user_share": round(us["dirty_users"] / U, 4),
                   "live_parts_ms": phases, "update_of_the_split_run": us_split,
                   "max_dirty_frac": recs.LIVE_MAX_DIRTY_FRAC if frac is None else frac,
                   "device": torch.cuda.get_device_name(0)}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
    if sweep:
        won = [r["dirty_item_share"] for r in rows_out if r["live_beats_parent_in_every_run"]]
        print(json.dumps({"sweep_default_max_dirty_frac": max(won) if won else 0.0}), flush=True)
    if a.md:
        def rng(r, key):
            x = r[key]
            return f"{x['median']:.1f} ({x['min']:.1f}–{x['max']:.1f})"
        with open(a.md, "a") as f:
            f.write(f"\n{E:,} edges per direction, {U:,} users x {I:,} items, d = {d}, k = {k}, "
                    f"{rows_out[0]['device']}; ms, median (min–max) of {a.runs}"
                    f"{'; sweep, max_dirty_frac = 1' if sweep else ''}\n\n")
            f.write("| batch | live | parent | parent / live | dirty users / items (share of items) "
                    "| redo rows | overflow rows | full | refresh / filter / merge / re-rank ms "
                    "| lists equal |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows_out:
                s, ph = r["update"], r["live_parts_ms"]
                parts = " / ".join(f"{ph.get(p, 0.0):.1f}" for p in ("refresh", "filter", "merge",
                                                                    "rerank"))
                f.write(f"| {r['batch']:,} | {rng(r, 'live_ms')} | {rng(r, 'parent_ms')} | "
                        f"{r['speedup_of_medians']:.2f} | {s['dirty_users']:,} / "
                        f"{s['dirty_items']:,} ({r['dirty_item_share']:.3f}) | {s['redo_rows']:,} | "
                        f"{s['overflow_rows']:,} | {s['full']} | {parts} | {r['lists_equal']} |\n")


if __name__ == "__main__":
    main()
