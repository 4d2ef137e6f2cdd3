"""IncrementalEmbeddings.refresh() against what a caller had before it — full_graph_embeddings
over the edited graph — on C2- and C4-sized bipartite graphs (buys / bought-by, d = 128,
two layers behind the NodeEmbeddings): a batch of new purchases joins both relations, then

  refresh   inc.refresh(): only the rows the batch can reach are recomputed;
  full      full_graph_embeddings(g, model) on the same edited graph.

Every run takes a NEW batch (a refresh consumes its edits; the graph grows by the batch each
run).  Median of `--runs` runs of each, alternating which goes first, a device
synchronisation around every run; after every run the refreshed tables are compared with the
full pass's, bit for bit, and the run fails when they differ.  Per batch size: the rows per
layer and type (|D_l|), whether a whole layer ran, the split of the refresh between its parts
(one more refresh with a synchronisation around every part: marks / scan / compact, row
extraction + gather + scatter, the layer kernels, the route check), and the whole-table
projections a row refresh still runs (ops.preproject of a pre-projected relation's source
table), timed alone.

--mark-sweep: the same comparison with the dirty share set directly — a share f of the users
and of the items is named with mark(), the row object falls back above f + 0.02, so layer 1
(share f) runs by rows in one object and whole in the other while layer 2 (every row dirty)
runs whole in both: one layer's row path against its whole-layer run at a known share.

--sweep: the threshold rule of max_dirty_frac.  Per batch size the same edits are refreshed by
two objects on one graph, one that never falls back (max_dirty_frac = 1) and one that always
runs whole layers (0); the default is the largest swept dirty share — the largest
|D_l[T]| / N_T of the refresh — at which all runs of the row path beat all runs of the whole
layers.

    python tools/bench_refresh.py [--users 1000000 --items 100000 --edges 50000000]
        [--batches 1000,0.01] [--zipf 0] [--sweep 10,100,1000,10000] [--md profiles/refresh_ab.md]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn-recsys_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gnnrec import nn as gnn  # noqa: E402
from gnnrec import ops  # noqa: E402
from gnnrec.graph import HeteroGraph  # noqa: E402
from gnnrec.inference import IncrementalEmbeddings, full_graph_embeddings  # noqa: E402

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
    ap.add_argument("--zipf", type=float, default=0.0, help="item Zipf exponent (0 = uniform)")
    ap.add_argument("--batches", type=str, default="1000,0.01",
                    help="edge counts (integers) or shares of --edges (floats)")
    ap.add_argument("--sweep", type=str, default=None,
                    help="batch sizes of the max_dirty_frac sweep (instead of --batches)")
    ap.add_argument("--mark-sweep", type=str, default=None,
                    help="shares of every type to name dirty with mark(): layer 1 alone by rows "
                         "against whole (layer 2 runs whole in both)")
    ap.add_argument("--max-dirty-frac", type=float, default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--md", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    U, I, E, d = a.users, a.items, a.edges, a.dim
    cdf = None
    if a.zipf > 0:
        w = 1.0 / np.arange(1, I + 1, dtype=np.float64) ** a.zipf
        cdf = torch.from_numpy(np.cumsum(w) / w.sum()).to(dev)
    u, i = ops.synth_edges(11, 0, E, U, I, dev, cdf)
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
    marks = a.mark_sweep is not None
    sweep = a.sweep is not None or marks
    spec = a.mark_sweep if marks else a.sweep if sweep else a.batches
    sizes = [float(b) for b in spec.split(",")] if marks else \
        [int(float(b) * E) if "." in b else int(b) for b in spec.split(",")]
    graph = {"users": U, "items": I, "edges_per_direction": E, "zipf": a.zipf, "d": d}
    with torch.no_grad():
        if sweep:
            incs = {"rows": IncrementalEmbeddings(g, model, max_dirty_frac=1.0),
                    "whole": IncrementalEmbeddings(g, model, max_dirty_frac=0.0)}
        else:
            incs = {"rows": IncrementalEmbeddings(g, model, max_dirty_frac=a.max_dirty_frac)}
    inc = incs["rows"]
    batch_no = [0]

    def edit():
        """A new batch into both relations, recorded in every object."""
        batch_no[0] += 1
        if marks:  # a share n of every type named dirty: no edge changes
            inc.max_dirty_frac = min(1.0, n + 0.02)  # layer 1 by rows, layer 2 (all) whole
            for nt, N in (("user", U), ("item", I)):
                ids = torch.randperm(N, device=dev)[:int(n * N)]
                for x in incs.values():
                    x.mark(nt, ids)
            return
        nu, ni = ops.synth_edges(100 + batch_no[0], 0, n, U, I, dev, cdf)
        nu, ni = nu.long(), ni.long()
        inc.add_edges(nu, ni, etype=BUYS)
        inc.add_edges(ni, nu, etype=BOUGHT)
        for k, other in incs.items():
            if other is not inc:  # the graph is edited already: name the destinations
                other.mark("item", ni)
                other.mark("user", nu)

    def equal(x):
        with torch.no_grad():
            h = full_graph_embeddings(g, model)
        return all(torch.equal(x.h[nt], h[nt]) for nt in h)

    rows_out = []
    for n in sizes:
        with torch.no_grad():
            edit()  # warm-up of this batch size, and the first equality check
            stats = {k: x.refresh() for k, x in incs.items()}
            same = all(equal(x) for x in incs.values())
            times = {k: [] for k in (*incs, "full")}
            last = stats["rows"]
            for r in range(a.runs):
                edit()
                order = [*incs, "full"] if r % 2 == 0 else ["full", *incs]
                for k in order:
                    if k == "full":
                        times[k].append(timed(lambda: full_graph_embeddings(g, model))[0])
                    else:
                        dt, st = timed(incs[k].refresh)
                        times[k].append(dt)
                        if k == "rows":
                            last = st
                same &= all(equal(x) for x in incs.values())
            # the split: one more refresh with a synchronisation around every part
            edit()
            inc.phase_ms = {}
            st = inc.refresh()
            phases, inc.phase_ms = {k: round(v, 3) for k, v in inc.phase_ms.items()}, None
            for k, other in incs.items():
                if other is not inc:
                    other.refresh()
            same &= all(equal(x) for x in incs.values())
            # the whole-table projections the row path still runs, alone
            resid = {}
            for li, layer in enumerate(model.layers, start=1):
                for ce in (BUYS, BOUGHT):
                    rg, mod = g.rel_graph(ce), layer.mods[ce[1]]
                    X = inc.layers[li - 1][ce[0]]
                    if ops.can_spmm_project(rg.indptr, X, inc.layers[li - 1][ce[2]],
                                            mod.fc_self.weight, mod.fc_neigh.weight) and \
                            ops.fused_preprojects(rg.indptr, X, inc.layers[li - 1][ce[2]], "mean"):
                        t = [timed(lambda: ops.preproject(X, mod.fc_neigh.weight))[0]
                             for _ in range(4)][1:]
                        resid[f"layer {li} {ce[1]} ({X.shape[0]:,} rows)"] = round(
                            statistics.median(t), 3)
        if not same:
            raise SystemExit(f"batch {n}: the refreshed tables differ from the full pass")
        share = max(c / (U if nt == "user" else I)
                    for per in last.rows for nt, c in per.items()) if any(last.rows) else 0.0
        row = {"graph": graph, "batch": n, "bitwise_equal": True,
               "rows_per_layer": last.rows, "whole_layer": last.whole_layer,
               "largest_dirty_share": round(share, 4),
               **{f"{'refresh' if k == 'rows' else k}_ms": summary(v) for k, v in times.items()},
               "refresh_beats_full_in_every_run": max(times["rows"]) < min(times["full"]),
               "refresh_parts_ms": phases, "whole_table_projections_ms": resid,
               "max_dirty_frac": inc.max_dirty_frac, "device": torch.cuda.get_device_name(0)}
        if sweep:
            row["rows_beat_whole_layers_in_every_run"] = max(times["rows"]) < min(times["whole"])
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if sweep:
        ok = [r["batch"] if marks else r["largest_dirty_share"] for r in rows_out
              if r["rows_beat_whole_layers_in_every_run"]]
        print(json.dumps({"sweep_default_max_dirty_frac": max(ok) if ok else 0.0}), flush=True)
    if a.md:
        def rng(r, k):
            x = r[k]
            return f"{x['median']:.2f} ({x['min']:.2f}–{x['max']:.2f})"
        with open(a.md, "a") as f:
            f.write(f"\n{E:,} edges per direction, {U:,} users x {I:,} items, zipf {a.zipf:g}, "
                    f"d = {d}, {rows_out[0]['device']}; ms, median (min–max) of {a.runs}"
                    f"{'; threshold sweep' if sweep else ''}\n\n")
            f.write("| batch | refresh | " + ("whole layers | " if sweep else "") +
                    "full pass | rows per layer (user / item) | largest dirty share | "
                    "marks / rows / layers / routes ms | whole-table projections ms | "
                    "bitwise equal |\n")
            f.write("|---|---|---|---|---|---|---|---|" + ("---|" if sweep else "") + "\n")
            for r in rows_out:
                per = "; ".join(f"L{li}: {p.get('user', 0):,} / {p.get('item', 0):,}" +
                                (" (whole)" if any(r["whole_layer"][li].values()) else "")
                                for li, p in enumerate(r["rows_per_layer"]) if li)
                ph = r["refresh_parts_ms"]
                parts = " / ".join(f"{ph.get(k, 0.0):.2f}" for k in ("marks", "rows", "layers",
                                                                    "routes"))
                res = "; ".join(f"{k}: {v:.2f}" for k, v in r["whole_table_projections_ms"].items())
                f.write(f"| {r['batch']:,} | {rng(r, 'refresh_ms')} | " +
                        (f"{rng(r, 'whole_ms')} | " if sweep else "") +
                        f"{rng(r, 'full_ms')} | {per} | {r['largest_dirty_share']:.4f} | {parts} | "
                        f"{res or '—'} | {r['bitwise_equal']} |\n")


if __name__ == "__main__":
    main()
