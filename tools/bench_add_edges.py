"""HeteroGraph.add_edges against the rebuild a caller had to do before it, on C2's graph
(1M users x 100k items, 50M edges per direction): a batch of new purchases joins `buys` and
`bought-by`, both in-CSRs cached, the `recency` edge field carried.

  merge     clone(), add_edges on both relations with the cached CSRs merged
            (gnnrec_csr_add_edges: the batch's CSR spliced into the old one);
  in-place  the same call with the cached CSRs rebuilt instead (what add_edges does above
            graph.ADD_EDGES_REBUILD_SHARE): gnnrec_csr_build of the whole COO;
  parent    what a caller had before add_edges: concatenate the COO and the edge field, build
            a new HeteroGraph, in_csr on both relations.

Batches of 1,000 edges, 1 % and 100 % of E.  Median of `--runs` runs of each, alternating, a
device synchronisation around every run (and a garbage collection before it, so every run
reuses the allocator's cached blocks); the three results are compared bit for bit first.  One
relation through ops.csr_add_edges alone is reported as GB/s of algorithmic traffic.  One JSON
line per batch size on stdout; --md writes the table.

    python tools/bench_add_edges.py [--edges 50000000] [--runs 5] [--md profiles/add_edges_ab.md]
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

from gnnrec import graph as graph_mod  # noqa: E402
from gnnrec import ops  # noqa: E402
from gnnrec.graph import HeteroGraph  # noqa: E402

BUYS, BOUGHT = ("user", "buys", "item"), ("item", "bought-by", "user")


def timed(fn):
    # a dropped HeteroGraph is freed by the cycle collector (its accessors refer back to it):
    # collect before the run, so its tensors return to the caching allocator and the run
    # measures neither hipMalloc of fresh blocks nor a collection
    gc.collect()
    gc.disable()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    gc.enable()
    return dt, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=50_000_000)
    ap.add_argument("--batches", type=str, default="1000,0.01,1.0",
                    help="edge counts (integers) or shares of --edges (floats)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--md", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nodes = {"user": a.users, "item": a.items}
    E = a.edges
    u, i = ops.synth_edges(11, 0, E, a.users, a.items, dev)
    u, i = u.long(), i.long()
    g = HeteroGraph({BUYS: (u, i), BOUGHT: (i, u)}, nodes, device=dev)
    g.edges["buys"].data["recency"] = torch.randint(1, 30, (E,), device=dev)
    for ce in (BUYS, BOUGHT):
        g.in_csr(ce)
    sizes = [int(float(b) * E) if "." in b else int(b) for b in a.batches.split(",")]
    med = statistics.median
    rows = []
    for n in sizes:
        nu, ni = ops.synth_edges(12, 0, n, a.users, a.items, dev)
        nu, ni = nu.long(), ni.long()
        rec = torch.randint(1, 30, (n,), device=dev)

        def add(share):
            def run():
                keep = graph_mod.ADD_EDGES_REBUILD_SHARE
                graph_mod.ADD_EDGES_REBUILD_SHARE = share
                try:
                    t = g.clone()
                    t.add_edges(nu, ni, {"recency": rec}, etype=BUYS)
                    t.add_edges(ni, nu, etype=BOUGHT)
                finally:
                    graph_mod.ADD_EDGES_REBUILD_SHARE = keep
                return t
            return run

        def parent():
            s, d = g.all_edges(etype=BUYS)
            s, d = torch.cat([s, nu]), torch.cat([d, ni])
            t = HeteroGraph({BUYS: (s, d), BOUGHT: (d, s)}, nodes, device=dev)
            t.edges["buys"].data["recency"] = torch.cat([g.edges["buys"].data["recency"], rec])
            for ce in (BUYS, BOUGHT):
                t.in_csr(ce)
            return t

        paths = {"merge": add(float("inf")), "in_place_rebuild": add(-1.0), "parent": parent}
        outs = {k: timed(fn)[1] for k, fn in paths.items()}  # warm-up and the equality check
        same = True
        for k in ("in_place_rebuild", "parent"):
            for ce in (BUYS, BOUGHT):
                same &= all(torch.equal(x, y) for x, y in
                            zip(outs["merge"].all_edges(etype=ce), outs[k].all_edges(etype=ce)))
                same &= all(torch.equal(x, y) for x, y in
                            zip(outs["merge"].in_csr(ce), outs[k].in_csr(ce)))
            same &= torch.equal(outs["merge"].edges["buys"].data["recency"],
                                outs[k].edges["buys"].data["recency"])
        del outs
        times = {k: [] for k in paths}
        for _ in range(a.runs):
            for k, fn in paths.items():
                times[k].append(timed(fn)[0])
        # one relation alone: the merge and the rebuild of the concatenated COO
        csr = g.in_csr(BUYS)
        s, d = g.all_edges(etype=BUYS)
        s2, d2 = torch.cat([s, nu]), torch.cat([d, ni])
        tk = [timed(lambda: ops.csr_add_edges(csr, nu, ni, a.users, a.items))[0]
              for _ in range(a.runs + 1)][1:]
        tb = [timed(lambda: ops.csr_build(s2, d2, a.items))[0] for _ in range(a.runs + 1)][1:]
        del s2, d2
        # old slot: indices + eids read and written, 24 B; batch edge: 16 read, 16 clamped copy
        # written and read again by its build (32), its CSR 12 written + 12 read, P 4 written +
        # 4 read + the gathers 16, 12 written: 108 B; indptr 24 B per row
        algo = 24 * E + 108 * n + 24 * (a.items + 1)
        row = {"graph": {"users": a.users, "items": a.items, "edges_per_direction": E},
               "batch": n, "bitwise_equal": bool(same),
               **{f"{k}_ms": {"median": round(med(v), 3), "min": round(min(v), 3),
                              "max": round(max(v), 3), "runs": [round(x, 3) for x in v]}
                  for k, v in times.items()},
               "merge_beats_in_place_rebuild_in_every_run":
                   max(times["merge"]) < min(times["in_place_rebuild"]),
               "merge_beats_parent_in_every_run": max(times["merge"]) < min(times["parent"]),
               "kernel_one_relation_ms": {"median": round(med(tk), 3),
                                          "runs": [round(x, 3) for x in tk]},
               "csr_build_one_relation_ms": {"median": round(med(tb), 3),
                                             "runs": [round(x, 3) for x in tb]},
               "kernel_beats_csr_build_in_every_run": max(tk) < min(tb),
               "kernel_algorithmic_GBps": round(algo / med(tk) / 1e6, 1),
               "device": torch.cuda.get_device_name(0)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.md:
        def rng(r, k):
            x = r[k]
            return f"{x['median']:.2f} ({x['min']:.2f}–{x['max']:.2f})"
        with open(a.md, "a") as f:
            f.write(f"\n{E:,} edges per direction, {a.users:,} users x {a.items:,} items, "
                    f"{rows[0]['device']}; ms, median (min–max) of {a.runs}\n\n")
            f.write("| batch | add_edges, merge | add_edges, rebuild | parent's rebuild | "
                    "csr_add_edges alone | csr_build alone | merge GB/s | bitwise equal |\n")
            f.write("|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                k, b = r["kernel_one_relation_ms"], r["csr_build_one_relation_ms"]
                f.write(f"| {r['batch']:,} | {rng(r, 'merge_ms')} | {rng(r, 'in_place_rebuild_ms')}"
                        f" | {rng(r, 'parent_ms')} | {k['median']:.2f} ({min(k['runs']):.2f}–"
                        f"{max(k['runs']):.2f}) | {b['median']:.2f} ({min(b['runs']):.2f}–"
                        f"{max(b['runs']):.2f}) | {r['kernel_algorithmic_GBps']:.0f} | "
                        f"{r['bitwise_equal']} |\n")


if __name__ == "__main__":
    main()
