#!/usr/bin/env python3
"""The C2 training step of bench.py --full's `minibatch` section with ConvLayer dropout on.

The same graph, model, loader, loss and optimizer as bench.py's minibatch_step /
captured_step (1M users x 100k items x 50M edges per direction, 2 SAGE 'mean' layers d = 64 +
NodeEmbedding, fanout [10, 10], 1024 positives x K uniform negatives, cosine head, max-margin
loss, fused Adam), at a given dropout, eager (sampling thread on) and captured, several runs of
each row in one process, interleaved so that drift hits every variant alike:

    fused   dropout inside the fused training nodes (csrc/dropout.hip), the default
    torch   GNNREC_TRAIN_DROPOUT=torch: nn.Dropout on the whole source tables and the
            per-relation autograd path (what a build without the fused dropout runs)
    p0      dropout = 0 beside them: what dropout itself costs

    python tools/bench_dropout_step.py --dropout 0.5 --runs 3
    python tools/bench_dropout_step.py --package OTHER/gnn-recsys_amd --variants torch

--package: import gnnrec from another checkout (its built libraries beside it), to time a
commit that has no fused dropout with this same script.  --gather-only: time the forward
gather alone, plain and with the mask, at the C2 first-block shape (bytes/s).
One JSON line per row on stdout, then one summary line (median and range per row).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--K", type=int, nargs="+", default=[10, 2500])
    ap.add_argument("--modes", nargs="+", default=["eager", "captured"],
                    choices=["eager", "captured"])
    ap.add_argument("--variants", nargs="+", default=["fused", "torch", "p0"],
                    choices=["fused", "torch", "p0"])
    ap.add_argument("--steps", type=int, default=0, help="0: 100 at K <= 100, else 40")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--package", default=os.path.join(ROOT, "gnn-recsys_amd"))
    ap.add_argument("--gather-only", action="store_true")
    return ap.parse_args(argv)


def model_of(g, dev, p):
    import torch
    from gnnrec import nn as gnn
    torch.manual_seed(0)
    return gnn.ConvModel(g, 3, {"user": 64, "item": 64, "hidden": 64, "out": 64}, True, p,
                         "mean", "cos", "sum", True).to(dev)


def loader_of(g, K, nw, static=False, caps="provable"):
    import torch
    from gnnrec.sampling import EdgeDataLoader, MultiLayerNeighborSampler, negative_sampler
    buys = ("user", "buys", "item")
    kw = dict(static_shapes=True, static_caps=caps) if static else {}
    return EdgeDataLoader(g, {buys: torch.arange(g.num_edges(buys))},
                          MultiLayerNeighborSampler([10, 10]), exclude="reverse_types",
                          reverse_etypes={"buys": "bought-by", "bought-by": "buys"},
                          negative_sampler=negative_sampler.Uniform(K), batch_size=1024,
                          shuffle=True, num_workers=nw, **kw)


def loss_of(K):
    from gnnrec import nn as gnn

    def f(m, batch):
        _, pos_g, neg_g, blocks = batch
        _, ps, ns = m(blocks, blocks[0].srcdata["features"], pos_g, neg_g, True)
        return gnn.max_margin_loss(ps, ns, 0.266, K, True, pos_g.edata["recency"])
    return f


def eager_row(g, dev, K, p, steps, warmup):
    import torch
    model = model_of(g, dev, p)
    opt = torch.optim.Adam(model.parameters(), lr=0.005, fused=True)
    it = iter(loader_of(g, K, 2))
    loss_fn = loss_of(K)

    def step():
        loss = loss_fn(model, next(it))
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    return {"ms_per_step": round(ms, 3), "loss": float(loss.detach())}


def captured_row(g, dev, K, p, steps, warmup):
    import torch
    from gnnrec.capture import CapturedTrainStep
    from gnnrec.sampling import EdgeDataLoader
    caps = "auto" if K > 100 else "provable"
    model = model_of(g, dev, p)
    opt = torch.optim.Adam(model.parameters(), lr=0.005, fused=True)
    model.train_fold = "1"  # as bench.py's captured step (no fold happens under dropout)
    step = CapturedTrainStep(model, opt, loss_of(K), warmup=2)
    el = loader_of(g, K, 2, static=True, caps=caps)
    if p == 0:
        el.sampler.first_transposes_below = 0  # what the fold sets (bench.py captured_step)
    it = iter(el)
    W = max(warmup, 3) + (EdgeDataLoader.STATIC_LEARN if caps == "auto" else 0)
    for _ in range(W):
        step(next(it))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step(next(it))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    res = {"ms_per_step": round(ms, 3), "loss": float(loss.detach()), "replays": step.replays,
           "eager_steps": step.eager_steps, "captures": step.captures}
    del it, el
    if step.graph is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            step.graph.replay()
        e1.record()
        e1.synchronize()
        res["gpu_ms_per_replay"] = round(e0.elapsed_time(e1) / 20, 3)
    return res


def gather_only(g, dev, p, reps=50):
    """The forward gather of the first C2 block (K = 10), plain and with the mask inside:
    microseconds and achieved bytes/s (edges x 256-B rows read + rows written + indices)."""
    import torch
    from gnnrec import ops
    batch = next(iter(loader_of(g, 10, 0)))
    block = batch[-1][0]
    out = {}
    for ce in block.canonical_etypes:
        rg = block.rel_graph(ce)
        ip, ix = rg.indptr, rg.indices
        nnz = ops._nnz(ip)
        X = torch.randn(block.number_of_src_nodes(ce[0]), 64, device=dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        keys = ops.dropout_keys(1, counter, 2)
        dst = torch.empty(ip.numel() - 1, 64, device=dev)

        def timed(fn):
            for _ in range(5):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3
        us_plain = timed(lambda: ops.spmm(ip, ix, X, "mean", out=dst, split=None))
        us_drop = timed(lambda: ops.spmm_dropout(ip, ix, X, "mean", keys, 0, p, "src", out=dst,
                                                 nnz=0))
        nbytes = nnz * (256 + 4) + (ip.numel() - 1) * (256 + 8)
        out["/".join(ce)] = {"rows": ip.numel() - 1, "edges": nnz, "src_rows": X.shape[0],
                             "plain_us": round(us_plain, 1), "dropout_us": round(us_drop, 1),
                             "plain_GBs": round(nbytes / us_plain / 1e3, 1),
                             "dropout_GBs": round(nbytes / us_drop / 1e3, 1)}
    return out


def main():
    args = parse()
    sys.path.insert(0, args.package)
    import torch
    from gnnrec.synth import minibatch_graph
    dev = torch.device("cuda:0")
    g = minibatch_graph(64, dev)
    if args.gather_only:
        print(json.dumps({"gather": gather_only(g, dev, args.dropout)}), flush=True)
        return
    rows = {}
    for K in args.K:
        steps = args.steps or (100 if K <= 100 else 40)
        for mode in args.modes:
            for run in range(args.runs):
                for variant in args.variants:  # interleaved: drift hits every variant alike
                    os.environ["GNNREC_TRAIN_DROPOUT"] = "torch" if variant == "torch" else "fused"
                    p = 0.0 if variant == "p0" else args.dropout
                    fn = eager_row if mode == "eager" else captured_row
                    res = fn(g, dev, K, p, steps, args.warmup)
                    res.update(K=K, mode=mode, variant=variant, run=run, dropout=p, steps=steps)
                    print(json.dumps(res), flush=True)
                    rows.setdefault((K, mode, variant), []).append(res["ms_per_step"])
    summary = {f"K{K}_{mode}_{variant}": {"median_ms": round(statistics.median(v), 3),
                                          "min_ms": min(v), "max_ms": max(v), "runs": len(v)}
               for (K, mode, variant), v in rows.items()}
    print(json.dumps({"summary": summary, "package": os.path.abspath(args.package),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
