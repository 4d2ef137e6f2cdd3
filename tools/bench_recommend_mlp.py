"""Many-user top-k for the MLP head (gnnrec.recs.recommend(head=...)) against get_recs(pred='nn'),
the path it stands beside, C4 item count, random normal tables, a PredictingLayer under
torch.manual_seed(0).  HIP events, warm-up, medians of alternating runs in one process.

    python tools/bench_recommend_mlp.py [--parent-pkg DIR] [--out profiles/recommend_mlp_ab.json]

1. one batch: 1024 users x 1M items, d = 128, k = 10, 50 bought items per user — the new path
   end to end and stage by stage (Q GEMM, P GEMM, sample pass, filter pass, ranking), and the
   grouped edge-MLP kernel at the C3 shape (1024 x 2500) for its share of the fp32 MFMA peak
   on the same machine;
2. per user count (1024 and 65536): recommend(head=...) end to end, get_recs(pred='nn') of
   this tree, and — with --parent-pkg, the gnn-recsys_amd directory of a checkout of the
   parent commit with its libraries built — the parent's get_recs(pred='nn') on the same
   seeded inputs.  Each get_recs is timed in a child process that imports its package
   (--baseline is the child's mode).  The lists of the three are compared.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PEAK_FP32_MFMA = 157.3e12        # MI355X fp32 MFMA peak, FLOP/s
MFMA_FLOP_PER_PAIR = 2 * 128 * 32  # the 128 x 32 layer; what the share of peak counts


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--users", default="1024,65536")
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--bought", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline", action="store_true", help="child mode: time get_recs only")
    ap.add_argument("--pkg", default=os.path.join(HERE, "..", "gnn-recsys_amd"))
    ap.add_argument("--lists", default=None, help="child mode: save the first 1024 lists here")
    return ap.parse_args()


a = parse()
sys.path.insert(0, os.path.abspath(a.pkg))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gnnrec import ops  # noqa: E402
from gnnrec.nn import PredictingLayer  # noqa: E402
from gnnrec.recs import get_recs, topk_rows  # noqa: E402


def inputs(n_u):
    """Seeded tables, exclusion CSR and head: the same in every process."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    h_item = torch.randn(a.items, a.d, device=dev, generator=g)
    h_user = torch.randn(n_u, a.d, device=dev, generator=g)
    ex_ptr = torch.arange(n_u + 1, device=dev) * a.bought
    ex_idx = torch.randint(0, a.items, (n_u * a.bought,), device=dev, generator=g,
                           dtype=torch.int32)
    torch.manual_seed(0)
    pl = PredictingLayer(a.d).to(dev).eval()
    return h_user, h_item, ex_ptr, ex_idx, pl


def model_of(pl):
    model = type("M", (), {})()
    model.pred_fn = type("P", (), {})()
    model.pred_fn.layer_nn = pl
    return model


def time_get_recs(n_u):
    """get_recs(pred='nn') of the imported package over n_u users: host dict in, host lists
    out, one warm-up batch first; the median of three runs up to 8192 users, one run
    above.  -> (seconds, every run's seconds, lists [min(n_u, 1024), k])."""
    h_user, h_item, ex_ptr, ex_idx, pl = inputs(n_u)
    exi = ex_idx.cpu().numpy().reshape(n_u, a.bought)
    bought = {u: exi[u].tolist() for u in range(n_u)}
    h = {"user": h_user, "item": h_item}
    with torch.no_grad():
        get_recs(None, h, model_of(pl), a.d, a.k, list(range(64)), bought, pred="nn")
        ts = []
        for _ in range(3 if n_u <= 8192 else 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            recs = get_recs(None, h, model_of(pl), a.d, a.k, list(range(n_u)), bought, pred="nn")
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
    return statistics.median(ts), ts, np.stack([recs[u] for u in range(min(n_u, 1024))])


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


def one_batch(res):
    from gnnrec.recs import _MlpHead, recommend
    B, k = 1024, a.k
    h_user, h_item, ex_ptr, ex_idx, pl = inputs(B)
    dev = h_item.device
    rows = torch.arange(B, device=dev)
    d = a.d
    W1 = pl.hidden_1.weight
    mlp = _MlpHead(pl, h_user, h_item)
    m = min(65536, a.items)
    st = {"P": mlp.P(rows)}

    def q_gemm():
        ops.gemm(h_item, W1[:, d:])

    def p_gemm():
        st["P"] = mlp.P(rows)

    def sample():
        s = mlp.store(st["P"], m)
        ops.mask_excluded(s, rows, ex_ptr, ex_idx)
        st["tau"] = topk_rows(s, k)[0][:, k - 1].contiguous()

    def filt():
        st["counts"] = torch.zeros(B, dtype=torch.int32, device=dev)
        st["cand"] = torch.empty((B, 1024), dtype=torch.int32, device=dev)
        st["cand_sc"] = torch.empty((B, 1024), dtype=torch.float32, device=dev)
        mlp.filter(st["P"], st["tau"], st["counts"], st["cand"], st["cand_sc"])

    def rank():
        ops.topk_scored_candidates(st["counts"], st["cand"], st["cand_sc"], k, rows, ex_ptr, ex_idx)

    def call():
        recommend(h_user, h_item, k, rows, (ex_ptr, ex_idx), batch_size=B, head=pl)

    # the grouped edge-MLP kernel at C3: 1024 sources x 2500 negatives over 100k items
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    K3, n3 = 2500, 100_000
    dst3 = torch.randint(0, n3, (B * K3,), device=dev, generator=g)
    Q3 = mlp.Q[:n3]

    def grouped_c3():
        ops.edge_mlp_grouped(rows, None, K3, dst3, st["P"], Q3, *mlp.tail)

    fns = {"Q GEMM (item half of hidden_1, once per call)": q_gemm,
           "P GEMM (user half of hidden_1, per batch)": p_gemm,
           "sample pass (dense store of the prefix, mask, top-k)": sample,
           "filter pass (dense MLP over all items)": filt,
           "ranking (scored candidates)": rank,
           "recommend(head=...) end to end, Q GEMM and readback included": call,
           "edge_mlp_grouped at C3 (1024 x 2500)": grouped_c3}
    timed(fns, 2)  # warm-up
    one = timed(fns, a.reps)
    f = one["filter pass (dense MLP over all items)"]
    c3 = one["edge_mlp_grouped at C3 (1024 x 2500)"]
    flop = MFMA_FLOP_PER_PAIR * float(B) * a.items
    flop3 = MFMA_FLOP_PER_PAIR * float(B) * K3
    share = lambda fl, ms: fl / (ms * 1e-3) / PEAK_FP32_MFMA  # noqa: E731
    one["filter pass share of the fp32 MFMA peak (median; slowest .. fastest run)"] = [
        share(flop, f["ms"]), share(flop, f["max_ms"]), share(flop, f["min_ms"])]
    one["edge_mlp_grouped at C3 share of the fp32 MFMA peak (median; slowest .. fastest run)"] = [
        share(flop3, c3["ms"]), share(flop3, c3["max_ms"]), share(flop3, c3["min_ms"])]
    one["filter pass TFLOP/s (128 x 32 layer only)"] = flop / (f["ms"] * 1e-3) / 1e12
    cnt = st["counts"].cpu().numpy()
    one["candidates (sample 65536, k %d)" % k] = {"mean": float(cnt.mean()), "max": int(cnt.max())}
    res["one batch of 1024 users"] = one


def many_users(res, n_u, child_times):
    from gnnrec.recs import recommend
    h_user, h_item, ex_ptr, ex_idx, pl = inputs(n_u)
    out = {}
    for bs in sorted({min(n_u, 1024), min(n_u, 8192)}):
        recommend(h_user[:bs], h_item, a.k, None, (ex_ptr[:bs + 1], ex_idx), batch_size=bs, head=pl)
        ts = []
        for _ in range(3 if n_u <= 8192 else 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            idx, vals, stats = recommend(h_user, h_item, a.k, None, (ex_ptr, ex_idx),
                                         batch_size=bs, return_stats=True, head=pl)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        dt = statistics.median(ts)
        out[f"recommend(head=...) batch_size {bs}"] = {
            "s": dt, "runs_s": ts, "users_per_s": n_u / dt, "stats": stats}
    got = idx[:1024].cpu().numpy()
    for who, key in (("this tree", "this"), ("parent commit", "parent")):
        p = child_times.get((key, n_u))
        if p is None:
            continue
        out[f"get_recs(pred='nn'), {who} (host dict in, host lists out)"] = {
            "s": p["s"], "runs_s": p["runs_s"], "users_per_s": n_u / p["s"]}
        out[f"rows whose list differs from get_recs ({who})"] = int(
            (got != np.load(p["lists"])).any(1).sum())
    if ("parent", n_u) in child_times:
        best = min(v["s"] for kk, v in out.items() if kk.startswith("recommend("))
        out["speed-up over the parent's get_recs"] = child_times[("parent", n_u)]["s"] / best
    res[f"{n_u} users"] = out


def main():
    if a.baseline:
        n_u = int(a.users)
        dt, ts, lists = time_get_recs(n_u)
        if a.lists:
            np.save(a.lists, lists)
        print("BASELINE " + json.dumps({"users": n_u, "s": dt, "runs_s": ts}))
        return
    counts = [int(x) for x in a.users.split(",")]
    # get_recs of the parent and of this tree, each in a child process of its own (the same
    # conditions for both), before this process opens the device
    child_times = {}
    tmp = os.path.dirname(os.path.abspath(a.out)) if a.out else os.getcwd()
    pkgs = ([("parent", a.parent_pkg)] if a.parent_pkg else []) + [("this", a.pkg)]
    for n_u in counts:
        for key, pkg in pkgs:
            path = os.path.join(tmp, f"_{key}_lists_{n_u}.npy")
            cmd = [sys.executable, os.path.abspath(__file__), "--baseline", "--pkg", pkg,
                   "--users", str(n_u), "--items", str(a.items), "--d", str(a.d), "--k", str(a.k),
                   "--bought", str(a.bought), "--lists", path]
            p = subprocess.run(cmd, capture_output=True, text=True, check=True)
            line = next(ln for ln in p.stdout.splitlines() if ln.startswith("BASELINE "))
            child_times[(key, n_u)] = dict(json.loads(line[len("BASELINE "):]), lists=path)
            print(key, line, flush=True)
    res = {"shape": {"users": counts, "items": a.items, "d": a.d, "k": a.k, "bought": a.bought,
                     "device": torch.cuda.get_device_name(0)}}
    one_batch(res)
    print(json.dumps(res["one batch of 1024 users"], indent=1), flush=True)
    for n_u in counts:
        many_users(res, n_u, child_times)
        print(json.dumps(res[f"{n_u} users"], indent=1), flush=True)
    for p in child_times.values():
        os.remove(p["lists"])
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
