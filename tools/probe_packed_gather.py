"""Does gathering 384-B packed rows beat gathering the 512-B dense rows of a ReLU-sparse table?

Gather-only (spmm 'sum', d = 128) on the two shapes of the C4 pass's second layer:
  fused   1M source rows, 10M destination rows of degree 50 (500M edges)
  tile    1.25M source rows (one of 8 source tiles), 1M destination rows of degree 55..70
with the source table half zeros.  Each shape is run dense, packed, packed with a share f of
the rows flagged `dense` (their escape to the dense table; f = 1 prices it, the others place
the packed_ok fraction) and through the packed kernel's dense fallback (packed_ok = 0).
Every packed result is compared bitwise with the dense one.

    python tools/probe_packed_gather.py [--scale 1.0] [--out result.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnn-recsys_amd"))
import torch  # noqa: E402

from gnnrec import ops  # noqa: E402

D = 128


def t(fn, reps=5, rounds=3):
    """ms per call: `rounds` timings of `reps` back-to-back calls each."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / reps)
    return sorted(out)


def table(n, dense_share, gen):
    """[n, 128], half zeros; a share of the rows fully non-zero (flagged `dense` when packed)."""
    x = torch.randn(n, D, device="cuda", generator=gen)
    x.masked_fill_(torch.rand(n, D, device="cuda", generator=gen) < 0.5, 0.0)
    if dense_share > 0:
        full = torch.rand(n, device="cuda", generator=gen) < dense_share
        x[full] = torch.rand(int(full.sum()), D, device="cuda", generator=gen) + 1.0
    return x


def shape(name, n_src, n_dst, deg_lo, deg_hi, gen, res, shares):
    dev = torch.device("cuda")
    deg = torch.randint(deg_lo, deg_hi + 1, (n_dst,), device=dev, generator=gen)
    ip = torch.zeros(n_dst + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=ip[1:])
    E = int(ip[-1])
    ix = torch.randint(0, n_src, (E,), device=dev, generator=gen, dtype=torch.int32)
    out_d = torch.empty(n_dst, D, device=dev)
    out_p = torch.empty(n_dst, D, device=dev)
    r = res[name] = {"n_src": n_src, "n_dst": n_dst, "edges": E}
    for share in shares:
        X = table(n_src, share, gen)
        P = ops.pack_rows(X, max_dense_frac=1.0)  # packed_ok stays 1: the escape is taken
        key = f"dense_share={share:g}"
        e = r[key] = {"dense_rows": int(P.status[1]), "packed_ok": int(P.status[0])}
        e["dense_ms"] = t(lambda: ops.spmm(ip, ix, X, "sum", out=out_d, split=None))
        e["packed_ms"] = t(lambda: ops.spmm_packed(ip, ix, P, "sum", out=out_p, split=None))
        e["bitwise"] = bool(torch.equal(out_d.view(torch.int32), out_p.view(torch.int32)))
        if share == 0:
            e["pack_ms"] = t(lambda: ops.pack_rows(X, into=P, max_dense_frac=1.0))
            P.status[0] = 0  # the fallback loop, forced
            out_p.zero_()
            e["fallback_ms"] = t(lambda: ops.spmm_packed(ip, ix, P, "sum", out=out_p, split=None))
            e["fallback_bitwise"] = bool(torch.equal(out_d.view(torch.int32),
                                                     out_p.view(torch.int32)))
        e["packed_over_dense"] = e["packed_ms"][1] / e["dense_ms"][1]
        print(json.dumps({name: {key: e}}), flush=True)
        del X, P
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrink both shapes (smoke runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    s = a.scale
    res = {"device": torch.cuda.get_device_name(0)}
    shares = (0.0, 1.0 / 64, 1.0 / 16, 0.25, 1.0)
    shape("fused", int(1_000_000 * s), int(10_000_000 * s), 50, 50, gen, res, shares)
    shape("tile", int(1_250_000 * s), int(1_000_000 * s), 55, 70, gen, res, shares)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
