#!/usr/bin/env python3
"""Output bits of the fused aggregate+project kernels (csrc/spmm_project.hip,
csrc/spmm_pair_mfma.hip) over a fixed case list.

The four kernels run on inputs from seeded CPU generators (those of tools/spmm_bits.py where
they fit), each through its explicit variant so no dispatch heuristic picks another, and the
sha256 of each output's bytes is written as {case name: digest}:

    python tools/fused_bits.py --out tests/fused_bits_parent.json

tests/test_gpu_fused_bits.py asserts the digests of a build against the committed file.
`cases()` is the list: (group, name, thunk returning a tensor).  All cases d = 128, a source
table of 300 rows; the small CSR has 70 rows of 0 to 129 edges (both sides of the 64-edge
lockstep limit in one group of four) and one row of 700.

Which case reaches which of the 26 kernel instantiations (R = sum / mean / max, W = u / w):

    spmm_project_kernel<R, W>              single/valu_{R}_{W}                      (6)
    spmm_project_mfma_kernel<R, W, PRE=0>  single/mfma_{R}_{W}                      (6)
    spmm_project_mfma_kernel<R, W, PRE=1>  pre/mfma_{sum,mean}_{W}                  (4)
    spmm_project2_pipe_kernel<WA, WB, 0>   project2/{combine}_{uu,wu,uw,ww}         (4)
    spmm_project2_pipe_kernel<0, 0, 1 | 2> project2/stream_a, project2/stream_b     (2)
    spmm_pair_mfma_kernel<WA, WB>          pair/{combine}_{uu,wu,uw,ww}             (4)

The other cases walk the run-time paths of those kernels: epilogues, accumulate modes (the
attention modes as a first / middle / last sequence over one output and state), out_div, the
two biases, a strided output, ragged row counts (n mod 2, 4 and 32) and the row queue.
"""
import argparse
import functools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402

import spmm_bits as sb  # noqa: E402  (also puts the package on sys.path)

D = 128
ROW_700 = 700
RAGGED = (1, 31, 33, 65, 257)
REDUCES = ("sum", "mean", "max")
COMBINES = ("add", "mean", "max", "attention")
WEIGHTS = ((False, False), (True, False), (False, True), (True, True))


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(None)
def small_csr(seed=5, n=70):
    """n rows (70: the listed degrees seven times over, from the largest down) shuffled by
    seed; with 70 rows, one of 700 edges."""
    g = torch.Generator().manual_seed(seed)
    reps = (n + len(sb.DEGREES) - 1) // len(sb.DEGREES)
    deg = torch.tensor((sb.DEGREES[::-1] * reps)[:n], dtype=torch.int64)
    deg = deg[torch.randperm(n, generator=g)]
    if n == 70:
        deg[17] = ROW_700
    return sb._csr_of(deg, seed + 100)


@functools.lru_cache(None)
def thin_csr(seed=31):
    """70 rows of 0 to 4 edges: under half the small CSR's edges (the GNNREC_SRC_STREAM forms)."""
    deg = torch.randint(0, 5, (70,), generator=torch.Generator().manual_seed(seed))
    return sb._csr_of(deg, seed + 100)


@functools.lru_cache(None)
def h_self(n):
    return _randn((n, D), 3000 + n).cuda()


@functools.lru_cache(None)
def weight(seed):
    return (_randn((D, D), 4000 + seed) / 8).cuda()


@functools.lru_cache(None)
def vec(seed):
    return _randn((D,), 5000 + seed).cuda()


def _nnz_tagged(ip, ix):
    ip = ip.clone()
    ip._gnnrec_nnz = ix.numel()
    return ip


def _single(csr, variant, reduce="mean", weighted=False, relu=True, l2=False, accum="store",
            out_div=0.0, biases=False, pad=0, pre=False):
    from gnnrec import ops
    ip, ix, ew = csr()
    n = ip.numel() - 1
    wide = None
    if accum == "store":
        wide = torch.full((n, D + pad), 3.0, device="cuda")
        out = wide[:, :D]
    else:
        out = sb.base_out(n, D).clone()
    res = ops.spmm_project(ip, ix, sb.table(D), h_self(n), weight(0), None if pre else weight(1),
                           reduce, ew if weighted else None, relu=relu, l2norm=l2, accum=accum,
                           out_div=out_div, out=out, bias=vec(0) if biases else None,
                           bias_nonempty=vec(1) if biases else None, variant=variant)
    return res if wide is None else wide


def _attention(variant):
    """Three relations into one output: attn_first, attn, attn_last over one state."""
    from gnnrec import ops
    out = torch.empty(70, D, device="cuda")
    state = torch.empty(70, 2, device="cuda")
    for k, accum in enumerate(("attn_first", "attn", "attn_last")):
        ip, ix, ew = small_csr(seed=5 + 8 * k)
        ops.spmm_project(ip, ix, sb.table(D, seed=k), h_self(70), weight(2 * k), weight(2 * k + 1),
                         REDUCES[k], ew if k == 1 else None, relu=True, l2norm=True, accum=accum,
                         out=out, attn_vec=vec(2), attn_state=state, variant=variant)
    return torch.cat([out.flatten(), state.flatten()])


def _two_kw(combine):
    kw = dict(relu=True, l2norm=True, combine="add" if combine == "mean" else combine)
    if combine == "mean":
        kw["out_div"] = 2.0
    if combine == "attention":
        kw["attn_vec"] = vec(2)
    return kw


def _project2(csr_a, csr_b, combine, wa=False, wb=False, stream=False):
    from gnnrec import ops
    ip_a, ix_a, ew_a = csr_a()
    ip_b, ix_b, ew_b = csr_b()
    if stream:  # the edge counts known on the host: the thinner relation's rows stream
        ip_a, ip_b = _nnz_tagged(ip_a, ix_a), _nnz_tagged(ip_b, ix_b)
    n = ip_a.numel() - 1
    return ops.spmm_project2((ip_a, ix_a, sb.table(D, seed=1), "mean", ew_a if wa else None, vec(3)),
                             (ip_b, ix_b, sb.table(D, seed=2), "sum", ew_b if wb else None, vec(4)),
                             h_self(n), weight(0), weight(2), vec(0), vec(1), **_two_kw(combine))


def _pair(csr_a, csr_b, combine, wa=False, wb=False):
    from gnnrec import ops
    ip_a, ix_a, ew_a = csr_a()
    ip_b, ix_b, ew_b = csr_b()
    n = ip_a.numel() - 1
    return ops.spmm_pair((ip_a, ix_a, "mean", ew_a if wa else None, vec(3)),
                         (ip_b, ix_b, "sum", ew_b if wb else None, vec(4)), sb.table(D),
                         h_self(n), weight(0), weight(1), weight(2), weight(3), vec(0), vec(1),
                         **_two_kw(combine))


def cases():
    """[(group, name, thunk)]: the thunk runs the case and returns its output tensor."""
    P = functools.partial
    c = []

    def add(group, name, fn):
        c.append((group, f"{group}/{name}", fn))

    other = P(small_csr, 21)
    for v in ("valu", "mfma"):
        for reduce in REDUCES:
            for w in (False, True):
                add("single", f"{v}_{reduce}_{'w' if w else 'u'}", P(_single, small_csr, v, reduce, w))
        add("single", f"{v}_epi_none", P(_single, small_csr, v, relu=False))
        add("single", f"{v}_epi_relu_l2", P(_single, small_csr, v, l2=True))
        add("single", f"{v}_accum_add", P(_single, small_csr, v, accum="add"))
        add("single", f"{v}_accum_max", P(_single, small_csr, v, "max", accum="max"))
        add("single", f"{v}_attention", P(_attention, v))
        add("single", f"{v}_out_div", P(_single, small_csr, v, accum="add", out_div=2.0))
        add("single", f"{v}_biases", P(_single, small_csr, v, "sum", True, l2=True, biases=True))
        add("single", f"{v}_strided_out", P(_single, small_csr, v, pad=12))
        for n in RAGGED:
            add("ragged", f"{v}_n{n}", P(_single, P(small_csr, 40 + n, n), v, l2=True, biases=True))
    for reduce in ("sum", "mean"):
        for w in (False, True):
            add("pre", f"mfma_{reduce}_{'w' if w else 'u'}",
                P(_single, small_csr, "mfma", reduce, w, l2=True, biases=True, pre=True))
    for n in RAGGED:
        a, b = P(small_csr, 40 + n, n), P(small_csr, 80 + n, n)
        add("ragged", f"project2_n{n}", P(_project2, a, b, "attention"))
        add("ragged", f"pair_n{n}", P(_pair, a, b, "attention"))
    for combine in COMBINES:
        for wa, wb in WEIGHTS:
            tag = f"{combine}_{'w' if wa else 'u'}{'w' if wb else 'u'}"
            add("project2", tag, P(_project2, small_csr, other, combine, wa, wb))
            add("pair", tag, P(_pair, small_csr, other, combine, wa, wb))
    add("project2", "stream_a", P(_project2, thin_csr, small_csr, "add", stream=True))
    add("project2", "stream_b", P(_project2, small_csr, thin_csr, "add", stream=True))
    q, q2 = sb.queued_csr, P(sb.queued_csr, seed=21)
    add("queued", "valu", lambda: sb._queued(P(_single, q, "valu", l2=True)))
    add("queued", "mfma", lambda: sb._queued(P(_single, q, "mfma", l2=True)))
    add("queued", "project2", lambda: sb._queued(P(_project2, q, q2, "add")))
    add("queued", "pair", lambda: sb._queued(P(_pair, q, q2, "add")))
    return c


def run(groups=None):
    """{case name: sha256 of the output bytes} of every case (of the given groups)."""
    from gnnrec import ops
    old = ops.get_concurrency()
    ops.set_concurrency(0, False)  # the static schedule, but in the queued cases
    try:
        return {name: sb.digest(fn()) for group, name, fn in cases()
                if groups is None or group in groups}
    finally:
        ops.set_concurrency(*old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--groups", nargs="+", default=None)
    args = ap.parse_args()
    res = run(args.groups)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(res)} cases -> {args.out}")


if __name__ == "__main__":
    main()
