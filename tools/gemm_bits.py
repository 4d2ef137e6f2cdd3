#!/usr/bin/env python3
"""Output bits of the fp32 GEMM (csrc/gemm.hip) over a fixed case list.

ops.gemm runs on inputs from seeded CPU generators and the sha256 of everything a call writes
(out, then row_norm / attn_state where the call has one) is written as {case name: digest}:

    python tools/gemm_bits.py --out tests/gemm_bits_parent.json

tests/test_gpu_gemm_bits.py asserts the digests of a build against the committed file.
`cases()` is the list: (group, name, thunk returning the written tensors).  `described()` is
the same list with each case as a `Case`: the CPU inputs and keyword arguments of its ops.gemm
calls, its M, N and pad, and which tensors it writes.  The thunk uploads and runs that
description (`run_case`); tests/gemm_reference.py computes from it, in fp64, what the case
must write (tests/test_gpu_gemm_reference.py).  Every case runs at
M = 1 (a partial wave), 129 (one row past a block) and 300 (three blocks, the last ragged);
the name ends in the M.  The groups are the kernels the dispatch of launch_gemm picks
(depth = K-tile depth of the LDS-DMA kernel, bn = output columns per block):

    d32_bn32    N <= 32, K multiples of 32: one to three tiles, (A1,W1)+(A2,W2) with both degree
                modes (degrees 0..7: dividing by 3, 5, 6, 7 and multiplying by the reciprocal
                round differently), the epilogues, accumulate modes, the attention sequence
                (first / middle / last over one output and state), out_div, a strided output,
                N = 20 (the column clamp)
    d32_bn256   128 < N <= 256 with the row norm or attention (what needs the whole row in one
                block): N = 256 and 200, row_norm, both degree modes
    d16_bn64    N <= 64 and N <= 128, K multiples of 16: one to five tiles (either side of the
    d16_bn128   three stages), the segment switch mid-pipeline (48 + 16), 128 + 128 with both
                degree modes, each compile-time epilogue FE = bias | relu << 1 | l2norm << 2 in
                {0, 1, 2, 3, 6, 7} at N == bn (6 and 7 also with row_norm), the run-time
                epilogue (sigmoid, accumulate, attention, bias_nonempty, out_div, a strided
                output, N = 40 / 100, and for bn128 N = 192: two column blocks)
    general     the register-staged kernel: K = 5, K = 34, an A1 that is not 16-B aligned
"""
import argparse
import dataclasses
import functools
import hashlib
import json
import os
import sys
from typing import List, Optional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PKG = os.path.join(ROOT, "gnn-recsys_amd")
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import torch  # noqa: E402

MS = (1, 129, 300)
GROUPS = ("d32_bn32", "d32_bn256", "d16_bn64", "d16_bn128", "general")
FE_FLAGS = {0: (False, False, False), 1: (True, False, False), 2: (False, True, False),
            3: (True, True, False), 6: (False, True, True), 7: (True, True, True)}


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(None)
def operand(m, k, seed):
    return _randn((m, k), 1000 * seed + 7 * m + k)


@functools.lru_cache(None)
def weight(n, k, seed):
    return _randn((n, k), 50000 + 1000 * seed + 7 * n + k) / 8


@functools.lru_cache(None)
def vec(n, seed):
    return _randn((n,), 90000 + 100 * seed + n)


@functools.lru_cache(None)
def degrees(m):
    return torch.randint(0, 8, (m,), generator=torch.Generator().manual_seed(300 + m),
                         dtype=torch.int32)


def base_out(m, n):
    return _randn((m, n), 2000 + m + n)


@dataclasses.dataclass
class Call:
    """One ops.gemm call of a case: its CPU inputs and keyword arguments.  A1 is columns
    [a1_shift, a1_shift + k1) of a1_table (a view of a wider table when the two differ)."""
    a1_table: torch.Tensor
    k1: int
    w1: torch.Tensor
    a1_shift: int = 0
    a2: Optional[torch.Tensor] = None
    w2: Optional[torch.Tensor] = None
    a2_deg: Optional[torch.Tensor] = None
    a2_mode: Optional[str] = None          # None | "div" | "zero"
    bias: Optional[torch.Tensor] = None
    bias_nonempty: Optional[torch.Tensor] = None
    attn_vec: Optional[torch.Tensor] = None
    relu: bool = False
    l2norm: bool = False
    sigmoid: bool = False
    accum: str = "store"
    out_div: float = 0.0

    @property
    def a1(self):
        return self.a1_table[:, self.a1_shift:self.a1_shift + self.k1]


@dataclasses.dataclass
class Case:
    """What a case runs: `calls` in order into one output, the [m, n] window at column `col`
    of the table `out_init` ([m + guard, col + n + pad]: `guard` rows the calls are not given).
    row_norm_init / attn_state_init: the initial row_norm [m + guard] / attn_state
    [m + guard, 2] where the calls have one.  `writes` names the tensors run_case returns."""
    m: int
    n: int
    calls: List[Call]
    out_init: torch.Tensor
    pad: int = 0
    col: int = 0
    guard: int = 0
    row_norm_init: Optional[torch.Tensor] = None
    attn_state_init: Optional[torch.Tensor] = None

    @property
    def writes(self):
        return ("out",) + (("row_norm",) if self.row_norm_init is not None else ()) + (
            ("attn_state",) if self.attn_state_init is not None else ())


_DEVICE = {}  # id(CPU tensor of a cached generator) -> (the tensor, its upload)


def _up(t):
    """The device copy of a generator's tensor, uploaded once (the generators cache their CPU
    tensors, so the id is stable)."""
    if t is None:
        return None
    hit = _DEVICE.get(id(t))
    if hit is None or hit[0] is not t:
        hit = _DEVICE[id(t)] = (t, t.cuda())
    return hit[1]


def run_case(case, after_call=None):
    """Run a case on the device -> the tensors it wrote, whole (guard rows and pad columns
    included), in the order of case.writes.  after_call(j, written) sees them after call j."""
    from gnnrec import _lib, ops
    m, n = case.m, case.n
    wide = case.out_init.cuda()
    whole = case.col == 0 and case.pad == 0
    out = wide[:m] if whole else wide[:m, case.col:case.col + n]
    written = [wide]
    row_norm = state = None
    if case.row_norm_init is not None:
        row_norm = case.row_norm_init.cuda()
        written.append(row_norm)
    if case.attn_state_init is not None:
        state = case.attn_state_init.cuda()
        written.append(state)
    for j, c in enumerate(case.calls):
        a1 = _up(c.a1_table)
        if c.a1_shift or c.k1 != c.a1_table.shape[1]:
            a1 = a1[:, c.a1_shift:c.a1_shift + c.k1]
        kw = {}
        if c.a2_deg is not None:
            kw["a2_deg"] = _up(c.a2_deg)
        if c.a2_mode is not None:
            kw["a2_mode"] = {"div": _lib.A2_DIV_DEG, "zero": _lib.A2_ZERO_DEG}[c.a2_mode]
        if row_norm is not None:
            kw["row_norm"] = row_norm[:m]
        if c.attn_vec is not None:
            kw["attn_vec"] = _up(c.attn_vec)
            kw["attn_state"] = state[:m]
        ops.gemm(a1, _up(c.w1), _up(c.a2), _up(c.w2), _up(c.bias), relu=c.relu, l2norm=c.l2norm,
                 sigmoid=c.sigmoid, accum=c.accum, out_div=c.out_div, out=out,
                 bias_nonempty=_up(c.bias_nonempty), **kw)
        if after_call is not None:
            after_call(j, written)
    return written


def _gemm(m, n, k1, k2=0, mode=None, bias=False, relu=False, l2=False, sigmoid=False,
          accum="store", out_div=0.0, pad=0, bias_ne=False, row_norm=False, a1_shift=0):
    """One ops.gemm call.  pad: the output is the first n columns of a [m, n + pad] table
    (returned whole).  a1_shift: A1 is a view `a1_shift` columns into a wider table."""
    call = Call(a1_table=operand(m, k1 + 4, 1) if a1_shift else operand(m, k1, 1), k1=k1,
                w1=weight(n, k1, 1), a1_shift=a1_shift, a2_mode=mode,
                bias=vec(n, 0) if bias else None, bias_nonempty=vec(n, 1) if bias_ne else None,
                relu=relu, l2norm=l2, sigmoid=sigmoid, accum=accum, out_div=out_div)
    if k2:
        call.a2, call.w2 = operand(m, k2, 2), weight(n, k2, 2)
    if mode is not None or bias_ne:
        call.a2_deg = degrees(m)
    if accum == "store":
        wide = torch.full((m, n + pad), 3.0)
    else:
        wide = base_out(m, n + pad)
    return Case(m=m, n=n, calls=[call], out_init=wide, pad=pad,
                row_norm_init=torch.full((m,), -1.0) if row_norm else None)


def _attention(m, n, k, l2=True):
    """Three relations into one output: attn_first, attn, attn_last over one state (the first
    call overwrites all of out and state, so their initial values never reach a result)."""
    calls = [Call(a1_table=operand(m, k, 3 + j), k1=k, w1=weight(n, k, 3 + j), bias=vec(n, 0),
                  relu=True, l2norm=l2, accum=accum, attn_vec=vec(n, 2))
             for j, accum in enumerate(("attn_first", "attn", "attn_last"))]
    return Case(m=m, n=n, calls=calls, out_init=torch.full((m, n), 3.0),
                attn_state_init=torch.full((m, 2), -1.0))


def _runtime_paths(add, n, k):
    """The run-time epilogue's paths at one (n, k)."""
    P = functools.partial
    add("sigmoid", P(_gemm, n=n, k1=k, bias=True, sigmoid=True))
    add("accum_add", P(_gemm, n=n, k1=k, relu=True, accum="add"))
    add("accum_max", P(_gemm, n=n, k1=k, accum="max"))
    add("attention", P(_attention, n=n, k=k))
    add("out_div", P(_gemm, n=n, k1=k, accum="add", out_div=2.0))
    add("strided_out", P(_gemm, n=n, k1=k, bias=True, relu=True, l2=True, pad=4))


def cases():
    """[(group, name, thunk)]: the thunk runs the case and returns the tensors it wrote."""
    return [(group, name, functools.partial(_run_described, describe))
            for group, name, describe in described()]


def _run_described(describe):
    return run_case(describe())


def described():
    """[(group, name, describe)] in the order of cases(): describe() returns the Case (CPU
    inputs, keyword arguments, sizes, what is written) that both the thunk of cases() and
    the fp64 reference of tests/gemm_reference.py run from."""
    P = functools.partial
    c = []

    def adder(group):
        def add(name, fn):
            for m in MS:
                c.append((group, f"{group}/{name}_m{m}", P(fn, m)))
        return add

    add = adder("d32_bn32")
    for n in (32, 20):
        for k in (32, 64, 96):
            add(f"n{n}_k{k}", P(_gemm, n=n, k1=k))
        for mode in ("div", "zero"):
            add(f"n{n}_k32+32_{mode}", P(_gemm, n=n, k1=32, k2=32, mode=mode))
        add(f"n{n}_bias_relu_l2", P(_gemm, n=n, k1=64, bias=True, relu=True, l2=True,
                                    row_norm=True))
    _runtime_paths(add, 32, 64)

    add = adder("d32_bn256")
    for n in (256, 200):
        add(f"n{n}_k32_l2", P(_gemm, n=n, k1=32, bias=True, relu=True, l2=True, row_norm=True))
        add(f"n{n}_attention", P(_attention, n=n, k=64, l2=False))
        for mode in ("div", "zero"):
            add(f"n{n}_k64+32_{mode}", P(_gemm, n=n, k1=64, k2=32, mode=mode, relu=True, l2=True))

    for bn, ragged in ((64, 40), (128, 100)):
        add = adder(f"d16_bn{bn}")
        for k in (16, 32, 48, 64, 80):
            add(f"k{k}", P(_gemm, n=bn, k1=k))
        add("k48+16", P(_gemm, n=bn, k1=48, k2=16))
        for mode in ("div", "zero"):
            add(f"k128+128_{mode}", P(_gemm, n=bn, k1=128, k2=128, mode=mode, relu=True, l2=True))
            add(f"k128+128_{mode}_sigmoid", P(_gemm, n=bn, k1=128, k2=128, mode=mode,
                                              sigmoid=True))
        for fe, (bias, relu, l2) in FE_FLAGS.items():
            add(f"fe{fe}", P(_gemm, n=bn, k1=48, k2=16, bias=bias, relu=relu, l2=l2))
            if l2:
                add(f"fe{fe}_row_norm", P(_gemm, n=bn, k1=48, k2=16, bias=bias, relu=relu, l2=l2,
                                          row_norm=True))
        _runtime_paths(add, bn, 48)
        add("bias_nonempty", P(_gemm, n=bn, k1=48, k2=16, mode="zero", bias=True, relu=True,
                               l2=True, bias_ne=True))
        add(f"n{ragged}", P(_gemm, n=ragged, k1=48, k2=16, mode="div", bias=True, relu=True,
                            l2=True, row_norm=True))
        if bn == 128:
            add("n192", P(_gemm, n=192, k1=48, k2=16, mode="div", bias=True, relu=True))

    add = adder("general")
    add("n32_k5", P(_gemm, n=32, k1=5, bias=True, relu=True, l2=True))
    add("n128_k5+5_div", P(_gemm, n=128, k1=5, k2=5, mode="div"))
    add("n64_k34", P(_gemm, n=64, k1=34, sigmoid=True))
    add("n200_k34_l2", P(_gemm, n=200, k1=34, relu=True, l2=True, row_norm=True))
    add("n128_k32_misaligned_a1", P(_gemm, n=128, k1=32, a1_shift=1))
    return c


def digest(tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def run(groups=None):
    """{case name: sha256 of the written bytes} of every case (of the given groups)."""
    return {name: digest(fn()) for group, name, fn in cases()
            if groups is None or group in groups}


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
