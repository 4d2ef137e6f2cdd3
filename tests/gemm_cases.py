"""GEMM cases for tests/test_gpu_gemm_reference.py beyond the pinned list of tools/gemm_bits.py.

The pinned cases (`pinned()`) have a parent digest each, so their list is closed.  `new()` are
the paths that list does not reach, built as the same `Case` description so that
tests/gemm_reference.py applies unchanged:

    scalar/     the scalar-store branch of the epilogue (N % 4 != 0, or a misaligned output):
                N = 30, 63, 127, 255 (l2norm or attention: the 256-column block) and N = 64 at
                column 1 of a 69-column table; bias + ReLU + l2norm + row_norm store, add with
                out_div, max, the three-step attention; the general loader (K = 34) at every
                width and the LDS-DMA loader (K = 48 + 16) where a 16-deep one exists
    blocks/     two column blocks of 128: N = 130 (the W row clamp), 190, 192
    rowepi/     N > 256 with a row norm or attention: GEMM, then row_epilogue_kernel
    deg/        both degree modes and bias_nonempty in the general kernel, BN 32 and BN 256
    neginf/     A2_ZERO_DEG over A2 rows of -inf (an empty max-aggregate), once per loader

Every output, row_norm and attn_state has one guard row / entry past M holding SENTINEL, which
the case passes no view of: a ragged block that writes past M changes it.

M is 1 (a partial wave), 128 (exactly one block), 129 and 300 (three blocks, the last ragged),
cut down where the M adds no path, to keep the list at 200:
  * scalar/ on the LDS-DMA loader runs M = 128 and 129 (either side of the block boundary):
    the epilogue is the code of the general loader's cases, which run every M;
  * rowepi/ runs M = 1, 129, 300: row_epilogue_kernel takes four rows per block, one wave
    each (1 and 129 end inside a block, 300 on its boundary); the two-step attention, whose
    calls are the first and last of the three-step one, runs 129 and 300;
  * deg/ runs M = 2 and 129: a degree vector must hold a zero and a non-zero degree, which
    one row cannot; both end inside a block, where the row clamp of the degree read matters.
"""
import functools
import importlib.util
import os
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "gemm_bits", os.path.join(os.path.dirname(HERE), "tools", "gemm_bits.py"))
gemm_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gemm_bits)
Call, Case = gemm_bits.Call, gemm_bits.Case

SENTINEL = -777.25
MS = (1, 128, 129, 300)
LOADERS = {"dma": (48, 16), "general": (34, 0)}


def pinned():
    """[(group, name, describe)] of tools/gemm_bits.py."""
    return gemm_bits.described()


@functools.lru_cache(None)
def _randn(shape, key):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(zlib.crc32(key.encode())))


@functools.lru_cache(None)
def _weight(shape, key):
    return _randn(shape, key) / 8


@functools.lru_cache(None)
def _degrees(m):
    """Degrees 0..7 with a zero in row 0 and a non-zero in the last row."""
    deg = torch.randint(0, 8, (m,), generator=torch.Generator().manual_seed(4100 + m),
                        dtype=torch.int32)
    deg[0], deg[m - 1] = 0, 5
    assert bool((deg == 0).any()) and bool((deg > 0).any()), "degrees need a zero and a non-zero"
    return deg


@functools.lru_cache(None)
def _neginf_rows(m, k, key):
    """A2 as ops.spmm(..., "max", empty_neginf=True) leaves it: -inf rows where the degree is 0."""
    a2 = _randn((m, k), key).clone()
    a2[_degrees(m) == 0] = float("-inf")
    return a2


def _build(name, m, n, k1, k2, steps, col=0, pad=0, row_norm=False, mode=None, bias_ne=False,
           neginf=False):
    """steps: the keyword arguments (Call fields) of each call; every call has its own A and
    W, all share the bias and the attention vector."""
    calls = []
    for j, kw in enumerate(steps):
        c = Call(a1_table=_randn((m, k1), f"{name}/a1/{j}"), k1=k1,
                 w1=_weight((n, k1), f"{name}/w1/{j}"), a2_mode=mode, **kw)
        if k2:
            c.a2 = (_neginf_rows(m, k2, f"{name}/a2/{j}") if neginf
                    else _randn((m, k2), f"{name}/a2/{j}"))
            c.w2 = _weight((n, k2), f"{name}/w2/{j}")
        if mode is not None or bias_ne:
            c.a2_deg = _degrees(m)
        if bias_ne:
            c.bias_nonempty = _randn((n,), f"{name}/bias_ne")
        calls.append(c)
    out_init = _randn((m + 1, col + n + pad), f"{name}/out").clone()
    out_init[m] = SENTINEL
    attn = any(c.attn_vec is not None for c in calls)
    return Case(m=m, n=n, calls=calls, out_init=out_init, pad=pad, col=col, guard=1,
                row_norm_init=torch.full((m + 1,), SENTINEL) if row_norm else None,
                attn_state_init=torch.full((m + 1, 2), SENTINEL) if attn else None)


def _ways(n, key, l2, l2_attn, row_norm=True):
    """{way: (steps, row_norm)}: the four uses of an output width.  l2: add and max also
    normalise (what sends N = 255 to the 256-column block and N > 256 to row_epilogue)."""
    bias, av = _randn((n,), f"{key}/bias"), _randn((n,), f"{key}/attn_vec")
    return {
        "epi": ([dict(bias=bias, relu=True, l2norm=True)], row_norm),
        "add_div": ([dict(accum="add", out_div=2.0, l2norm=l2)], False),
        "max": ([dict(accum="max", l2norm=l2)], False),
        "attn3": ([dict(bias=bias, relu=True, l2norm=l2_attn, accum=a, attn_vec=av)
                   for a in ("attn_first", "attn", "attn_last")], False),
    }


def new():
    """[(group, name, describe)]: describe() returns the Case."""
    c = []

    def add(group, name, ms, **kw):
        for m in ms:
            full = f"{group}/{name}_m{m}"
            c.append((group, full, functools.partial(_build, full, m, **kw)))

    # the scalar-store epilogue
    for n, col, pad in ((30, 0, 0), (63, 0, 0), (127, 0, 0), (255, 0, 0), (64, 1, 4)):
        tag = f"n{n}" + (f"_col{col}" if col else "")
        for loader, (k1, k2) in LOADERS.items():
            if loader == "dma" and n not in (63, 127, 64):
                continue  # 48 + 16 is no multiple of the 32-deep tiles of BN 32 and BN 256
            ways = _ways(n, f"scalar/{tag}", l2=n == 255, l2_attn=n % 2 == 0)
            for way, (steps, row_norm) in ways.items():
                add("scalar", f"{tag}_{loader}_{way}", MS if loader == "general" else (128, 129),
                    n=n, k1=k1, k2=k2, steps=steps, col=col, pad=pad, row_norm=row_norm)

    # two column blocks
    for n in (130, 190, 192):
        bias = _randn((n,), f"blocks/n{n}/bias")
        add("blocks", f"n{n}_dma_bias_relu", MS, n=n, k1=48, k2=16,
            steps=[dict(bias=bias, relu=True)])
        add("blocks", f"n{n}_general_add", MS, n=n, k1=34, k2=0, steps=[dict(accum="add")])

    # N > 256 with a row norm or attention: GEMM + row_epilogue_kernel
    for n, pad in ((260, 0), (300, 4), (384, 0)):
        ways = _ways(n, f"rowepi/n{n}", l2=True, l2_attn=True, row_norm=False)
        ways["attn3_plain"] = (_ways(n, f"rowepi/n{n}", l2=True, l2_attn=False)["attn3"][0], False)
        for way, (steps, _) in ways.items():
            add("rowepi", f"n{n}_{way}", (1, 129, 300), n=n, k1=48, k2=16, steps=steps, pad=pad)
        first, _, last = ways["attn3_plain"][0]
        add("rowepi", f"n{n}_attn2", (129, 300), n=n, k1=48, k2=16, steps=[first, last], pad=pad)

    # degree modes and bias_nonempty outside depth 16 x BN 64 / 128
    for kernel, n, k1, k2, l2 in (("general", 100, 48, 5, False), ("bn32", 32, 64, 32, False),
                                  ("bn256", 200, 32, 64, True)):
        for mode in ("zero", "div"):
            add("deg", f"{kernel}_{mode}", (2, 129), n=n, k1=k1, k2=k2, mode=mode,
                steps=[dict(relu=True, l2norm=l2)])
        add("deg", f"{kernel}_bias_nonempty", (2, 129), n=n, k1=k1, k2=k2, bias_ne=True,
            steps=[dict(bias=_randn((n,), f"deg/{kernel}/bias"), relu=True, l2norm=l2)])

    # A2_ZERO_DEG over -inf rows
    for loader, n, k1, k2 in (("depth16", 64, 48, 16), ("depth32", 32, 32, 32),
                              ("general", 64, 48, 5)):
        add("neginf", f"{loader}_zero", (129,), n=n, k1=k1, k2=k2, mode="zero", neginf=True,
            steps=[dict(relu=True)])
    return c


GROUPS_NEW = ("scalar", "blocks", "rowepi", "deg", "neginf")

