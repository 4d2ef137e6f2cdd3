#!/usr/bin/env python3
"""Register, scratch, LDS and occupancy table of a set of kernels (default: the a1 aggregation
kernels), two trees side by side, from the compiler's own report (no GPU):

    python tools/spmm_resources.py --parent OTHER/gnn-recsys_amd/csrc > profiles/spmm_unify_resources.md
    python tools/spmm_resources.py --parent OTHER/gnn-recsys_amd/csrc --title "fused \
        aggregate+project kernels" --files spmm_project.hip spmm_pair_mfma.hip \
        > profiles/fused_share_resources.md

Builds the device code of the files (spmm.hip and dropout.hip) of both trees with the Makefile's
flags plus --cuda-device-only -Rpass-analysis=kernel-resource-usage, and prints one markdown line
per kernel of the parent tree with its counterpart in this tree: VGPRs, scratch bytes per
lane, LDS bytes per block, waves per SIMD.  Kernels are named as the parent names them; a
tree whose row / chunk / combine kernels take a policy type is mapped back:

    spmm_csr_kernel<DenseAgg<L,V,R,W,U,StoreRow<V,R>,true>>            spmm_csr_kernel<L,V,R,W,U>
    spmm_csr_kernel<DenseAgg<L,V,R,W,U,DropStoreRow<V,R,WHERE>,false>>  drop_csr_kernel<L,V,R,W,U,WHERE>
    spmm_csr_kernel<PackedAgg<R,U>>                                    spmm_csr_packed_kernel<R,U>
    (chunk and combine kernels alike; a dropout chunk kernel has no REDUCE, and with the
     mask at the output row it is the plain sum's chunk kernel)

Exit status 1 if a parent kernel has no counterpart, or its counterpart has more scratch than
it, another LDS size or fewer waves per SIMD, or if this tree builds more kernels than the
parent.
"""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("spmm.hip", "dropout.hip")
FIELDS = {"VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "waves", "LDS Size [bytes/block]": "lds"}


def remarks(csrc, name):
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(csrc))), "include")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3",
           "-std=c++17", "-fPIC", "-mcode-object-version=5", f"-I{inc}", "-Wall",
           "-Wno-unused-result", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", name, "-o", os.devnull]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{csrc}/{name}: {r.stderr[-2000:]}")
    return r.stderr


def canonical(name):
    """A demangled kernel name as the parent tree spells it."""
    name = name.replace("gnnrec::(anonymous namespace)::", "").replace("void ", "")
    name = re.sub(r"\(.*", "", name).replace(" ", "")
    m = re.match(r"spmm_(csr|chunk)_kernel<DenseAgg<(\d+),(\d+),(\d+),(\w+),(\d+),"
                 r"(Drop)?StoreRow<\d+,\d+(?:,(\d+))?>,\w+>>$", name)
    if m:
        kind, L, V, R, W, U, drop, where = m.groups()
        if not drop:
            return f"spmm_{kind}_kernel<{L},{V},{R},{W},{U}>"
        if kind == "csr":
            return f"drop_csr_kernel<{L},{V},{R},{W},{U},{where}>"
        return f"drop_chunk_kernel<{L},{V},{W},{U},{where}>"
    m = re.match(r"spmm_(csr|chunk)_kernel<PackedAgg<(\d+),(\d+)>>$", name)
    if m:
        return f"spmm_{m.group(1)}_packed_kernel<{m.group(2)},{m.group(3)}>"
    m = re.match(r"spmm_combine_kernel<(Drop)?StoreRow<(\d+),(\d+)(?:,(\d+))?>>$", name)
    if m:
        drop, V, R, where = m.groups()
        return f"drop_combine_kernel<{V},{R},{where}>" if drop else f"spmm_combine_kernel<{V},{R}>"
    return name


def table(csrc, files):
    with ThreadPoolExecutor(len(files)) as ex:
        text = "".join(ex.map(lambda f: remarks(csrc, f), files))
    rows, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True,
                           text=True, check=True).stdout.splitlines()
    return {canonical(n): v for n, v in zip(names, rows.values())}, len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="csrc directory of the tree to compare with")
    ap.add_argument("--new", default=os.path.join(ROOT, "gnn-recsys_amd", "csrc"))
    ap.add_argument("--files", nargs="+", default=list(FILES), help="sources to compile")
    ap.add_argument("--title", default="a1 aggregation kernels")
    args = ap.parse_args()
    with ThreadPoolExecutor(2) as ex:
        (par, n_par), (new, n_new) = ex.map(lambda c: table(c, args.files),
                                            (args.parent, args.new))
    bad = []
    print(f"# {args.title}: resources, parent and new\n")
    print("From `tools/spmm_resources.py` (hipcc -O3 --offload-arch=gfx950, "
          f"`-Rpass-analysis=kernel-resource-usage`; {' + '.join(args.files)}).  Kernels under "
          "the parent's names; REDUCE 0 / 1 / 2 = sum / mean / max, WHERE 0 / 1 = SRC / OUT.\n")
    print("| kernel | VGPRs | scratch B | LDS B | waves/SIMD | new VGPRs | new scratch B | "
          "new LDS B | new waves/SIMD |")
    print("|---|---|---|---|---|---|---|---|---|")
    for k in sorted(par):
        p = par[k]
        # the mask at the output row: the chunk partials are the plain sum's
        m = re.match(r"drop_chunk_kernel<(\d+),(\d+),(\w+),(\d+),1>$", k)
        alt = f"spmm_chunk_kernel<{m.group(1)},{m.group(2)},0,{m.group(3)},{m.group(4)}>" if m else k
        n = new.get(k) or new.get(alt)
        if n is None:
            bad.append(f"{k}: no counterpart")
            print(f"| `{k}` | {p['vgpr']} | {p['scratch']} | {p['lds']} | {p['waves']} | - | - | - | - |")
            continue
        if n["scratch"] > p["scratch"] or n["lds"] != p["lds"] or n["waves"] < p["waves"]:
            bad.append(f"{k}: {p} -> {n}")
        print(f"| `{k}` | {p['vgpr']} | {p['scratch']} | {p['lds']} | {p['waves']} | "
              f"{n['vgpr']} | {n['scratch']} | {n['lds']} | {n['waves']} |")
    if n_new > n_par:
        bad.append(f"{n_new} kernels, the parent builds {n_par}")
    print(f"\nKernels built: parent {n_par}, new {n_new}.")
    print("\nVerdict: " + ("every parent kernel has its counterpart with no more scratch, the "
                           "same LDS size and at least its waves per SIMD." if not bad else
                           "FAILED\n\n" + "\n".join(f"- {b}" for b in bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
