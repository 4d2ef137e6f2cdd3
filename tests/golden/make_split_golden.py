"""Generate the train/valid split fixtures by running the reference's own train_valid_split.

TEST INFRASTRUCTURE.  Runs only where a checkout of the reference is at hand (GNNREC_REFERENCE,
the default as in make_golden.py); it writes nothing elsewhere.  It imports the reference's src/sampling.py
UNMODIFIED under a stub `dgl` module (the function only names dgl.DGLHeteroGraph in an
annotation) and hands it a small numpy graph class with the five methods the function calls,
each restating DGL 0.5.2's documented behaviour: clone, remove_edges (surviving edges keep
their order and are renumbered), find_edges, number_of_edges, num_nodes.  The cases and the
seeded graph are tests/split_cases.py; the fixtures tests/golden/split_<case>.npz hold
integer arrays only.  No reference source is copied: only numbers are stored.

    python tests/golden/make_split_golden.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GNNREC_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import split_cases as sc  # noqa: E402


class NumpyGraph:
    """What train_valid_split asks of a DGL heterograph, over numpy COO lists."""

    def __init__(self, edges, num_nodes):
        self.edges = {ce: (np.array(s), np.array(d)) for ce, (s, d) in edges.items()}
        self._num_nodes = dict(num_nodes)

    def clone(self):
        return NumpyGraph(self.edges, self._num_nodes)

    def number_of_edges(self, etype):
        return len(self.edges[tuple(etype)][0])

    def num_nodes(self, ntype):
        return self._num_nodes[ntype]

    def find_edges(self, eids, etype):
        s, d = self.edges[tuple(etype)]
        eids = np.asarray(eids, dtype=np.int64)
        return s[eids], d[eids]

    def remove_edges(self, eids, etype):
        s, d = self.edges[tuple(etype)]
        keep = np.ones(len(s), dtype=bool)
        keep[np.asarray(eids, dtype=np.int64)] = False
        self.edges[tuple(etype)] = (s[keep], d[keep])


def load_reference_split():
    sys.dont_write_bytecode = True  # never write into the read-only reference tree
    dgl = types.ModuleType("dgl")
    dgl.DGLHeteroGraph = object
    sys.modules["dgl"] = dgl
    spec = importlib.util.spec_from_file_location("ref_sampling",
                                                  os.path.join(REF, "src", "sampling.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.train_valid_split


def main():
    if not os.path.isdir(REF):
        print(f"no reference at {REF}: nothing written")
        return
    split = load_reference_split()
    edges, gt_test = sc.make_inputs()
    nodes = {"user": sc.N_USER, "item": sc.N_ITEM}
    for name, case in sc.CASES.items():
        res = split(NumpyGraph(edges, nodes), gt_test, **sc.split_kwargs(case))
        flat = sc.flatten(res, lambda g, ce: g.edges[ce])
        np.savez_compressed(os.path.join(HERE, f"split_{name}.npz"), **flat)
        print(name, {k: v.shape for k, v in flat.items() if "order" not in k and "src" not in k
                     and "dst" not in k})
    try:
        split(NumpyGraph(edges, nodes), gt_test, **sc.split_kwargs(sc.RAISING))
    except KeyError as e:
        print("raising case: KeyError", e)
    else:
        raise SystemExit("the raising case did not raise")


if __name__ == "__main__":
    main()
