"""recs.rank_items(head=) returns the bits it returned while it had kernels of its own.

tests/golden/rank_mlp_bits.json holds one SHA-256 per case of (rank, the int32 bit patterns of
vals), recorded on an MI355X from the last tree whose rank_items(head=) ran the pair count
modes and the pair resolve kernel of csrc/heads.hip: the `_case` tables of
test_ranks_are_the_definition and the `_pop_case` tables of the popularity tests, each with
and without the exclusion lists.  The pairs now run as one-slot rows of the list kernels
(DESIGN.md §26); vals come from the same rating() of the same edge_mlp score and the ranks
are exact integers, so every digest must be reproduced."""
import hashlib
import json
import os

import numpy as np
import pytest

import rank_mlp_cases as rm
import recommend_mlp_cases as mc
from test_gpu_rank_mlp import _bits, _case, _cu, _pop_case, _rank

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rank_mlp_bits.json")
CASES = [("plain", kind, d) for kind in mc.KINDS for d in mc.DIMS] + \
        [("popularity", w) for w in rm.POP_WEIGHTS]


def case_name(case):
    return "-".join(str(c) for c in case)


def digests(case):
    """{'excluded': sha, 'all': sha} of the case: rank int64 then vals' bits, little endian."""
    if case[0] == "plain":
        hu, hi, pl, _, excl, us, gs, _, _ = _case(*case[1:])
        kw = {}
    else:
        hu, hi, pl, pop, _, excl, us, gs, _ = _pop_case(case[1])
        kw = dict(popularity=_cu(pop), weight_popularity=case[1])
    out = {}
    for name, ex in (("excluded", excl), ("all", None)):
        rank, vals, _ = _rank(pl, hu, hi, us, gs, ex, **kw)
        h = hashlib.sha256(rank.astype("<i8").tobytes())
        h.update(_bits(vals).astype("<i4").tobytes())
        out[name] = h.hexdigest()
    return out


def test_golden_names_the_cases():
    with open(GOLDEN) as f:
        assert sorted(json.load(f)) == sorted(case_name(c) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_rank_items_reproduces_the_recorded_bits(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case_name(case)]
    assert digests(case) == want
