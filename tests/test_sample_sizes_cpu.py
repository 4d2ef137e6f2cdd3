"""CPU-side checks of the fused sampler's size record (gnnrec.ops.SampleSizes): the flat
layout gnnrec::sample_blocks returns — node entries [L + 1][T] (the seeds first), edge entries
[L][R], dump rows [L][T] — decoded by ops.sample_sizes, and the sizes_out / static_shapes
pairing ops.sample_blocks insists on (its own check: the op itself has no CPU or meta form)."""
import pytest
import torch

L, T, R = 2, 2, 3
FLAT = [60, 0,              # seeds: 60 of type 0, none of type 1
        61, 120, 300, 121,  # the sources of step 0, of step 1
        600, 0, 7,          # step 0's edges per relation
        610, 1200, 9,       # step 1's
        2, 1, 1, 3]         # dump rows after step 0's / step 1's destinations


def test_sample_sizes_decodes_the_flat_record():
    from gnnrec import ops
    s = ops.sample_sizes(FLAT, L, T, R)
    assert s.nodes == [[60, 0], [61, 120], [300, 121]]
    assert s.edges == [[600, 0, 7], [610, 1200, 9]]
    assert s.dump == [[2, 1], [1, 3]]
    assert s == ops.SampleSizes(s.nodes, s.edges, s.dump)
    with pytest.raises(ValueError):
        ops.sample_sizes(FLAT[:-1], L, T, R)
    with pytest.raises(ValueError):
        ops.sample_sizes(FLAT, L, T, R, dump=False)


def test_sample_sizes_of_a_tensor_are_views_of_it():
    from gnnrec import ops
    flat = torch.tensor(FLAT[:(L + 1) * T + L * R])  # the device array holds no dump rows
    s = ops.sample_sizes(flat, L, T, R, dump=False)
    assert s.dump == []
    assert [[int(x) for x in row] for row in s.nodes] == [[60, 0], [61, 120], [300, 121]]
    assert [[int(x) for x in row] for row in s.edges] == [[600, 0, 7], [610, 1200, 9]]
    flat[2 * T + 1] = 5  # step 1's sources of type 1
    assert s.nodes[2][1].shape == (1,) and int(s.nodes[2][1]) == 5
    out, views = ops.sample_sizes_out(L, T, R, "meta")
    assert out.shape == flat.shape and out.dtype == torch.int64
    assert len(views.nodes) == L + 1 and len(views.edges) == L and views.dump == []


@pytest.mark.parametrize("static, with_sizes_out", [(False, True), (True, False)])
def test_sample_blocks_pairs_sizes_out_with_static_shapes(static, with_sizes_out):
    from gnnrec import ops
    sizes_out = torch.empty((L + 1) * T + L * R, dtype=torch.int64, device="meta")
    with pytest.raises(ValueError, match="sizes_out"):
        ops.sample_blocks([], [], [], [], [], [], [10] * T, [], [], [[]] * L, [[]] * L, 1,
                          static_shapes=static, sizes_out=sizes_out if with_sizes_out else None)
