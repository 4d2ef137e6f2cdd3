"""The packed row format (csrc/pack_rows.hpp) through the library's host routines
(gnnrec_pack_rows_host / gnnrec_unpack_rows_host, no GPU) against a numpy restatement: the
mask is a bit test, `pre` the popcount prefix, rows above 88 non-zeros are flagged and store
no values, padding is zero, and unpack(pack(x)) is x bit for bit."""
import numpy as np

from gnnrec import ops
from packed_rows_cases import (D, DENSE_BIT, HDR, NNZ_CASES, SLOTS, WORDS, edge_rows, numpy_pack,
                               numpy_unpack, relu_table, row_with_nnz)


def test_constants():
    assert (ops.PACK_D, ops.PACK_WORDS, ops.PACK_SLOTS) == (D, WORDS, SLOTS)
    assert ops.PACK_DENSE_BIT == int(DENSE_BIT)


def test_host_pack_equals_the_numpy_restatement():
    rng = np.random.default_rng(0)
    x = np.concatenate([edge_rows(rng), relu_table(rng, 200), relu_table(rng, 50, 0.2)])
    p, dense = ops.pack_rows_host(x)
    ref = numpy_pack(x)
    assert p.shape == (len(x), WORDS) and p.dtype == np.uint32
    np.testing.assert_array_equal(p, ref)
    assert dense == int(((ref[:, 5] & DENSE_BIT) != 0).sum()) > 0


def test_header_fields_and_padding():
    rng = np.random.default_rng(1)
    for nnz in NNZ_CASES:
        x = row_with_nnz(rng, nnz)[None]
        p = ops.pack_rows_host(x)[0][0]
        nz = x[0].view(np.uint32) != 0
        mask = [int(p[w]) for w in range(4)]
        assert [bin(m).count("1") for m in mask] == [int(nz[32 * w:32 * w + 32].sum())
                                                     for w in range(4)]
        pre = [(int(p[4]) >> (8 * w)) & 255 for w in range(4)]
        assert pre == [int(nz[:32 * w].sum()) for w in range(4)]
        assert int(p[5]) & 0x7FFFFFFF == nnz
        assert bool(p[5] & DENSE_BIT) == (nnz > SLOTS)
        assert p[6] == 0 and p[7] == 0
        stored = 0 if nnz > SLOTS else nnz
        np.testing.assert_array_equal(p[HDR:HDR + stored], x[0].view(np.uint32)[nz][:stored])
        assert not p[HDR + stored:].any()  # unused slots, and every slot of a dense row


def test_special_values_are_kept():
    x = edge_rows(np.random.default_rng(2))
    p, _ = ops.pack_rows_host(x)
    last = x[-1].view(np.uint32)  # -0.0, NaN, a denormal, all ones at the word ends
    assert [int(p[-1, w]) for w in range(4)] == [1 | (1 << 31), 1, 0, 1 << 31]
    np.testing.assert_array_equal(p[-1, HDR:HDR + 4], last[[0, 31, 32, 127]])


def test_round_trip_is_bitwise():
    rng = np.random.default_rng(3)
    x = np.concatenate([edge_rows(rng), relu_table(rng, 300), relu_table(rng, 40, 0.1)])
    p, _ = ops.pack_rows_host(x)
    back = ops.unpack_rows_host(p, x)
    np.testing.assert_array_equal(back.view(np.uint32), x.view(np.uint32))
    np.testing.assert_array_equal(numpy_unpack(p, x).view(np.uint32), x.view(np.uint32))
    # rows that are not flagged decode without the dense table
    keep = (p[:, 5] & DENSE_BIT) == 0
    blank = np.zeros_like(x)
    np.testing.assert_array_equal(ops.unpack_rows_host(p, blank)[keep].view(np.uint32),
                                  x[keep].view(np.uint32))
