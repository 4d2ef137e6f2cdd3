"""gnnrec_topk_rows_f32 (csrc/topk.hip, through gnnrec.recs.topk_rows) against the ranking
definition on every scan path: the three KMAX instantiations as first and as later passes,
the float4 scan with no, one and two trips of its unrolled loop and with a ragged end, the
scalar scan reached by stride and by base alignment, worst-case insertion, the LDS exclusion
search and the overflow scan behind it, -inf and +inf scores, and row addressing.

The order (score desc, column asc) is total: indices are compared for equality and values
bit for bit, every call is made twice and must repeat itself, and the last column of the
values is checked against the k-th largest eligible score (the threshold the prefiltered
paths take from this kernel).  tests/test_topk_cases_cpu.py shows that the inputs in
tests/topk_cases.py reach the paths they are named for."""
import functools

import numpy as np
import pytest
import torch

import topk_cases as tc

pytestmark = pytest.mark.gpu

CALLS = [0]  # topk_rows calls made by this file (each is ceil(k / 64) kernel launches)


def _topk(scores, k, indptr=None, indices=None):
    from gnnrec.recs import topk_rows
    CALLS[0] += 1
    return topk_rows(scores, k, indptr, indices)


def _device_view(scores, layout):
    """The scores on the device, carved out of an allocation as the layout says."""
    n_cols = scores.shape[1]
    big, start = tc.embed(scores, layout)
    view = torch.from_numpy(big).cuda()[:, start:start + n_cols]
    vec = view.data_ptr() % 16 == 0 and max(view.stride(0), n_cols) % 4 == 0
    assert vec == tc.is_vec(layout, n_cols), (layout, n_cols, view.data_ptr(), view.stride())
    return view


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared inputs are read-only


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _check(scores, layout, k, indptr=None, indices=None, names=None):
    """One case: the kernel's (idx, vals) equal the definition's, bit for bit; a second call
    repeats the first; vals[:, k - 1] is the k-th largest eligible score -> (idx, vals)."""
    view = _device_view(scores, layout)
    ip = ix = None
    if indptr is not None:
        ip, ix = _dev(indptr), _dev(indices)
    vals, idx = _topk(view, k, ip, ix)
    vals2, idx2 = _topk(view, k, ip, ix)
    assert vals.shape == idx.shape == (scores.shape[0], k)
    got_idx, got_vals = idx.cpu().numpy(), vals.cpu().numpy()
    ref_idx, ref_vals = tc.ranked(scores, k, indptr, indices)
    for r in range(scores.shape[0]):
        what = f"row {r}" + (f" ({names[r]})" if names else "")
        np.testing.assert_array_equal(got_idx[r], ref_idx[r], err_msg=what)
        np.testing.assert_array_equal(_bits(got_vals[r]), _bits(ref_vals[r]), err_msg=what)
    assert torch.equal(idx, idx2) and torch.equal(vals.view(torch.int32), vals2.view(torch.int32))
    np.testing.assert_array_equal(_bits(got_vals[:, k - 1]),
                                  _bits(tc.kth_eligible(scores, k, indptr, indices)))
    return got_idx, got_vals


@pytest.mark.parametrize("n_cols,layout,k", tc.SCAN_CASES)
def test_scan_paths(n_cols, layout, k):
    """Every column count at an edge of the three scan loops, in the four layouts, with a
    first pass of each KMAX: `normal` rows and `ints` rows (ties across threads)."""
    s, names = tc.scan_scores(n_cols)
    _check(s, layout, k, names=names)


@functools.lru_cache(maxsize=None)
def _pass_result(n_cols, k):
    s, names = tc.pass_scores(n_cols)
    return _check(s, tc.PASS_LAYOUT, k, names=names)


@pytest.mark.parametrize("n_cols,k", tc.PASS_CASES)
def test_passes(n_cols, k):
    """Every k: last passes of 1, 16, 17, 32, 33 and 64 columns, each KMAX as a first and as
    a later pass, over ties that straddle the pass boundary (`ints`, `const`), -inf and +inf."""
    _pass_result(n_cols, k)


@pytest.mark.parametrize("n_cols,k", tc.PASS_CASES)
def test_neg_inf_is_a_score_not_a_pad(n_cols, k):
    """A -inf column is a valid result, ordered by column after every finite score: the
    callers (recs._rows_exact) rewrite those indices to -1 themselves."""
    s, names = tc.pass_scores(n_cols)
    idx, vals = _pass_result(n_cols, k)
    assert k <= n_cols
    rows = [r for r, name in enumerate(names) if name == "neg_inf"]
    for r in rows:
        assert (idx[r] >= 0).all()
        n_fin = min(k, int(np.isfinite(s[r]).sum()))
        assert np.isfinite(vals[r, :n_fin]).all() and np.isneginf(vals[r, n_fin:]).all()
        np.testing.assert_array_equal(idx[r, n_fin:], np.nonzero(np.isneginf(s[r]))[0][:k - n_fin])
    np.testing.assert_array_equal(idx[rows[-1]], np.arange(k))   # the row of -inf throughout
    if n_cols == 257 and k >= 128:
        assert np.isneginf(vals[rows[0], -1]) and np.isfinite(vals[rows[0], 0])


@pytest.mark.parametrize("n_cols,layout,k", tc.INSERT_CASES)
def test_insertion(n_cols, layout, k):
    """Ascending rows insert at every offer and shift the whole register list; one_owner rows
    make one thread's list hold every winner and its head walk to the end of it."""
    s, names = tc.insert_scores(n_cols, layout, k)
    _check(s, layout, k, names=names)


@pytest.mark.parametrize("builder,n_cols,layout,k", tc.EXCL_CASES)
def test_exclusions(builder, n_cols, layout, k):
    """Unsorted, duplicated, odd and even, out-of-range, LDS-filling and overflowing lists,
    and lists that leave 0, 1, k - 1, k, k + 1 or 64 columns."""
    s, indptr, indices = tc.excl_inputs(builder, n_cols, k)
    _check(s, layout, k, indptr, indices, names=[f"{builder} list of {n}" for n in np.diff(indptr)])


@pytest.mark.parametrize("n_rows,layout", tc.ROW_CASES)
def test_rows(n_rows, layout):
    """One row, and more rows than compute units, each with its own list length and its own
    scores: row r's result is row r's, with a row stride equal to and above n_cols."""
    s, indptr, indices = tc.row_inputs(n_rows)
    _check(s, layout, tc.ROW_K, indptr, indices)


@pytest.mark.parametrize("builder,k", tc.ROUTE_CASES)
def test_list_route_and_mask_route_agree(builder, k):
    """topk_rows with the lists, against mask_excluded on a copy, topk_rows without lists
    and the rewrite of -inf results to -1 that recs._rows_exact does."""
    from gnnrec import ops
    s, indptr, indices = tc.route_inputs(builder, k)
    assert np.isfinite(s).all()
    ip = _dev(indptr)
    a_vals, a_idx = _topk(_dev(s), k, ip, _dev(indices))
    masked = _dev(s)
    ops.mask_excluded(masked, None, ip, _dev(indices.astype(np.int32)))
    b_vals, b_idx = _topk(masked, k)
    b_idx = torch.where(b_vals == float("-inf"), torch.full_like(b_idx, -1), b_idx)
    assert torch.equal(a_idx, b_idx)
    assert torch.equal(a_vals.view(torch.int32), b_vals.view(torch.int32))
    ref_idx, ref_vals = tc.ranked(s, k, indptr, indices)
    np.testing.assert_array_equal(a_idx.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(_bits(a_vals.cpu().numpy()), _bits(ref_vals))


@pytest.mark.parametrize("k", [tc.ROW_K, 100])
def test_no_write_outside_the_result(k):
    """The op, called directly on the middle rows of sentinel-filled buffers with a guard row
    on either side, gives topk_rows' result and leaves the guards alone (rows that run out of
    columns, and so write pads in every pass, included)."""
    from gnnrec import _lib
    s, indptr, indices = tc.row_inputs(300)
    n = s.shape[0]
    S = _dev(s)
    ip, ix = _dev(indptr), _dev(indices)
    vals, idx = _topk(S, k, ip, ix)
    vbuf = torch.full((n + 2, k), 12345.0, dtype=torch.float32, device="cuda")
    ibuf = torch.full((n + 2, k), -777, dtype=torch.int64, device="cuda")
    CALLS[0] += 1
    _lib.torch_ops().topk_rows(S, k, ip, ix, vbuf[1:n + 1], ibuf[1:n + 1])
    assert torch.equal(ibuf[1:n + 1], idx)
    assert torch.equal(vbuf[1:n + 1].view(torch.int32), vals.view(torch.int32))
    for g in (0, n + 1):
        assert (vbuf[g] == 12345.0).all() and (ibuf[g] == -777).all()
    wide = torch.full((n, k + 3), 12345.0, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="out_vals must be a contiguous"):  # a column slice
        _lib.torch_ops().topk_rows(S, k, ip, ix, wide[:, :k], ibuf[1:n + 1])
    assert (wide == 12345.0).all()
    with pytest.raises(ValueError, match="exclude_indptr must be contiguous with n_rows"):
        _lib.torch_ops().topk_rows(S, k, ip[:-1], ix, vbuf[1:n + 1], ibuf[1:n + 1])


def test_zz_call_count():
    """The whole file stays at several hundred cases, each run twice."""
    print(f"topk_rows calls made by this file: {CALLS[0]}")
    assert CALLS[0] <= 1100
