"""CPU-side checks of torch.ops.gnnrec.csr_remove_edges (csrc/torch_ops.cpp over
csrc/csr_filter.hip): its schema declares every output mutable, the Meta kernel stops after
the shape and dtype checks (nothing launches here), and CPU tensors are refused."""
import pytest
import torch


def _T():
    from gnnrec import _lib
    return _lib.torch_ops()


def _meta(*shape, dtype=torch.int64):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _args(E=20, n_dst=5, R=3, dev="meta", **over):
    i64, i32 = torch.int64, torch.int32
    mk = lambda n, dt=i64: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    a = dict(src=mk(E), dst=mk(E), indptr=mk(n_dst + 1), indices=mk(E, i32), eids=mk(E),
             rm=mk(R), workspace=mk(4096, torch.uint8), src_out=mk(E), dst_out=mk(E),
             kept_eids=mk(E), indptr_out=mk(n_dst + 1), indices_out=mk(E, i32), eids_out=mk(E),
             status=mk(2))
    a.update(over)
    return list(a.values())


def test_schema_declares_the_outputs_mutable():
    s = str(_T().csr_remove_edges.default._schema)
    for out in ("workspace", "src_out", "dst_out", "kept_eids", "indptr_out", "indices_out",
                "eids_out", "status"):
        assert f"!) {out}" in s, s
    assert s.endswith("-> ()")
    assert "!) rm" not in s and "!) src," not in s
    assert int(_T().csr_remove_edges_workspace_bytes(0, 0)) > 0
    small, large = (int(_T().csr_remove_edges_workspace_bytes(e, 7)) for e in (1000, 10 ** 6))
    assert small < large < 10 ** 6  # well under a byte per edge


def test_meta_kernel_checks_shapes_and_dtypes():
    T = _T()
    T.csr_remove_edges(*_args())  # fine: nothing launches on meta
    T.csr_remove_edges(*_args(E=0, R=0))
    # the COO alone: every CSR operand empty
    T.csr_remove_edges(*_args(indptr=_meta(0), indices=_meta(0, dtype=torch.int32),
                              eids=_meta(0), indptr_out=_meta(0),
                              indices_out=_meta(0, dtype=torch.int32), eids_out=_meta(0)))
    with pytest.raises(ValueError, match="one length"):
        T.csr_remove_edges(*_args(src=_meta(19)))
    with pytest.raises(ValueError, match="the CSR must be"):
        T.csr_remove_edges(*_args(eids=_meta(19)))
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_remove_edges(*_args(indptr_out=_meta(5)))
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_remove_edges(*_args(kept_eids=_meta(21)))
    with pytest.raises(ValueError, match="output sizes"):
        T.csr_remove_edges(*_args(status=_meta(1)))
    with pytest.raises(ValueError, match="indices must be Int"):
        T.csr_remove_edges(*_args(indices=_meta(20)))
    with pytest.raises(ValueError, match="rm must be Long"):
        T.csr_remove_edges(*_args(rm=_meta(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="rm must be a contiguous 1-D"):
        T.csr_remove_edges(*_args(rm=_meta(3, 2)))


def test_cpu_tensors_are_refused():
    with pytest.raises(ValueError, match="HIP device tensor"):
        _T().csr_remove_edges(*_args(dev="cpu"))
    from gnnrec import ops
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.csr_remove_edges(z, z, z[:1])


def test_ops_wrapper_traces_on_meta():
    from gnnrec import ops
    s, d, csr = _meta(20), _meta(20), (_meta(6), _meta(20, dtype=torch.int32), _meta(20))
    s2, d2, kept, csr2 = ops.csr_remove_edges(s, d, _meta(3), csr)
    assert s2.shape == d2.shape == kept.shape == (20,) and csr2[0].shape == (6,)
    assert csr2[1].dtype == torch.int32 and csr2[2].shape == (20,)
    assert ops.csr_remove_edges(s, d, _meta(3))[3] is None
