"""bench.py --dump-outputs / --full on CPU: the dumped rows are a fixed, seeded, ascending sample
within the byte budget, the files hold exactly those rows of the pass's output in fp32, and the
extras of a run are off unless --full asks for them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


class _Shard:
    def __init__(self, p_lo, p_hi, S):
        self.p_lo, self.p_hi, self.shard_rows = p_lo, p_hi, {"item": S}


def test_dump_rows_are_a_fixed_ascending_sample_within_the_budget():
    assert sum(bench.DUMP_BYTES.values()) <= 64 << 20
    r = bench.dump_rows(1_000_000, 128, 1 << 20, 0)
    assert r.dtype == np.int64 and r.size == (1 << 20) // (4 * 128)
    assert (np.diff(r) > 0).all() and r[0] >= 0 and r[-1] < 1_000_000
    assert (bench.dump_rows(1_000_000, 128, 1 << 20, 0) == r).all()  # the same rows every run
    assert (bench.dump_rows(1_000_000, 128, 1 << 20, 1) != r).any()  # another seed, other rows
    assert (bench.dump_rows(100, 128, 1 << 20, 0) == np.arange(100)).all()  # fits: every row


def test_dump_outputs_writes_the_sampled_rows_as_fp32(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", {"user": 64 * 16 * 4, "item": 32 * 16 * 4})
    g = torch.Generator().manual_seed(0)
    users, items = torch.randn(900, 16, generator=g), torch.randn(100, 16, generator=g)
    args = bench.parse(["--users", "900", "--items", "100"])
    out = {"user": users, "item": torch.cat([items, torch.zeros(4, 16)])}  # padded item block
    d = str(tmp_path / "dump")
    bench.dump_outputs(d, args, _Shard(0, 900, 104), out, 0, 1, torch.device("cpu"))
    assert sorted(os.listdir(d)) == ["item.npy", "user.npy"]
    u, i = np.load(os.path.join(d, "user.npy")), np.load(os.path.join(d, "item.npy"))
    assert u.dtype == np.float32 and i.dtype == np.float32
    assert u.shape == (64, 16) and i.shape == (32, 16)
    assert (u == users.numpy()[bench.dump_rows(900, 16, 64 * 16 * 4, 0)]).all()
    assert (i == items.numpy()[bench.dump_rows(100, 16, 32 * 16 * 4, 1)]).all()


def test_extras_are_off_without_full():
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d", "--steps", "7"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7
