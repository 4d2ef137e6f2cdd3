"""The counter-based dropout mask (csrc/dropout.hpp) through the library's host routine
(gnnrec_dropout_mask_host, no GPU): it equals a numpy restatement of the hash, and its keep
rate and the independence of streams, steps and seeds are within 5 sigma of exact."""
import numpy as np
import pytest

from gnnrec import ops

U = np.uint64
P = (0.1, 0.5, 0.8)


def mix64(z):
    z = np.asarray(z, dtype=U)
    with np.errstate(over="ignore"):
        z = z + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def hash3(seed, a, b):
    with np.errstate(over="ignore"):
        return mix64(mix64(U(seed) ^ mix64(U(a))) ^
                     (np.asarray(b, dtype=U) * U(0xD1B54A32D192ED03)))


def threshold(p):
    return int(np.rint(p * 65536.0))  # ties to even, as the library's nearbyint


def numpy_mask(seed, step, stream, n_rows, d, p):
    """key = hash3(seed, step, stream); word(r, q) = mix64(key ^ (r * Q + q)), Q = ceil(d / 4);
    column c draws the 16 bits of word(r, c / 4) from bit 16 * (c % 4); keep iff draw >= T."""
    key = hash3(seed, step, stream)
    Q = (d + 3) // 4
    r = np.arange(n_rows, dtype=U)[:, None]
    c = np.arange(d, dtype=U)[None, :]
    with np.errstate(over="ignore"):
        word = mix64(key ^ (r * U(Q) + c // U(4)))
    draw = (word >> (U(16) * (c % U(4)))) & U(0xFFFF)
    return draw >= U(threshold(p))


@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("d", (6, 64, 128))
def test_host_mask_equals_the_numpy_restatement(p, d):
    for seed, step, stream in ((0, 0, 0), (1, 2, 3), (2 ** 63 + 11, 977, (5 << 16) + 3),
                               (2 ** 64 - 1, 2 ** 40, 1)):
        got = ops.dropout_mask_host(seed, step, stream, 1000, d, p)
        assert got.shape == (1000, d) and got.dtype == bool
        np.testing.assert_array_equal(got, numpy_mask(seed, step, stream, 1000, d, p))


@pytest.mark.parametrize("p", P)
def test_keep_rate_and_scale(p):
    n = 1 << 20
    q = 1.0 - threshold(p) / 65536.0
    sigma = np.sqrt(q * (1 - q) / n)
    keep = ops.dropout_mask_host(7, 3, 1, n // 128, 128, p)
    assert keep.size == n
    assert abs(keep.mean() - q) <= 5 * sigma
    # the expectation of a dropped element is the element: scale = 1 / keep probability
    assert ops.dropout_scale(p) == np.float32(65536.0) / np.float32(65536 - threshold(p))
    assert abs(ops.dropout_scale(p) * q - 1.0) < 1e-6


@pytest.mark.parametrize("p", P)
def test_streams_steps_and_seeds_draw_independent_masks(p):
    n = 1 << 20
    q = 1.0 - threshold(p) / 65536.0
    a = q * q + (1 - q) * (1 - q)  # two independent masks agree on this fraction
    sigma = np.sqrt(a * (1 - a) / n)
    base = ops.dropout_mask_host(7, 3, 0, n // 64, 64, p)
    for other in (ops.dropout_mask_host(7, 3, 1, n // 64, 64, p),   # another stream
                  ops.dropout_mask_host(7, 4, 0, n // 64, 64, p),   # another step
                  ops.dropout_mask_host(8, 3, 0, n // 64, 64, p)):  # another seed
        agree = (base == other).mean()
        assert abs(agree - a) <= 5 * sigma, (agree, a, sigma)


def test_threshold_zero_keeps_everything():
    assert ops.dropout_mask_host(5, 1, 2, 257, 30, 0.0).all()
    assert ops.dropout_scale(0.0) == 1.0
    # p = 1 drops everything and scales by 0 (no infinity)
    assert not ops.dropout_mask_host(5, 1, 2, 257, 30, 1.0).any()
    assert ops.dropout_scale(1.0) == 0.0
