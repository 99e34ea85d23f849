"""csrc/half_input_kernels.hip on the host SIMT emulator (no GPU): the two streams between a caller's sample-major 16-bit matrix [n][n_dims]
and the feature-major matrices [padded][n] the network kernels read and write, bit for bit against numpy -- the pad kernel's output is the
input's bits transposed plus rows of 1.0, the un-pad kernel's is the first n_dims rows transposed back.

Widths 3 -> 16, 17 -> 32 and 40 -> 48 at one and two tiles of 256 samples (n = 256, 512) as the 16-byte paths see them; beyond those, every
other path of the kernels: 16 -> 16 and 64 -> 64 (nothing to pad), 100 -> 112 and 136 -> 144 (two and three feature chunks, the first no
multiple of 8), a ragged last tile (n = 300: only the emulator can ask for one, the library takes multiples of 256), and matrices that
start 2 and 8 bytes behind a 16-byte boundary (the 2-byte paths).  Both 16-bit types: the padding's pattern differs, nothing else does."""
import numpy as np
import pytest

import emu_half_input as E

pytestmark = pytest.mark.skipif(not E.available(), reason="no host compiler for the emulator")
WIDTHS = [(3, 16), (17, 32), (40, 48)]
MORE_WIDTHS = [(16, 16), (64, 64), (20, 32), (100, 112), (136, 144)]


def _bits(shape, seed):
    """every 16-bit pattern is fair game: the kernels must not interpret them (NaN payloads, subnormals, both zeros included)"""
    return np.random.default_rng(seed).integers(0, 1 << 16, size=shape, dtype=np.uint16)


def _expected_pad(x, padded, bf16):
    n, d = x.shape
    want = np.full((padded, n), E.ONE[bf16], dtype=np.uint16)
    want[:d] = x.T
    return want


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", [256, 512])
@pytest.mark.parametrize("d,padded", WIDTHS)
def test_pad_is_the_input_bits_plus_ones(d, padded, n, bf16):
    x = _bits((n, d), seed=d * 1000 + n)
    assert np.array_equal(E.pad(x, padded, bf16=bf16), _expected_pad(x, padded, bf16))


@pytest.mark.parametrize("n", [256, 512])
@pytest.mark.parametrize("d,padded", WIDTHS)
def test_unpad_is_the_first_columns(d, padded, n):
    dy = _bits((padded, n), seed=d * 1000 + n + 1)
    assert np.array_equal(E.unpad(dy, d), dy[:d].T)


@pytest.mark.parametrize("n", [256, 768, 300])
@pytest.mark.parametrize("d,padded", WIDTHS + MORE_WIDTHS)
def test_other_widths_and_a_ragged_tile(d, padded, n):
    x = _bits((n, d), seed=d + n)
    assert np.array_equal(E.pad(x, padded), _expected_pad(x, padded, False))
    dy = _bits((padded, n), seed=d + n + 1)
    assert np.array_equal(E.unpad(dy, d), dy[:d].T)


@pytest.mark.parametrize("in_offset,out_offset", [(1, 0), (4, 0), (0, 1), (0, 4), (4, 4)])
@pytest.mark.parametrize("d,padded", [(3, 16), (16, 16), (40, 48), (100, 112)])
def test_matrices_off_the_16_byte_boundary(d, padded, in_offset, out_offset):
    n = 512
    x = _bits((n, d), seed=d)
    assert np.array_equal(E.pad(x, padded, in_offset=in_offset, out_offset=out_offset), _expected_pad(x, padded, False))
    dy = _bits((padded, n), seed=d + 1)
    assert np.array_equal(E.unpad(dy, d, in_offset=in_offset, out_offset=out_offset), dy[:d].T)


def test_round_trip():
    x = _bits((512, 20), seed=7)
    assert np.array_equal(E.unpad(E.pad(x, 32), 20), x)
