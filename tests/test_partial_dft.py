"""tests/partial_dft.py (single lines of irfftn from the half spectrum, and its Parseval sums) against numpy's full transform."""
import numpy as np
import pytest

import partial_dft


@pytest.mark.parametrize("shape", [(10, 14, 24), (40, 60, 80)])
@pytest.mark.parametrize("chunk_bytes", [1 << 30, 40000])          # one chunk; and chunks of a few planes with a ragged last one
def test_partial_dft_lines_against_irfftn(shape, chunk_bytes):
    """Lines along z, y and x at first, last and interior positions agree with np.fft.irfftn to 1e-12 (of the field's rms) -- on an
    array whose DC / Nyquist planes are NOT Hermitian, so that numpy's rule for those bins (imaginary parts dropped by the last,
    real transform) is part of the check -- and the Parseval moments on a Hermitian one."""
    rng = np.random.RandomState(3)
    nx, ny, nz = shape
    K = rng.normal(size=(nx, ny, nz // 2 + 1)) + 1j * rng.normal(size=(nx, ny, nz // 2 + 1))
    ref = np.fft.irfftn(K, s=shape, axes=(0, 1, 2))
    rms = ref.std()
    zl = [(0, 0), (nx - 1, ny - 1), (3, 5), (nx // 2, 1)]
    yl = [(0, 0), (nx - 1, nz - 1), (3, 7), (1, nz // 2)]
    xl = [(0, 0), (ny - 1, nz - 1), (5, 7), (ny // 2, 3)]
    for dtype in (np.complex128, np.complex64):
        Kd = K.astype(dtype)
        want = ref if dtype == np.complex128 else np.fft.irfftn(Kd.astype(np.complex128), s=shape, axes=(0, 1, 2))
        oz, oy, ox = partial_dft.field_lines(Kd, zl, yl, xl, chunk_bytes=chunk_bytes)
        for (x0, y0), got in zip(zl, oz):
            assert got.shape == (nz,) and np.max(np.abs(got - want[x0, y0, :])) <= 1e-12 * rms
        for (x0, z0), got in zip(yl, oy):
            assert got.shape == (ny,) and np.max(np.abs(got - want[x0, :, z0])) <= 1e-12 * rms
        for (y0, z0), got in zip(xl, ox):
            assert got.shape == (nx,) and np.max(np.abs(got - want[:, y0, z0])) <= 1e-12 * rms
    Kh = np.fft.rfftn(rng.normal(size=shape) + 0.25)
    f = np.fft.irfftn(Kh, s=shape, axes=(0, 1, 2))
    mean, std = partial_dft.parseval_moments(Kh, chunk_bytes=chunk_bytes)
    assert abs(mean - f.mean()) <= 1e-12 * f.std() and abs(std - f.std()) <= 1e-12 * f.std()
