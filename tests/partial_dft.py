"""Exact lines of ``np.fft.irfftn(K)`` without transforming the whole array (numpy, float64) -- test tooling.

A packed half spectrum K[nx][ny][nz/2+1] too large for a float64 reference transform (1000^3: 10^9 cells) still pins single
lines of its field: contracting two axes with the phase vectors of one position is a sum over the array, and the remaining axis
is one 1-D numpy transform.  With wx[kx] = exp(2 pi i kx x0 / nx) / nx, wy likewise, and the weights of numpy's ``irfft`` along z,
wz[kz] = c_kz exp(2 pi i kz z0 / nz) / nz with c = 1 for the DC and Nyquist bins and 2 in between (the real part taken at the end
drops the imaginary parts of those two bins exactly as ``irfft`` does, and as oracle.cpu_ref.c2r does through ``irfftn``):

    along z at (x0, y0):  irfft(sum_kx,ky wx wy K[kx, ky, :], n=nz)
    along y at (x0, z0):  Re ifft(sum_kx,kz wx wz K[kx, :, kz])             (the 1 / ny of ifft is that axis's own normalisation)
    along x at (y0, z0):  Re ifft(sum_ky,kz wy wz K[:, ky, kz])

The array is walked once, in chunks of x planes whose complex128 copy stays below ``chunk_bytes``; every requested line takes its
share of each chunk.  Also the Parseval sums of the field (mean and population variance) from K alone.
"""
import numpy as np


def _phase(n, pos):
    """exp(2 pi i k pos / n), k = 0 .. n - 1, with the product k * pos reduced mod n in integers (exact arguments)"""
    k = (np.arange(n, dtype=np.int64) * int(pos)) % n
    return np.exp(2j * np.pi * k / n)


def _z_weights(nz, z0):
    """the weights of np.fft.irfft along z at position z0, without its 1 / nz: 1 for kz = 0 and nz / 2, 2 in between"""
    nzh = nz // 2 + 1
    k = (np.arange(nzh, dtype=np.int64) * int(z0)) % nz
    w = 2.0 * np.exp(2j * np.pi * k / nz)
    w[0] = 1.0
    w[nzh - 1] = 1.0 if z0 % 2 == 0 else -1.0
    return w


def field_lines(K, z_lines=(), y_lines=(), x_lines=(), chunk_bytes=1 << 30):
    """Lines of np.fft.irfftn(K, axes=(0, 1, 2)) of a packed half spectrum K (nx, ny, nz/2+1), nz even, any complex dtype.

    z_lines: (x0, y0) pairs -> arrays of nz values;  y_lines: (x0, z0) pairs -> ny values;  x_lines: (y0, z0) pairs -> nx values.
    Returns three lists of float64 arrays in the order asked."""
    nx, ny, nzh = K.shape
    nz = 2 * (nzh - 1)
    accz = [np.zeros(nzh, np.complex128) for _ in z_lines]
    accy = [np.zeros(ny, np.complex128) for _ in y_lines]
    accx = [np.zeros(nx, np.complex128) for _ in x_lines]
    # the z positions both kinds of transverse lines contract with: one matrix product per chunk
    zpos = sorted({z0 for _, z0 in y_lines} | {z0 for _, z0 in x_lines})
    Wz = np.stack([_z_weights(nz, z0) for z0 in zpos], axis=1) if zpos else None           # (nzh, nzpos)
    Pyz = np.stack([_phase(ny, y0) for _, y0 in z_lines], axis=0) if z_lines else None       # (nlines, ny)
    planes = max(1, int(chunk_bytes // (16 * ny * nzh)))
    for a in range(0, nx, planes):
        b = min(nx, a + planes)
        Kc = K[a:b].astype(np.complex128)
        if z_lines:
            px = [_phase(nx, x0)[a:b] for x0, _ in z_lines]
            for i in range(b - a):
                t = Pyz @ Kc[i]                                      # (nlines, nzh)
                for j in range(len(z_lines)):
                    accz[j] += px[j][i] * t[j]
        if zpos:
            A = (Kc.reshape(-1, nzh) @ Wz).reshape(b - a, ny, len(zpos))          # z contracted: (planes, ny, nzpos)
            for j, (x0, z0) in enumerate(y_lines):
                accy[j] += _phase(nx, x0)[a:b] @ A[:, :, zpos.index(z0)]
            for j, (y0, z0) in enumerate(x_lines):
                accx[j][a:b] = A[:, :, zpos.index(z0)] @ _phase(ny, y0)
        del Kc
    norm_xy = 1.0 / (nx * ny)
    outz = [np.fft.irfft(c * norm_xy, n=nz) for c in accz]
    outy = [np.fft.ifft(c).real / (nx * nz) for c in accy]
    outx = [np.fft.ifft(c).real / (ny * nz) for c in accx]
    return outz, outy, outx


def parseval_moments(K, chunk_bytes=1 << 30):
    """(mean, population std) of np.fft.irfftn(K) from K alone, in float64: the mean is Re K[0, 0, 0] / N and
    sum f^2 = (1 / N) sum_k c_kz |K_k|^2 with c = 1 on the kz = 0 and nz / 2 planes and 2 in between.  The two planes must be
    Hermitian in (kx, ky) for the identity to hold (irfftn drops what is not)."""
    nx, ny, nzh = K.shape
    nz = 2 * (nzh - 1)
    n3 = float(nx) * ny * nz
    c = np.full(nzh, 2.0)
    c[0] = c[nzh - 1] = 1.0
    total = 0.0
    planes = max(1, int(chunk_bytes // (16 * ny * nzh)))
    for a in range(0, nx, planes):
        Kc = K[a:a + planes].astype(np.complex128)
        total += float(np.dot((Kc.real ** 2 + Kc.imag ** 2).reshape(-1, nzh).sum(axis=0), c))
    mean = float(K[0, 0, 0].real) / n3
    var = total / (n3 * n3) - mean * mean
    return mean, float(np.sqrt(var))
