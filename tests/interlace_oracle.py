"""The definitions of the interlaced paint restated for the tests.  It shares nothing with the package's numpy
backend (randomfield_amd/particles.py, powertools.py), the emulator or the kernels; from tests/cic_oracle.py and tests/tsc_oracle.py it
takes the unshifted per-axis terms, the weights of the triangular-shaped cloud and the displacement sets.

Shifted paint, per axis, on top of cic_oracle.axis_terms (finite, j0, j1, t), all in integers:
    t2 = t + 32768;  carry = t2 >= 65536;  t' = t2 - 65536 if carry else t2;  j0' = j1 if carry else j0;  j1' = (j0' + 1) mod n
    cloud in cell: w0' = 65536 - t' on j0', w1' = t' on j1';  triangular-shaped cloud: tsc_oracle's rule on (t', j0').
Combine, per cell, in float64 on REAL arrays, one numpy operation per rounding (numpy's complex product may contract):
    a = px py (ar = xr yr - xi yi, ai = xr yi + xi yr);  p = a pz;  q = p K;  out = (T)(0.5 (S + q)) per component.
Default tables: p_a[i] = cos(pi m / n) + i sin(pi m / n), m the signed mode number; p_a[0] = 1, p_a[n / 2] = 0."""
import math

import numpy as np

import cic_oracle as corc
import tsc_oracle as torc
from cic_oracle import ONE, total  # noqa: F401  (re-exported for the tests)

CIC, TSC = 2, 3


def shift_axis(t, j0, n):
    """(t', j0', carry) of one axis in Python integers"""
    t2 = t + 32768
    carry = t2 >= 65536
    return (t2 - 65536 if carry else t2), ((j0 + 1) % n if carry else j0), carry


def axis_terms(s, inv_h, axis):
    """(finite, j0', t') of one component after the shift: int64 arrays, every step an exact integer operation"""
    n = np.asarray(s).shape[axis]
    finite, (j0, j1), (_, t) = corc.axis_terms(s, inv_h, axis)
    t2 = t.astype(np.int64) + 32768
    carry = t2 >= 65536
    t1 = np.where(carry, t2 - 65536, t2)
    assert t1.min() >= 0 and t1.max() <= 65535
    return finite, np.where(carry, j1, j0), t1


def paint(s3, inv_h, scheme=CIC):
    """A (uint64, the grid's shape) of the SHIFTED paint and the number of dropped particles (decided on u, before the shift)"""
    s3 = [np.asarray(s) for s in s3]
    shape = s3[0].shape
    cells, weights, keep = [], [], np.ones(shape, bool)
    for a in range(3):
        n = shape[a]
        finite, j0, t = axis_terms(s3[a], inv_h[a], a)
        keep = keep & finite
        if scheme == CIC:
            cells.append([j0, (j0 + 1) % n])
            weights.append([(65536 - t).astype(np.uint64), t.astype(np.uint64)])
        else:
            up = t >= 32768
            tau = np.where(up, t - 32768, t + 32768)
            jc = np.where(up, (j0 + 1) % n, j0)
            wm, wp = ((65536 - tau) ** 2) >> 17, (tau ** 2) >> 17
            cells.append([(jc - 1) % n, jc, (jc + 1) % n])
            weights.append([w.astype(np.uint64) for w in (wm, 65536 - wm - wp, wp)])
    A = np.zeros(int(np.prod(shape)), np.uint64)
    for cx in range(scheme):
        for cy in range(scheme):
            for cz in range(scheme):
                w = np.broadcast_to(weights[0][cx] * weights[1][cy] * weights[2][cz], shape)
                cell = np.broadcast_to((cells[0][cx] * shape[1] + cells[1][cy]) * shape[2] + cells[2][cz], shape)
                np.add.at(A, cell[keep], w[keep])
    return A.reshape(shape), int(keep.size - np.count_nonzero(keep))


def unshifted(s3, inv_h, scheme=CIC):
    return corc.paint(s3, inv_h) if scheme == CIC else torc.paint(s3, inv_h)


def delta(A, real_dtype):
    return corc.delta(A, real_dtype)


def one_particle(shape, q, s, inv_h, scheme=CIC):
    """{cell: weight} of a single SHIFTED particle at lattice cell q displaced by s, in Python numbers alone"""
    per_axis = []
    for a in range(3):
        u = float(s[a]) * float(inv_h[a])
        c = math.floor(u)
        t = math.floor((u - c) * 65536.0)
        j0 = int(math.fmod(c, shape[a]) + q[a]) % shape[a]
        t1, j0s, _ = shift_axis(t, j0, shape[a])
        if scheme == CIC:
            per_axis.append([(j0s, 65536 - t1), ((j0s + 1) % shape[a], t1)])
        else:
            jc = (j0s + (1 if t1 >= 32768 else 0)) % shape[a]
            per_axis.append([((jc + d) % shape[a], w) for d, w in zip((-1, 0, 1), torc.weights(t1))])
    cells = {}
    for jx, wx in per_axis[0]:
        for jy, wy in per_axis[1]:
            for jz, wz in per_axis[2]:
                if wx * wy * wz:
                    cells[jx, jy, jz] = cells.get((jx, jy, jz), 0) + wx * wy * wz
    return cells


def phases(shape):
    """the default tables: complex128 arrays of nx, ny, nz/2 + 1 entries"""
    tabs = []
    for n, count in zip(shape, (shape[0], shape[1], shape[2] // 2 + 1)):
        p = np.empty(count, np.complex128)
        for i in range(count):
            m = i if i <= n // 2 else i - n
            p[i] = complex(math.cos(math.pi * m / n), math.sin(math.pi * m / n))
        p[0] = 1.0
        p[n // 2] = 0.0
        tabs.append(p)
    return tabs


def _mul(xr, xi, yr, yi):
    rr = xr * yr
    ii = xi * yi
    ri = xr * yi
    ir = xi * yr
    return rr - ii, ri + ir


def combine(S, K, tables=None):
    """(T)(0.5 (S + p K)) with p = px py pz; tables: None or three complex tables (each may be None = all ones)"""
    S, K = np.asarray(S), np.asarray(K)
    tabs = [None] * 3 if tables is None else list(tables)
    re, im = [], []
    for a, n in enumerate(K.shape):
        t = np.ones(n, np.complex128) if tabs[a] is None else np.asarray(tabs[a], np.complex128)
        assert t.shape == (n,)
        shape = [1, 1, 1]
        shape[a] = n
        re.append(np.array(t.real, np.float64).reshape(shape))
        im.append(np.array(t.imag, np.float64).reshape(shape))
    with np.errstate(invalid="ignore", over="ignore"):
        ar, ai = _mul(re[0], im[0], re[1], im[1])
        pr, pi = _mul(ar, ai, re[2], im[2])
        qr, qi = _mul(pr, pi, np.array(K.real, np.float64), np.array(K.imag, np.float64))
        sr = np.array(S.real, np.float64) + qr
        si = np.array(S.imag, np.float64) + qi
        out = np.empty(K.shape, K.dtype)
        out.real = (0.5 * sr).astype(out.real.dtype)
        out.imag = (0.5 * si).astype(out.imag.dtype)
    return out


def interlaced(s3, inv_h, scheme, real_dtype):
    """(K, field, dropped) of the whole interlaced paint in float64: rfftn of the two deltas as rounded to the real type, the combine
    with the default tables in complex128, irfftn"""
    s3 = [np.asarray(s) for s in s3]
    shape = s3[0].shape
    A1, dropped = unshifted(s3, inv_h, scheme)
    A2, dropped2 = paint(s3, inv_h, scheme)
    assert dropped == dropped2
    K1 = np.fft.rfftn(delta(A1, real_dtype).astype(np.float64), axes=(0, 1, 2))
    K2 = np.fft.rfftn(delta(A2, real_dtype).astype(np.float64), axes=(0, 1, 2))
    K = combine(K1, K2, phases(shape))
    return K, np.fft.irfftn(K, s=shape, axes=(0, 1, 2)), dropped


def lattice_displacements(shape, spacing, seed, cells=5.0):
    """random displacements on the 2^-16-cell lattice within +-cells cells: (3,) + shape, float64 (exact in float32 too)"""
    rng = np.random.RandomState(seed)
    k = rng.randint(-int(cells * 65536), int(cells * 65536) + 1, size=(3,) + tuple(shape))
    return k.astype(np.float64) * (spacing / 65536.0)
