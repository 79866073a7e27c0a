"""Cloud-in-cell painting of displaced lattice particles in numpy: the numpy backend of ``Generator.paint_particles`` and the
definition the device kernels (csrc/rf_core.h ``cic_axis``) follow.

One particle of unit mass per lattice cell q = (ix, iy, iz) with displacement s_a(q).  Per axis, in float64: u = s_a * inv_h[a] (one
rounded product), c = floor(u), t = floor((u - c) * 65536); the integer weights 65536 - t and t go to the cells j0 = (i_a + c) mod n_a
(formed in float64) and j1 = (j0 + 1) mod n_a.  The eight products of three weights sum to 2**48 per particle and are added to a
``uint64`` grid, so the result does not depend on the order of the additions.  Particles with a non-finite u on any axis are dropped and
counted.  Fewer than 65536 particles' worth of mass may land in one cell."""
import numpy as np

WEIGHT_ONE = 1 << 48


def _axis(s, inv_h, axis):
    n = s.shape[axis]
    u = np.asarray(s, np.float64) * np.float64(inv_h)
    ok = np.isfinite(u)
    u = np.where(ok, u, 0.0)
    c = np.floor(u)
    t = np.floor((u - c) * 65536.0).astype(np.uint64)
    i = np.arange(n, dtype=np.float64).reshape([-1 if a == axis else 1 for a in range(3)])
    r = i + np.fmod(c, float(n))
    r = np.where(r < 0, r + n, r)
    r = np.where(r >= n, r - n, r)
    j0 = r.astype(np.int64)
    return ok, (j0, (j0 + 1) % n), (np.uint64(65536) - t, t)


def paint_counts(displacements, inv_h):
    """``(A, dropped)``: the uint64 accumulator grid of the particles displaced by ``displacements`` (3, nx, ny, nz) and the number
    of dropped particles."""
    s = np.asarray(displacements)
    shape = s.shape[1:]
    terms = [_axis(s[a], inv_h[a], a) for a in range(3)]
    ok = terms[0][0] & terms[1][0] & terms[2][0]
    A = np.zeros(int(np.prod(shape)), np.uint64)
    for k in range(8):
        bits = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
        w = terms[0][2][bits[0]] * terms[1][2][bits[1]] * terms[2][2][bits[2]]
        cell = (terms[0][1][bits[0]] * shape[1] + terms[1][1][bits[1]]) * shape[2] + terms[2][1][bits[2]]
        np.add.at(A, cell[ok], w[ok])
    return A.reshape(shape), int(ok.size - np.count_nonzero(ok))


def gather(displacements, inv_h, field, coeff=1.0, first=True, out=None):
    """``(out, dropped)``: the cloud-in-cell interpolation of ``field`` (nx, ny, nz) at the particles displaced by ``displacements``
    (3, nx, ny, nz), the adjoint of :func:`paint_counts` over the same indices and integer weights.  In float64, every product and
    sum rounded on its own: along z first, a = wz0 v0 + wz1 v1, then y, then x, the result scaled by 2**-48;
    ``out[q] = coeff * g`` (``first``) or ``out[q] + coeff * g``, rounded once to the field's type.  Zero weights are not skipped
    (a non-finite field value reaches every particle whose eight cells contain it); a dropped particle gathers 0: ``first`` writes
    0, otherwise ``out[q]`` stays."""
    s = np.asarray(displacements)
    field = np.asarray(field)
    shape = s.shape[1:]
    terms = [_axis(s[a], inv_h[a], a) for a in range(3)]
    ok = terms[0][0] & terms[1][0] & terms[2][0]
    (jx, jy, jz), (wx, wy, wz) = [t[1] for t in terms], [[w.astype(np.float64) for w in t[2]] for t in terms]
    flat = field.ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        b = []
        for cx in (0, 1):
            a = []
            for cy in (0, 1):
                row = (jx[cx] * shape[1] + jy[cy]) * shape[2]
                v0, v1 = flat[row + jz[0]].astype(np.float64), flat[row + jz[1]].astype(np.float64)
                a.append(wz[0] * v0 + wz[1] * v1)
            b.append(wy[0] * a[0] + wy[1] * a[1])
        g = (wx[0] * b[0] + wx[1] * b[1]) * 2.0 ** -48
        term = np.float64(coeff) * g
        if out is None:
            out = np.zeros(shape, field.dtype)
        if first:
            out[...] = np.where(ok, term, 0.0).astype(field.dtype)
        else:
            out[...] = np.where(ok, (out.astype(np.float64) + term).astype(field.dtype), out)
    return out, int(ok.size - np.count_nonzero(ok))


def counts_to_delta(A, dtype):
    """delta = A * 2**-48 - 1 in float64, rounded once to ``dtype``"""
    return (A.astype(np.float64) * (1.0 / WEIGHT_ONE) - 1.0).astype(dtype)
