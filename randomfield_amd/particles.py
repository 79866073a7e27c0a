"""Cloud-in-cell painting of displaced lattice particles in numpy: the numpy backend of ``Generator.paint_particles`` and the
definition the device kernels (csrc/rf_core.h ``cic_axis``) follow.

One particle of unit mass per lattice cell q = (ix, iy, iz) with displacement s_a(q).  Per axis, in float64: u = s_a * inv_h[a] (one
rounded product), c = floor(u), t = floor((u - c) * 65536); the integer weights 65536 - t and t go to the cells j0 = (i_a + c) mod n_a
(formed in float64) and j1 = (j0 + 1) mod n_a.  The eight products of three weights sum to 2**48 per particle and are added to a
``uint64`` grid, so the result does not depend on the order of the additions.  Particles with a non-finite u on any axis are dropped and
counted.  Fewer than 65536 particles' worth of mass may land in one cell.

``order=3`` is the triangular-shaped cloud (csrc/rf_core.h ``tsc_axis``) over the same u, c, t and j0: up = t >= 32768,
tau = t - 32768 if up else t + 32768, the centre cell jc = (j0 + 1) mod n if up else j0, and the integer weights
Wm = (65536 - tau)**2 >> 17, Wp = tau**2 >> 17, W0 = 65536 - Wm - Wp on the cells jc - 1, jc, jc + 1 (mod n): 27 products per particle,
still 2**48 in all.  The gather reduces three values at a time, (wm vm + w0 v0) + wp vp, along z, then y, then x."""
import numpy as np

WEIGHT_ONE = 1 << 48


def _axis(s, inv_h, axis, half=False):
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
    if half:        # the particle at u + 1/2, in integers: t + 32768 with its carry into the WRAPPED index (never through c)
        t2 = t + np.uint64(32768)
        carry = t2 >= np.uint64(65536)
        t = np.where(carry, t2 - np.uint64(65536), t2)
        j0 = np.where(carry, (j0 + 1) % n, j0)
    return ok, (j0, (j0 + 1) % n), (np.uint64(65536) - t, t)


def _axis_tsc(s, inv_h, axis, half=False):
    """the three cells and weights of the triangular-shaped cloud from the cloud-in-cell terms of the same axis"""
    n = s.shape[axis]
    ok, (j0, j1), (_, t) = _axis(s, inv_h, axis, half)
    up = t >= np.uint64(32768)
    tau = np.where(up, t - np.uint64(32768), t + np.uint64(32768))
    jc = np.where(up, j1, j0)
    wm = ((np.uint64(65536) - tau) ** 2) >> np.uint64(17)
    wp = (tau ** 2) >> np.uint64(17)
    return ok, ((jc - 1) % n, jc, (jc + 1) % n), (wm, np.uint64(65536) - wm - wp, wp)


def _terms(s, inv_h, order, half=False):
    if order not in (2, 3):
        raise ValueError("Invalid order: {0!r} (expected 2, cloud in cell, or 3, triangular-shaped cloud).".format(order))
    axis = _axis if order == 2 else _axis_tsc
    return [axis(s[a], inv_h[a], a, half) for a in range(3)]


def paint_counts(displacements, inv_h, order=2, half_cell=False):
    """``(A, dropped)``: the uint64 accumulator grid of the particles displaced by ``displacements`` (3, nx, ny, nz) and the number
    of dropped particles.  ``order``: 2 cloud in cell, 3 triangular-shaped cloud.  ``half_cell``: the particles at u + 1/2 on every
    axis -- the second grid of an interlaced paint (csrc/rf_core.h ``cic_axis_half``): per axis t2 = t + 32768, carry = t2 >= 65536,
    t' = t2 - 65536 if carry else t2, j0' = (j0 + 1) mod n if carry else j0; the triangular-shaped cloud takes (t', j0') in place of
    (t, j0).  Particles are dropped by u, before the shift."""
    s = np.asarray(displacements)
    shape = s.shape[1:]
    terms = _terms(s, inv_h, order, bool(half_cell))
    ok = terms[0][0] & terms[1][0] & terms[2][0]
    A = np.zeros(int(np.prod(shape)), np.uint64)
    if order == 3:
        for cx in range(3):
            for cy in range(3):
                for cz in range(3):
                    w = np.broadcast_to(terms[0][2][cx] * terms[1][2][cy] * terms[2][2][cz], shape)
                    cell = np.broadcast_to((terms[0][1][cx] * shape[1] + terms[1][1][cy]) * shape[2] + terms[2][1][cz], shape)
                    np.add.at(A, cell[ok], w[ok])
        return A.reshape(shape), int(ok.size - np.count_nonzero(ok))
    for k in range(8):
        bits = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
        w = terms[0][2][bits[0]] * terms[1][2][bits[1]] * terms[2][2][bits[2]]
        cell = (terms[0][1][bits[0]] * shape[1] + terms[1][1][bits[1]]) * shape[2] + terms[2][1][bits[2]]
        np.add.at(A, cell[ok], w[ok])
    return A.reshape(shape), int(ok.size - np.count_nonzero(ok))


def gather(displacements, inv_h, field, coeff=1.0, first=True, out=None, order=2):
    """``(out, dropped)``: the cloud-in-cell interpolation of ``field`` (nx, ny, nz) at the particles displaced by ``displacements``
    (3, nx, ny, nz), the adjoint of :func:`paint_counts` over the same indices and integer weights.  In float64, every product and
    sum rounded on its own: along z first, a = wz0 v0 + wz1 v1, then y, then x, the result scaled by 2**-48;
    ``out[q] = coeff * g`` (``first``) or ``out[q] + coeff * g``, rounded once to the field's type.  Zero weights are not skipped
    (a non-finite field value reaches every particle whose eight cells contain it); a dropped particle gathers 0: ``first`` writes
    0, otherwise ``out[q]`` stays.  ``order=3``: the triangular-shaped cloud's three cells and weights per axis, reduced as
    (wm vm + w0 v0) + wp vp in the same order of axes."""
    s = np.asarray(displacements)
    field = np.asarray(field)
    shape = s.shape[1:]
    terms = _terms(s, inv_h, order)
    ok = terms[0][0] & terms[1][0] & terms[2][0]
    (jx, jy, jz), (wx, wy, wz) = [t[1] for t in terms], [[w.astype(np.float64) for w in t[2]] for t in terms]
    flat = field.ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        def lerp(w, v):
            r = w[0] * v[0] + w[1] * v[1]
            return r if order == 2 else r + w[2] * v[2]
        b = []
        for cx in range(order):
            a = []
            for cy in range(order):
                row = (jx[cx] * shape[1] + jy[cy]) * shape[2]
                a.append(lerp(wz, [flat[row + jz[cz]].astype(np.float64) for cz in range(order)]))
            b.append(lerp(wy, a))
        g = lerp(wx, b) * 2.0 ** -48
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
