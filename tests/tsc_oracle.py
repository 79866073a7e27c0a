"""The definitions of the triangular-shaped-cloud paint and gather restated for the tests: numpy float64 for
the per-axis terms, uint64 / Python integers for the weights, float64 with every product and sum on its own for the gather.  It
shares nothing with the package's numpy backend (randomfield_amd/particles.py), the emulator or the kernels; from tests/cic_oracle.py
it takes only the displacement sets, the unit of mass and the integer sum.

Per axis of a particle at lattice index i with displacement s, inv_h = 1 / spacing:
    u = s * inv_h (one rounded float64 product), dropped if not finite;  c = floor(u);  t = floor((u - c) * 65536) in [0, 65536];
    j0 = (i + c) mod n, formed in float64;
    up = t >= 32768;  tau = t - 32768 if up else t + 32768;  jc = (j0 + 1) mod n if up else j0;
    cells jm = (jc - 1) mod n, jc, jp = (jc + 1) mod n;  Wm = (65536 - tau)^2 >> 17,  Wp = tau^2 >> 17,  W0 = 65536 - Wm - Wp.
Paint: the 27 products go to a uint64 grid.  Gather: lerp3(w, v) = (wm vm + w0 v0) + wp vp along z, then y, then x, times 2^-48."""
import math

import numpy as np

from cic_oracle import ONE, displacement_sets, total  # noqa: F401  (re-exported for the tests)


def weights(t):
    """(Wm, W0, Wp) of one t in [0, 65536], Python integers"""
    tau = t - 32768 if t >= 32768 else t + 32768
    wm = ((65536 - tau) ** 2) >> 17
    wp = (tau ** 2) >> 17
    return wm, 65536 - wm - wp, wp


def axis_terms(s, inv_h, axis):
    """(finite, [jm, jc, jp], [Wm, W0, Wp], c_lo) of one component; indices int64, weights uint64, c_lo float64"""
    s = np.asarray(s)
    n = s.shape[axis]
    with np.errstate(over="ignore"):
        u = s.astype(np.float64) * np.float64(inv_h)
    finite = np.isfinite(u)
    u = np.where(finite, u, 0.0)
    c = np.floor(u)
    t = np.floor((u - c) * 65536.0).astype(np.int64)
    assert t.min() >= 0 and t.max() <= 65536
    shape = [1, 1, 1]
    shape[axis] = n
    i = np.arange(n, dtype=np.float64).reshape(shape)
    r = i + np.fmod(c, np.float64(n))
    r = np.where(r < 0, r + n, r)
    r = np.where(r >= n, r - n, r)
    assert np.all((r >= 0) & (r < n) & (r == np.floor(r)))
    j0 = r.astype(np.int64)
    up = t >= 32768
    tau = np.where(up, t - 32768, t + 32768)
    assert tau.min() >= 0 and tau.max() <= 65535
    jc = np.where(up, (j0 + 1) % n, j0)
    wm = ((65536 - tau) ** 2) >> 17
    wp = (tau ** 2) >> 17
    w0 = 65536 - wm - wp
    assert wm.min() >= 0 and w0.min() >= 0 and wp.min() >= 0
    return finite, [(jc - 1) % n, jc, (jc + 1) % n], [w.astype(np.uint64) for w in (wm, w0, wp)], c + up - 1.0


def paint(s3, inv_h):
    """A (uint64, the grid's shape) and the number of dropped particles"""
    s3 = [np.asarray(s) for s in s3]
    nx, ny, nz = s3[0].shape
    terms = [axis_terms(s3[a], inv_h[a], a) for a in range(3)]
    keep = terms[0][0] & terms[1][0] & terms[2][0]
    A = np.zeros(nx * ny * nz, np.uint64)
    for cx in range(3):
        for cy in range(3):
            for cz in range(3):
                w = terms[0][2][cx] * terms[1][2][cy] * terms[2][2][cz]
                cell = (terms[0][1][cx] * ny + terms[1][1][cy]) * nz + terms[2][1][cz]
                w, cell = np.broadcast_to(w, keep.shape), np.broadcast_to(cell, keep.shape)
                np.add.at(A, cell[keep], w[keep])
    return A.reshape(nx, ny, nz), int(keep.size - np.count_nonzero(keep))


def delta(A, real_dtype):
    """(double)A * 2^-48 - 1 rounded once to the real type"""
    return (np.asarray(A).astype(np.float64) * 2.0 ** -48 - 1.0).astype(real_dtype)


def _lerp3(w, v):
    return (w[0] * v[0] + w[1] * v[1]) + w[2] * v[2]


def gather_g(s3, inv_h, W):
    """(g, finite): the float64 value before coeff and the rounding to the field's type"""
    s3 = [np.asarray(s) for s in s3]
    W = np.asarray(W)
    nx, ny, nz = W.shape
    terms = [axis_terms(s3[a], inv_h[a], a) for a in range(3)]
    keep = terms[0][0] & terms[1][0] & terms[2][0]
    (jx, jy, jz) = [t[1] for t in terms]
    (wx, wy, wz) = [[w.astype(np.float64) for w in t[2]] for t in terms]
    flat = W.ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        b = []
        for cx in range(3):
            a = []
            for cy in range(3):
                row = (jx[cx] * ny + jy[cy]) * nz
                a.append(_lerp3(wz, [flat[row + jz[cz]].astype(np.float64) for cz in range(3)]))
            b.append(_lerp3(wy, a))
        g = _lerp3(wx, b) * 2.0 ** -48
    return g, keep


def gather(s3, inv_h, W, coeff=1.0, first=True, G=None):
    """(G, dropped): G = (T)(coeff g) (first) or (T)((double)G + coeff g); a dropped particle writes 0 (first) or leaves G"""
    W = np.asarray(W)
    g, keep = gather_g(s3, inv_h, W)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.float64(coeff) * g
        if first:
            out = np.where(keep, p, 0.0).astype(W.dtype)
        else:
            G = np.asarray(G)
            out = np.where(keep, (G.astype(np.float64) + p).astype(W.dtype), G).astype(W.dtype)
    return out, int(keep.size - np.count_nonzero(keep))


def adjoint_sums(s3, inv_h, Wint):
    """(sum_q g 2^48, sum_cells A W) in Python integers, for an integer-valued field"""
    g, keep = gather_g(s3, inv_h, np.asarray(Wint, np.float64))
    scaled = np.where(keep, g, 0.0) * 2.0 ** 48
    assert np.all(scaled == np.floor(scaled))
    A, _ = paint(s3, inv_h)
    return sum(int(v) for v in scaled.ravel()), sum(int(a) * int(w) for a, w in zip(A.ravel(), np.asarray(Wint).ravel()))


def one_particle(shape, q, s, inv_h):
    """{cell: weight} of a single particle at lattice cell q displaced by s, in Python numbers alone"""
    per_axis = []
    for a in range(3):
        u = float(s[a]) * float(inv_h[a])
        c = math.floor(u)
        t = math.floor((u - c) * 65536.0)
        jc = (q[a] + c + (1 if t >= 32768 else 0)) % shape[a]
        per_axis.append([((jc + d) % shape[a], w) for d, w in zip((-1, 0, 1), weights(t))])
    cells = {}
    for jx, wx in per_axis[0]:
        for jy, wy in per_axis[1]:
            for jz, wz in per_axis[2]:
                if wx * wy * wz:
                    cells[jx, jy, jz] = cells.get((jx, jy, jz), 0) + wx * wy * wz
    return cells


def stays_in_tile(s3, inv_h, brick, halo):
    """boolean mask: the particles whose 27 cells all fall inside their brick's tile (the tile rule with P = 3)"""
    s3 = [np.asarray(s) for s in s3]
    shape = s3[0].shape
    stay = np.ones(shape, bool)
    for a in range(3):
        clo = axis_terms(s3[a], inv_h[a], a)[3]
        l = (np.arange(shape[a]) % brick[a]).reshape([-1 if c == a else 1 for c in range(3)])
        lo = l + clo
        stay &= (lo >= -halo) & (lo <= brick[a] + halo - 3)
    return stay


def extra_sets(shape, spacing, seed=23):
    """the displacement sets beyond cic_oracle's: the edges of the TSC rule"""
    rng = np.random.RandomState(seed)
    sets = {}
    sets["half"] = np.full((3,) + shape, 0.5 * spacing)                 # tau = 0: weights 1/2, 1/2, 0
    sets["tiny_minus"] = np.full((3,) + shape, -(2.0 ** -60) * spacing)  # t = 65536
    sets["uniform"] = rng.uniform(-0.5, 0.5, size=(3,) + shape) * spacing
    sets["rms0.6"] = rng.normal(scale=0.6, size=(3,) + shape) * spacing  # straddles `up`
    sets["rms7"] = rng.normal(scale=7.0, size=(3,) + shape) * spacing    # most particles leave the tile
    huge = rng.normal(scale=0.6, size=(3,) + shape) * spacing
    huge[(0,) + tuple(n // 2 for n in shape)] = 1e30
    sets["huge"] = huge
    return sets
