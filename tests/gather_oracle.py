"""The definition of the cloud-in-cell gather restated for the tests in numpy float64, over the per-axis terms
of tests/cic_oracle.py.  It shares nothing with the package's numpy backend (randomfield_amd/particles.py), the emulator or the kernels.

For the particle of lattice cell q, with the indices j0 / j1 and the integer weights w0 / w1 (w0 + w1 = 65536) of cic_oracle.axis_terms
per axis and W the field, all in float64, every product and every sum one IEEE operation of its own:
    v(cx,cy,cz) = W[jx_cx, jy_cy, jz_cz]
    a(cx,cy)    = wz0 * v(cx,cy,0) + wz1 * v(cx,cy,1)
    b(cx)       = wy0 * a(cx,0) + wy1 * a(cx,1)
    g           = (wx0 * b(0) + wx1 * b(1)) * 2^-48
    out         = T(coeff * g)  (first)   or   T(float64(G[q]) + coeff * g)
Zero weights are not skipped.  A particle with a non-finite u on some axis gathers g = 0: `first` writes 0, otherwise G[q] stays."""
import numpy as np

import cic_oracle

SCALE = 2.0 ** -48


def gather_g(s3, inv_h, W):
    """(g float64 of the grid's shape -- 0 where the particle is dropped --, finite mask)"""
    s3 = [np.asarray(s) for s in s3]
    W = np.asarray(W)
    shape = W.shape
    finite, idx, wts = [], [], []
    for a in range(3):
        f, j, w = cic_oracle.axis_terms(s3[a], inv_h[a], a)
        finite.append(f)
        idx.append([np.broadcast_to(v, shape) for v in j])
        wts.append([np.broadcast_to(v, shape).astype(np.float64) for v in w])
    ok = finite[0] & finite[1] & finite[2]

    def v(cx, cy, cz):
        return W[idx[0][cx], idx[1][cy], idx[2][cz]].astype(np.float64)

    with np.errstate(invalid="ignore", over="ignore"):
        b = [None, None]
        for cx in (0, 1):
            a = [None, None]
            for cy in (0, 1):
                p0 = wts[2][0] * v(cx, cy, 0)
                p1 = wts[2][1] * v(cx, cy, 1)
                a[cy] = p0 + p1
            q0 = wts[1][0] * a[0]
            q1 = wts[1][1] * a[1]
            b[cx] = q0 + q1
        r0 = wts[0][0] * b[0]
        r1 = wts[0][1] * b[1]
        g = (r0 + r1) * SCALE
    return np.where(ok, g, 0.0), ok


def gather(s3, inv_h, W, coeff=1.0, first=True, G=None):
    """(the new G, a new array of W's type; the number of dropped particles)"""
    W = np.asarray(W)
    g, ok = gather_g(s3, inv_h, W)
    with np.errstate(invalid="ignore", over="ignore"):
        term = np.float64(coeff) * g
        if first:
            out = np.where(ok, term, 0.0).astype(W.dtype)
        else:
            G = np.asarray(G)
            assert G.dtype == W.dtype and G.shape == W.shape
            out = np.where(ok, (G.astype(np.float64) + term).astype(W.dtype), G)
    return out, int(ok.size - np.count_nonzero(ok))


def adjoint_sums(s3, inv_h, W):
    """(sum over the particles of g 2^48, sum over the cells of A W) in Python integers, for an integer-valued field W; the second from
    cic_oracle.paint.  Every |g 2^48| must stay below 2^53 for the first to be exact (asserted)."""
    g, ok = gather_g(s3, inv_h, W)
    scaled = g * 2.0 ** 48
    assert np.all(np.abs(scaled) < 2.0 ** 53) and np.all(scaled == np.floor(scaled))
    A, _ = cic_oracle.paint(s3, inv_h)
    lhs = sum(int(x) for x in scaled.ravel())
    rhs = sum(int(a) * int(w) for a, w in zip(A.ravel(), np.asarray(W).ravel()))
    return lhs, rhs
