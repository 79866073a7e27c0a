"""Float64 numpy restatement of the second-order (2LPT) definitions of DESIGN.md section 3.14 -- test tooling, shared by
tests/test_emulator_lpt2.py and tests/test_gpu_lpt2.py.

    m_a          signed mode number along axis a, 0 at index 0 and at the axis' own Nyquist index (rf_core.h grad_mode)
    D_a          multiply by i dk_a m_a
    H_ab(k)      D_a D_b phi(k) = -scale (dk_a m_a)(dk_b m_b) phi(k), the Nyquist planes dropped on the diagonal too
    S(x)         sum over a < b of H_aa H_bb - H_ab^2 (scale = 1)
    phi2(k)      rfftn(S)(k) / k^2, 0 at DC, k^2 = (kx2 + ky2) + kz2 from the plan's tables
    psi2_a(x)    (3/7) irfftn(i dk_a m_a phi2(k))
"""
import numpy as np

PAIRS = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]            # the order of the device's sweep


def dk_of(shape, spacing):
    return [2 * np.pi / (n * spacing) for n in shape]


def modes(shape, axis):
    """signed mode numbers of the half spectrum along `axis`, broadcastable, the Nyquist entry 0"""
    n = shape[axis]
    m = np.arange(shape[2] // 2 + 1, dtype=np.float64) if axis == 2 else np.fft.fftfreq(n, 1.0 / n)
    m = np.array(m, np.float64)
    m[n // 2] = 0.0
    return m.reshape([-1 if a == axis else 1 for a in range(3)])


def ksq_grid(shape, spacing):
    from randomfield_amd import powertools
    kx2, ky2, kz2 = (np.asarray(a, np.float64) for a in powertools.ksq_axes(*shape, spacing))
    return (kx2[:, None, None] + ky2[None, :, None]) + kz2[None, None, :]


def hessian_factor(shape, spacing, a, b, scale=1.0):
    """the real factor of H_ab, float64, broadcast to the half spectrum's shape"""
    dk = dk_of(shape, spacing)
    f = -scale * dk[a] * dk[b] * (modes(shape, a) * modes(shape, b))
    return np.broadcast_to(f, (shape[0], shape[1], shape[2] // 2 + 1))


def hessian_k(src, shape, spacing, a, b, scale=1.0, divide=False):
    """H_ab(k) from phi(k), or with divide from delta(k); exact zeros where m_a m_b = 0"""
    f = np.array(hessian_factor(shape, spacing, a, b, scale))
    if divide:
        k2 = ksq_grid(shape, spacing)
        k2[0, 0, 0] = 1.0
        f = f / k2
    return f * np.asarray(src, np.complex128)


def irfftn(k, shape):
    return np.fft.irfftn(k, s=shape, axes=(0, 1, 2))


def rfftn(x):
    return np.fft.rfftn(np.asarray(x, np.float64), axes=(0, 1, 2))


def hessian_fields(phi_k, shape, spacing):
    """{(a, b): H_ab(x)} with scale = 1"""
    return {ab: irfftn(hessian_k(phi_k, shape, spacing, *ab), shape) for ab in PAIRS}


def source_from(H):
    return (H[0, 0] * H[1, 1] - H[0, 1] ** 2) + (H[0, 0] * H[2, 2] - H[0, 2] ** 2) + (H[1, 1] * H[2, 2] - H[1, 2] ** 2)


def source(phi_k, shape, spacing):
    return source_from(hessian_fields(phi_k, shape, spacing))


def source_magnitude(H):
    """A(x) = sum of the absolute values of the six products S is made of"""
    return (np.abs(H[0, 0] * H[1, 1]) + np.abs(H[0, 0] * H[2, 2]) + np.abs(H[1, 1] * H[2, 2])
            + H[0, 1] ** 2 + H[0, 2] ** 2 + H[1, 2] ** 2)


def potential2(S, shape, spacing):
    k2 = ksq_grid(shape, spacing)
    k2[0, 0, 0] = 1.0
    out = rfftn(S) / k2
    out[0, 0, 0] = 0.0
    return out


def displacement2_from_source(S, shape, spacing, axis, scale=1.0):
    """(3/7) scale^2 psi2_axis(x) from a given source field"""
    dk = dk_of(shape, spacing)
    return irfftn(1j * (3.0 / 7.0) * scale ** 2 * dk[axis] * modes(shape, axis) * potential2(S, shape, spacing), shape)


def displacement2(phi_k, shape, spacing, axis, scale=1.0):
    return displacement2_from_source(source(phi_k, shape, spacing), shape, spacing, axis, scale)


def dropped_ksq(shape, spacing):
    """sum over a of (dk_a m_a)^2: k^2 with every axis' Nyquist plane dropped"""
    dk = dk_of(shape, spacing)
    return sum((dk[a] * modes(shape, a)) ** 2 for a in range(3))


def divergence(psi, shape, spacing):
    """sum_a D_a psi_a of three real fields"""
    dk = dk_of(shape, spacing)
    return sum(irfftn(1j * dk[a] * modes(shape, a) * rfftn(psi[a]), shape) for a in range(3))


def two_wave_potential(shape, spacing, A, B, mx, my, px=0.0, py=0.0):
    """phi(k) of phi(x) = A cos(k1 x + px) + B cos(k2 y + py), k1 = dk_x mx, k2 = dk_y my (0 < mx < nx/2, 0 < my < ny/2), and the closed
    form S = A B k1^2 k2^2 cos(k1 x + px) cos(k2 y + py).  (Phases keep the cosines away from exact zeros on the grid, where a bound
    that is linear in the components' errors has nothing to hold on to.)"""
    nx, ny, nz = shape
    dk = dk_of(shape, spacing)
    x = np.arange(nx)[:, None, None] * spacing
    y = np.arange(ny)[None, :, None] * spacing
    k1, k2 = dk[0] * mx, dk[1] * my
    phi = A * np.cos(k1 * x + px) + B * np.cos(k2 * y + py) + np.zeros(shape)
    S = A * B * k1 ** 2 * k2 ** 2 * np.cos(k1 * x + px) * np.cos(k2 * y + py) + np.zeros(shape)
    return rfftn(phi), S


def oblique_wave_potential(shape, spacing, A, m):
    """phi(k) of one plane wave A cos(k . x + 0.3), k = (dk_x m[0], dk_y m[1], dk_z m[2]) away from the Nyquist planes: S = 0"""
    dk = dk_of(shape, spacing)
    g = np.meshgrid(*[np.arange(n) * spacing for n in shape], indexing="ij")
    return rfftn(A * np.cos(sum(dk[a] * m[a] * g[a] for a in range(3)) + 0.3))
