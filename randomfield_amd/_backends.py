"""
The two backends of :class:`randomfield_amd.generate.Generator`, one object each with the same operations.  ``Generator`` checks
arguments and keeps the tables and the public attributes; its backend does everything that touches the field and owns what only it
knows how to hold between calls.  Importing this module does not load the library: ``_hip`` does on first use, which only a
``HipBackend`` makes.
"""
import os
import weakref

import numpy as np

from . import _hip, cosmotools, particles, powertools, random as rf_random, transform


class _Backend(object):
    def __init__(self, gen):
        # (the Generator by weak reference: a cycle would keep a dropped Generator's plan, and its device memory, until the collector runs)
        self._gen, self.plan, self.spacing = weakref.ref(gen), gen.plan_c2r, gen.grid_spacing_Mpc_h
        self.field_on_host = False          # the plan's host buffer holds the current field
        # None, or as the backend holds them: displacements, gathered values, the last interlaced spectrum, the second-order potential
        self.particles = self.gathered = self.interlaced = self.lpt2 = None
        self._unit_sums = {}                # bispectrum: the unit run's sums per (edges, triples), a function of the grid alone

    def unit_sums(self, k_edges, triples, run):
        """the triangle-count sums of a bispectrum measurement: ``run()`` once per (edges, triples), the last few kept"""
        key = (np.asarray(k_edges, np.float64).tobytes(), np.asarray(triples, np.intc).tobytes())
        if key not in self._unit_sums:
            if len(self._unit_sums) >= 8:
                self._unit_sums.pop(next(iter(self._unit_sums)))
            self._unit_sums[key] = run()
        return self._unit_sums[key]

    @property
    def gen(self):
        return self._gen()

    def new_field(self):
        # (displacements belong to the field they were made for or set beside, and so do the values gathered at them)
        self.particles = self.gathered = self.lpt2 = None

    def dk3(self):
        return [2 * np.pi / (n * self.spacing) for n in self.plan.shape]

    def field_to_host(self):
        return self.plan.data_out

    def make_current(self, field):
        self.plan.data_out[...] = field
        self.field_on_host = True


class NumpyBackend(_Backend):
    """The reference's host code on the plan's host buffers.  The field is on the host by nature: ``download`` matters only where
    ``False`` returns None (the gather; the paints through ``download_field``).  Displacements and gathered values are
    ``(3, nx, ny, nz)`` arrays, the interlaced spectrum is a complex128 array, the second-order potential one of the plan's type."""
    fused_density = False

    def __init__(self, gen):
        super(NumpyBackend, self).__init__(gen)
        self._building = None               # the displacements while particle_displacements() sums them

    def realise_delta(self, power, seed, save_potential, download):
        """-> (delta, rms, potential): generate.py:191-219"""
        data = self.plan.data_in
        powertools.fill_with_log10k(data, spacing=self.spacing, packed=True)
        powertools.tabulate_sigmas(data, power=power, spacing=self.spacing, packed=True)
        rf_random.randomize(data, seed=seed)
        transform.symmetrize(data, packed=True)
        potential = None
        if save_potential:
            potential = self.gen.potential if self.gen.potential is not None else np.empty_like(data)
            potential.imag = 0.
            kx2, ky2, kz2 = powertools.create_ksq_grids(potential, spacing=self.spacing, packed=True)
            np.add(kx2, ky2, out=potential.real, casting="same_kind")
            np.add(potential.real, kz2, out=potential.real, casting="same_kind")
            with np.errstate(divide="ignore"):
                np.reciprocal(potential.real, out=potential.real)
            potential[0, 0, 0] = 0.
            potential *= data
        delta = self.plan.execute()
        self.field_on_host = True
        return delta, np.std(delta.reshape(-1)), potential

    def binned_sums(self, k_edges, source, los=None, window=None):
        """the per-bin sums of P(k) (``los`` None) or of its multipoles along ``los``, of the current field or the interlaced spectrum"""
        spectrum = self.interlaced if source == "kspace" else np.fft.rfftn(np.asarray(self.plan.data_out, np.float64), axes=(0, 1, 2))
        if los is None:
            return powertools.bin_power(spectrum, self.spacing, k_edges)
        return powertools.bin_multipoles(spectrum, self.spacing, k_edges, los, window)

    def bispectrum_sums(self, k_edges, triples, source, window=None):
        """-> (the per-bin sums of P(k) on the same edges and spectrum -- compensated with ``window`` --, sum3, sum3 of the unit run)"""
        spectrum = self.interlaced if source == "kspace" else np.fft.rfftn(np.asarray(self.plan.data_out, np.float64), axes=(0, 1, 2))
        if window is None:
            power = powertools.bin_power(spectrum, self.spacing, k_edges)
        else:
            power = powertools.bin_multipoles(spectrum, self.spacing, k_edges, 2, window)[:3]
        amp = None if window is None else [None if t is None else np.sqrt(t) for t in window]
        sum3 = powertools.bin_bispectrum(spectrum, self.spacing, k_edges, triples, amp)
        unit = self.unit_sums(k_edges, triples, lambda: powertools.bin_bispectrum(spectrum, self.spacing, k_edges, triples, unit=True))
        return power, sum3, unit

    def delta_to_density(self, growth, density, rms, lognormal, download):
        delta = self.plan.data_out
        if lognormal:
            delta = cosmotools.apply_lognormal_transform(delta, growth, sigma=rms)
        else:
            delta *= growth
            delta += 1
        delta *= density
        return delta

    def newtonian(self, potential, scale, growth, redshifts, download):
        self.plan.data_in[:] = potential
        self.plan.data_in *= scale
        field = self.plan.execute()
        if growth is not None:
            field *= growth
            field /= 1 + redshifts
        return field

    def _modes(self, axis):
        """signed mode numbers along ``axis`` of the half spectrum (broadcastable), 0 at the axis' Nyquist index"""
        shape = self.plan.shape
        n = shape[axis]                 # (even: transform.Plan accepts nothing else)
        m = np.arange(shape[2] // 2 + 1, dtype=float) if axis == 2 else np.fft.fftfreq(n, 1.0 / n)
        m = np.where(np.abs(m) == n // 2, 0.0, m)
        return m.reshape([-1 if a == axis else 1 for a in range(3)])

    def _derivative(self, source, factor):
        """the plan's inverse transform of ``source * factor``: every spectral derivative of this backend.  (The factor is rounded to
        the array's COMPLEX type here, where the device rounds the real factor once and multiplies the two parts -- rf_core.h grad_cell;
        both are two roundings per component, the fields agree to a few float32 ulp)"""
        data = self.plan.data_in
        data[:] = source
        data *= factor.astype(data.dtype)
        return self.plan.execute()

    def _lpt2_source(self):
        """S(x) in the plan's real type (a new array): the six Hessian components through the plan's own inverse transform"""
        dk3, H = self.dk3(), {}
        for a in range(3):
            for b in range(a, 3):
                H[a, b] = self._derivative(self.gen.potential, -(dk3[a] * self._modes(a)) * (dk3[b] * self._modes(b)) + 0j).copy()
        S = H[0, 0] * H[1, 1]
        S += (H[0, 0] + H[1, 1]) * H[2, 2]
        for ab in ((0, 1), (0, 2), (1, 2)):
            S -= H[ab] * H[ab]
        return S

    def lpt2_source(self, download):
        self.make_current(self._lpt2_source())
        return self.plan.data_out

    def gradient(self, order, axis, coeff, dk, factor, download):
        """one component of the gradient of the saved potential (``order`` 1) or of the second-order potential (2, formed once per
        field), times ``coeff`` and the optional (nz,) ``factor``"""
        if order == 2 and self.lpt2 is None:
            kx2, ky2, kz2 = (np.asarray(a, np.float64) for a in powertools.ksq_axes(*self.plan.shape, self.spacing))
            k2 = (kx2[:, None, None] + ky2[None, :, None]) + kz2[None, None, :]
            k2[0, 0, 0] = 1.0
            phi2 = np.fft.rfftn(np.asarray(self._lpt2_source(), np.float64), axes=(0, 1, 2)) / k2
            phi2[0, 0, 0] = 0.0
            self.lpt2 = phi2.astype(self.plan.data_in.dtype)
        field = self._derivative(self.gen.potential if order == 1 else self.lpt2, 1j * coeff * dk * self._modes(axis))
        if factor is not None:
            field *= factor
        return field

    def accumulate_displacement(self, axis, coeff, first):
        if self._building is None:
            self._building = np.empty((3,) + tuple(self.plan.shape), self.plan.data_out.dtype)
        term = self.plan.data_out.dtype.type(coeff) * self.plan.data_out
        self._building[axis] = term if first else self._building[axis] + term

    def displacements_complete(self):
        self.particles, self._building = self._building, None

    def set_displacements(self, s):
        self.particles = s.copy()

    def download_displacements(self):
        return self.particles.copy()              # (a new array on both backends)

    def paint(self, inv_h, order, tables=None):
        """-> dropped.  ``tables``: the phases of an interlaced paint (a second grid half a cell on), whose spectrum is kept"""
        rtype = self.plan.data_out.dtype
        A, dropped = particles.paint_counts(self.particles, inv_h, order)
        delta = particles.counts_to_delta(A, rtype)
        if tables is not None:
            B, _ = particles.paint_counts(self.particles, inv_h, order, half_cell=True)
            spectra = [np.fft.rfftn(d.astype(np.float64), axes=(0, 1, 2)) for d in (delta, particles.counts_to_delta(B, rtype))]
            self.interlaced = powertools.interlace_combine(spectra[0], spectra[1], tables)
            delta = np.fft.irfftn(self.interlaced, s=tuple(self.plan.shape), axes=(0, 1, 2))
        self.make_current(delta)
        return dropped

    def gather(self, inv_h, slot, coeff, first, order, download):
        """-> (dropped, the slot's values or None)"""
        if self.gathered is None:
            self.gathered = np.zeros((3,) + tuple(self.plan.shape), self.plan.data_out.dtype)
        _, dropped = particles.gather(self.particles, inv_h, self.plan.data_out, coeff, first, self.gathered[slot], order)
        return dropped, self.gathered[slot].copy() if download else None

    def shift(self, axis, slot, coeff):
        self.particles[axis] += self.plan.data_out.dtype.type(coeff) * self.gathered[slot]

    def lensing(self, cotK, i_min):
        dPhi = self.plan.data_out
        psi = np.empty_like(dPhi)
        h = float(self.spacing)
        for i in range(dPhi.shape[2], i_min, -1):
            psi[:, :, i_min:i] = dPhi[:, :, i_min:i]
            psi[:, :, i_min:i] *= -2 * (cotK[i_min:i] - cotK[i - 1])
            psi[:, :, i - 1] = cosmotools.simps_avg(psi[:, :, i_min:i], h)
        if i_min > 0:
            psi[:, :, :i_min] = 0.
        return psi


class _DevicePotential(object):
    """Marker for a saved delta(k)/k**2 field that lives in device memory."""

    def __init__(self, generator):
        self._generator = generator

    def download(self):
        """Host copy (nx, ny, nz/2+1) of the saved potential."""
        backend = self._generator._backend
        backend.interlaced = None
        backend.dev.load_potential(1.0)
        return backend.dev.download_k()


class _RegeneratedPotential(object):
    """The saved potential of a ``generate_delta_field(save_potential=True)`` call that was NOT written to memory: the native
    generator is keyed by (seed, cell) and the replayed reference stream stays resident on the device, so delta(k)/k**2 is
    formed again inside the generation pass when :meth:`Generator.calculate_newtonian_potential` asks for it
    (rf_realise_scaled_potential) -- the default call writes 20 instead of 28 B/cell and the later transform reads nothing."""

    def __init__(self, generator, seed, noise):
        self._generator, self.seed, self.noise = generator, seed, noise
        dev = generator.plan_c2r.device
        # the device state this potential is a function of: the power / k tables, and (replayed stream) the resident deviates
        self._epochs = (dev.power_epoch, dev.noise_epoch if noise is not None else None)

    def check_current(self):
        """Raise unless the device plan still holds what the delta field was made from.  The reference's stored
        ``self.potential`` cannot change behind the caller's back; a regenerated one could, if somebody replaced the resident
        deviates (``reference_noise``, a same-seed batch, host deviates) or the power tables (``set_power``) through
        ``plan_c2r.device`` in between -- the result would silently belong to another field."""
        dev = self._generator.plan_c2r.device
        now = (dev.power_epoch, dev.noise_epoch if self.noise is not None else None)
        if now != self._epochs:
            what = "power / k tables" if now[0] != self._epochs[0] else "resident deviates"
            raise RuntimeError("The saved potential of the last generate_delta_field() call can no longer be formed: the device "
                               "plan's {0} have changed since.  Generate the field again, or use "
                               "Generator(store_potential=True) to keep delta(k)/k**2 in memory.".format(what))

    def download(self):
        """Host copy (nx, ny, nz/2+1) of the potential.  Runs the storing form of the call (rf_realise_potential) with the same
        seed.  Side effect: the plan's FIELD buffer is overwritten with the delta field of that seed again -- whatever
        ``convert_delta_to_density`` / ``calculate_newtonian_potential`` had left there is gone (download the field first)."""
        self.check_current()
        backend = self._generator._backend
        backend.interlaced = None
        backend.dev.realise_potential(self.seed, self.noise)
        backend.dev.load_potential(1.0)
        backend.field_on_host = False
        return backend.dev.download_k()


class HipBackend(_Backend):
    """The device plan behind ``plan_c2r.device``.  Displacements, gathered values and the interlaced spectrum are in device memory:
    here they are ``True`` or None; ``lpt2`` is the potential object the device's second-order potential was formed from."""

    def __init__(self, gen):
        super(HipBackend, self).__init__(gen)
        self.dev = self.plan.device
        self.single = self.plan.data_out.dtype == np.float32   # (a complex64 plan keeps float32 copies of the deviates: its cells sigma * g are float32 anyway)
        self.sink_armed = False             # the C plan delivers its next realisation into the plan's host buffer
        self.shared_replay_ran = False      # distributed: the first shared replay of the reference stream is behind us
        self.z_tables = None                # the (growth, density) tables the device plan was last given, as bytes
        self.fused_density = not gen.distributed and self.dev.nranks == 1 and self.dev.tiled      # rf_realise_lognormal serves the plan

    def _set_power(self, power):
        log10_k, sigma = powertools.sigma_table(power, tuple(self.plan.shape), self.spacing)
        # same power and smoothing as the tables the device plan holds: nothing to upload (a stream sync and a table rebuild
        # per call otherwise); the plan itself remembers what it was last given, whoever gave it
        self.dev.set_power(log10_k, sigma, if_changed=True)

    def _on_device(self, download, factor=None):
        """the tail of a call that leaves a new field on the device: the optional (nz,) factor, then the host copy or None"""
        if factor is not None:
            self.dev.scale_z(factor)
        self.field_on_host = False
        return self.field_to_host() if download else None

    def realise_delta(self, power, seed, save_potential, download):
        """-> (delta or None, rms, potential)"""
        dev = self.dev
        self._set_power(power)
        # generate.py:184-189,230 returns a HOST array, and the device -> host copy is 15 x the realisation at 1024^3: armed with
        # the plan's host buffer, the realisation below delivers slab by slab behind its z pass (rf_set_host_sink)
        self.sink_armed = bool(download) and not self.gen.distributed and dev.arm_host_sink(self.plan.data_out_padded, padded=True)
        try:
            potential = self._realise_delta(seed, save_potential)
            mean, std = dev.moments()
        finally:
            # (a call that raised too: a plan left armed delivers the NEXT field into the old buffer and stays off the graph replay)
            self.field_on_host = bool(self.sink_armed and dev.host_sink_delivered())
            self.sink_armed = False
        return (self.field_to_host() if download else None), std, potential

    def _realise_delta(self, seed, save_potential):
        """the field of ``seed`` on the device, by the shortest of the routes the plan offers -> potential"""
        gen, dev = self.gen, self.dev
        realised = False
        if gen.rng == "reference":
            # RandomState(seed).normal (random.py:24): MT19937 + polar method replayed on the GPU from the seed's
            # 624-word start state -- integer seeds, array seeds (init_by_array) and None alike; no host deviates
            if seed is None and gen.distributed:
                seed = self.plan.agree_on(int.from_bytes(os.urandom(4), "little"))
            if gen.distributed and dev.nranks > 1 and dev.tiled and dev.share_segments()[0] >= dev.nranks:
                # one stream, P ranks: each replays 1/P of it, one all-to-all of deviates (rf_mt_share_*); the first
                # time round under the watchdog that names a rank which never arrived (slab.Deadline)
                if self.shared_replay_ran:
                    dev.reference_noise_shared(seed, single=self.single)
                else:
                    with self.plan.dist.deadline("first shared replay of the reference stream"):
                        dev.reference_noise_shared(seed, single=self.single)
                    self.shared_replay_ran = True
            elif self.single and not gen.distributed and not (save_potential and gen.store_potential) and dev.can_batch_reference():
                # one device call: the replay and the passes queued back to back (no host synchronisation between them,
                # untimed passes: the z pass of a slab shares its launch with the y pass of the next) -- a same-seed
                # batch of one (rf_realise_batch_reference); the deviates stay resident as float32 pairs
                dev.realise_batch_reference([seed], want_rms=False)
                realised = True
            else:
                dev.reference_noise(seed, single=self.single)
            noise, dseed = "resident", 0
        else:
            noise, dseed = None, self._native_seed(seed)
        # generate.py:200-217.  Native noise: delta(k)/k**2 is a second store stream of the generation pass;
        # otherwise the library runs rows K,T,R,S -> k-space, the division, and the c2r transform.
        if save_potential and (gen.store_potential or not dev.can_regenerate_potential(noise)):
            dev.realise_potential(dseed, noise)
            return _DevicePotential(gen)
        if not realised:
            self._realise(dseed, noise)             # fused: k-space never materialised
        # nothing to store: the potential can be formed again from the seed / the resident deviates on demand
        return _RegeneratedPotential(gen, dseed, noise) if save_potential else None

    def _native_seed(self, seed):
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
            if self.gen.distributed:
                seed = self.plan.agree_on(seed >> 12)          # 52 bits survive the float64 all-reduce
        return int(seed) & (2 ** 64 - 1)

    def _realise(self, dseed, noise):
        """One fused realisation on the device.  Native generator on a single-GPU tiled plan: replayed from a captured
        one-realisation hipGraph (rf_realise_batch with one seed, read from device memory) -- the call is ~35 kernel launches, and
        their launch gaps are 5 % of a 1024^3 realisation when issued one by one; everything else issues them eagerly."""
        dev = self.dev
        if noise is None and not self.gen.distributed and dev.tiled and dev.nranks == 1 and not self.sink_armed:
            dev.realise_batch(np.array([dseed], np.uint64), want_rms=False)       # (a captured graph keeps its field on the device: not with a host sink)
        else:
            dev.realise(dseed, noise)

    def realise_density(self, power, growth, density, seed):
        """-> rms of the Gaussian field; its lognormal density field is the current field (rf_realise_lognormal)"""
        self._set_power(power)
        tables = (np.asarray(growth, np.float64).tobytes(), np.asarray(density, np.float64).tobytes())
        if self.z_tables != tables:
            self.dev.set_z_tables(growth, density)
            self.z_tables = tables
        if self.gen.rng == "reference":
            self.dev.reference_noise(seed, single=self.single)
            rms = self.dev.realise_lognormal(0, "resident")
        else:
            rms = self.dev.realise_lognormal(self._native_seed(seed), None)
        self.field_on_host = False
        return rms

    def field_to_host(self):
        if not self.field_on_host:
            self.dev.download_real(self.plan.data_out_padded, padded=True)
            self.field_on_host = True
        return self.plan.data_out

    def make_current(self, field):
        super(HipBackend, self).make_current(field)
        self.dev.upload_real(self.plan.data_out_padded, padded=True)

    def binned_sums(self, k_edges, source, los=None, window=None):
        source = _hip.RF_POWER_FROM_KSPACE if source == "kspace" else _hip.RF_POWER_FROM_FIELD
        if los is None:
            return self.dev.measure_power(k_edges, source)
        return self.dev.measure_multipoles(k_edges, los, source, window)

    def bispectrum_sums(self, k_edges, triples, source, window=None):
        """as :meth:`NumpyBackend.bispectrum_sums`: the field transformed into the k buffer first (``source='field'``), then everything
        reads the k buffer; the device copy of the field is consumed"""
        if source != "kspace":
            self.dev.execute_r2c()
        if window is None:
            power = self.dev.measure_power(k_edges, _hip.RF_POWER_FROM_KSPACE)
        else:
            power = self.dev.measure_multipoles(k_edges, 2, _hip.RF_POWER_FROM_KSPACE, window)[:3]
        amp = None if window is None else [None if t is None else np.sqrt(t) for t in window]
        sum3 = self.dev.measure_bispectrum(k_edges, triples, amp)
        unit = self.unit_sums(k_edges, triples, lambda: self.dev.measure_bispectrum(k_edges, triples, unit=True))
        return power, sum3, unit

    def delta_to_density(self, growth, density, rms, lognormal, download):
        if lognormal:
            a_z, b_z = cosmotools.lognormal_tables(growth, rms, self.plan.shape[2])
            self.dev.lognormal(a_z, b_z, float(rms))
        else:
            self.dev.affine_z(growth, 1.0)
        return self._on_device(download, density)

    def newtonian(self, potential, scale, growth, redshifts, download):
        factor = None if growth is None else growth / (1 + redshifts)
        if isinstance(potential, _RegeneratedPotential):
            potential.check_current()
            self.dev.realise_scaled_potential(potential.seed, potential.noise, scale, factor_z=factor)
            factor = None           # (applied by the z pass itself)
        else:
            self.dev.load_potential(scale)
            self.dev.execute_c2r()
        return self._on_device(download, factor)

    def _store_potential(self):
        """the potential in device memory: a regenerated one is stored by running the storing form of the realisation once (the field
        buffer is about to be overwritten anyway), and ``Generator.potential`` becomes the stored potential of the same field"""
        potential = self.gen.potential
        if isinstance(potential, _RegeneratedPotential):
            potential.check_current()
            self.dev.realise_potential(potential.seed, potential.noise)
            self.gen.potential = _DevicePotential(self.gen)

    def lpt2_source(self, download):
        self._store_potential()
        self.lpt2 = None                          # (the accumulators take the second-order potential's memory)
        self.dev.lpt2_source(self.dk3())
        return self._on_device(download)

    def gradient(self, order, axis, coeff, dk, factor, download):
        """as :meth:`NumpyBackend.gradient`"""
        dev, potential = self.dev, self.gen.potential
        if order == 1 and isinstance(potential, _RegeneratedPotential) and potential.noise is None:
            potential.check_current()
            dev.generate(potential.seed, None)                      # delta(k) again: one generation sweep
            dev.execute_gradient(axis, coeff, dk, _hip.RF_GRAD_FROM_KSPACE)
            return self._on_device(download, factor)
        # (the replayed reference stream is resident as float32 pairs, which only the fused generation pass reads -- rf_generate wants
        # float64 deviates -- and the second order needs the potential in memory: what is stored now serves every later call)
        self._store_potential()
        if order == 2 and (self.lpt2 is not self.gen.potential or not dev.lpt2_valid):
            dev.lpt2_potential(self.dk3())
            self.lpt2 = self.gen.potential
        dev.execute_gradient(axis, coeff, dk, _hip.RF_GRAD_FROM_POTENTIAL if order == 1 else _hip.RF_GRAD_FROM_POTENTIAL2)
        return self._on_device(download, factor)

    def accumulate_displacement(self, axis, coeff, first):
        self.dev.particles_accumulate(axis, coeff, first=first)

    def displacements_complete(self):
        self.particles = True

    def set_displacements(self, s):
        for axis in range(3):
            self.dev.particles_upload(axis, s[axis])
        self.particles = True

    def download_displacements(self):
        return np.stack([self.dev.particles_download(axis) for axis in range(3)])

    def paint(self, inv_h, order, tables=None):
        """as :meth:`NumpyBackend.paint`; the spectrum of an interlaced paint is left in the k buffer"""
        if tables is None:
            dropped = self.dev.particles_paint(inv_h, order)
        else:
            dropped = self.dev.particles_paint_interlaced(inv_h, order, tables)
            self.interlaced = True
        self.field_on_host = False
        return dropped

    def gather(self, inv_h, slot, coeff, first, order, download):
        dropped = self.dev.particles_gather(inv_h, slot, coeff, first, order)
        self.gathered = True
        return dropped, self.dev.particles_gather_download(slot) if download else None

    def shift(self, axis, slot, coeff):
        self.dev.particles_shift(axis, slot, coeff)

    def lensing(self, cotK, i_min):
        self.dev.lensing_potential(cotK, self.spacing, i_min)
        return self.dev.download_aux()
