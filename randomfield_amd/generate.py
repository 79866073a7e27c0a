"""
High-level functions to generate random fields -- mirror of
``randomfield/generate.py`` :class:`Generator` for the Fourier-space sampling
path, running on MI355X through ``librandomfield_hip.so``.

Same constructor / method signatures as the reference (generate.py:74-75,
144-146, 232-233, 282) plus keyword-only extensions.  The call order of the
reference's ``generate_delta_field`` (generate.py:191-199,218-219)

    fill_with_log10k -> filter_power -> tabulate_sigmas -> randomize
    -> symmetrize -> [save potential] -> Plan.execute -> np.std

is preserved in meaning, but on the ``hip`` backend the first five steps are
evaluated per cell inside the first FFT pass of one fused GPU pipeline
(``rf_realise``); the k-space array is only materialised when
``save_potential=True`` needs it.

Out of scope here (host-only side-cars of the reference):
``plot_slice``.
"""
from __future__ import annotations

import functools

import numpy as np

from . import _backends, powertools, transform
from ._backends import _DevicePotential, _RegeneratedPotential  # noqa: F401  (hip-backend objects, importable from here as before)

__all__ = ["Generator"]


def _assignment_order(assignment):
    """the cells per axis (the window order) of a mass-assignment scheme's name"""
    orders = {"cic": 2, "tsc": 3}
    if assignment not in orders:
        raise ValueError("Invalid assignment: {0!r} (expected 'cic' or 'tsc').".format(assignment))
    return orders[assignment]


def _replaces_kspace(method):
    """a Generator method that may write the k buffer: the spectrum of the last interlaced paint is gone (``source='kspace'``)"""
    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        self._backend.interlaced = None
        return method(self, *args, **kwargs)
    return wrapper


class Generator(object):
    """
    Manage random field generation for a specified geometry.

    Parameters (as the reference, generate.py:43-73)
    ----------
    nx, ny, nz : int
        Grid size; z is the line-of-sight direction.
    grid_spacing_Mpc_h : float
        Uniform grid spacing in Mpc/h.
    num_plot_sections : int
        Kept for compatibility: nz must be divisible by it (generate.py:86-90).
    cosmology : object, optional
        Kept for the caller's reference; the package never evaluates it.  The O(nz)
        tables the reference derives from it (generate.py:104-129) are separate
        arguments below, and passing ``cosmology`` without ``growth_function`` and
        ``mean_matter_density`` raises ``ValueError``.  Only its ``Om0`` attribute is
        read, by :meth:`calculate_newtonian_potential` when ``scale`` is not given.
    power : numpy.ndarray, optional
        Structured array with fields 'k', 'Pk' (powertools.validate_power).
        Defaults to the shipped Planck13 table.
    verbose : bool, optional

    Keyword-only extensions
    -----------------------
    backend : 'hip' (default) or 'numpy'
        See :mod:`randomfield_amd.transform`.  'hip' raises RuntimeError when the
        GPU path is unavailable; it never falls back to the CPU.
    dtype : numpy complex dtype
        complex64 (reference behaviour, generate.py:77) or complex128.
    rng : 'reference' (default) or 'native'
        'reference' draws the reference's own stream (``RandomState(seed).normal``,
        random.py:24) -- replayed on the GPU (MT19937 with jump-ahead + polar method)
        for integer seeds -- so the same seed gives the reference's field (to float32
        FFT rounding).
        'native' uses the GPU's counter-based Philox4x32-7 + Box-Muller generator:
        no host work, different (statistically equivalent) realisations.
    growth_function, mean_matter_density, redshifts : (nz,) arrays, optional
        The cosmology tables along z (the reference builds them with astropy, generate.py:104-129).
    transverse_distance : (nz,) array, optional
        Comoving transverse distance DA along z in Mpc/h (``self.DA`` of the reference,
        generate.py:117-118), for :meth:`calculate_lensing_potential`.
    curvature_K : float, optional
        Curvature constant K in (Mpc/h)**-2 (generate.py:380-381: -Ok0 (H0/c)**2); 0 = flat.
    distributed : bool, optional
        One process per GPU (RANK / WORLD_SIZE / LOCAL_RANK from the environment, as ``torch.distributed.run`` sets
        them): k space is split by kz planes, the field by x planes, and every method works on this rank's
        ``nx / WORLD_SIZE`` planes of the field (``data_out`` has that many; see :mod:`randomfield_amd.slab`).  All ranks
        must make the same calls with the same arguments; ``seed=None`` is agreed between the ranks.
    exchange : {None, 'auto', 'direct', 'rccl'}, optional
        ``distributed=True``: how the blocks move between the y and z passes -- 'direct': every rank's y pass stores its output
        straight into the IPC-mapped receive buffers of its peers (no send / receive kernels, no extra sweep of local memory);
        'rccl': one grouped ncclSend / ncclRecv all-to-all; 'auto' (default, also ``RANDOMFIELD_EXCHANGE``): direct if every
        rank can, else rccl.  The fields are identical.  ``exchange_chunks`` (or ``RANDOMFIELD_EXCHANGE_CHUNKS``: 'auto' = 1, or
        a power of two) cuts the rank's kz slab into sub-slabs that travel while the next one is being generated.
    store_potential : bool, optional
        hip backend: ``generate_delta_field(save_potential=True)`` normally does not write delta(k)/k**2 to memory when it can be
        formed again on demand from the seed (``rng='native'``) or from the replayed deviates still on the device (complex64,
        ``rng='reference'``): :meth:`calculate_newtonian_potential` then regenerates it inside its generation pass.  ``True``
        stores it at generation time as the reference does (generate.py:200-217).  The results agree to float32 rounding.
    """

    def __init__(self, nx, ny, nz, grid_spacing_Mpc_h, num_plot_sections=4, cosmology=None, power=None,
                 verbose=False, *, backend=None, dtype=np.complex64, rng="reference", growth_function=None,
                 mean_matter_density=None, redshifts=None, transverse_distance=None, curvature_K=0.0, distributed=False,
                 store_potential=False, exchange_chunks=None, exchange=None):
        self.backend = transform.resolve_backend(backend)
        self.distributed = bool(distributed)
        self.store_potential = bool(store_potential)
        if self.distributed and self.backend != "hip":
            raise ValueError("distributed=True needs backend='hip'.")
        if rng not in ("reference", "native"):
            raise ValueError("Invalid rng: {0} (expected 'reference' or 'native').".format(rng))
        if rng == "native" and self.backend != "hip":
            raise ValueError("rng='native' is the GPU generator; it needs backend='hip'.")
        self.rng = rng
        if self.distributed:
            from . import slab
            if nx % 2 or ny % 2 or nz % 2:
                raise ValueError("All shape dimensions must be even.")
            self.plan_c2r = slab.SlabHostPlan(slab.DistributedPlan(nx, ny, nz, dtype, exchange=exchange), dtype)
            # every call here is ONE realisation.  Its all-to-all can be cut into sub-slabs that travel while the next sub-slab is
            # still being generated and transformed (RF_FLAG_EXCHANGE_CHUNKS) -- OPT-IN (`exchange_chunks=` or the environment
            # variable RANDOMFIELD_EXCHANGE_CHUNKS): the two-stream schedule is verified with virtual ranks and the forced slab
            # path on one GPU only; the default stays the plain forward -> exchange -> backward sequence on one stream until a
            # multi-GPU run has shown the same field and a gain
            chunks = slab.exchange_chunks_setting(exchange_chunks)      # (one parser for bench.py and this class)
            if chunks == "auto":
                chunks = 1
            if self.plan_c2r.device.nranks > 1 and chunks > 1:
                self.plan_c2r.device.set_exchange_chunks(chunks)
        else:
            self.plan_c2r = transform.Plan(shape=(nx, ny, nz), dtype_in=dtype, packed=True, overwrite=True,
                                           inverse=True, use_pyfftw=True, backend=self.backend)
        # generate.py:79-80: the forward plan over the same memory (a distributed rank: its window of the field in, its kz planes out)
        self.plan_r2c = self.plan_c2r.create_reverse_plan(reuse_output=True, overwrite=True)
        self.grid_spacing_Mpc_h = grid_spacing_Mpc_h
        self.k_min, self.k_max = powertools.get_k_bounds(self.plan_c2r.data_in, grid_spacing_Mpc_h, packed=True)
        self.potential = None
        self.particles_dropped = 0
        # (everything that touches the field, and what of it is kept between calls: _backends.py)
        self._backend = _backends.HipBackend(self) if self.backend == "hip" else _backends.NumpyBackend(self)

        if nz % num_plot_sections != 0:
            raise ValueError("Z-axis does not evenly divided into {0} plot sections.".format(num_plot_sections))
        self.num_plot_sections = num_plot_sections

        # The reference derives its O(nz) background tables (redshifts, growth function, mean matter density, DA;
        # generate.py:104-129) from an astropy cosmology.  That derivation is outside this package:
        # the tables are constructor arguments.  A `cosmology` object is kept for the caller's reference only, and
        # asking for one WITHOUT the tables it would have produced is refused here rather than failing later.
        self.cosmology = cosmology
        if cosmology is not None and (growth_function is None or mean_matter_density is None):
            raise ValueError("cosmology= is not evaluated by this package: pass the tables it implies as arrays "
                             "(growth_function=, mean_matter_density=, and redshifts= / transverse_distance= if "
                             "needed).")
        if power is None:
            if cosmology is not None:
                raise ValueError("A tabulated power= is required with a custom cosmology "
                                 "(the CLASS-based calculate_power is not part of this package).")
            power = powertools.load_default_power()
        self.power = powertools.validate_power(power)

        self.redshifts = None if redshifts is None else np.asarray(redshifts, float).reshape(nz)
        self.growth_function = None if growth_function is None else np.asarray(growth_function, float).reshape(nz)
        self.mean_matter_density = (None if mean_matter_density is None
                                    else np.asarray(mean_matter_density, float).reshape(nz))
        self.DC = np.arange(nz) * self.grid_spacing_Mpc_h
        self.DA = None if transverse_distance is None else np.asarray(transverse_distance, float).reshape(nz)
        self.curvature_K = float(curvature_K)

        self.delta_field_rms = None
        self.smoothed_power = None
        if self.backend == "hip":
            dev = self.plan_c2r.device
            dev.set_kgrid(*powertools.ksq_axes(nx, ny, nz, grid_spacing_Mpc_h))
            # (shapes that are not powers of two: dev.set_fused_generation(True) makes their realisations generate inside the first FFT
            # pass too -- same field bit for bit, 8 ... 27 % faster; left OFF here because the 1000^3 float32 gain, 0.925, misses the
            # 0.9 set for making it the default: DESIGN.md section 3.7)

        self.verbose = verbose
        if self.verbose:
            Mb = (self.plan_c2r.nbytes_allocated + (self.plan_r2c.nbytes_allocated if self.plan_r2c else 0)) / 2.0 ** 20
            print("Allocated {0:.1f} Mb for {1} x {2} x {3} grid.".format(Mb, nx, ny, nz))
            print("{0} Mpc/h spacing covered by k = {1:.5f} - {2:.5f} h/Mpc."
                  .format(self.grid_spacing_Mpc_h, self.k_min, self.k_max))
            if self.backend == "hip":
                print("Device buffers: {0:.1f} Mb.".format(self.plan_c2r.device.nbytes / 2.0 ** 20))

    # ------------------------------------------------------------------
    @property
    def shape(self):
        return self.plan_c2r.shape

    @_replaces_kspace
    def generate_delta_field(self, smoothing_length_Mpc_h=0., seed=None, save_potential=True, show_plot=False,
                             save_plot_name=None, *, download=True):
        """
        Generate a delta-field realization (generate.py:144-230).

        The delta field is calculated at redshift zero and sampled from a
        distribution with mean zero and k-space variance proportional to the
        smoothed power spectrum.  ``seed=None`` draws a fresh seed.

        Returns a 3D array of delta values that is a *view* of the plan's host
        buffer and will be overwritten by subsequent operations (as in the
        reference).  With ``download=False`` (hip backend) the field stays on the
        GPU, ``None`` is returned, and :meth:`download_field` fetches it later.
        """
        if show_plot or save_plot_name is not None:
            raise NotImplementedError("plot_slice is outside the accelerated path (see DESIGN.md).")
        self._begin_field(smoothing_length_Mpc_h)
        delta, rms, self.potential = self._backend.realise_delta(self.smoothed_power, seed, save_potential, download)
        self._set_rms(rms)
        return delta

    def _begin_field(self, smoothing_length_Mpc_h):
        """every new field: its smoothed power, and nothing left of the particles and the second-order potential of the last one"""
        self.smoothed_power = powertools.filter_power(self.power, smoothing_length_Mpc_h)
        self._backend.new_field()

    def _set_rms(self, rms):
        self.delta_field_rms = self.plan_c2r.data_out.dtype.type(rms)
        if self.verbose:
            print("Delta field has standard deviation {0:.3f}.".format(self.delta_field_rms))

    @_replaces_kspace
    def generate_density_field(self, smoothing_length_Mpc_h=0., seed=None, *, download=True):
        """
        ``generate_delta_field(save_potential=False)`` followed by ``convert_delta_to_density(apply_lognormal_transform=True)``
        (generate.py:191-199,218-219 and 266-273) as ONE device call (an extension; the reference has no such method).

        On a single-GPU hip plan with power-of-two axes the rms of the Gaussian field is taken from the transform's second
        pass (Parseval) and the lognormal map and the mean-density factor run in the epilogue of the last pass
        (``rf_realise_lognormal``): five sweeps of the array instead of seven, no host round trip for sigma.  The result is
        the reference's density field up to a few ulp in the argument of ``exp``.  Everywhere else (numpy backend, multi-GPU
        plans, generic shapes) the two reference calls run one after the other.  ``delta_field_rms`` is set as usual.
        """
        growth = self._need_table("growth_function")
        density = self._need_table("mean_matter_density")
        if not self._backend.fused_density:
            self.generate_delta_field(smoothing_length_Mpc_h, seed, save_potential=False, download=False)
            return self.convert_delta_to_density(apply_lognormal_transform=True, download=download)
        self._begin_field(smoothing_length_Mpc_h)
        rms = self._backend.realise_density(self.smoothed_power, growth, density, seed)
        self.potential = None
        self._set_rms(rms)
        return self.download_field() if download else None

    def download_field(self):
        """Copy the device-resident field into the plan's host buffer and return the view."""
        return self._backend.field_to_host()

    @property
    def _field_on_host(self):
        return self._backend.field_on_host

    def measure_power_spectrum(self, field=None, *, k_edges=None, nbins=None, window=None, source="field"):
        """
        Binned power spectrum of a field on this grid (an extension; the reference has no such method): the estimator that
        closes P(k) -> delta(x) -> P^(k).

        ``field=None`` measures the current field -- the one on the device (hip backend) or ``plan_c2r.data_out`` (numpy backend);
        an ``(nx, ny, nz)`` array is uploaded (hip) or copied into the plan's host buffer (numpy) first and becomes the current
        field.  ``k_edges`` are ``nbins + 1`` strictly increasing, non-negative bin edges in h/Mpc, at most 1024 bins; by default
        ``powertools.default_k_edges(shape, spacing, nbins)``: linear from ``k_min`` to ``k_max``, ``min(shape) // 2`` bins.

        Every mode of the forward transform with ``edges[b] <= |k| < edges[b+1]`` (decided on squared values) enters bin b, the
        stored half spectrum standing for the full one (weight 2 away from the planes kz = 0 and nz/2); the DC mode is dropped.
        Returns a structured array with the fields ``'k'`` (mean |k| of the bin's modes), ``'Pk'`` (V / N**2 times the mean of
        |delta(k)|**2, V the box volume and N the number of cells -- the convention of ``self.power``, so the two can be compared
        directly) and ``'nmodes'`` (number of modes); empty bins hold NaN.

        hip backend: one sweep on the device (``rf_measure_power``), reproducible bit for bit from call to call.  On
        power-of-two grids (the tiled kernels) the forward transform runs in place and the DEVICE COPY OF THE FIELD IS CONSUMED:
        a later :meth:`download_field` needs the field to be on the host already (it is after ``generate_delta_field()`` with
        the default ``download=True`` and after passing ``field``); other shapes keep the field on the device.
        ``distributed=True`` raises ``NotImplementedError``.

        ``window`` (None, ``'ngp'`` / ``'cic'`` / ``'tsc'``, or three per-axis tables as ``powertools.window_compensation`` makes
        them) divides a mass-assignment window out of |delta(k)|**2: ``'Pk'`` is then the compensated monopole of
        :meth:`measure_power_multipoles` (``rf_measure_multipoles``).  With the default nothing changes.

        ``source``: ``'field'`` (the default: everything above) or ``'kspace'``, which measures the spectrum left by the last
        ``paint_particles(interlaced=True)`` without transforming anything and leaves field and spectrum as they are.  It raises
        ``RuntimeError`` if there is no such spectrum or a later call of this object has replaced it; ``field=`` together with it is
        a ``ValueError``.  Among the calls that replace it is every ``source='field'`` measurement, on both backends and every grid
        (the device transforms the field into the k buffer on grids that are no power of two; the rule is the same everywhere so that
        one sequence of calls behaves alike): measure with ``source='kspace'`` first, then the field.
        """
        if self.distributed:
            raise NotImplementedError("measure_power_spectrum runs on single-GPU plans.")
        self._check_source(field, source)
        if window is not None:
            res = self.measure_power_multipoles(field, los=2, k_edges=k_edges, nbins=nbins, window=window, source=source)
            out = np.empty(len(res), [("k", float), ("Pk", float), ("nmodes", np.uint64)])
            out["k"], out["Pk"], out["nmodes"] = res["k"], res["P0"], res["nmodes"]
            return out
        shape, k_edges = self._power_inputs(field, k_edges, nbins, source)
        sums = self._backend.binned_sums(k_edges, source)
        return powertools.power_estimate(*sums, shape=shape, spacing=self.grid_spacing_Mpc_h)

    def measure_power_multipoles(self, field=None, *, los=2, k_edges=None, nbins=None, window=None, source="field"):
        """
        Monopole, quadrupole and hexadecapole of the binned power spectrum with the line of sight along grid axis ``los`` (0, 1, 2:
        plane-parallel) -- what a mock painted in redshift space (:meth:`particle_displacements` with ``rsd_axis``) is measured with.

        ``field``, ``k_edges``, ``nbins``, the binning, the weights, the normalisation and what happens to the device copy of the
        field are those of :meth:`measure_power_spectrum`.  Per bin the moments M0, M2, M4 of mu**2 = k_los**2 / k**2 weighted by
        |delta(k)|**2 are summed (every term non-negative) and combined as P0 = M0, P2 = (5/2)(3 M2 - M0),
        P4 = (9/8)(35 M4 - 30 M2 + 3 M0).  ``window``: None, a scheme name (``'ngp'``, ``'cic'``, ``'tsc'``:
        ``powertools.window_compensation``) or three per-axis tables of nx, ny, nz/2 + 1 finite positive factors multiplied onto
        |delta(k)|**2 (each may be None).  The compensation is the standard one for well-mixed particles, not an exact inverse of
        the paint of a cold lattice.  Returns a structured array with the fields ``'k'``, ``'P0'``, ``'P2'``, ``'P4'``, ``'nmodes'``;
        empty bins hold NaN.  hip backend: one sweep on the device (``rf_measure_multipoles``), the same bits on every call.
        ``source`` as in :meth:`measure_power_spectrum`.
        """
        if self.distributed:
            raise NotImplementedError("measure_power_multipoles runs on single-GPU plans.")
        self._check_source(field, source)
        if los not in (0, 1, 2):
            raise ValueError("Invalid los: {0!r} (expected 0, 1 or 2).".format(los))
        if isinstance(window, str):
            window = powertools.window_compensation(tuple(self.plan_c2r.shape), window)
        elif window is not None:
            window = powertools._compensation_tables(window, tuple(self.plan_c2r.shape))
        shape, k_edges = self._power_inputs(field, k_edges, nbins, source)
        sums = self._backend.binned_sums(k_edges, source, los, window)
        return powertools.multipole_estimate(*sums, shape=shape, spacing=self.grid_spacing_Mpc_h)

    def measure_bispectrum(self, field=None, *, k_edges=None, nbins=None, triangles="closed", window=None, source="field"):
        """
        Binned bispectrum of a field on this grid by the FFT estimator (Scoccimarro 2015; Sefusatti et al. 2016) -- the three-point
        statistic that tells a second-order (2LPT) mock from a Zel'dovich one of nearly the same P(k).

        ``field`` and ``source`` behave as in :meth:`measure_power_spectrum`: ``source='field'`` transforms the current field first
        (and, by the same one rule, the spectrum of the last interlaced paint is gone), ``source='kspace'`` reads the spectrum left by
        ``paint_particles(interlaced=True)`` and leaves it.  ``k_edges`` are ``nbins + 1`` strictly increasing non-negative edges in
        h/Mpc, at most 32 bins, by default ``powertools.default_bispectrum_edges(shape, spacing, nbins)``: linear up to 2/3 of the
        Nyquist frequency.  The shells are the bins of :meth:`measure_power_spectrum`.  ``triangles``: ``'closed'``, ``'all'`` or
        ``'equilateral'`` (``powertools.bispectrum_triples``) or an ``(ntriples, 3)`` array of bins b1 <= b2 <= b3, at most 8192.

        For shell b, D_b(x) is the inverse transform of the spectrum restricted to the shell; a triple sums D_b1 D_b2 D_b3 over the
        grid, which counts every ordered triangle k1 + k2 + k3 = 0 MODULO THE GRID with k_i in shell b_i.  Triangles that close only
        through aliasing are part of that sum: none exists while the last edge stays at or below 2/3 of the Nyquist frequency, which
        is why the default edges end there; with edges beyond it they enter both the data's sum and the triangle count.

        Returns a structured array, one row per triple: ``'bins'`` (three integers), ``'k1'``, ``'k2'``, ``'k3'`` (the mean |k| of
        each shell's modes), ``'B'`` = (V**2 / N**3) sum_data / sum_unit -- the convention of :meth:`measure_power_spectrum` one order
        up --, ``'Q'`` = B / (P1 P2 + P2 P3 + P3 P1) with the P(k) of the same spectrum and edges, and ``'ntriangles'`` (float64, the
        integer number of ordered triangles); rows without a triangle hold NaN in B and Q.  ``window`` (None, ``'ngp'`` / ``'cic'`` /
        ``'tsc'`` or three per-axis tables as ``powertools.window_compensation`` makes them): delta(k) is multiplied by the square
        root of the compensation and P is the compensated monopole.

        hip backend: ``rf_measure_bispectrum``, the same bits on every call; the triangle counts are measured once per
        (edges, triples) and kept, so a second field costs one run.  The device copy of the field is consumed on every grid, and the
        call keeps one masked spectrum and ``nbins`` fields of device memory until ``plan_c2r.device.bispectrum_release()``.
        ``distributed=True`` raises ``NotImplementedError``.
        """
        if self.distributed:
            raise NotImplementedError("measure_bispectrum runs on single-GPU plans.")
        self._check_source(field, source)
        shape = tuple(self.plan_c2r.shape)
        if isinstance(window, str):
            window = powertools.window_compensation(shape, window)
        elif window is not None:
            window = powertools._compensation_tables(window, shape)
        if k_edges is None:
            k_edges = powertools.default_bispectrum_edges(shape, self.grid_spacing_Mpc_h, nbins)
        k_edges = np.asarray(k_edges, np.float64).ravel()
        if not 1 <= len(k_edges) - 1 <= 32:
            raise ValueError("measure_bispectrum takes between 1 and 32 bins.")
        if isinstance(triangles, str):
            triples = powertools.bispectrum_triples(k_edges, triangles)
        else:
            triples = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3), np.intc)
        if not 1 <= len(triples) <= 8192:
            raise ValueError("measure_bispectrum takes between 1 and 8192 triples.")
        shape, k_edges = self._power_inputs(field, k_edges, nbins, source)
        power, sum3, unit = self._backend.bispectrum_sums(k_edges, triples, source, window)
        return powertools.bispectrum_estimate(triples, sum3, unit, *power, shape=shape, spacing=self.grid_spacing_Mpc_h)

    def _check_source(self, field, source):
        if source not in ("field", "kspace"):
            raise ValueError("Invalid source: {0!r} (expected 'field' or 'kspace').".format(source))
        if source == "kspace":
            if field is not None:
                raise ValueError("source='kspace' measures the spectrum of the last interlaced paint: it takes no field.")
            if self._backend.interlaced is None:
                raise RuntimeError("No interlaced spectrum: call paint_particles(interlaced=True) first (a later call that writes "
                                   "the k buffer replaces it).")

    def _power_inputs(self, field, k_edges, nbins, source):
        """the edges of a power spectrum measurement, and ``field`` (if given) made the current field: (shape, k_edges)"""
        shape = tuple(self.plan_c2r.shape)
        if k_edges is None:
            k_edges = powertools.default_k_edges(shape, self.grid_spacing_Mpc_h, nbins)
        k_edges = np.asarray(k_edges, np.float64).ravel()
        if nbins is not None and len(k_edges) != int(nbins) + 1:
            raise ValueError("k_edges must have nbins + 1 entries.")
        if field is not None:
            self._make_current(field)
        if source == "field":
            # one rule for both backends and every grid: the device transforms the field into the k buffer on grids that are no power
            # of two, so the spectrum of the last interlaced paint is gone
            self._backend.interlaced = None
        return shape, k_edges

    def _make_current(self, field):
        """``field`` copied into the plan's host buffer and (hip backend) uploaded: it becomes the current field"""
        shape = tuple(self.plan_c2r.shape)
        field = np.asarray(field)
        if field.shape != shape:
            raise ValueError("field must have the shape {0}.".format(shape))
        self._backend.make_current(field)

    def _need_particles(self):
        if self._backend.particles is None:
            raise RuntimeError("No particle displacements: call particle_displacements() or set_particle_displacements() first.")

    @staticmethod
    def _check_slot(slot):
        if slot not in (0, 1, 2):
            raise ValueError("Invalid slot: {0!r} (expected 0, 1 or 2).".format(slot))

    def _need_table(self, name):
        value = getattr(self, name)
        if value is None:
            arg = {"DA": "transverse_distance"}.get(name, name)
            raise RuntimeError("Generator.{0} is not available: pass {1}= (an (nz,) array) to the constructor "
                               "(astropy-based tables are outside the accelerated path).".format(name, arg))
        return value

    def convert_delta_to_density(self, apply_lognormal_transform=True, show_plot=False, save_plot_name=None, *,
                                 download=True):
        """
        Convert a delta field into a density field with light-cone evolution
        (generate.py:232-280): lognormal map with sigma = delta_field_rms and the
        growth function along z (or ``delta*growth + 1``), then multiplication by
        the mean matter density along z.
        """
        if show_plot or save_plot_name is not None:
            raise NotImplementedError("plot_slice is outside the accelerated path (see DESIGN.md).")
        if self.delta_field_rms is None:
            raise RuntimeError("No delta field has been generated.")
        growth = self._need_table("growth_function")
        density = self._need_table("mean_matter_density")
        return self._backend.delta_to_density(growth, density, self.delta_field_rms, apply_lognormal_transform, download)

    @_replaces_kspace
    def calculate_newtonian_potential(self, light_cone=True, show_plot=False, save_plot_name=None, *,
                                      scale=None, download=True):
        """
        Calculate the Newtonian potential Phi(r) (generate.py:282-350): inverse
        transform of ``scale * delta(k)/k**2`` with scale = -3/2 H0**2 Omega_m
        (in s**-2, H0 = 100 km/s/Mpc), optionally times G(z)/(1+z) along z.

        ``scale`` may be given explicitly; otherwise it is -3/2 H0**2 ``cosmology.Om0``.
        """
        if show_plot or save_plot_name is not None:
            raise NotImplementedError("plot_slice is outside the accelerated path (see DESIGN.md).")
        if self.potential is None:
            raise RuntimeError("No saved potential field.")
        if scale is None:
            om0 = getattr(self.cosmology, "Om0", None)
            if om0 is None:
                raise RuntimeError("calculate_newtonian_potential needs scale= (or a cosmology= object with Om0).")
            H0 = 100.0 / 3.0856775814913673e19          # 100 km/s/Mpc in 1/s
            scale = -1.5 * H0 ** 2 * float(om0)
        growth = redshifts = None
        if light_cone:
            growth, redshifts = self._need_table("growth_function"), self._need_table("redshifts")
        return self._backend.newtonian(self.potential, scale, growth, redshifts, download)

    @_replaces_kspace
    def calculate_displacement_field(self, axis, light_cone=False, *, order=1, scale=1.0, factor_z=None, download=True):
        """
        One component of the vector field of the saved potential (an extension: the reference keeps delta(k)/k**2 "for later
        calculations of the lensing potential or the bulk velocity vector field", generate.py:200-217, and has no method for the
        latter):

            psi_a(r) = irfftn( i k_a * scale * delta(k) / k**2 ),    a = ``axis`` in (0, 1, 2) or ('x', 'y', 'z'),

        so that div psi = -scale * delta: with ``scale=1`` the Zel'dovich displacement in Mpc/h.  The mode of the axis' own
        Nyquist frequency is dropped (i k is not Hermitian there).  ``light_cone=True`` multiplies plane z by
        ``growth_function[z]``; ``factor_z`` is any (nz,) table used instead -- a H f G along z (expansion factor, Hubble rate,
        growth rate, growth function) turns the displacement into a peculiar velocity.

        Returns a *view* of the plan's buffer that later calls overwrite; ``delta_field_rms`` and the saved potential are left
        alone, so the three components can be asked for one after another.  hip backend: a stored potential
        (``Generator(store_potential=True)``) is differentiated on the device as it is.  A regenerated one (the default where the
        plan can form delta(k)/k**2 again) costs one generation sweep of k space per call with ``rng='native'``; with
        ``rng='reference'`` the first call runs the storing form of the realisation once (one realisation, and from then on the
        device memory of ``store_potential=True``: ``self.potential`` becomes the stored potential of the same field) and every
        later call reads what it stored.

        ``order=2`` returns the second-order Lagrangian (2LPT) term instead,

            (3/7) * scale**2 * psi2_a(r),    psi2_a = irfftn( i k_a * rfftn(S) / k**2 ),
            S = sum over a < b of  H_aa H_bb - H_ab**2,    H_ab = D_a D_b irfftn(delta(k) / k**2),

        D_a the same spectral derivative (so the Nyquist planes are dropped on the diagonal of H too), with the convention
        x = q + D1 psi1 + D1**2 psi2, i.e. D2 = -(3/7) D1**2 and div psi2 = -(3/7) S.  ``light_cone=True`` multiplies plane z by
        ``growth_function[z]**2``; ``factor_z`` overrides it.  The second-order potential is formed once per field (six Hessian
        transforms, one forward transform) and kept until the next field; each component is then one gradient transform.  hip
        backend: it needs the potential in device memory, so a regenerated one is first turned into a stored one by running the
        storing form of the realisation once (``self.potential`` becomes the stored potential of the same field, the field
        buffer is overwritten).  Any other ``order`` raises ``ValueError``.
        """
        if order not in (1, 2):
            raise ValueError("Invalid order: {0!r} (expected 1 or 2).".format(order))
        if self.distributed:
            raise NotImplementedError("calculate_displacement_field runs on single-GPU plans (distributed=False).")
        if self.potential is None:
            raise RuntimeError("No saved potential field.")
        if isinstance(axis, str) and axis in ("x", "y", "z"):
            axis = "xyz".index(axis)
        if axis not in (0, 1, 2):
            raise ValueError("Invalid axis: {0!r} (expected 0, 1, 2, 'x', 'y' or 'z').".format(axis))
        axis = int(axis)
        shape = self.plan_c2r.shape
        if factor_z is not None:
            factor = np.asarray(factor_z, float).reshape(shape[2])
        elif light_cone:
            factor = self._need_table("growth_function")
            if order == 2:
                factor = factor * factor
        else:
            factor = None
        dk = 2 * np.pi / (shape[axis] * self.grid_spacing_Mpc_h)
        # (second order: the 3/7 and the square of the first order's coefficient)
        coeff = scale if order == 1 else 3.0 / 7.0 * float(scale) ** 2
        return self._backend.gradient(order, axis, coeff, dk, factor, download)

    @_replaces_kspace
    def lpt2_source(self, download=True):
        """
        The source of the second-order potential, S(r) = sum over a < b of H_aa H_bb - H_ab**2 (see
        :meth:`calculate_displacement_field`, ``order=2``), of the saved potential.  Returns a view of the plan's buffer; on the
        hip backend S becomes the current device field (``download=False`` leaves it there).
        """
        if self.distributed:
            raise NotImplementedError("lpt2_source runs on single-GPU plans (distributed=False).")
        if self.potential is None:
            raise RuntimeError("No saved potential field.")
        return self._backend.lpt2_source(download)

    # ---- particles: the displaced lattice and its cloud-in-cell paint ---------
    def particle_displacements(self, order=2, D1=1.0, download=True, *, rsd_axis=None, f1=0.0, f2=None):
        """
        The Lagrangian displacements s = D1 psi1 (``order=1``) or D1 psi1 + D1**2 psi2 (``order=2``) of the lattice particles, one
        per cell, in Mpc/h -- from :meth:`calculate_displacement_field`, whose ``order=2`` term already carries the 3/7.  The three
        components are kept together (hip backend: in a device buffer, ``rf_particles_accumulate``) for :meth:`paint_particles`
        and :meth:`particle_positions`, until the next field is generated (``generate_delta_field`` / ``generate_density_field``
        drop them).  Returns a new ``(3, nx, ny, nz)`` array of the plan's real type, or None with ``download=False``.  The field
        buffer is left holding the last component transformed.

        Redshift space: with ``rsd_axis = a`` (0, 1, 2) the component along grid axis a alone takes the coefficients D1 (1 + f1) and
        D1**2 (1 + f2) -- formed in float64, then handled as the plain coefficients are -- which moves the particles along that one
        axis by their peculiar velocity in units of the Hubble flow: a plane-parallel line of sight.  ``f1`` is the linear growth
        rate d ln D1 / d ln a, ``f2`` the second-order one (``None``: 2 f1).  The two other components, the default call and the
        displacement fields of :meth:`calculate_displacement_field` are untouched.
        """
        if order not in (1, 2):
            raise ValueError("Invalid order: {0!r} (expected 1 or 2).".format(order))
        if rsd_axis is not None and rsd_axis not in (0, 1, 2):
            raise ValueError("Invalid rsd_axis: {0!r} (expected None, 0, 1 or 2).".format(rsd_axis))
        d1, d2 = float(D1), float(D1) * float(D1)
        coeffs = [(d1, d2)] * 3
        if rsd_axis is not None:
            g1 = float(f1)
            g2 = 2.0 * g1 if f2 is None else float(f2)
            coeffs[rsd_axis] = (d1 * (1.0 + g1), d2 * (1.0 + g2))
        for axis in range(3):
            for n in range(order):
                self.calculate_displacement_field(axis, order=n + 1, download=False)
                self._backend.accumulate_displacement(axis, coeffs[axis][n], first=n == 0)
        self._backend.displacements_complete()
        return self._download_particles() if download else None

    def set_particle_displacements(self, s):
        """Bring your own displacements: a ``(3, nx, ny, nz)`` array in Mpc/h, converted to the plan's real type (copied; kept until
        the next field is generated, as those of :meth:`particle_displacements`)."""
        if self.distributed:
            raise NotImplementedError("particles live on single-GPU plans (distributed=False).")
        s = np.asarray(s)
        if s.shape != (3,) + tuple(self.plan_c2r.shape):
            raise ValueError("displacements must have the shape {0}.".format((3,) + tuple(self.plan_c2r.shape)))
        self._backend.set_displacements(np.ascontiguousarray(s, self.plan_c2r.data_out.dtype))

    def _download_particles(self):
        self._need_particles()
        return self._backend.download_displacements()

    def particle_positions(self):
        """float64 ``(3, nx, ny, nz)``: (q h + s) mod L per axis, q the lattice index, h the grid spacing, L = n h the box length."""
        Q = self._download_particles()
        h = float(self.grid_spacing_Mpc_h)
        out = np.empty(Q.shape, np.float64)
        for axis, n in enumerate(self.plan_c2r.shape):
            q = np.arange(n, dtype=np.float64).reshape([-1 if a == axis else 1 for a in range(3)])
            out[axis] = np.mod(q * h + Q[axis].astype(np.float64), n * h)
        return out

    def paint_particles(self, download=True, *, assignment="cic", interlaced=False):
        """
        Cloud-in-cell mass assignment of the displaced particles onto the grid: delta_cic = (mass per cell) - 1 becomes the current
        field, so ``measure_power_spectrum()`` with no argument measures the particles.  The weights are integers in units of
        2**-16 per axis, summed in a ``uint64`` grid: the result is the same bit for bit on every call (hip backend:
        ``rf_particles_paint``, integer atomics).  Particles with a non-finite displacement are dropped and counted in
        ``self.particles_dropped``.  Fewer than 65536 particles' worth of mass may land in one cell.  Returns the field, or None
        with ``download=False``.

        ``assignment``: ``'cic'`` (two cells per axis) or ``'tsc'``, the triangular-shaped cloud over three cells per axis with
        integer weights of the same unit (``particles.py``; hip backend: ``rf_particles_paint_ex``), bit for bit the same on both
        backends.  Pass the same name as ``window=`` to :meth:`measure_power_spectrum` / :meth:`measure_power_multipoles` to divide
        the assignment window out of the painted field: ``window='cic'`` after ``assignment='cic'``, ``window='tsc'`` after ``'tsc'``.

        ``interlaced=True`` (Sefusatti et al. 2016): the particles are painted a second time on a grid shifted by half a cell on
        every axis and the two spectra are combined with the phase that undoes the shift, ``(delta1 + p delta2) / 2`` with the
        tables of ``powertools.interlace_phases``: every aliased image with an odd sum of image indices cancels, the dominant first
        image on each axis among them, which the window compensation alone does not remove.  The current field, and the array
        returned, is the inverse transform of the combined spectrum; the spectrum itself is kept, and
        ``measure_power_spectrum(source='kspace', window=...)`` / ``measure_power_multipoles(source='kspace', ...)`` measure it
        without another transform.  hip backend: ``rf_particles_paint_interlaced``, everything on the device.  numpy backend:
        ``rfftn`` / ``irfftn`` in float64 on the two deltas as rounded to the plan's real type.
        """
        order = _assignment_order(assignment)
        self._need_particles()
        inv_h = [1.0 / float(self.grid_spacing_Mpc_h)] * 3
        self._backend.interlaced = None
        tables = powertools.interlace_phases(tuple(self.plan_c2r.shape)) if interlaced else None
        self.particles_dropped = self._backend.paint(inv_h, order, tables)
        return self.download_field() if download else None

    def interpolate_at_particles(self, field=None, *, slot=0, coeff=1.0, first=True, download=True, assignment="cic"):
        """
        Cloud-in-cell interpolation of a field at the displaced particles, the adjoint of :meth:`paint_particles` over the same
        cells and integer weights: what carries a grid field -- a force component, a reconstruction displacement, the density --
        back to the particles.  ``field=None`` gathers the current field (the one on the device, hip backend; ``plan_c2r.data_out``,
        numpy backend); an ``(nx, ny, nz)`` array is uploaded first and becomes the current field, as in
        :meth:`measure_power_spectrum`.  The field is left as it is.

        The values go to one of three slots (``slot`` 0, 1, 2: the components of a vector field can be gathered at the same
        positions before :meth:`shift_particles` moves anything): ``G[slot] = coeff * g`` with ``first=True``, otherwise
        ``G[slot] + coeff * g``, g formed in float64 and the sum rounded once to the plan's real type -- the same bits on both
        backends and on every call (hip backend: ``rf_particles_gather``, no atomics).  A particle with a non-finite displacement
        gathers 0 and is counted in ``self.particles_dropped``.  The gathered values are kept until the next field is generated, as
        the displacements are.  Returns a new ``(nx, ny, nz)`` array indexed by the particle's lattice cell, or None with
        ``download=False``.

        ``assignment``: ``'cic'`` or ``'tsc'``, the kernel of :meth:`paint_particles` with the same name (hip backend:
        ``rf_particles_gather_ex``).  Gathering with the kernel the density was painted with puts the same window on both legs (no
        self-force); a field measured from that painted density takes ``window=`` of the same name in
        :meth:`measure_power_spectrum` / :meth:`measure_power_multipoles`.
        """
        order = _assignment_order(assignment)
        if self.distributed:
            raise NotImplementedError("particles live on single-GPU plans (distributed=False).")
        self._check_slot(slot)
        self._need_particles()
        if field is not None:
            self._make_current(field)                            # (as measure_power_spectrum(field=...) does)
        inv_h = [1.0 / float(self.grid_spacing_Mpc_h)] * 3
        self.particles_dropped, values = self._backend.gather(inv_h, slot, coeff, first, order, download)
        return values

    def shift_particles(self, axis, slot=None, coeff=1.0):
        """Move the particles along ``axis`` by the gathered values: ``s[axis] += coeff * G[slot]`` (``slot=None``: the slot of the
        same number as the axis), one fused multiply-add in the plan's real type (hip backend: ``rf_particles_shift``)."""
        if axis not in (0, 1, 2):
            raise ValueError("Invalid axis: {0!r} (expected 0, 1 or 2).".format(axis))
        slot = axis if slot is None else slot
        self._check_slot(slot)
        self._need_particles()
        if self._backend.gathered is None:
            raise RuntimeError("No gathered values: call interpolate_at_particles() first.")
        self._backend.shift(axis, slot, coeff)

    @_replaces_kspace
    def calculate_lensing_potential(self, i_min=None, show_plot=False, save_plot_name=None):
        """
        Calculate the lensing potential psi(r) (generate.py:352-416):

            psi(r, z) = integral from D_min to D_src of -2 [cotK(D) - cotK(D_src)] dPhi(r, z) dD

        with the reference's Simpson rule along z, D_min = ``DC[i_min]`` (default nz // 32).
        Call :meth:`calculate_newtonian_potential` (``light_cone=True``) just before.  Needs the
        ``transverse_distance=`` table (and ``curvature_K=`` for a curved cosmology).

        Returns a new array; the plan's buffer (the Newtonian potential) is not modified.  On the
        hip backend the O(nz**2)-per-column loop of the reference runs as one prefix scan per row.
        """
        if show_plot or save_plot_name is not None:
            raise NotImplementedError("plot_slice is outside the accelerated path (see DESIGN.md).")
        nDC = self.DC.size
        if i_min is None:
            i_min = nDC // 32
        if i_min < 0 or i_min >= nDC:
            raise ValueError("Invalid i_min {}. Expected 0 - {}.".format(i_min, nDC - 1))
        DA = self._need_table("DA")
        K = self.curvature_K
        if K < 0:
            cosK = np.cosh(np.sqrt(-K) * self.DC)
        elif K > 0:
            cosK = np.cos(np.sqrt(K) * self.DC)
        else:
            cosK = np.ones_like(DA, dtype=float)
        cotK = np.ones_like(cosK)
        cotK[1:] = cosK[1:] / DA[1:]
        return self._backend.lensing(cotK, i_min)

    def plot_slice(self, *args, **kwargs):
        raise NotImplementedError("plot_slice is outside the accelerated path (see DESIGN.md).")
