"""A recording stand-in for ``_hip.DevicePlan`` (tests/test_generator_device_calls.py): no library, no GPU.  Every method call is
appended to a log as text -- the name, scalars by ``repr``, arrays as dtype and shape -- and answered from a table the test sets
per case.  ``power_epoch``, ``noise_epoch`` and ``lpt2_valid`` move as the real plan's do; ``tiled`` follows the shape (powers of
two), ``nranks`` is 1.  A plan that is not tiled arms no host sink and serves no reference batch, whatever the table says, as the
real one."""
import numpy as np

ANSWERS = dict(arm_host_sink=True, host_sink_delivered=True, can_batch_reference=True, can_regenerate_potential=True,
               moments=(0.0, 1.25), realise_lognormal=0.75, particles_paint=3, particles_paint_interlaced=5, particles_gather=7)


def text(value):
    if isinstance(value, np.ndarray):
        return "%s%r" % (value.dtype.name, tuple(value.shape))
    if isinstance(value, np.generic):
        return repr(value.item())
    if isinstance(value, (list, tuple)):
        body = ", ".join(text(v) for v in value)
        return "[%s]" % body if isinstance(value, list) else "(%s)" % body
    return repr(value)


def make_plan_class(log, answers, raising=()):
    """a DevicePlan class that writes to ``log`` and answers from ``answers``; the methods named in ``raising`` (a mutable
    collection) raise a plain RuntimeError after they are recorded"""

    class RecordingPlan(object):
        def __init__(self, nx, ny, nz, dtype=np.complex64, device=0, nranks=1, rank=0, unpacked=False):
            self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
            self.nranks, self.rank, self.nx_local = 1, 0, int(nx)
            self.tiled = all(n >= 8 and n & (n - 1) == 0 for n in (self.nx, self.ny, self.nz))
            self.complex_dtype = np.dtype(dtype)
            self.real_dtype = np.dtype(np.float32 if self.complex_dtype == np.complex64 else np.float64)
            self.noise_epoch = self.power_epoch = 0
            self.lpt2_valid = False
            self.nbytes = 0
            self._power_key = None
            log.append("DevicePlan(%d, %d, %d, %s, unpacked=%r)" % (self.nx, self.ny, self.nz, self.complex_dtype.name, bool(unpacked)))

        @property
        def k_shape(self):
            return (self.nx, self.ny, self.nz // 2 + 1)

        def _real(self):
            return np.zeros((self.nx, self.ny, self.nz), self.real_dtype)

        def __getattr__(self, name):
            if name.startswith("_"):
                raise AttributeError(name)

            def call(*args, **kwargs):
                log.append("%s(%s)" % (name, ", ".join([text(a) for a in args] + ["%s=%s" % (k, text(v)) for k, v in kwargs.items()])))
                if name in raising:
                    raise RuntimeError("stand-in: %s failed" % name)
                return getattr(self, "_do_" + name, lambda *a, **k: None)(*args, **kwargs)
            return call

        # ---- the calls whose answer or side effect the Generator can see ----
        def _do_set_kgrid(self, *tables):
            self._power_key = None
            self.power_epoch += 1

        def _do_set_power(self, log10k, sigma, if_changed=False):
            key = (np.asarray(log10k, np.float64).tobytes(), np.asarray(sigma, np.float64).tobytes())
            if if_changed and key == self._power_key:
                return False
            self.power_epoch += 1
            self._power_key = key
            return True

        def _bump_noise(self, *args, **kwargs):
            self.noise_epoch += 1
            return 0

        _do_reference_noise = _do_realise_batch_reference = _bump_noise

        def _do_arm_host_sink(self, out, padded=False):
            return bool(self.tiled and answers["arm_host_sink"])

        def _do_host_sink_delivered(self):
            return bool(answers["host_sink_delivered"])

        def _do_can_batch_reference(self):
            return bool(self.tiled and answers["can_batch_reference"])

        def _do_can_regenerate_potential(self, noise=None):
            return bool(answers["can_regenerate_potential"])

        def _do_moments(self):
            return answers["moments"]

        def _do_realise_lognormal(self, seed=0, noise=None, want_sigma=True):
            return answers["realise_lognormal"]

        def _do_realise_potential(self, seed=0, noise=None):
            self.lpt2_valid = False

        _do_save_potential = _do_lpt2_source = _do_realise_potential

        def _do_lpt2_potential(self, dk):
            self.lpt2_valid = True

        def _do_download_k(self, out=None):
            return np.zeros(self.k_shape, self.complex_dtype)

        def _do_download_real(self, out=None, padded=False, x0=0, x1=None):
            return out

        def _do_download_aux(self, *args, **kwargs):
            return self._real()

        def _do_particles_download(self, axis, out=None):
            return self._real()

        def _do_particles_gather_download(self, slot, out=None):
            return self._real()

        def _do_particles_paint(self, *args, **kwargs):
            return answers["particles_paint"]

        def _do_particles_paint_interlaced(self, *args, **kwargs):
            return answers["particles_paint_interlaced"]

        def _do_particles_gather(self, *args, **kwargs):
            return answers["particles_gather"]

        def _do_measure_power(self, edges, source=None):
            n = len(edges) - 1
            return np.ones(n, np.uint64), np.ones(n), np.ones(n)

        def _do_measure_multipoles(self, edges, los, source=None, compensation=None):
            n = len(edges) - 1
            return (np.ones(n, np.uint64),) + tuple(np.ones(n) for _ in range(4))

    return RecordingPlan


def install(monkeypatch, log, answers, raising=()):
    """``_hip.require_gpu`` and ``_hip.shape_supported`` accept, ``_hip.DevicePlan`` records"""
    from randomfield_amd import _hip
    monkeypatch.setattr(_hip, "require_gpu", lambda: 1)
    monkeypatch.setattr(_hip, "shape_supported", lambda *args, **kwargs: True)
    monkeypatch.setattr(_hip, "DevicePlan", make_plan_class(log, answers, raising))
