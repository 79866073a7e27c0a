#!/usr/bin/env python3
"""Does a build of librandomfield_hip.so launch the tiled kernels as another build does?

    python tools/launch_parity.py [path/to/librandomfield_hip.so] > digests.txt

Prints one line per result -- `shape dtype call: sha256` -- for fields, k space, moments and potentials over a matrix of tiny grids chosen
so that every branch of the tiled launchers is reached (rf_select.h: whole columns and Col2 halves, split and unsplit generation passes,
tile pairs, the side buffer and the owning lane's repair, the merged y+z launch, 64-bit lane offsets ...), and, first, over every
exchanging form of a plan's route (rf_route.h: grouped copy or storing y pass, whole or in sub-slabs, single calls and pipelined batches, the
two stand-ins of a virtual rank), and, last, over the MT19937 replay (replay_lines).  A call the library refuses
prints the refusal text instead of a digest.  Run it once per build (the default is the library of this tree) and diff the two outputs:
every line must be equal.  Under `rocprofv3 --kernel-trace -- python tools/launch_parity.py LIB` the ordered list of (kernel, grid,
workgroup) of two builds can be compared the same way.  Each call takes milliseconds; this is a comparison tool, not a test of values."""
import ctypes
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from randomfield_amd import _hip, powertools  # noqa: E402

SPACING = 2.5
SHAPES = [(8, 8, 16), (64, 32, 128), (512, 8, 32), (1024, 8, 32), (1024, 8, 64), (2048, 8, 16), (2048, 8, 32), (8, 1024, 64), (8, 2048, 32),
          (8, 1024, 1024)]
MERGED = (8, 1024, 1024)          # with the y / z passes slab by slab: queue_yz takes the merged sequence (float32)
LINES = []


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def record(key, fn):
    """fn() -> arrays to digest; a refusal (RuntimeError / ValueError) is recorded by its text"""
    try:
        out = fn()
        val = sha(*out) if isinstance(out, (tuple, list)) else sha(out)
    except (RuntimeError, ValueError) as exc:
        val = "REFUSED " + " ".join(str(exc).split())
    LINES.append("%s: %s" % (key, val))
    print(LINES[-1], flush=True)


def tables(plan, power):
    nx, ny, nz = plan.nx, plan.ny, plan.nz
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
    plan.set_power(*powertools.sigma_table(power, (nx, ny, nz), SPACING))
    return plan


def field(plan):
    return plan.download_real(), np.array(plan.moments())


def potential(plan):
    plan.load_potential(1.0)
    return plan.download_k()


def single_plan(shape, dtype, power, key):
    nx, ny, nz = shape
    f32 = np.dtype(dtype) == np.dtype(np.complex64)
    noise = np.random.RandomState(5).normal(size=2 * nx * ny * (nz // 2 + 1))
    plan = tables(_hip.DevicePlan(nx, ny, nz, dtype), power)

    def then(call, result=field):
        def run():
            call()
            return result(plan)
        return run

    record(key + " realise native", then(lambda: plan.realise(seed=11)))
    record(key + " r2c", then(plan.execute_r2c, lambda p: p.download_k()))
    plan.set_exact_generation(True)
    record(key + " realise exact", then(lambda: plan.realise(seed=11)))
    plan.set_exact_generation(False)
    record(key + " realise host noise", then(lambda: plan.realise(noise=noise)))
    record(key + " generate + c2r", then(lambda: (plan.generate(seed=12), plan.execute_c2r())))
    record(key + " realise_potential native", then(lambda: plan.realise_potential(seed=11), lambda p: field(p) + (potential(p),)))
    record(key + " realise_potential host noise", then(lambda: plan.realise_potential(noise=noise), lambda p: field(p) + (potential(p),)))
    fz = np.linspace(0.5, 1.5, nz)
    record(key + " scaled potential native", then(lambda: plan.realise_scaled_potential(seed=11, scale=-1.5)))
    record(key + " scaled potential native z", then(lambda: plan.realise_scaled_potential(seed=11, scale=-1.5, factor_z=fz)))
    plan.set_z_tables(np.linspace(1.0, 0.5, nz), np.linspace(0.9, 1.1, nz))
    record(key + " lognormal", then(lambda: plan.realise_lognormal(seed=11)))
    for single in ([False, True] if f32 else [False]):
        tag = key + (" deviates32" if single else " deviates64")
        record(tag + " replay", lambda: np.array([plan.reference_noise(321, single=single)], np.uint64))
        record(tag + " realise", then(lambda: plan.realise(noise="resident")))
        record(tag + " realise_potential", then(lambda: plan.realise_potential(noise="resident"), lambda p: field(p) + (potential(p),)))
        record(tag + " scaled potential", then(lambda: plan.realise_scaled_potential(noise="resident", scale=2.0)))
        record(tag + " lognormal", then(lambda: plan.realise_lognormal(noise="resident")))
    plan.set_transposed_intermediate(True)
    record(key + " transposed realise", then(lambda: plan.realise(seed=11)))
    record(key + " transposed host noise", then(lambda: plan.realise(noise=noise)))
    plan.set_transposed_intermediate(False)
    plan.set_yz_slab_planes(2)
    if shape == MERGED:
        plan.set_merged_yz(2)
    record(key + " yz slabs realise", then(lambda: plan.realise(seed=11)))
    if shape == MERGED:
        LINES.append("%s merged launch count: %s" % (key, _try(lambda: plan.merged_yz_ms()[1])))
        print(LINES[-1], flush=True)
        plan.set_merged_yz(1)
    record(key + " yz slabs scaled potential z", then(lambda: plan.realise_scaled_potential(seed=11, scale=-1.5, factor_z=fz)))
    plan.set_yz_slab_planes(-1)
    record(key + " batch n=2", lambda: (plan.realise_batch(np.array([3, 4], np.uint64)), plan.download_real()))
    plan.set_force_slab_path(True)
    record(key + " slab path realise", then(lambda: plan.realise(seed=11)))
    record(key + " slab path direct", then(lambda: (plan.enable_direct_exchange(True), plan.realise(seed=11))))
    record(key + " slab path direct batch", lambda: (plan.realise_batch(np.array([3, 4], np.uint64)), plan.download_real()))
    plan.close()


def _try(fn):
    try:
        return fn()
    except (RuntimeError, ValueError) as exc:
        return "REFUSED " + " ".join(str(exc).split())


def virtual_ranks(shape, dtype, power, key, nranks=2):
    nx, ny, nz = shape
    plans = []
    try:
        for r in range(nranks):
            plans.append(tables(_hip.DevicePlan(nx, ny, nz, dtype, nranks=nranks, rank=r), power))
    except (RuntimeError, ValueError) as exc:
        LINES.append("%s ranks=%d: REFUSED %s" % (key, nranks, " ".join(str(exc).split())))
        print(LINES[-1], flush=True)
        for p in plans:
            p.close()
        return

    def pipeline(direct, **forward):
        def run():
            for p in plans:
                p.slab_forward(**forward)
            if not direct:
                _hip.DevicePlan.slab_exchange_local(plans)
            for p in plans:
                p.slab_backward()
            return [p.download_real() for p in plans] + [np.array(p.slab_stats()) for p in plans]
        return run

    tag = "%s ranks=%d" % (key, nranks)
    noise = np.random.RandomState(5).normal(size=2 * nx * ny * (nz // 2 + 1))
    record(tag + " pipeline native", pipeline(False, seed=11))
    record(tag + " pipeline host noise", pipeline(False, noise=noise))
    record(tag + " pipeline potential", pipeline(False, seed=11, source="potential"))
    for chunks in (1, 2):
        record(tag + " chunks=%d" % chunks, lambda: [p.set_exchange_chunks(chunks) for p in plans] and pipeline(False, seed=11)())
        record(tag + " chunks=%d link" % chunks, lambda: np.array([0]) if _hip.DevicePlan.slab_link_direct(plans) is None else np.array([1]))
        record(tag + " chunks=%d direct native" % chunks, pipeline(True, seed=11))
        record(tag + " chunks=%d direct host noise" % chunks, pipeline(True, noise=noise))
        record(tag + " chunks=%d unlink" % chunks, lambda: np.array([0]) if _hip.DevicePlan.slab_link_direct(plans, False) is None else np.array([1]))
    record(tag + " chunks reset", lambda: np.array([p.set_exchange_chunks(1) is None for p in plans]))
    for p in plans:
        record(tag + " rank %d replicated" % p.rank, lambda: (p.set_replicated_generation(True), p.realise(seed=11), p.download_real(), np.array(p.slab_stats()))[2:])
        record(tag + " rank %d replicated batch" % p.rank, lambda: (p.realise_batch(np.array([3, 4], np.uint64), want_rms=False), p.download_real())[1:])
        p.close()


def c2c_plan(shape, dtype, key):
    nx, ny, nz = shape
    try:
        plan = _hip.DevicePlan(nx, ny, nz, dtype, unpacked=True)
    except (RuntimeError, ValueError) as exc:
        LINES.append("%s c2c: REFUSED %s" % (key, " ".join(str(exc).split())))
        print(LINES[-1], flush=True)
        return
    rng = np.random.RandomState(7)
    data = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype)
    record(key + " c2c forward", lambda: (plan.upload_c(data), plan.execute_c2c(False), plan.download_c())[2:])
    record(key + " c2c inverse", lambda: (plan.execute_c2c(True), plan.download_c())[1:])
    plan.close()


def exchanging_forms(shape, dtype, power, key):
    """Every exchanging form of the single calls and of the pipelined batch on a single-rank plan forced onto the slab path: grouped
    copy or storing y pass, whole or in two sub-slabs (a single-rank plan runs the direct form with direct_overlap = 1, the default:
    only the stand-in below sets it)."""
    nx, ny, nz = shape
    noise = np.random.RandomState(5).normal(size=2 * nx * ny * (nz // 2 + 1))
    seeds = np.array([3, 4, 5], np.uint64)
    plan = tables(_hip.DevicePlan(nx, ny, nz, dtype), power)
    plan.set_force_slab_path(True)
    for direct in (False, True):
        for chunks in (1, 2):
            tag = "%s forced slab %s chunks=%d" % (key, "direct" if direct else "rccl", chunks)
            record(tag + " set", lambda: np.array([plan.set_exchange_chunks(chunks) is None, plan.enable_direct_exchange(direct)]))
            record(tag + " realise native", lambda: ((plan.realise(seed=11),) + field(plan))[1:])
            record(tag + " realise host noise", lambda: ((plan.realise(noise=noise),) + field(plan))[1:])
            record(tag + " realise_potential native", lambda: ((plan.realise_potential(seed=11),) + field(plan) + (potential(plan),))[1:])
            record(tag + " realise_potential host noise", lambda: ((plan.realise_potential(noise=noise),) + field(plan) + (potential(plan),))[1:])
            record(tag + " batch n=3", lambda: (plan.realise_batch(seeds), plan.download_real(), np.array(plan.moments())))
    plan.close()


def standin_tails(shape, dtype, power, key):
    """One rank of a 2-rank job without a communicator under the two stand-ins: the real schedule of a multi-GPU rank, whose result is
    not a field -- the download's refusal is the record, the local moments come out"""
    nx, ny, nz = shape
    seeds = np.array([3, 4, 5], np.uint64)
    try:
        plan = tables(_hip.DevicePlan(nx, ny, nz, dtype, nranks=2, rank=1), power)
    except (RuntimeError, ValueError) as exc:
        LINES.append("%s stand-in: REFUSED %s" % (key, " ".join(str(exc).split())))
        print(LINES[-1], flush=True)
        return

    def calls(tag):
        record(tag + " realise moments", lambda: (plan.realise(seed=11), np.array(plan.moments()))[1:])
        record(tag + " realise field", plan.download_real)
        record(tag + " batch n=3 rms", lambda: (plan.realise_batch(seeds), np.array(plan.moments())))
        record(tag + " batch n=3 field", plan.download_real)

    for chunks in (1, 2):
        tag = "%s stand-in chunks=%d" % (key, chunks)
        record(tag + " set", lambda: np.array([plan.set_exchange_chunks(chunks) is None]))
        record(tag + " exchange on", lambda: np.array([plan.set_exchange_standin(8) is None]))
        calls(tag + " exchange")
        for overlap in (True, False):
            record(tag + " direct overlap=%d on" % overlap, lambda: np.array([plan.set_direct_standin(True, overlap) is None]))
            calls(tag + " direct overlap=%d" % overlap)
        record(tag + " direct off", lambda: np.array([plan.set_direct_standin(False) is None]))
    plan.close()


# the smallest power-of-two grids (float64, float32) on which rf_plan_set_flag takes 2 exchange chunks of a single-rank plan in direct mode
# (nz / 4 planes per sub-slab = one y-pass tile: col_direct_supported), the (64, 32, 128) of the matrix above, which takes them too, and
# (64, 32, 256), where a rank of a 2-rank job takes them as well (the stand-ins in sub-slabs)
ROUTE_SHAPES = [(8, 8, 64), (8, 8, 128), (64, 32, 128), (64, 32, 256)]


def replay_lines(power):
    """The MT19937 replay (rf_capi_mt.hip): the deviates and the accepted count of the whole-stream replay at segment lengths that grow
    the jump tree by one, two and three stages, the float32 form read by a realisation, the replay shared between two virtual ranks in
    both modes of its transport, a same-seed batch, and every share call made out of its order, recorded by its refusal"""
    def deviates(plan, accepted):
        return plan.download_noise(), np.array([accepted], np.uint64)

    for shape, bps in (((8, 8, 16), 1), ((8, 8, 16), 2), ((16, 16, 32), 1), ((32, 32, 64), 3)):
        key = "replay %dx%dx%d bps=%d" % (shape + (bps,))
        plan = tables(_hip.DevicePlan(*shape, np.complex64), power)
        plan.set_mt_segment_blocks(bps)
        record(key + " deviates64", lambda: deviates(plan, plan.reference_noise(321)))
        record(key + " deviates64 second seed", lambda: deviates(plan, plan.reference_noise((2026, 4, 0xFFFFFFFF, 7))))
        plan.close()
    key = "replay 32x32x64 default"
    plan = tables(_hip.DevicePlan(32, 32, 64, np.complex64), power)
    record(key + " deviates32 accepted", lambda: np.array([plan.reference_noise(321, single=True)], np.uint64))
    record(key + " deviates32 download", plan.download_noise)
    record(key + " deviates32 realise", lambda: (plan.realise(noise="resident"),) and field(plan))
    record(key + " batch reference", lambda: (plan.realise_batch_reference([321, 322]), plan.download_real(), np.array(plan.moments())))
    record(key + " batch reference realise", lambda: (plan.realise(noise="resident"),) and field(plan))
    plan.close()

    shape, key = (64, 64, 256), "replay 64x64x256 bps=1 ranks=2"
    plans = [tables(_hip.DevicePlan(*shape, np.complex64, nranks=2, rank=r), power) for r in range(2)]
    for p in plans:
        p.set_mt_segment_blocks(1)
    for single in (False, True):
        tag = key + (" float32" if single else " float64")
        record(tag + " shared", lambda: np.array(_hip.DevicePlan.reference_noise_shared_local(plans, 141, single=single), np.uint64))
        for p in plans:
            record(tag + " rank %d deviates" % p.rank, p.download_noise)
    # the share calls out of order: before any replay, after the replay, after the pack, after the exchange, after the end
    p, arr = plans[1], (ctypes.c_void_p * 2)(*[q._h.value for q in plans])
    nseg = p.share_segments()[0]
    calls = [("gather", p.share_gather), ("pack", lambda: p.share_pack(np.zeros(nseg, np.uint64))), ("exchange", p.share_exchange),
             ("exchange_local", lambda: _hip.check(_hip.load().rf_mt_share_exchange_local(arr, 2), "rf_mt_share_exchange_local")),
             ("finish", p.share_finish)]

    def done(tag, call):
        record("%s %s" % (key, tag), lambda: (call(), np.array([0]))[1:])

    def out_of_order(tag, skip=()):
        for name, call in calls:
            if name not in skip:
                done("out of order %s: %s" % (tag, name), call)

    def begin_and_pack(modes):
        counts = np.concatenate([q.share_begin(141, single) for q, single in zip(plans, modes)])
        for q in plans:
            q.share_pack(counts)

    out_of_order("idle")
    done("begin", lambda: [q.share_begin(141, True) for q in plans])
    out_of_order("replayed", skip=("pack",))                 # (gather: refused for the communicator it lacks, not for the step)
    done("begin and pack", lambda: begin_and_pack((True, True)))
    out_of_order("packed", skip=("exchange", "exchange_local"))
    done("rank 0 replayed again", lambda: plans[0].share_begin(141, True))
    done("out of order rank 0 replayed again: exchange_local", calls[3][1])
    done("begin and pack in two modes", lambda: begin_and_pack((False, True)))
    done("out of order packed in two modes: exchange_local", calls[3][1])
    done("begin and pack again", lambda: begin_and_pack((True, True)))
    done("exchange_local", calls[3][1])
    out_of_order("exchanged", skip=("finish",))
    record(key + " finish", lambda: np.array([q.share_finish() for q in plans], np.uint64))
    out_of_order("finished")
    for q in plans:
        record(key + " after the calls rank %d deviates" % q.rank, q.download_noise)
        q.close()


def main():
    if len(sys.argv) > 1:
        _hip.LIB_PATH = os.path.abspath(sys.argv[1])
    _hip.require_gpu()
    power = powertools.load_default_power()
    for shape in ROUTE_SHAPES:
        for dtype in (np.complex64, np.complex128):
            key = "%dx%dx%d %s" % (shape + (np.dtype(dtype).name,))
            exchanging_forms(shape, dtype, power, key)
            standin_tails(shape, dtype, power, key)
    for shape in SHAPES:
        for dtype in (np.complex64, np.complex128):
            key = "%dx%dx%d %s" % (shape + (np.dtype(dtype).name,))
            supported = _hip.shape_supported(*shape, dtype=dtype)
            LINES.append("%s shape_supported: %d" % (key, supported))
            print(LINES[-1], flush=True)
            if supported:
                single_plan(shape, dtype, power, key)
                virtual_ranks(shape, dtype, power, key)
            c2c_plan(shape, dtype, key)
    replay_lines(power)
    print("# %d lines, sha256 of all: %s" % (len(LINES), hashlib.sha256("\n".join(LINES).encode()).hexdigest()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
