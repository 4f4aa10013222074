"""Life cycle of the context's device memory over EVERY family of buffers, through the public Python API only: contexts
that have run every call which allocates on first use or grows a buffer are created and destroyed in turn, fwi_destroy
reports no refused free ("fwi_destroy: hipFree(<member>[<index>]): ..." in fwi_last_error(NULL)), and free device memory
ends where it was after a warm-up cycle.

Measurement and bound are those of test_gpu_placement.py::test_destroy_gives_back_every_placed_array: one warm-up cycle
(the runtime's own first-use allocations are not leaks), a reading of free device memory, four cycles, and at most
14 MiB (the pad of one placed array) between that reading and the last.  The small contexts here could leak a buffer and
stay below it; what this file is for is the free the runtime refuses and the pointer freed twice, which show in the
message, at every size."""
import ctypes as C

import numpy as np
import pytest

from full_waveform_inversion_amd import Engine, _lib
from full_waveform_inversion_amd.datafit import hilbert_taps
from full_waveform_inversion_amd.points import Spread

pytestmark = pytest.mark.gpu
MIB = 1 << 20
BOUND = 14 * MIB
FIXED = "fixed:1,3,5,7,2"  # every movable array at its own non-zero offset (test_gpu_placement.py)


def _free_bytes():
    hip = C.CDLL("libamdhip64.so")
    fr, tot = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return fr.value


def _run(what, cycle):
    """One warm-up cycle, four measured ones; no refused free after any destroy, free memory back within BOUND"""
    lib = _lib.load()

    def once(i):
        cycle()
        msg = lib.fwi_last_error(None) or b""
        assert not msg.startswith(b"fwi_destroy:"), (i, msg.decode())

    once(-1)
    start = _free_bytes()
    for i in range(4):
        once(i)
    drift = start - _free_bytes()
    print("life cycle %s: free memory fell by %.2f MiB over 4 cycles" % (what, drift / MIB))
    assert abs(drift) <= BOUND, "four cycles of %s lost %.1f MiB of device memory" % (what, drift / MIB)


# ---------------------------------------------------------------------------------------------------------------------
# 2-D: every on-demand family on one context (nx % 4 != 0: host arrays cross through the `logical` staging buffer)
# ---------------------------------------------------------------------------------------------------------------------
def _cycle_2d(dtype):
    shape, h, dt, nt, nt_max = (24, 30), 10.0, 1e-3, 40, 70
    rng = np.random.default_rng(7)
    c = (2000.0 + 300.0 * rng.random(shape)).astype(dtype)
    src = [[11.3, 14.6]]
    rec = np.stack([3.0 + 17.0 * rng.random(5), 2.0 + 25.0 * rng.random(5)], 1)
    wav = rng.standard_normal(nt).astype(dtype)
    taps = np.array([1.0, 0.5, 0.3, 0.2, 0.1, 0.05, 0.02, 0.01])  # R = 7
    with Engine(shape, h, dt, nt_max, order=4, npml=4, sigma_max=200.0, dtype=dtype) as e:
        # 1. off-grid points: the spread sets, pts_a / pts_d
        d = e.forward_at(c, (src, wav), rec, save=True)
        assert np.isfinite(d).all() and np.abs(d).max() > 0
        d_obs = (0.9 * d + 0.05 * np.abs(d).max() * rng.standard_normal(d.shape)).astype(dtype)
        amax = float(np.abs(d_obs).max())
        W = (0.5 + rng.random(d.shape)).astype(dtype)
        TW = 0.25 + rng.random(d.shape[1])
        # 2. every data misfit once, with weights, taps and trace weights where the call takes them
        e.misfit_l2(d_obs)
        e.misfit_weighted(d_obs, W, taps)
        e.misfit_matched(d_obs, 2, 1e-3 * float((d_obs.astype(np.float64) ** 2).sum()) + 1e-12, W, taps)
        e.misfit_envelope(d_obs, hilbert_taps(3), power=2, eps=0.01 * amax, weights=W, taps=taps)
        e.misfit_correlation(d_obs, 0.01 * amax, W, taps, TW)
        e.misfit_traveltime(d_obs, 6, W, taps, TW)
        e.misfit_transport(d_obs, "linear", 50.0 * amax, W, taps, TW)
        e.misfit_adaptive(d_obs, 4, 1e-2, W, taps, TW)
        freqs = np.arange(1, 4) / (nt * dt)
        e.misfit_spectral(d_obs, freqs, "l2", 0.01 * amax, W, taps, np.linspace(1.0, 2.0, 3), TW)
        e.residual_median(d_obs, W, taps)
        e.misfit_robust(d_obs, "huber", 0.1 * amax, W, taps, TW, keep_irls=True)
        # 3. the misfit's residual back
        e.adjoint(None)
        g = e.gradient()
        assert np.isfinite(g).all()
        # 4. Born data, then both Gauss-Newton weights on them
        e.born((10.0 * rng.standard_normal(shape)).astype(dtype))
        e.residual_weight(W, taps)
        e.residual_weight_robust(taps)
        # 5. a longer shot with more receivers: every buffer that follows the shot's size grows
        rec2 = np.stack([3.0 + 17.0 * rng.random(9), 2.0 + 25.0 * rng.random(9)], 1)
        d2 = e.forward_at(None, (src, rng.standard_normal(nt_max).astype(dtype)), rec2, save=True)
        e.misfit_weighted((0.9 * d2).astype(dtype), (0.5 + rng.random(d2.shape)).astype(dtype), taps)
        # 6. illumination on, one forward / adjoint pair, off again
        e.set_illumination(True)
        rec_idx = [[3, 4], [20, 25], [12, 7]]
        dd = e.forward(None, ([[12, 15]], wav), rec_idx, save=True)
        e.adjoint(dd)
        assert np.isfinite(e.illumination()).all()
        e.set_illumination(False)
        # 7. the Fourier store (refused while illumination is on, hence behind it), spectral imaging, off again
        e.set_fourier_store(freqs)
        dd = e.forward(None, ([[12, 15]], wav), rec_idx, save=True)
        e.adjoint_spectral(dd)
        assert np.isfinite(e.fourier_gradient()).all()
        e.set_fourier_store(None)
        # 8. the optimiser's vectors and the scratch arrays of their first calls
        e.vec_create(3)
        e.vec_upload(0, c)
        e.vec_smooth(0, 1.5)
        e.vec_regularizer(0, out=1, kind="tikhonov")
        assert np.isfinite(e.vec_dot(0, 1))
        # 9. first arrivals from the source, read at the receivers
        e.eikonal(src[0], 0, 1)
        assert np.isfinite(e.eikonal_times(0, Spread(rec, shape))).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_every_family_2d(gpu, dtype):
    _run("2-D %s" % dtype, lambda: _cycle_2d(dtype))


# ---------------------------------------------------------------------------------------------------------------------
# 3-D fp32 under FWI_PLACEMENT_TUNE=fixed: moved arrays, the checkpoint buffers, the bf16 store
# ---------------------------------------------------------------------------------------------------------------------
PLACED = {"increment": dict(update_form="increment"),
          "cpml": dict(abc="cpml", pml_alpha_max=20.0),
          "cpml_increment": dict(abc="cpml", pml_alpha_max=20.0, update_form="increment")}
# The checkpointed and the bf16 context are standard-form sponge contexts, which place nothing and ignore "fixed:"
# (test_gpu_placement.py::test_contexts_that_place_nothing_ignore_fixed; bf16 exists in no other form): the condition
# "pointers were moved" cannot hold for them and is asserted for the contexts that place.  The checkpointed
# increment-form context is there so that the checkpoint buffers (with fwv) are also freed beside moved pointers.
SMALL = {"ckpt": (dict(ckpt_interval=4), False),
         "bf16": (dict(store_dtype="bf16"), False),
         "ckpt_increment": (dict(ckpt_interval=4, update_form="increment"), True)}


def _cycle_3d(shape, npml, kw, moved):
    rng = np.random.default_rng(11)
    c = (2000.0 + 300.0 * rng.random(shape)).astype(np.float32)
    w = rng.standard_normal(12).astype(np.float32)
    with Engine(shape, 10.0, 1e-3, 12, npml=npml, sigma_max=200.0, **kw) as e:
        assert any(e.placement_info()[2]) == moved
        dd = e.forward(c, ([[s // 2 for s in shape]], w), [[3, 4, 5], [s - 4 for s in shape]], save=True)
        e.adjoint(dd)
        assert np.isfinite(e.gradient()).all()


@pytest.mark.parametrize("kind", list(PLACED))
def test_placed_3d(gpu, monkeypatch, kind):
    monkeypatch.setenv("FWI_PLACEMENT_TUNE", FIXED)
    _run("3-D placed %s" % kind, lambda: _cycle_3d((80, 72, 96), 8, PLACED[kind], True))


@pytest.mark.parametrize("kind", list(SMALL))
def test_checkpoint_and_bf16_3d(gpu, monkeypatch, kind):
    monkeypatch.setenv("FWI_PLACEMENT_TUNE", FIXED)
    kw, moved = SMALL[kind]
    _run("3-D %s" % kind, lambda: _cycle_3d((24, 20, 28), 3, kw, moved))
