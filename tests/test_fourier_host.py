"""The Fourier-compressed forward-term store without a GPU: the NumPy twin's definition (all bins give the history back,
fewer bins project it, the weights at DC and at the Nyquist frequency), ``fourier_bins`` at its edges, and the agreement
of header, library and binding on the new calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from full_waveform_inversion_amd import _lib, fourier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWI_EINVAL = 1
DT = 1.3e-3
NEW_CALLS = ("fwi_set_fourier_store", "fwi_fourier_spectrum", "fwi_store_bytes")


def _history(nt, shape=(3, 5), seed=0):
    return np.random.default_rng(seed).standard_normal((nt,) + shape)


@pytest.mark.parametrize("nt,S", [(33, 1), (32, 1), (33, 4), (40, 4), (5, 1), (1, 1)])  # N = 33, 32, 9, 10, 5, 1
def test_all_bins_give_the_sampled_history_back(nt, S):
    q = _history(nt)
    f = fourier.fourier_bins(nt, DT, S, 0.0, np.inf)
    N = fourier.n_samples(nt, S)
    assert f.size == N // 2 + 1
    p = fourier.project(q, nt, S, DT, f)
    assert p.shape == q.shape
    assert np.max(np.abs(p[::S] - q[::S])) < 64 * N * 2.0 ** -53 * np.max(np.abs(q))
    rest = np.ones(nt, bool)
    rest[::S] = False
    assert not p[rest].any()  # the steps the imaging never reads
    # the same in batches, as the device accumulates: nothing but round-off depends on the batch
    for B in (1, 4, 8):
        assert np.allclose(fourier.project(q, nt, S, DT, f, batch=B), p, rtol=0, atol=1e-13 * np.max(np.abs(q)))


@pytest.mark.parametrize("nt,S", [(33, 1), (32, 1), (33, 4), (40, 4)])
def test_a_subset_of_bins_is_the_orthogonal_projection_onto_them(nt, S):
    q = _history(nt, seed=1)
    f = fourier.fourier_bins(nt, DT, S, 0.0, np.inf)
    sub = f[1::3]
    p = fourier.project(q, nt, S, DT, sub)
    assert np.allclose(fourier.project(p, nt, S, DT, sub), p, rtol=0, atol=1e-13)  # idempotent
    assert abs(np.vdot(p[::S], (q - p)[::S])) < 1e-12 * np.vdot(q, q)  # the remainder is orthogonal to it
    # and the bins left out carry the remainder: the two projections add up to the history
    rest = np.setdiff1d(f, sub)
    assert np.allclose(p[::S] + fourier.project(q, nt, S, DT, rest)[::S], q[::S], rtol=0, atol=1e-13)
    # against the plain DFT of the sampled axis
    N = fourier.n_samples(nt, S)
    k = np.rint(sub * N * S * DT).astype(int)
    assert np.allclose(fourier.analyse(q[::S], nt, S, DT, sub), np.fft.fft(q[::S], axis=0)[k], rtol=0, atol=1e-12)


def test_weights_at_dc_and_at_the_nyquist_frequency():
    nt, S = 40, 4  # N = 10: the bin k = 5 is the Nyquist frequency
    N = fourier.n_samples(nt, S)
    f = fourier.fourier_bins(nt, DT, S, 0.0, np.inf)
    w = fourier.weights(nt, S, DT, f)
    assert w[0] == 1.0 / N and w[-1] == 1.0 / N and np.all(w[1:-1] == 2.0 / N)
    assert abs(f[-1] * 2 * S * DT - 1.0) < 1e-12
    # N odd: no bin is the Nyquist frequency, but the frequency itself still takes the weight 1 / N
    f9 = fourier.fourier_bins(33, DT, 4, 0.0, np.inf)
    w9 = fourier.weights(33, 4, DT, f9)
    assert w9[0] == 1.0 / 9 and np.all(w9[1:] == 2.0 / 9)
    assert fourier.weights(33, 4, DT, [1.0 / (2 * 4 * DT)])[0] == 1.0 / 9
    # an off-bin frequency: phase-sensitive detection, weight 2 / N
    assert fourier.weights(nt, S, DT, [0.37 / (S * DT)])[0] == 2.0 / N


def test_fp32_twin_rounds_where_the_device_rounds():
    q = _history(33, seed=2)
    f = fourier.fourier_bins(33, DT, 1, 0.0, np.inf)
    p64 = fourier.project(q, 33, 1, DT, f)
    p32 = fourier.project(q, 33, 1, DT, f, np.float32, batch=4)
    assert p32.dtype == np.float32
    err = np.linalg.norm(p32 - p64) / np.linalg.norm(p64)
    assert 2.0 ** -26 < err < 64 * 2.0 ** -24


def test_fourier_bins_edges():
    nt, S = 40, 4
    N = 10
    df = 1.0 / (N * S * DT)
    same = lambda a, b: np.shape(a) == np.shape(b) and np.allclose(a, b, rtol=1e-14, atol=0)  # noqa: E731
    assert same(fourier.fourier_bins(nt, DT, S, 0.0, np.inf), np.arange(6) * df)
    assert same(fourier.fourier_bins(nt, DT, S, df, 3 * df), np.arange(1, 4) * df)  # both ends count
    assert same(fourier.fourier_bins(nt, DT, S, 1.01 * df, 2.99 * df), [2 * df])
    assert fourier.fourier_bins(nt, DT, S, 1.1 * df, 1.9 * df).size == 0  # a band between two bins
    assert fourier.fourier_bins(nt, DT, S, 3 * df, df).size == 0  # fmin > fmax
    assert np.array_equal(fourier.fourier_bins(nt, DT, S, -1.0, 0.0), [0.0])
    assert np.array_equal(fourier.fourier_bins(1, DT, 1, 0.0, np.inf), [0.0])  # one sample: DC alone
    assert same(fourier.fourier_bins(nt, DT, S, 0.0, 1e9)[-1:], [5 * df])  # above the Nyquist frequency: the highest bin
    with pytest.raises(ValueError):
        fourier.fourier_bins(0, DT, 1, 0.0, 1.0)


def test_twin_refuses_what_the_engine_refuses():
    nyq = 1.0 / (2 * DT)
    for bad in ([-1.0], [np.nan], [np.inf], [1.01 * nyq], [10.0, 10.0], []):
        with pytest.raises(ValueError):
            fourier.phases(32, 1, DT, bad)
    fourier.phases(32, 1, DT, [nyq])  # the Nyquist frequency itself is allowed


def test_header_library_and_binding_agree_on_the_fourier_calls():
    lib = _lib.load()
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    header = open(os.path.join(ROOT, "include", "fwi.h")).read()
    for name in NEW_CALLS:
        assert re.search(r"^int %s\(fwi_ctx \*ctx," % name, header, re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name][0] is C.c_int
    assert int(re.search(r"#define FWI_FOURIER_FMAX (\d+)", header).group(1)) == _lib.FOURIER_FMAX == 64
    assert int(re.search(r"#define FWI_FOURIER_BMAX (\d+)", header).group(1)) == _lib.FOURIER_BMAX == 8
    # argument counts of the declarations and of the binding
    for name in NEW_CALLS:
        args = re.search(r"^int %s\(([^)]*)\);" % name, header, re.M).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_fourier_calls_reject_a_null_context():
    lib = _lib.load()
    f = np.array([10.0])
    buf = np.zeros(16, np.float32)
    n = C.c_int64(-1)
    assert lib.fwi_set_fourier_store(None, 1, f.ctypes.data_as(C.c_void_p), 4) == FWI_EINVAL
    assert lib.fwi_set_fourier_store(None, 0, None, 0) == FWI_EINVAL
    assert lib.fwi_fourier_spectrum(None, 0, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)) == FWI_EINVAL
    assert lib.fwi_store_bytes(None, C.byref(n)) == FWI_EINVAL and n.value == -1
