"""Models, reflectors, sources and surveys shared by the walled / slot-started eikonal tests (tests/test_eikonal_stage_host.py,
tests/test_gpu_eikonal_stage.py)."""
import numpy as np

from full_waveform_inversion_amd import shots as sh

H = 10.0


def curved_reflector(shape):
    """depth (cells, first axis) per column: around 0.6 of the grid, a few cells of smooth relief"""
    d = 0.6 * shape[0] + 2.0 * np.sin(np.arange(shape[-1]) / 6.0)
    if len(shape) == 3:
        d = d[None, :] + np.cos(np.arange(shape[1]) / 4.0)[:, None]
    return np.clip(d, 1.0, shape[0] - 2.0)  # a shallow grid: at least the rows 0 and 1 above it, one row below


def source(shape):
    """off-grid, in the upper layer"""
    return tuple(0.2 * n + 0.3 for n in shape)


def top_receivers(shape, step=3):
    """nodes of the plane z = 1, every `step`-th per axis"""
    ax = [np.arange(1 if len(shape) == 3 else 0, n, step) for n in shape[1:]]
    mesh = np.meshgrid(*ax, indexing="ij")
    return np.stack([np.ones(mesh[0].size, np.int64)] + [m.ravel() for m in mesh], axis=1)


def survey(shape):
    """three shots above every reflector of these tests: node and off-grid sources, node and off-grid receivers"""
    wav = np.zeros(4)
    rec = top_receivers(shape)
    pts = np.array([[0.3] + [0.37 * n + 0.2 * k for n in shape[1:]] for k in range(6)])
    return [sh.Shot(np.array([[1] + [n // 4 for n in shape[1:]]]), wav, rec),
            sh.Shot.at_coordinates([list(source(shape))], wav, pts, shape),
            sh.Shot(np.array([[0] + [3 * n // 4 for n in shape[1:]]]), wav, rec)]
