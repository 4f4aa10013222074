"""Models shared by the eikonal tests (tests/test_eikonal_host.py, tests/test_gpu_eikonal.py)."""
import numpy as np


def smooth_model(shape, seed=0):
    """2000 m/s +- ~300 m/s of smooth random structure (a few passes of a 3-point average per axis)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape)
    for _ in range(6):
        for d in range(len(shape)):
            a = (np.roll(a, 1, d) + 2.0 * a + np.roll(a, -1, d)) / 4.0
    return 2000.0 + 300.0 * a / np.abs(a).max()


def layered_model(shape, seed=1):
    """1500 over 3000 m/s with 5 % noise"""
    rng = np.random.default_rng(seed)
    z = np.arange(shape[0]).reshape((-1,) + (1,) * (len(shape) - 1))
    return np.where(z < shape[0] // 2, 1500.0, 3000.0) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, shape))
