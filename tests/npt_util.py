"""The fp64 yardstick of the barostat tests: the stochastic-cell-rescaling move, the internal pressure and the perpendicular
widths in plain numpy, plus the fp32 ulp measure the kernel tests use.  Shares no code with ``gotennet_amd``."""
import numpy as np


def delta_eps(p_int, volume, p0, beta, tau, dt, kT, xi=None):
    """d ln V of one step: -(beta / tau) (P0 - P_int) dt + sqrt(2 kT beta dt / (V tau)) xi, element-wise in fp64 (``xi`` is
    not looked at when kT == 0)."""
    p_int, volume = np.asarray(p_int, dtype=np.float64), np.asarray(volume, dtype=np.float64)
    de = -(np.float64(beta) / np.float64(tau)) * (np.float64(p0) - p_int) * np.float64(dt)
    if kT > 0:
        de = de + np.sqrt(2.0 * np.float64(kT) * np.float64(beta) * np.float64(dt) / (volume * np.float64(tau))) * np.asarray(xi, dtype=np.float64)
    return de


def scale(de):
    """The length factor s = exp(d_eps / 3), fp64."""
    return np.exp(np.asarray(de, dtype=np.float64) / 3.0)


def pressure(ke, stress, volume):
    """2 K / (3 V) - tr(sigma) / 3 per box, fp64; ``stress`` [n, 3, 3]."""
    ke, volume = np.asarray(ke, dtype=np.float64), np.asarray(volume, dtype=np.float64)
    s = np.asarray(stress, dtype=np.float64).reshape(-1, 3, 3)
    return 2.0 * ke / (3.0 * volume) - (s[:, 0, 0] + s[:, 1, 1] + s[:, 2, 2]) / 3.0


def widths(cell):
    """[n, 3] perpendicular widths V / |a_j x a_k| and [n] volumes |det|, fp64."""
    c = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    faces = np.stack([np.cross(c[:, 1], c[:, 2]), np.cross(c[:, 2], c[:, 0]), np.cross(c[:, 0], c[:, 1])], axis=1)
    vol = np.abs(np.einsum("ni,ni->n", c[:, 0], faces[:, 0]))
    return vol[:, None] / np.linalg.norm(faces, axis=2), vol


def ulps32(got, ref):
    """|got - ref| in units of the fp32 spacing at ref, element-wise (``got`` fp32 values, ``ref`` fp64)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
