"""Device process noise for the sensor-network flows (``edh.EDHFlowPF`` on its dense routes and
``ledh_dense.LEDHFlowPF``).

The reference's filters take ``process_noise_sampler = lambda N, nx: rng.multivariate_normal(0, Q, N)`` and
draw on the host, which on these paths means N x d doubles drawn and uploaded per step.  A
:class:`DeviceGaussianNoise` given in the sampler's place (``step``) or as ``process_noise`` (``run``)
makes the device draw ``v = zeta chol(Q)^T`` itself, ``zeta`` the fp64 Box-Muller normals of the project's
Philox counters (``csrc/philox.h``, restated by ``oracle/philox.normals``) and ``Q`` the filter's own
``log_trans_pdf.Q``, which the transition term of the weights assumes anyway
(``csrc/pf_noise_dense_kernels.h``).  The object is only the position in the counter space: ``seed`` is the
Philox key and ``epoch`` the next step's counter word, advanced by the filter after every call that
succeeds, so two filters given equal objects draw equal noise and a failed call can be repeated.
"""

from __future__ import annotations

import operator

__all__ = ["DeviceGaussianNoise"]


def _integer(value, name, bits):
    if isinstance(value, bool):
        raise TypeError(f"{name} must be an integer, not a bool")
    try:
        v = operator.index(value)
    except TypeError:
        raise TypeError(f"{name} must be an integer") from None
    if not 0 <= v < (1 << bits):
        raise ValueError(f"{name} must be in [0, 2^{bits})")
    return v


class DeviceGaussianNoise:
    """``N(0, Q)`` process noise drawn on the device: ``seed`` in [0, 2^64), ``epoch`` in [0, 2^32)."""

    def __init__(self, seed, epoch=0) -> None:
        self._seed = _integer(seed, "seed", 64)
        self.epoch = epoch

    @property
    def seed(self) -> int:
        return self._seed

    @property
    def epoch(self) -> int:
        return self._epoch

    @epoch.setter
    def epoch(self, value) -> None:
        self._epoch = _integer(value, "epoch", 32)

    def __repr__(self) -> str:
        return f"DeviceGaussianNoise(seed={self._seed}, epoch={self._epoch})"
