"""The offset table of NeighborSearchMethod::DIRECT_RADIUS in numpy, and tests/vgicp_reference.py run over it.

The table follows src/fast_gicp/cuda/fast_vgicp_cuda.cu:77-91 line by line: every integer (i, j, k) of [-ceil(r), ceil(r)]^3, in nested i, j, k
order, with ``sqrt(double(i*i + j*j + k*k)) <= r + 1e-3``.  ``method(r)`` registers the table in ``vgicp_reference.OFFSETS`` under a key of its
own and returns the key, so ``vr.correspondences / linearize / compute_error`` take it like "DIRECT27"; nothing else of that module changes.
"""
from __future__ import annotations

import math

import numpy as np

import vgicp_reference as vr

# radius -> table size, computed from the rule above
COUNTS = {0.0: 1, 0.5: 1, 0.998: 1, 0.999: 7, 1.0: 7, 1.4132: 7, 1.4133: 19, 1.5: 19, 1.7310: 19, 1.7311: 27, 1.9: 27, 2.0: 33, 2.2351: 57,
          3.0: 123, 4.9: 485}
MAX_OFFSETS = 512            # RGC_NDT_MAX_OFFSETS: the largest table the library takes
DIRECT_RADIUS = 3            # NeighborSearchMethod's enum order (gicp_settings.hpp:8)


def offsets(radius: float) -> np.ndarray:
    """(n, 3) int64, the reference's order"""
    r = float(radius)
    assert math.isfinite(r) and r >= 0.0
    rng = int(math.ceil(r))
    out = []
    for i in range(-rng, rng + 1):
        for j in range(-rng, rng + 1):
            for k in range(-rng, rng + 1):
                if math.sqrt(float(i * i + j * j + k * k)) <= r + 1e-3:
                    out.append((i, j, k))
    return np.array(out, np.int64).reshape(-1, 3)


def method(radius: float) -> str:
    """the key of this radius's table in vr.OFFSETS (registered on first use)"""
    key = "DIRECT_RADIUS(%r)" % float(radius)
    if key not in vr.OFFSETS:
        vr.OFFSETS[key] = offsets(radius)
    return key
