"""The probes and meshes of the sphere-ray generator's test (test_irradiance_volume.py), shared with the CPU check of their choice."""
import numpy as np

from conftest import pkg

# one probe inside the ball (every ray hits), three beside the meshes (some rays do), one far from them and from the render box.
# Chosen off the meshes' symmetry planes, so that the brute-force reference flags (next to) none of their rays as ambiguous:
# test_irradiance_volume_cpu.py::test_generator_points_are_unambiguous holds that without a device.
GEN_POINTS = np.float32([[0.61, 0.316, 0.133], [0.113, 0.751, 0.83], [0.774, 1.032, 0.642], [1.464, 1.213, -0.494], [2.5, -1.0, 0.3]])
GEN_SHAPES = [(1, 1), (7, 5), (12, 10)]
UNSAFE_CAP = 0.02


def gen_meshes():
    mi = pkg("meshio")
    return [(mi.icosphere(2), (0.0, 0.0, 0.0)), (mi.torus(24, 12, R=1.0, r=0.2), (0.3, 0.1, 0.0))]
