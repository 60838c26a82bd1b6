"""Traced irradiance without a GPU: the entries exist, are bound and refuse a host-only context."""
import numpy as np
import pytest


def test_traced_irradiance_entries_refuse_host_only(native):
    L = native.load_library()
    for name in ("ngp_trace_nerf_rays", "ngp_irradiance_rays", "ngp_irradiance_traced"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    p, n = np.float32([[0.5, 0.5, 0.5]]), np.float32([[0.0, 0.0, 1.0]])
    with pytest.raises(RuntimeError, match="no HIP device"):
        ctx.trace_nerf_rays(p, n)
    with pytest.raises(RuntimeError, match="no HIP device"):
        ctx.irradiance_rays(p, n)
    with pytest.raises(RuntimeError, match="no HIP device"):
        ctx.irradiance_traced(p, n)
    ctx.close()


def test_irradiance_desc_layout(native):
    d = native.IrradianceTraceDesc()
    assert [f for f, _ in d._fields_] == ["n_u", "n_v", "offset", "min_transmittance", "occlude_by_meshes"]
    assert native.C.sizeof(d) == 20
