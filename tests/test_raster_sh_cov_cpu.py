"""CPU checks of the rasterizer's optional sources (SH colours, precomputed 3-D covariances): the gsvc_raster_*_ex entry points
are declared and exported, and their host-side validation rejects bad gsvc_raster_sources with a message (no GPU is touched:
every case fails before a launch)."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = ("gsvc_raster_visible_filter_ex", "gsvc_raster_forward_ex", "gsvc_raster_backward_ex")


@pytest.fixture(scope="module")
def hip_lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "gsvc_amd", "csrc", "libgsvc_hip.so")):
        g.build()
    from gsvc_amd import _lib
    return _lib


def test_ex_entry_points_declared_and_exported(hip_lib):
    header = open(os.path.join(ROOT, "include", "gsvc_hip.h")).read()
    raw = C.CDLL(hip_lib.LIB_PATH)
    for name in EX:
        assert name + "(" in header, name
        assert name in hip_lib.declared_symbols(), name
        assert hasattr(raw, name), name
    assert "typedef struct gsvc_raster_sources" in header and "GSVC_RASTER_SH_VIEW_AXIS 128u" in header
    assert hip_lib.RASTER_SH_VIEW_AXIS == 128
    # the struct's layout as the header gives it: shs, sh_degree, sh_coeffs, campos[3], cov3D
    assert C.sizeof(hip_lib.RasterSourcesC) == 40 and hip_lib.RasterSourcesC.cov3D.offset == 32


def _settings(hip_lib):
    s = hip_lib.RasterSettingsC()
    s.image_height, s.image_width = 64, 96
    s.scale, s.threshold, s.scale_modifier = 1.0, 1.0, 1.0
    return s


FAKE = 0x10000      # a non-NULL, aligned address that is never dereferenced: validation fails before any launch


def _forward(hip_lib, src, colors=FAKE, scales=FAKE, rotations=FAKE):
    L = hip_lib.lib()
    s = _settings(hip_lib)
    return L.gsvc_raster_forward_ex(C.byref(s), 10, 100, FAKE, colors, FAKE, scales, rotations, C.byref(src), FAKE, FAKE, FAKE,
                                    FAKE, FAKE, None)


def _backward(hip_lib, src, colors=FAKE, scales=FAKE, rotations=FAKE):
    L = hip_lib.lib()
    s = _settings(hip_lib)
    return L.gsvc_raster_backward_ex(C.byref(s), 10, 100, FAKE, colors, FAKE, scales, rotations, C.byref(src), FAKE, FAKE, FAKE,
                                     FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None, FAKE, None)


def _src(hip_lib, shs=None, degree=0, coeffs=1, cov=None):
    src = hip_lib.RasterSourcesC()
    src.shs, src.sh_degree, src.sh_coeffs, src.cov3D = shs, degree, coeffs, cov
    return src


@pytest.mark.parametrize("call", [_forward, _backward])
def test_ex_host_side_validation_without_gpu(hip_lib, call):
    L = hip_lib.lib()
    # SH degree outside 0..3
    assert call(hip_lib, _src(hip_lib, shs=FAKE, degree=4, coeffs=25), colors=None) == -1
    assert b"sh_degree must be 0..3" in L.gsvc_last_error()
    assert call(hip_lib, _src(hip_lib, shs=FAKE, degree=-1, coeffs=16), colors=None) == -1
    assert b"sh_degree must be 0..3" in L.gsvc_last_error()
    # too few coefficients per row for the degree
    assert call(hip_lib, _src(hip_lib, shs=FAKE, degree=3, coeffs=15), colors=None) == -1
    assert b"sh_coeffs (15) must be >= (sh_degree+1)^2 = 16" in L.gsvc_last_error()
    assert call(hip_lib, _src(hip_lib, shs=FAKE, degree=1, coeffs=3), colors=None) == -1
    assert b"sh_coeffs" in L.gsvc_last_error()
    # both / neither colour sources
    assert call(hip_lib, _src(hip_lib, shs=FAKE, degree=0, coeffs=1)) == -1
    assert b"exactly one of shs and colors (got both)" in L.gsvc_last_error()
    assert call(hip_lib, _src(hip_lib), colors=None) == -1
    assert b"exactly one of shs and colors (got neither)" in L.gsvc_last_error()
    # both / neither covariance sources
    assert call(hip_lib, _src(hip_lib, cov=FAKE)) == -1
    assert b"exactly one of cov3D and scales + rotations (got both)" in L.gsvc_last_error()
    assert call(hip_lib, _src(hip_lib), scales=None, rotations=None) == -1
    assert b"exactly one of cov3D and scales + rotations (got neither)" in L.gsvc_last_error()
    assert call(hip_lib, _src(hip_lib), rotations=None) == -1
    assert b"(got neither)" in L.gsvc_last_error()


def test_visible_filter_ex_validation_without_gpu(hip_lib):
    L = hip_lib.lib()
    s = _settings(hip_lib)
    src = _src(hip_lib, cov=FAKE)
    assert L.gsvc_raster_visible_filter_ex(C.byref(s), 10, FAKE, FAKE, FAKE, C.byref(src), FAKE, None) == -1
    assert b"exactly one of cov3D and scales + rotations (got both)" in L.gsvc_last_error()
    src = _src(hip_lib)
    assert L.gsvc_raster_visible_filter_ex(C.byref(s), 10, FAKE, None, None, C.byref(src), FAKE, None) == -1
    assert b"(got neither)" in L.gsvc_last_error()
    # the colour source plays no part in the visibility test: shs alone is not an error there, and P = 0 launches nothing
    src = _src(hip_lib, shs=FAKE, degree=9, coeffs=1, cov=FAKE)
    assert L.gsvc_raster_visible_filter_ex(C.byref(s), 0, FAKE, None, None, C.byref(src), FAKE, None) == 0


def test_rasterizer_keeps_the_lineage_exceptions():
    import torch
    from gsvc_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(image_height=8, image_width=8, x_min=0.0, y_min=0.0, scale=1.0, threshold=1.0,
                                       bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3))
    r = GaussianRasterizer(raster_settings=rs)
    m = torch.zeros(2, 3)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.ones(2, 1), shs=torch.zeros(2, 1, 3), colors_precomp=torch.zeros(2, 3),
          scales=torch.ones(2, 3), rotations=torch.zeros(2, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=torch.ones(2, 1), colors_precomp=torch.zeros(2, 3), scales=torch.ones(2, 3),
          rotations=torch.zeros(2, 4), cov3D_precomp=torch.zeros(2, 6))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r.visible_filter(means3D=m)
