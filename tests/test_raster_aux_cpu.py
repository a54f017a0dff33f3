"""CPU checks of the rasterizer's depth / alpha maps: gsvc_raster_forward_aux / _backward_aux are declared and exported, and their
host-side validation rejects bad arguments with a message (no GPU is touched: every case fails before a launch)."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUX = ("gsvc_raster_forward_aux", "gsvc_raster_backward_aux")
FAKE = 0x10000      # a non-NULL, aligned address that is never dereferenced: validation fails before any launch


@pytest.fixture(scope="module")
def hip_lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "gsvc_amd", "csrc", "libgsvc_hip.so")):
        g.build()
    from gsvc_amd import _lib
    return _lib


def _settings(hip_lib):
    s = hip_lib.RasterSettingsC()
    s.image_height, s.image_width = 64, 96
    s.scale, s.threshold, s.scale_modifier = 1.0, 1.0, 1.0
    return s


def _src(hip_lib, shs=None, degree=0, coeffs=1, cov=None):
    src = hip_lib.RasterSourcesC()
    src.shs, src.cov3D = shs, cov
    src.sh_degree, src.sh_coeffs = degree, coeffs
    return src


def _forward(hip_lib, settings, src, colors=FAKE, scales=FAKE, rotations=FAKE):
    return hip_lib.lib().gsvc_raster_forward_aux(settings, 10, 100, FAKE, colors, FAKE, scales, rotations, src, FAKE, FAKE,
                                                 FAKE, FAKE, FAKE, FAKE, FAKE, None)


def _backward(hip_lib, settings, src, colors=FAKE, scales=FAKE, rotations=FAKE):
    return hip_lib.lib().gsvc_raster_backward_aux(settings, 10, 100, FAKE, colors, FAKE, scales, rotations, src, FAKE, FAKE,
                                                  FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None,
                                                  FAKE, None)


def test_aux_entry_points_declared_and_exported(hip_lib):
    header = open(os.path.join(ROOT, "include", "gsvc_hip.h")).read()
    raw = C.CDLL(hip_lib.LIB_PATH)
    for name in AUX:
        assert name + "(" in header, name
        assert name in hip_lib.declared_symbols(), name
        assert hasattr(raw, name), name


def test_null_settings(hip_lib):
    L = hip_lib.lib()
    assert _forward(hip_lib, None, None) == -1
    assert b"settings is NULL" in L.gsvc_last_error()
    assert _backward(hip_lib, None, None) == -1
    assert b"settings is NULL" in L.gsvc_last_error()


@pytest.mark.parametrize("call", [_forward, _backward])
def test_both_colour_sources(hip_lib, call):
    L = hip_lib.lib()
    src = _src(hip_lib, shs=FAKE, degree=0, coeffs=1)
    assert call(hip_lib, C.byref(_settings(hip_lib)), C.byref(src)) == -1
    err = L.gsvc_last_error()
    assert b"_aux" in err and b"exactly one of shs and colors" in err and b"both" in err, err


@pytest.mark.parametrize("call", [_forward, _backward])
@pytest.mark.parametrize("degree", [-1, 4])
def test_bad_sh_degree(hip_lib, call, degree):
    L = hip_lib.lib()
    src = _src(hip_lib, shs=FAKE, degree=degree, coeffs=16)
    assert call(hip_lib, C.byref(_settings(hip_lib)), C.byref(src), colors=None) == -1
    err = L.gsvc_last_error()
    assert b"_aux" in err and b"sh_degree must be 0..3" in err, err


@pytest.mark.parametrize("call", [_forward, _backward])
def test_null_sources_need_the_plain_inputs(hip_lib, call):
    """sources = NULL is the plain colors + scales / rotations form: without colours it is rejected before any launch."""
    L = hip_lib.lib()
    assert call(hip_lib, C.byref(_settings(hip_lib)), None, colors=None) == -1
    assert b"exactly one of shs and colors" in L.gsvc_last_error()
    assert call(hip_lib, C.byref(_settings(hip_lib)), None, scales=None) == -1
    assert b"exactly one of cov3D and scales + rotations" in L.gsvc_last_error()
