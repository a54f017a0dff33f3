"""CPU test of the drop-in boundary: libgsvc_hip.so loads without a GPU and exports every entry point that
include/gsvc_hip.h declares (no compute is called), argument validation works on the host side, and the
product package never imports the oracle."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_in_header():
    text = open(os.path.join(ROOT, "include", "gsvc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsvc_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def hip_lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "gsvc_amd", "csrc", "libgsvc_hip.so")):
        g.build()
    from gsvc_amd import _lib
    return _lib


def test_header_and_binding_agree(hip_lib):
    names = _declared_in_header()
    assert names == hip_lib.declared_symbols()
    assert len(names) >= 16


def test_library_exports_every_declared_symbol(hip_lib):
    raw = C.CDLL(hip_lib.LIB_PATH)
    for name in _declared_in_header():
        assert hasattr(raw, name), name
    assert hip_lib.lib().gsvc_version().startswith(b"gsvc_hip")


def test_every_entry_point_has_a_stream_contract_case_or_a_stated_reason(hip_lib):
    """tests/_abi_contract_cases.py against the header and the binding's signature table: an entry point that takes a stream is the
    `entries` of exactly one case of tests/test_abi_contract_gpu.py, or one of the rasterizer's forward / backward entries (which keep
    their own graph test), or stands in WITHDRAWN (a case that was taken out again, with what happened), or in NOT_COVERED with a reason — a capped table that may hold front-end analysis entries only; an
    entry point without a stream stands in NO_STREAM.  A new entry point cannot land without its case."""
    from tests import _abi_contract_cases as A
    streamed = A.streamed_entries()
    declared = A.header_entries()
    assert sorted(declared) == hip_lib.declared_symbols()
    for name, at in streamed.items():       # the header's `void *stream` is a void pointer of the binding, the last but for one entry
        args = hip_lib._SIGNATURES[name][1]
        assert args[at] is C.c_void_p and (at == len(args) - 1 or name == "gsvc_generate_all_backward"), name
    owners = {}
    for case in A.CASES:
        assert case.entries, case
        for name in case.entries:
            owners.setdefault(name, []).append(case.name)
        assert set(case.also) <= set(streamed) and not set(case.also) & set(case.entries), case
    twice = {n: o for n, o in owners.items() if len(o) > 1}
    assert not twice, twice
    assert len({case.name for case in A.CASES}) == len(A.CASES)
    tables = [set(owners), set(A.NOT_COVERED), set(A.RASTER_GRAPH_TEST), set(A.WITHDRAWN), set(A.NO_STREAM)]
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not a & b, sorted(a & b)
    covered_or_excused = tables[0] | tables[1] | tables[2] | tables[3]
    orphans = sorted(set(streamed) - covered_or_excused)
    assert not orphans, f"entry points with a stream argument and no contract case: {orphans}"
    assert covered_or_excused <= set(streamed), sorted(covered_or_excused - set(streamed))
    assert set(A.NO_STREAM) == set(declared) - set(streamed), sorted(set(A.NO_STREAM) ^ (set(declared) - set(streamed)))
    assert all(also in owners for case in A.CASES for also in case.also)
    assert len(A.NOT_COVERED) <= A.NOT_COVERED_CAP and set(A.NOT_COVERED) <= A.FRONT_END, sorted(set(A.NOT_COVERED) - A.FRONT_END)
    assert all(isinstance(r, str) and r for r in list(A.NOT_COVERED.values()) + list(A.WITHDRAWN.values()) + list(A.NO_STREAM.values()))
    assert all(n.startswith("gsvc_raster_") for n in A.RASTER_GRAPH_TEST)
    # WITHDRAWN is no second NOT_COVERED: it holds the two entries of the one case that was taken out, and nothing can be added to it
    assert set(A.WITHDRAWN) == {"gsvc_generate_all_forward", "gsvc_generate_all_backward"}


def test_host_side_validation_without_gpu(hip_lib):
    L = hip_lib.lib()
    s = hip_lib.RasterSettingsC()
    s.image_height, s.image_width = 1080, 1920
    sz = hip_lib.RasterSizesC()
    assert L.gsvc_raster_sizes_query(C.byref(s), 200000, 800000, C.byref(sz)) == 0
    assert sz.geom_bytes >= 200000 * 80 and sz.binning_bytes >= 800000 * 20 and sz.image_bytes >= 1080 * 1920 * 8
    s.image_height = 0
    assert L.gsvc_raster_sizes_query(C.byref(s), 1, 1, C.byref(sz)) == -1
    assert b"image size must be positive" in L.gsvc_last_error()
    with pytest.raises(hip_lib.GsvcError):
        hip_lib.check(-1, "probe")


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gsvc_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "libgsvc_oracle" not in text, f


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    from gsvc_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.GsvcError, match="no CPU fallback"):
        _lib.lib()
