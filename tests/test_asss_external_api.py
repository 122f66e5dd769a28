"""The external slice sampler's surface without a GPU: the constructor
keyword, the six C entries (include/amh.h) with their ctypes bindings, and
amh_asss_ext_work_size, which needs no handle and no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("amh_asss_ext_work_size", "amh_asss_ext_begin", "amh_asss_ext_shrink", "amh_asss_ext_finish",
           "amh_asss_ext_pnx_begin", "amh_asss_ext_pnx_finish")


@pytest.fixture(scope="module")
def lib():
    from kernels_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_constructor_keyword():
    from kernels_amd import ASSS
    k = ASSS(potential_fn=lambda z: 0.5 * (z * z).sum(-1), host_shrink=True)
    assert k.shrink_rounds == 0
    with pytest.raises(ValueError, match="host_shrink"):
        import posteriors as P
        ASSS(potential_fn=P.correlated_gaussian(4), host_shrink=True)


def test_header_declares_and_binding_matches(lib):
    src = open(os.path.join(ROOT, "include", "amh.h")).read()
    assert re.search(r"#define\s+AMH_ASSS_EXT_ROUNDS\s+51\b", src)
    assert lib.AMH_ASSS_EXT_ROUNDS == 51
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = lib.lib()
    for name in ENTRIES:
        m = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S)
        assert m, f"{name}: not declared in include/amh.h"
        n = " ".join(m.group(1).split()).count(",") + 1
        assert len(getattr(L, name).argtypes) == n, name


def test_work_size(lib):
    L = lib.lib()
    n = ctypes.c_int64(0)
    for d in range(1, 65):
        n.value = 0
        assert L.amh_asss_ext_work_size(d, ctypes.byref(n)) == 0
        assert n.value > 0
    for d in (0, 65):
        assert L.amh_asss_ext_work_size(d, ctypes.byref(n)) == -1  # AMH_EINVAL
        assert b"amh_asss_ext_work_size" in L.amh_last_error(None)
    assert L.amh_asss_ext_work_size(4, None) == -1
