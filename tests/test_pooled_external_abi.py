"""The pooled external-potential entries of the C ABI without a GPU:
include/amh.h declares amh_pooled_propose and amh_pooled_stats_external, the
ctypes binding exports and binds them, and a null handle is refused with a
status code and a message that names the entry."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"amh_pooled_propose": 6, "amh_pooled_stats_external": 11}


@pytest.fixture(scope="module")
def lib():
    from kernels_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_header_declares_the_entries():
    src = open(os.path.join(ROOT, "include", "amh.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, arity in ENTRIES.items():
        m = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S)
        assert m, f"{name} not declared"
        assert m.group(1).count(",") + 1 == arity, name


def test_binding_exports_and_binds_the_entries(lib):
    L = lib.lib()
    for name, arity in ENTRIES.items():
        assert name in lib.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity, name


def test_null_handle_is_refused(lib):
    L = lib.lib()
    assert L.amh_pooled_propose(None, 1, None, 0, None, None) == -1  # AMH_EINVAL
    assert b"amh_pooled_propose" in L.amh_last_error(None)
    assert L.amh_pooled_stats_external(None, 1, None, 0, None, None, None, None, None, 0, None) == -1
    assert b"amh_pooled_stats_external" in L.amh_last_error(None)
