"""The pooled external slice sampler's surface without a GPU: the
constructor keyword of PooledASSS with its ValueErrors, and the three C
entries (include/amh.h) with their ctypes bindings."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("amh_pooled_asss_ext_begin", "amh_pooled_asss_ext_finish", "amh_pooled_asss_ext_update")


def U(z):
    return 0.5 * (z * z).sum(-1)


@pytest.fixture(scope="module")
def lib():
    from kernels_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_constructor_keyword():
    import posteriors as P
    from kernels_amd import PooledASSS
    k = PooledASSS(potential_fn=U, host_shrink=True, num_chains=8, sync_every=2, overlap=True)
    assert k.shrink_rounds == 0 and k._host_shrink is True and k._external()
    assert k.sync_every == 2 and k.overlap is True
    assert PooledASSS(potential_fn=P.correlated_gaussian(4))._host_shrink is False


def test_constructor_value_errors():
    import posteriors as P
    from kernels_amd import PooledASSS
    with pytest.raises(ValueError, match="host_shrink=True"):  # a callable without the keyword: refused as before
        PooledASSS(potential_fn=U)
    with pytest.raises(ValueError, match="host_shrink"):
        PooledASSS(potential_fn=P.correlated_gaussian(4), host_shrink=True)
    with pytest.raises(ValueError, match="host_shrink"):
        PooledASSS(model=P.eight_schools, host_shrink=True)
    with pytest.raises(ValueError, match="exact_sums"):
        PooledASSS(potential_fn=U, host_shrink=True, exact_sums=True)
    with pytest.raises(ValueError, match="exact_sums"):
        PooledASSS(potential_fn=P.correlated_gaussian(4), exact_sums=True)


def test_header_declares_and_binding_matches(lib):
    src = open(os.path.join(ROOT, "include", "amh.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = lib.lib()
    for name in ENTRIES:
        m = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S)
        assert m, f"{name}: not declared in include/amh.h"
        params = " ".join(m.group(1).split())
        assert params.startswith("amh_handle* h")
        assert len(getattr(L, name).argtypes) == params.count(",") + 1, name
        assert name in lib.EXPORTS


def test_null_handle_is_refused_before_any_argument(lib):
    L = lib.lib()
    assert L.amh_pooled_asss_ext_begin(None, 1, None, 0, None, None, None, None) == -1  # AMH_EINVAL
    assert b"amh_pooled_asss_ext_begin: null handle" in L.amh_last_error(None)
    assert L.amh_pooled_asss_ext_finish(None, 1, None, None, None, None, None, None, 0, None) == -1
    assert b"amh_pooled_asss_ext_finish: null handle" in L.amh_last_error(None)
    assert L.amh_pooled_asss_ext_update(None, None, None, None, 1, None) == -1
    assert b"amh_pooled_asss_ext_update: null handle" in L.amh_last_error(None)
