"""srw_cluster_set_sources / _clear_sources / _sources without a GPU: the symbols, their NULL-cluster behaviour, the binding's surface."""
import ctypes as C
import re

from helpers import ROOT, pkg

NAMES = ["srw_cluster_set_sources", "srw_cluster_clear_sources", "srw_cluster_sources"]


def test_cluster_sources_symbols_are_exported_and_declared():
    P = pkg()
    L = P.lib()
    header = open(ROOT + "/include/stellar_rw.h").read()
    for name in NAMES:
        assert name in P.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, header), name


def test_cluster_sources_refuse_a_null_cluster():
    P = pkg()
    L = P.lib()
    ids = (C.c_int32 * 2)(1, 2)
    n = C.c_int64(7)
    assert L.srw_cluster_set_sources(None, ids, 2) == P.ERR_INVALID
    assert L.srw_cluster_set_sources(None, None, 0) == P.ERR_INVALID
    assert L.srw_cluster_clear_sources(None) == P.ERR_INVALID
    assert L.srw_cluster_sources(None, C.byref(n)) == P.ERR_INVALID and n.value == 7


def test_cluster_binding_has_the_methods():
    P = pkg()
    for m in ("set_sources", "clear_sources", "sources_len"):
        assert callable(getattr(P.Cluster, m))
    import inspect
    assert "sources" in inspect.signature(P.Cluster.walk).parameters
    assert "sources" in inspect.signature(P.Cluster.walk_and_save).parameters
