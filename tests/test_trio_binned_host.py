"""The binned finish / strike entry points (include/rufus_hip.h) are exported by the built library and bound by capi."""
import ctypes as C
import os
import re

from rufus_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rfx_count_finish_binned", "rfx_binned_size", "rfx_binned_bits", "rfx_binned_free", "rfx_binned_strike",
         "rfx_candidates_strike", "rfx_candidates_size", "rfx_candidates_get", "rfx_candidates_free")


def test_binned_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rufus_hip.h")).read()
    lib = capi.lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), f"{name} is not declared in rufus_hip.h"
        fn = getattr(lib, name)
        assert fn.argtypes is not None and C.c_void_p in fn.argtypes, f"{name} has no ctypes signature"


def test_null_handles_are_harmless():
    lib = capi.lib()
    assert lib.rfx_binned_size(None) == 0 and lib.rfx_binned_bits(None) == 0 and lib.rfx_candidates_size(None) == 0
    lib.rfx_binned_free(None)
    lib.rfx_candidates_free(None)
    assert lib.rfx_candidates_get(None, None) != 0 and lib.rfx_candidates_strike(None, None) != 0
    assert not lib.rfx_count_finish_binned(None, 0, 0, None)
