"""CPU-only: the argument checks of the binned read-out / exclude wrappers (rufus_amd/capi.py) and the hash list text of a
run's result (tools.hash_list_of_run).  No device is opened."""
import ctypes as C

import numpy as np
import pytest

from rufus_amd import capi, tools


def test_wrapper_argument_checks_and_hash_list_of_run():
    L = capi.lib()
    n = C.c_uint64(7)
    out = np.zeros(5, np.uint64)
    # the C-ABI refuses a missing handle / output before it touches a device
    assert L.rfx_binned_get(None, None, None, None, None, 0, C.byref(n)) == capi.E_INVAL
    assert L.rfx_binned_checksum(None, capi._p(out, capi.u64p)) == capi.E_INVAL
    assert L.rfx_binned_verify(None, 0, 1, capi._p(out, capi.u64p)) == capi.E_INVAL
    assert L.rfx_binned_query(None, None, 0, None) == capi.E_INVAL
    assert L.rfx_candidates_get_counts(None, None) == capi.E_INVAL
    assert L.rfx_candidates_strike_records(None, None) == capi.E_INVAL
    assert L.rfx_binned_dev_keys(None) is None and L.rfx_binned_dev_counts(None) is None
    # a NULL handle is an error of the call that made it
    with pytest.raises(capi.RufusError):
        capi.Binned(None, None)
    # the wrappers: a freed store, a range that is none, keys that are no flat array, records that are none
    b = capi.Binned(None, 1)
    b._h = None
    for call in (b.get, b.checksum, b.verify, b.dev_ptrs, lambda: b.query(np.zeros(3, np.uint64))):
        with pytest.raises(capi.RufusError):
            call()
    with pytest.raises(ValueError):
        b.verify(3, 2)
    with pytest.raises(ValueError):
        b.verify(-1, 2)
    with pytest.raises(ValueError):
        b.verify(0, 2**64)
    with pytest.raises(ValueError):
        b.query(np.zeros((2, 2), np.uint64))
    cand = capi.Candidates(None, 1)
    for bad in (None, np.zeros(3, np.uint64), b):
        with pytest.raises(TypeError):
            cand.strike_records(bad)
    freed = capi.Records(None, 1)
    freed._h = None
    with pytest.raises(TypeError):
        cand.strike_records(freed)
    cand._h = None      # (nothing to free: the handle was never the library's)

    # tools.hash_list_of_run: `kmer count` lines in the order of the result, as tools.hash_list writes them
    k = 5
    kmers = ["ACGTA", "AAAAA", "TTGCA"]
    res = {"mutant_keys": np.array([tools.text_to_key(x) for x in kmers], np.uint64),
           "mutant_counts": np.array([7, 5, 4000000000], np.uint32)}
    assert tools.hash_list_of_run(res, k) == "ACGTA 7\nAAAAA 5\nTTGCA 4000000000\n"
    assert tools.hash_list_of_run({"mutant_keys": np.zeros(0, np.uint64), "mutant_counts": np.zeros(0, np.uint32)}, k) == ""
    with pytest.raises(ValueError):
        tools.hash_list_of_run({"mutant_keys": np.zeros(2, np.uint64), "mutant_counts": np.zeros(3, np.uint32)}, k)
    with pytest.raises(KeyError):
        tools.hash_list_of_run({"mutant_keys": np.zeros(2, np.uint64)}, k)
