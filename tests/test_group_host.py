"""Fit-group entry points without a device: every tamcmc_group_* call refuses NULL or invalid arguments with
TAMCMC_E_INVALID before it touches HIP."""
import ctypes as C

import numpy as np

from tamcmc_amd import capi


def test_group_entry_points_refuse_invalid_arguments():
    lib = capi.load_library()
    g = C.c_void_p(123)
    assert lib.tamcmc_group_create(None, 1, None) == capi.E_INVALID
    assert lib.tamcmc_group_create(C.byref(g), 1, None) == capi.E_INVALID and not g.value
    assert lib.tamcmc_group_create(C.byref(g), 0, (C.c_void_p * 1)()) == capi.E_INVALID
    assert lib.tamcmc_group_create(C.byref(g), -3, (C.c_void_p * 1)()) == capi.E_INVALID
    assert lib.tamcmc_group_create(C.byref(g), 1, (C.c_void_p * 1)(None)) == capi.E_INVALID
    assert lib.tamcmc_group_create(C.byref(g), 1025, (C.c_void_p * 1025)()) == capi.E_INVALID
    n = np.ones(1, dtype=np.int32)
    d = np.zeros(8)
    st = np.zeros(1, dtype=np.int32)
    assert lib.tamcmc_group_eval(None, capi._iptr(n), capi._iptr(n), capi._dptr(d), capi._dptr(d), capi._dptr(d), capi._iptr(st)) == capi.E_INVALID
    assert lib.tamcmc_group_eval_device(None, capi._iptr(n), capi._iptr(n), None, None, None, None) == capi.E_INVALID
    assert lib.tamcmc_group_set_stream(None, None) == capi.E_INVALID
    assert lib.tamcmc_group_synchronize(None) == capi.E_INVALID
    assert lib.tamcmc_group_destroy(None) == capi.OK
    assert "tamcmc_group_create" in capi.EXPORTS
