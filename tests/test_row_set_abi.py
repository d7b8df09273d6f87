"""CPU: praos_debug_row_set's place in the ABI: declared, exported, bound, and its argument checks
need no device."""
import re

import numpy as np

from praos_hip import abi


def test_row_set_entry_point():
    hdr = open(abi.HEADER_PATH).read()
    assert re.search(r"^int praos_debug_row_set\(", hdr, flags=re.M)
    assert "#define PRAOS_ABI_VERSION 15" in hdr
    lib = abi.load()
    assert hasattr(lib, "praos_debug_row_set") and "praos_debug_row_set" in abi.SIGNATURES
    assert callable(abi.Context.debug_row_set)
    total = np.array([7], np.uint32)
    p_total = abi.ptr(total, abi.u32p)
    assert lib.praos_debug_row_set(None, 0, None, None, None, 0, 1, None, None, p_total) == abi.E_ARG
    assert total[0] == 7                                            # nothing written without a context
    c = abi.Context(abi.HOST_ONLY)
    h, E_STATE, OK = c.h, -4, 0
    try:
        assert lib.praos_debug_row_set(h, 0, None, None, None, 0, 1, None, None, None) == abi.E_ARG
        assert lib.praos_debug_row_set(h, 0, None, None, None, 0, 1, None, None, p_total) == OK and total[0] == 0
        assert lib.praos_debug_row_set(h, 1 << 24, None, None, None, 0, 1, None, None, p_total) == abi.E_ARG
        flag, rows = np.zeros(4, np.uint8), np.zeros(4, np.uint32)
        args = (abi.ptr(flag), None, None, 0xFFFFFFFF)
        assert lib.praos_debug_row_set(h, 4, *args, 1, None, abi.ptr(rows, abi.u32p), p_total) == abi.E_ARG   # no keys
        assert lib.praos_debug_row_set(h, 4, *args, 0, None, None, p_total) == abi.E_ARG                       # no output
        assert lib.praos_debug_row_set(h, 4, *args, 0, None, abi.ptr(rows, abi.u32p), p_total) == E_STATE
    finally:
        c.close()
