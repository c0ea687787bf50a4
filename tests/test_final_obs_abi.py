"""GYMRS_FINAL_OBS at the C boundary, without a GPU: the flag's value, the two accessors exported and bound, the flag refused
without GYMRS_AUTO_RESET (before any device is looked for), and the accessors' NULL checks."""
import ctypes as C
import re
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW = ("gymrs_final_obs_ptrs", "gymrs_get_final_obs")
EINVAL = 1


def test_flag_value_and_header(gymrs):
    assert gymrs.FINAL_OBS == 8 and "FINAL_OBS" in gymrs.__all__
    assert gymrs.FINAL_OBS & (gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT) == 0
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    assert re.search(r"GYMRS_FINAL_OBS\s*=\s*8u", text)
    for name in NEW:
        assert re.search(rf"^gymrs_status {name}\(gymrs_engine\* e, [^;\n]*\);$", text, flags=re.M), name


def test_symbols_exported_and_bound(gymrs):
    lib = gymrs.load_library()
    sigs = import_module("gym-rs_amd._lib").SIGNATURES
    for name in NEW:
        assert hasattr(lib, name) and name in sigs
    assert sigs["gymrs_final_obs_ptrs"] == sigs["gymrs_obs_ptrs"]
    assert sigs["gymrs_get_final_obs"] == sigs["gymrs_get_obs"]
    assert lib.gymrs_abi_version() == 3  # additive: callers detect it by symbol


def test_final_obs_needs_auto_reset(gymrs):
    lib = gymrs.load_library()
    h = C.c_void_p()
    for flags in (gymrs.FINAL_OBS, gymrs.FINAL_OBS | gymrs.TIME_LIMIT):
        for kind in (gymrs.CARTPOLE, gymrs.MOUNTAIN_CAR, gymrs.PENDULUM):
            assert lib.gymrs_engine_create(kind, 16, 0, 0, None, flags, C.byref(h)) == EINVAL
            assert not h.value
            msg = lib.gymrs_last_error().decode()
            assert "GYMRS_FINAL_OBS" in msg and "GYMRS_AUTO_RESET" in msg
    assert lib.gymrs_engine_create(gymrs.CARTPOLE, 16, 0, 0, None, 16, C.byref(h)) == EINVAL  # the next bit is still unknown
    assert "unknown flag" in lib.gymrs_last_error().decode()


def test_accessors_refuse_null(gymrs):
    lib = gymrs.load_library()
    ptrs, dim = (C.c_void_p * 4)(), C.c_int()
    out = (C.c_float * 4)()
    assert lib.gymrs_final_obs_ptrs(None, ptrs, C.byref(dim)) == EINVAL
    assert "gymrs_final_obs_ptrs" in lib.gymrs_last_error().decode()
    assert lib.gymrs_get_final_obs(None, 0, 1, out) == EINVAL
    assert "gymrs_get_final_obs" in lib.gymrs_last_error().decode()
