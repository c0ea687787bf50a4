"""Per-lane parameter tables at the C boundary, without a GPU: the six entry points declared, exported, bound in Python and
declared in the Rust binding; their NULL checks; a C99 caller of them compiles and links."""
import ctypes as C
import re
import spawn_server
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW = ("gymrs_set_param_table", "gymrs_get_param_table", "gymrs_param_index_ptr", "gymrs_set_param_index",
       "gymrs_get_param_index", "gymrs_get_lane_params")
EINVAL = 1


def test_prototypes_in_header():
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    for name in NEW:
        assert re.search(rf"^gymrs_status {name}\(gymrs_engine\* e, [^;\n]*\);$", text, flags=re.M), name
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text)


def test_exported_bound_and_in_rust_ffi(gymrs):
    lib = gymrs.load_library()
    sigs = import_module("gym-rs_amd._lib").SIGNATURES
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    for name in NEW:
        assert hasattr(lib, name) and name in sigs, name
        assert re.search(rf"pub fn {name}\(e: \*mut GymrsEngine", ffi), name
    assert sigs["gymrs_set_param_index"] == sigs["gymrs_get_param_index"]
    assert lib.gymrs_abi_version() == 3  # additive: callers detect it by symbol


def test_calls_refuse_null_engine(gymrs):
    lib = gymrs.load_library()
    rows = gymrs.CartPoleParams()
    k = C.c_uint32()
    ptr = C.c_void_p()
    idx = (C.c_uint16 * 4)()
    calls = {
        "gymrs_set_param_table": lambda: lib.gymrs_set_param_table(None, C.byref(rows), 1),
        "gymrs_get_param_table": lambda: lib.gymrs_get_param_table(None, None, 0, C.byref(k)),
        "gymrs_param_index_ptr": lambda: lib.gymrs_param_index_ptr(None, C.byref(ptr)),
        "gymrs_set_param_index": lambda: lib.gymrs_set_param_index(None, 0, 4, idx),
        "gymrs_get_param_index": lambda: lib.gymrs_get_param_index(None, 0, 4, idx),
        "gymrs_get_lane_params": lambda: lib.gymrs_get_lane_params(None, 0, C.byref(rows)),
    }
    assert sorted(calls) == sorted(NEW)
    for name, call in calls.items():
        assert call() == EINVAL, name
        assert name in lib.gymrs_last_error().decode(), name


def test_python_mirror_has_the_methods(gymrs):
    for m in ("set_param_table", "param_table", "param_index_ptr", "set_param_index", "get_param_index", "lane_params"):
        assert callable(getattr(gymrs.BatchedEngine, m)), m
    hpp = (ROOT / "include" / "gymrs_env.hpp").read_text()
    for name in NEW:
        assert name + "(" in hpp, name


def test_header_with_tables_compiles_as_c(tmp_path):
    src = tmp_path / "tables.c"
    src.write_text(r'''
#include "gymrs_amd.h"
#include <stdio.h>
#include <string.h>
int main(void) {
    gymrs_cartpole_params rows[2];
    uint32_t k = 7;
    uint16_t idx[2] = {0, 1};
    uint16_t* view = NULL;
    if (gymrs_default_params(GYMRS_CARTPOLE, &rows[0]) != GYMRS_OK) return 1;
    rows[1] = rows[0];
    rows[1].length = 0.75;
    if (gymrs_set_param_table(NULL, rows, 2) != GYMRS_EINVAL) return 2;
    if (gymrs_get_param_table(NULL, rows, 2, &k) != GYMRS_EINVAL) return 3;
    if (gymrs_param_index_ptr(NULL, &view) != GYMRS_EINVAL) return 4;
    if (gymrs_set_param_index(NULL, 0, 2, idx) != GYMRS_EINVAL) return 5;
    if (gymrs_get_param_index(NULL, 0, 2, idx) != GYMRS_EINVAL) return 6;
    if (gymrs_get_lane_params(NULL, 0, &rows[0]) != GYMRS_EINVAL) return 7;
    printf("%s\n", gymrs_last_error());
    return strstr(gymrs_last_error(), "gymrs_get_lane_params") ? 0 : 8;
}
''')
    exe = tmp_path / "tables"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                      f"-L{lib_dir}", "-lgymrs_amd", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"],
                     check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
