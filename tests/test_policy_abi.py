"""Closed-loop rollouts at the C boundary, without a GPU: the eight entry points declared, exported, bound in Python and declared
in the Rust binding; their NULL checks; gymrs_policy_size (host only); a C99 caller of them compiles and links."""
import ctypes as C
import re
import spawn_server
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ENGINE_CALLS = ("gymrs_set_policy", "gymrs_get_policy", "gymrs_policy_weights_ptr", "gymrs_policy_actions", "gymrs_rollout_policy",
                "gymrs_rollout_policy_record")
NEW = ("gymrs_policy_size",) + ENGINE_CALLS
OK, EINVAL = 0, 1
CARTPOLE, MOUNTAIN_CAR, PENDULUM = 0, 1, 2


def test_prototypes_in_header():
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    for name in ENGINE_CALLS:
        assert re.search(rf"^gymrs_status {name}\(gymrs_engine\* e[^;\n]*\);$", text, flags=re.M), name
    assert re.search(r"^gymrs_status gymrs_policy_size\(gymrs_env_kind kind, uint32_t hidden, uint64_t\* n_floats\);$", text, flags=re.M)
    assert re.search(r"typedef struct \{ uint32_t hidden; uint32_t n_policies; uint64_t lanes_per_policy; \} gymrs_policy_desc;", text)
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text)
    # the header says what clone and snapshot do with a policy
    assert re.search(r"policy is NOT part of gymrs_engine_clone or of a snapshot", text)


def test_exported_bound_and_in_rust_ffi(gymrs):
    lib = gymrs.load_library()
    sigs = import_module("gym-rs_amd._lib").SIGNATURES
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    for name in NEW:
        assert hasattr(lib, name) and name in sigs, name
    for name in ENGINE_CALLS:
        assert re.search(rf"pub fn {name}\(e: \*mut GymrsEngine", ffi), name
    assert re.search(r"pub fn gymrs_policy_size\(kind: c_int, hidden: u32, n_floats: \*mut u64\)", ffi)
    assert re.search(r"pub struct GymrsPolicyDesc", ffi)
    assert lib.gymrs_abi_version() == 3  # additive: callers detect it by symbol


def test_calls_refuse_null_engine(gymrs):
    lib = gymrs.load_library()
    desc = gymrs.engine.PolicyDesc(0, 1, 1)
    w = (C.c_float * 10)()
    ptr = C.c_void_p()
    n = C.c_uint64()
    traj = gymrs.engine.Trajectory()
    calls = {
        "gymrs_set_policy": lambda: lib.gymrs_set_policy(None, C.byref(desc), w),
        "gymrs_get_policy": lambda: lib.gymrs_get_policy(None, C.byref(desc), w, 10),
        "gymrs_policy_weights_ptr": lambda: lib.gymrs_policy_weights_ptr(None, C.byref(ptr), C.byref(n)),
        "gymrs_policy_actions": lambda: lib.gymrs_policy_actions(None, w),
        "gymrs_rollout_policy": lambda: lib.gymrs_rollout_policy(None, 1),
        "gymrs_rollout_policy_record": lambda: lib.gymrs_rollout_policy_record(None, 1, C.byref(traj)),
    }
    assert sorted(calls) == sorted(ENGINE_CALLS)
    for name, call in calls.items():
        assert call() == EINVAL, name
        assert name in lib.gymrs_last_error().decode(), name


def test_policy_size(gymrs):
    lib = gymrs.load_library()
    n = C.c_uint64()
    for kind, hidden, want in ((CARTPOLE, 0, 10), (MOUNTAIN_CAR, 0, 9), (CARTPOLE, 16, 114), (CARTPOLE, 64, 450),
                               (MOUNTAIN_CAR, 8, 8 * 3 + 3 * 9), (CARTPOLE, 1, 5 + 2 * 2)):
        assert lib.gymrs_policy_size(kind, hidden, C.byref(n)) == OK and n.value == want, (kind, hidden)
        assert gymrs.engine.policy_size(kind, hidden) == want
    assert lib.gymrs_policy_size(PENDULUM, 0, C.byref(n)) == EINVAL
    assert lib.gymrs_policy_size(CARTPOLE, 65, C.byref(n)) == EINVAL
    assert lib.gymrs_policy_size(CARTPOLE, 0, None) == EINVAL
    assert "gymrs_policy_size" in lib.gymrs_last_error().decode()


def test_python_mirror_has_the_methods(gymrs):
    for m in ("set_policy", "get_policy", "policy_weights_ptr", "policy_actions", "rollout_policy", "rollout_policy_record"):
        assert callable(getattr(gymrs.BatchedEngine, m)), m
    assert callable(gymrs.policy_size)
    hpp = (ROOT / "include" / "gymrs_env.hpp").read_text()
    for name in NEW:
        assert name + "(" in hpp, name
    assert re.search(r"pub fn rollout_policy\(", (ROOT / "bindings" / "rust" / "src" / "engine.rs").read_text())


def test_header_with_policies_compiles_as_c(tmp_path):
    src = tmp_path / "policy.c"
    src.write_text(r'''
#include "gymrs_amd.h"
#include <stdio.h>
#include <string.h>
int main(void) {
    gymrs_policy_desc d = {0, 1, 1};
    gymrs_trajectory t;
    float w[10] = {0};
    float* view = NULL;
    uint64_t n = 0;
    memset(&t, 0, sizeof t);
    if (gymrs_policy_size(GYMRS_CARTPOLE, 16, &n) != GYMRS_OK || n != 114) return 1;
    if (gymrs_policy_size(GYMRS_PENDULUM, 0, &n) != GYMRS_EINVAL) return 2;
    if (gymrs_set_policy(NULL, &d, w) != GYMRS_EINVAL) return 3;
    if (gymrs_get_policy(NULL, &d, w, 10) != GYMRS_EINVAL) return 4;
    if (gymrs_policy_weights_ptr(NULL, &view, &n) != GYMRS_EINVAL) return 5;
    if (gymrs_policy_actions(NULL, w) != GYMRS_EINVAL) return 6;
    if (gymrs_rollout_policy(NULL, 1) != GYMRS_EINVAL) return 7;
    if (gymrs_rollout_policy_record(NULL, 1, &t) != GYMRS_EINVAL) return 8;
    printf("%s\n", gymrs_last_error());
    return strstr(gymrs_last_error(), "gymrs_rollout_policy_record") ? 0 : 9;
}
''')
    exe = tmp_path / "policy"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                      f"-L{lib_dir}", "-lgymrs_amd", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"],
                     check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
