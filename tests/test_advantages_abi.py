"""gymrs_advantages and the critic calls at the C boundary, without a GPU: the flag constant, the descriptor and the six prototypes in
the header, exported by the library, bound in Python and declared in the Rust binding; a plain-C translation unit that static-asserts
the descriptor's layout and the ABI version and calls the host-only functions; the NULL checks; the mirrors' new members.

The descriptor is 112 bytes: four 4-byte words, the 48-byte gymrs_trajectory by value, five pointers and the reserved word."""
import ctypes as C
import inspect
import re
import spawn_server
from importlib import import_module
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EINVAL = 1
LINK = ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
SIZE = 112
OFFSETS = [("n_steps", 0), ("flags", 4), ("gamma", 8), ("lam", 12), ("record", 16), ("final_obs", 64), ("start_obs", 72), ("advantages", 80),
           ("returns", 88), ("values", 96), ("reserved", 104)]
PROTOTYPES = {
    "gymrs_critic_size": r"gymrs_status gymrs_critic_size\(gymrs_env_kind kind, uint32_t hidden, uint64_t\* n_floats\);",
    "gymrs_set_critic": r"gymrs_status gymrs_set_critic\(gymrs_engine\* e, const gymrs_policy_desc\* d, const float\* weights_host\);",
    "gymrs_get_critic": r"gymrs_status gymrs_get_critic\(gymrs_engine\* e, gymrs_policy_desc\* d_out, float\* weights_out, uint64_t capacity_floats\);",
    "gymrs_critic_weights_ptr": r"gymrs_status gymrs_critic_weights_ptr\(gymrs_engine\* e, float\*\* dev_out, uint64_t\* n_floats\);",
    "gymrs_critic_value": r"gymrs_status gymrs_critic_value\(gymrs_env_kind kind, uint32_t hidden, const float\* weights, const float\* obs, float\* v\);",
    "gymrs_advantages": r"gymrs_status gymrs_advantages\(gymrs_engine\* e, const gymrs_advantages_desc\* d\);",
}


def test_constant_struct_and_prototypes_in_header():
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text)  # additive: callers detect the feature by symbol
    assert re.search(r"^#define GYMRS_ADVANTAGES_CRITIC 1u\b", text, flags=re.M)
    assert re.search(r"typedef struct \{\s*uint32_t n_steps;[^\n]*\n\s*uint32_t flags;[^\n]*\n\s*float gamma, lambda;[^\n]*\n\s*gymrs_trajectory record;[^\n]*\n"
                     r"[^\n]*\n\s*const float\* final_obs;[^\n]*\n\s*const float\* start_obs;[^\n]*\n\s*float\* advantages;[^\n]*\n\s*float\* returns;[^\n]*\n"
                     r"\s*float\* values;[^\n]*\n\s*uint64_t reserved;[^\n]*\n\} gymrs_advantages_desc;\s*/\* 112 bytes \*/", text)
    for name, proto in PROTOTYPES.items():
        assert re.search("^" + proto + "$", text, flags=re.M), name
    doc = re.search(r"/\* Advantages:(.*?)\*/", text, flags=re.S).group(1)
    for phrase in ("ended   = done[k] != 0 || (truncated != NULL && truncated[k] != 0)", "x_next  = (final_obs != NULL && ended) ? final_obs[k] : obs[k]",
                   "v_next  = done[k] != 0 ? +0.0f : V(x_next)", "v_cur   = V(k == 0 ? start_obs : obs[k-1])",
                   "delta   = fmaf(gamma, v_next, reward[k]) - v_cur", "carry   = ended ? +0.0f : A[k+1]", "A[k]    = fmaf(gl, carry, delta)",
                   "R[k] = A[k] + v_cur", "v = fmaf(W2[h], r, v)", "S = H*(D+2) + 1", "no sharded counterpart", "n_steps == 0", "gymrs_set_critic",
                   "padding lanes"):
        assert phrase in doc, phrase
    assert text.index("/* Advantages:") > text.index("/* Transitions:")  # the block after "Transitions"


def test_exported_bound_and_in_rust_ffi(gymrs):
    lib = gymrs.load_library()
    sigs = import_module("gym-rs_amd._lib").SIGNATURES
    for name in PROTOTYPES:
        assert hasattr(lib, name) and name in sigs, name
    f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    assert sigs["gymrs_advantages"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert sigs["gymrs_critic_size"] == (C.c_int, [C.c_int, C.c_uint32, u64p]) and sigs["gymrs_set_critic"] == sigs["gymrs_set_policy"]
    assert sigs["gymrs_get_critic"] == sigs["gymrs_get_policy"] and sigs["gymrs_critic_weights_ptr"] == sigs["gymrs_policy_weights_ptr"]
    assert sigs["gymrs_critic_value"] == (C.c_int, [C.c_int, C.c_uint32, f32p, f32p, f32p])
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    assert re.search(r"pub const GYMRS_ADVANTAGES_CRITIC: u32 = 1;", ffi)
    assert re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct GymrsAdvantagesDesc \{\s*pub n_steps: u32,\s*pub flags: u32,\s*pub gamma: f32,"
                     r"\s*pub lambda: f32,\s*pub record: Trajectory,\s*pub final_obs: \*const f32,\s*pub start_obs: \*const f32,\s*pub advantages: \*mut f32,"
                     r"\s*pub returns: \*mut f32,\s*pub values: \*mut f32,\s*pub reserved: u64,\s*\}", ffi)
    assert re.search(r"pub fn gymrs_advantages\(e: \*mut GymrsEngine, d: \*const GymrsAdvantagesDesc\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_critic_size\(kind: c_int, hidden: u32, n_floats: \*mut u64\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_set_critic\(e: \*mut GymrsEngine, d: \*const GymrsPolicyDesc, weights_host: \*const f32\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_get_critic\(e: \*mut GymrsEngine, d_out: \*mut GymrsPolicyDesc, weights_out: \*mut f32, capacity_floats: u64\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_critic_weights_ptr\(e: \*mut GymrsEngine, dev_out: \*mut \*mut f32, n_floats: \*mut u64\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_critic_value\(kind: c_int, hidden: u32, weights: \*const f32, obs: \*const f32, v: \*mut f32\) -> c_int;", ffi)
    assert lib.gymrs_abi_version() == 3


def test_python_desc_and_constant(gymrs):
    desc = gymrs.AdvantagesDesc
    assert desc is gymrs.engine.AdvantagesDesc and gymrs.ADVANTAGES_CRITIC == 1 == gymrs.engine.ADVANTAGES_CRITIC
    assert C.sizeof(desc) == SIZE and [(n, getattr(desc, n).offset) for n, _ in desc._fields_] == OFFSETS
    assert C.sizeof(gymrs.engine.Trajectory) == 48


def test_critic_size_values_and_refusals(gymrs):
    assert gymrs.critic_size(gymrs.CARTPOLE, 0) == 5 and gymrs.critic_size(gymrs.CARTPOLE, 16) == 97 and gymrs.critic_size(gymrs.MOUNTAIN_CAR, 0) == 3
    assert gymrs.critic_size(gymrs.MOUNTAIN_CAR, 64) == 64 * 4 + 1 and gymrs.critic_size(gymrs.CARTPOLE, 64) == 64 * 6 + 1
    for kind in (gymrs.CARTPOLE, gymrs.MOUNTAIN_CAR):
        for hidden in (1, 7, 64):  # the policy layout with one action
            d = 4 if kind == gymrs.CARTPOLE else 2
            assert gymrs.critic_size(kind, hidden) == hidden * (d + 1) + 1 * (hidden + 1)
    with pytest.raises(gymrs.GymrsError, match="Pendulum") as err:
        gymrs.critic_size(gymrs.PENDULUM, 0)
    assert err.value.status == EINVAL
    with pytest.raises(gymrs.GymrsError, match="hidden must be <= 64") as err:
        gymrs.critic_size(gymrs.CARTPOLE, 65)
    assert err.value.status == EINVAL
    lib = gymrs.load_library()
    assert lib.gymrs_critic_size(0, 0, None) == EINVAL and b"gymrs_critic_size" in lib.gymrs_last_error()


def test_calls_refuse_null_arguments(gymrs):
    lib = gymrs.load_library()
    desc = gymrs.AdvantagesDesc(3, 0, 1.0, 1.0, gymrs.engine.Trajectory(16, None, 48, 64, 80, 128), 96, 112, 128, None, None, 0)
    assert lib.gymrs_advantages(None, C.byref(desc)) == EINVAL and b"gymrs_advantages" in lib.gymrs_last_error()
    assert lib.gymrs_advantages(None, None) == EINVAL and b"gymrs_advantages" in lib.gymrs_last_error()
    pd = gymrs.engine.PolicyDesc(0, 1, 1)
    w = (C.c_float * 5)()
    assert lib.gymrs_set_critic(None, C.byref(pd), w) == EINVAL and b"gymrs_set_critic" in lib.gymrs_last_error()
    assert lib.gymrs_get_critic(None, C.byref(pd), None, 0) == EINVAL and b"gymrs_get_critic" in lib.gymrs_last_error()
    p, n = C.c_void_p(), C.c_uint64()
    assert lib.gymrs_critic_weights_ptr(None, C.byref(p), C.byref(n)) == EINVAL and b"gymrs_critic_weights_ptr" in lib.gymrs_last_error()
    x, v = (C.c_float * 4)(), C.c_float()
    for args in ((None, x, C.byref(v)), (w, None, C.byref(v)), (w, x, None)):
        assert lib.gymrs_critic_value(0, 0, *args) == EINVAL and b"gymrs_critic_value" in lib.gymrs_last_error()
    assert lib.gymrs_critic_value(2, 0, w, x, C.byref(v)) == EINVAL and b"Pendulum" in lib.gymrs_last_error()
    assert lib.gymrs_critic_value(0, 65, w, x, C.byref(v)) == EINVAL and b"hidden" in lib.gymrs_last_error()
    w[0], w[4], x[0] = 2.0, 0.5, 3.0
    assert lib.gymrs_critic_value(0, 0, w, x, C.byref(v)) == 0 and v.value == 6.5


def test_mirrors_have_the_members(gymrs):
    params = inspect.signature(gymrs.BatchedEngine.advantages).parameters
    assert list(params)[:2] == ["self", "n_steps"]
    for name, default in (("final_obs", None), ("returns", None), ("values", None), ("critic", False)):
        assert params[name].default is default and params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in ("record", "start_obs", "advantages", "gamma", "lam"):
        assert params[name].default is inspect.Parameter.empty and params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in ("set_critic", "critic", "critic_weights_ptr"):
        assert callable(getattr(gymrs.BatchedEngine, name)), name
    assert list(inspect.signature(gymrs.BatchedEngine.set_critic).parameters) == ["self", "weights", "hidden", "lanes_per_critic"]
    for name in ("advantages", "set_critic", "critic", "critic_weights_ptr"):
        assert not hasattr(gymrs.ShardedEngine, name), name  # records are refused there: no sharded counterpart
    assert callable(gymrs.critic_size) and callable(gymrs.critic_value)
    hpp = (ROOT / "include" / "gymrs_env.hpp").read_text()
    assert "gymrs_advantages" in hpp and "gymrs_advantages_desc" in hpp and "gymrs_set_critic" in hpp
    engine = (ROOT / "bindings" / "rust" / "src" / "engine.rs").read_text()
    assert "pub unsafe fn advantages(" in engine and "GymrsAdvantagesDesc" in engine and "pub fn set_critic(" in engine
    for text, name in ((ROOT / "INTEGRATION.md").read_text(), "INTEGRATION.md"), ((ROOT / "README.md").read_text(), "README.md"):
        assert "gymrs_advantages" in text, name
    assert re.search(r"^#+ .*Advantages", (ROOT / "INTEGRATION.md").read_text(), flags=re.M)


def test_layout_and_null_checks_from_c(tmp_path):
    src = tmp_path / "advantages.c"
    src.write_text(r'''
#include "gymrs_amd.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
_Static_assert(GYMRS_ABI_VERSION == 3, "additive");
_Static_assert(GYMRS_ADVANTAGES_CRITIC == 1u, "flag");
_Static_assert(sizeof(gymrs_advantages_desc) == 112 && sizeof(gymrs_trajectory) == 48, "desc size");
_Static_assert(offsetof(gymrs_advantages_desc, n_steps) == 0 && offsetof(gymrs_advantages_desc, flags) == 4, "desc layout");
_Static_assert(offsetof(gymrs_advantages_desc, gamma) == 8 && offsetof(gymrs_advantages_desc, lambda) == 12, "desc layout");
_Static_assert(offsetof(gymrs_advantages_desc, record) == 16 && offsetof(gymrs_advantages_desc, final_obs) == 64, "desc layout");
_Static_assert(offsetof(gymrs_advantages_desc, start_obs) == 72 && offsetof(gymrs_advantages_desc, advantages) == 80, "desc layout");
_Static_assert(offsetof(gymrs_advantages_desc, returns) == 88 && offsetof(gymrs_advantages_desc, values) == 96, "desc layout");
_Static_assert(offsetof(gymrs_advantages_desc, reserved) == 104, "desc layout");
int main(void) {
    gymrs_advantages_desc d;
    uint64_t s = 0;
    float w[5] = {1.0f, 0.0f, 0.0f, -2.0f, 0.25f}, x[4] = {3.0f, 9.0f, 9.0f, 0.5f}, v = 0.0f;
    memset(&d, 0, sizeof d);
    d.n_steps = 64;
    d.flags = GYMRS_ADVANTAGES_CRITIC;
    if (gymrs_abi_version() != 3) return 1;
    if (gymrs_advantages(NULL, &d) != GYMRS_EINVAL) return 2;
    if (!strstr(gymrs_last_error(), "gymrs_advantages")) return 3;
    if (gymrs_advantages(NULL, NULL) != GYMRS_EINVAL) return 4;
    if (gymrs_critic_size(GYMRS_CARTPOLE, 16, &s) != GYMRS_OK || s != 97) return 5;
    if (gymrs_critic_size(GYMRS_MOUNTAIN_CAR, 0, &s) != GYMRS_OK || s != 3) return 6;
    if (gymrs_critic_size(GYMRS_PENDULUM, 0, &s) != GYMRS_EINVAL || gymrs_critic_size(GYMRS_CARTPOLE, 65, &s) != GYMRS_EINVAL) return 7;
    if (gymrs_critic_value(GYMRS_CARTPOLE, 0, w, x, &v) != GYMRS_OK || v != 2.25f) return 8;
    if (gymrs_set_critic(NULL, NULL, NULL) != GYMRS_EINVAL || gymrs_get_critic(NULL, NULL, NULL, 0) != GYMRS_EINVAL) return 9;
    if (gymrs_critic_weights_ptr(NULL, NULL, NULL) != GYMRS_EINVAL) return 10;
    printf("ADVANTAGES_ABI_OK\n");
    return 0;
}
''')
    exe = tmp_path / "advantages"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                      f"-L{lib_dir}", "-lgymrs_amd", f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "ADVANTAGES_ABI_OK" in res.stdout, res.stdout + res.stderr


def test_cpp_mirror_members_compile(tmp_path):
    """A small program of its own that names the new members of include/gymrs_env.hpp (their signatures are part of the check); it
    runs no engine: it only has to compile, link and start."""
    src = tmp_path / "advantages_mirror.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include "gymrs_env.hpp"
using gymrs::VecEnv;
int main() {
    void (VecEnv::*a)(const gymrs_advantages_desc&) = &VecEnv::advantages;
    void (VecEnv::*b)(std::uint32_t, const gymrs_trajectory&, const float*, const float*, float*, float*, float*, float, float, bool) = &VecEnv::advantages;
    void (VecEnv::*c)(const float*, std::uint32_t, std::uint32_t, std::uint64_t) = &VecEnv::set_critic;
    void (VecEnv::*d)() = &VecEnv::clear_critic;
    gymrs_policy_desc (VecEnv::*e)(float*, std::uint64_t) = &VecEnv::critic;
    float* (VecEnv::*f)(std::uint64_t*) = &VecEnv::critic_weights_view;
    std::uint64_t (*g)(gymrs_env_kind, std::uint32_t) = &VecEnv::critic_size;
    float (*h)(gymrs_env_kind, std::uint32_t, const float*, const float*) = &VecEnv::critic_value;
    static_assert(sizeof(gymrs_advantages_desc) == 112, "size");
    const bool all = a && b && c && d && e && f && g && h && g(GYMRS_CARTPOLE, 16) == 97;
    std::printf(all ? "ADVANTAGES_MIRROR_OK\n" : "missing\n");
    return all ? 0 : 1;
}
''')
    exe = tmp_path / "advantages_mirror"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib_dir}", "-lgymrs_amd",
                      f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "ADVANTAGES_MIRROR_OK" in res.stdout, res.stdout + res.stderr
