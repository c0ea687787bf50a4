"""Softmax sampling at the C boundary, without a GPU: the flag constant, the settings struct and the five prototypes in the header,
exported by the library, bound in Python and declared in the Rust binding; a plain-C translation unit that static-asserts the
constant, the struct's layout and the ABI version and calls the host-only draw; the NULL checks and refusals; the mirrors' members."""
import ctypes as C
import inspect
import re
import spawn_server
from importlib import import_module
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PROTOTYPES = {
    "gymrs_set_sampling": r"gymrs_status gymrs_set_sampling\(gymrs_engine\* e, const gymrs_sampling\* x\);",
    "gymrs_get_sampling": r"gymrs_status gymrs_get_sampling\(gymrs_engine\* e, gymrs_sampling\* x_out\);",
    "gymrs_sample_actions": r"gymrs_status gymrs_sample_actions\(gymrs_engine\* e, void\* actions_dev, float\* prob_dev\);",
    "gymrs_sample_draw": r"gymrs_status gymrs_sample_draw\(const gymrs_sampling\* x, uint32_t n_actions, const float\* logits, uint64_t global_id, "
                         r"uint64_t tick, uint8_t\* action,\s+float\* probs\);",
    "gymrs_sharded_set_sampling": r"gymrs_status gymrs_sharded_set_sampling\(gymrs_sharded\* h, const gymrs_sampling\* x\);",
}
EINVAL = 1
LINK = ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]


def test_constant_struct_and_prototypes_in_header():
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    assert re.search(r"^#define GYMRS_CLOSED_LOOP_SAMPLE 32u\b", text, flags=re.M)
    assert re.search(r"^#define GYMRS_CLOSED_LOOP_EXPLORE 16u\b", text, flags=re.M) and re.search(r"^#define GYMRS_CLOSED_LOOP_FITNESS 1u\b", text, flags=re.M)
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text)  # additive: callers detect the feature by the symbol gymrs_set_sampling
    assert re.search(r"^typedef struct \{ uint64_t seed; float scale; uint32_t reserved; \} gymrs_sampling;", text, flags=re.M)
    for name, proto in PROTOTYPES.items():
        assert re.search("^" + proto + "$", text, flags=re.M), name
    # the definition, to the bit
    for phrase in ("m     = y[greedy]", "d[a]  = (y[a] - m) * scale", "!(d[a] >= -126.0f) ? 0.0f", "ldexpf(P(d[a] - floorf(d[a])), (int)floorf(d[a]))",
                   "0x1.62e430p-1, 0x1.ebfc40p-3, 0x1.c69f6ap-5, 0x1.3c4a8ap-7, 0x1.4ca4ccp-10, 0x1.b4d1e4p-13", "total = ((w[0] + w[1]) + w[2])",
                   "3 << 16", "thr   = ((float)(word >> 8) * 0x1p-24f) * total", "prob[a] = w[a] / total", "scale = log2(e) /"):
        assert phrase in text, phrase


def test_exported_bound_and_in_rust_ffi(gymrs):
    lib = gymrs.load_library()
    sigs = import_module("gym-rs_amd._lib").SIGNATURES
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    for name in PROTOTYPES:
        assert hasattr(lib, name) and name in sigs, name
    for name in ("gymrs_set_sampling", "gymrs_get_sampling", "gymrs_sharded_set_sampling"):
        assert sigs[name] == (C.c_int, [C.c_void_p, C.c_void_p]), name
    assert sigs["gymrs_sample_actions"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    f32p = C.POINTER(C.c_float)
    assert sigs["gymrs_sample_draw"] == (C.c_int, [C.c_void_p, C.c_uint32, f32p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint8), f32p])
    assert re.search(r"pub const GYMRS_CLOSED_LOOP_SAMPLE: u32 = 32;", ffi)
    assert re.search(r"pub struct GymrsSampling \{\s*pub seed: u64,\s*pub scale: f32,\s*pub reserved: u32,\s*\}", ffi)
    assert re.search(r"pub fn gymrs_set_sampling\(e: \*mut GymrsEngine, x: \*const GymrsSampling\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_get_sampling\(e: \*mut GymrsEngine, x_out: \*mut GymrsSampling\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_sample_actions\(e: \*mut GymrsEngine, actions_dev: \*mut c_void, prob_dev: \*mut f32\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_sample_draw\(\s*x: \*const GymrsSampling,\s*n_actions: u32,\s*logits: \*const f32,\s*global_id: u64,\s*tick: u64,\s*"
                     r"action: \*mut u8,\s*probs: \*mut f32,?\s*\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_sharded_set_sampling\(h: \*mut GymrsSharded, x: \*const GymrsSampling\) -> c_int;", ffi)
    assert lib.gymrs_abi_version() == 3


def test_python_constant_struct_and_settings(gymrs):
    assert gymrs.CLOSED_LOOP_SAMPLE == 32 == gymrs.engine.CLOSED_LOOP_SAMPLE
    x = gymrs.Sampling
    assert C.sizeof(x) == 16 and [(n, getattr(x, n).offset) for n, _ in x._fields_] == [("seed", 0), ("scale", 8), ("reserved", 12)]
    make = gymrs.engine._closed_loop_desc
    assert make(100, 7, False, False, None, sample=True).flags == 32 and make(100, 7, True, True, None, sample=True).flags == 37
    assert make(100, 7, True, True, None).flags == 5 and make(100, 7, False, False, None, flags=6, sample=True).flags == 6  # raw flags override
    assert make(100, 7, False, False, None, None, True, True).flags == 48  # both: the library refuses it, not the binding
    s = gymrs.engine._sampling
    assert s(3, 1.0, None).scale == C.c_float(1.4426950408889634).value and s(3, None, 0.0).scale == 0.0 and s(3, 2.0, None).scale == C.c_float(0.7213475204444817).value
    assert s(-1, None, 2.5).seed == 2**64 - 1 and s(3, None, 2.5).scale == 2.5 and s(3, None, 5).reserved == 0
    for bad in ((3, None, None), (3, 1.0, 1.0), (3, 0.0, None), (3, -1.0, None)):
        with pytest.raises(ValueError):
            s(*bad)


def test_calls_refuse_null_arguments_and_bad_settings(gymrs):
    lib = gymrs.load_library()
    x = gymrs.Sampling(1, 1.0, 0)
    for name in ("gymrs_set_sampling", "gymrs_get_sampling", "gymrs_sharded_set_sampling"):
        assert getattr(lib, name)(None, C.byref(x)) == EINVAL, name
        assert name in lib.gymrs_last_error().decode(), name
        assert getattr(lib, name)(None, None) == EINVAL, name
    assert lib.gymrs_sample_actions(None, C.byref(x), None) == EINVAL and "gymrs_sample_actions" in lib.gymrs_last_error().decode()
    y = (C.c_float * 8)(0.3, -0.2, 1.1, 0, 0, 0, 0, 0)
    a, p = C.c_uint8(9), (C.c_float * 8)()
    assert lib.gymrs_sample_draw(None, 3, y, 0, 0, C.byref(a), p) == EINVAL and "gymrs_sample_draw" in lib.gymrs_last_error().decode()
    assert lib.gymrs_sample_draw(C.byref(x), 3, None, 0, 0, C.byref(a), p) == EINVAL and "logits" in lib.gymrs_last_error().decode()
    for n in (0, 1, 9, 256):
        assert lib.gymrs_sample_draw(C.byref(x), n, y, 0, 0, C.byref(a), p) == EINVAL and "n_actions" in lib.gymrs_last_error().decode()
    for scale in (float("nan"), float("inf"), -1.0, -1e-30):
        bad = gymrs.Sampling(1, scale, 0)
        assert lib.gymrs_sample_draw(C.byref(bad), 3, y, 0, 0, C.byref(a), p) == EINVAL and "scale" in lib.gymrs_last_error().decode(), scale
    bad = gymrs.Sampling(1, 1.0, 1)
    assert lib.gymrs_sample_draw(C.byref(bad), 3, y, 0, 0, C.byref(a), p) == EINVAL and "reserved" in lib.gymrs_last_error().decode()
    assert a.value == 9  # a refused call writes nothing
    for n in (2, 3, 8):  # host only: no engine, no GPU
        assert lib.gymrs_sample_draw(C.byref(x), n, y, 5, 9, C.byref(a), p) == 0 and a.value < n
        assert abs(sum(p[:n]) - 1) < 1e-6
        assert lib.gymrs_sample_draw(C.byref(x), n, y, 5, 9, None, None) == 0
    action, probs = gymrs.sample_draw(1, 1.0, [0.3, -0.2, 1.1], 5, 9)
    assert lib.gymrs_sample_draw(C.byref(x), 3, y, 5, 9, C.byref(a), p) == 0
    assert action == a.value and probs.shape == (3,) and probs.dtype.name == "float32" and list(probs) == list(p[:3])
    zero = gymrs.Sampling(1, 0.0, 0)  # scale 0: the uniform policy
    assert lib.gymrs_sample_draw(C.byref(zero), 3, y, 5, 9, C.byref(a), p) == 0 and list(p[:3]) == [C.c_float(1 / 3).value] * 3


def test_mirrors_have_the_members(gymrs):
    for cls in (gymrs.BatchedEngine, gymrs.ShardedEngine):
        params = inspect.signature(cls.rollout_closed_loop).parameters
        assert params["sample"].default is False and params["sample"].kind is inspect.Parameter.KEYWORD_ONLY, cls
        params = inspect.signature(cls.set_sampling).parameters
        assert list(params)[:2] == ["self", "seed"], cls
        for name in ("temperature", "scale"):
            assert params[name].default is None and params[name].kind is inspect.Parameter.KEYWORD_ONLY, (cls, name)
        assert callable(cls.sampling) and callable(cls.sample_actions), cls
    params = inspect.signature(gymrs.BatchedEngine.rollout_transitions).parameters
    assert params["sample"].default is False and params["sample"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(gymrs.BatchedEngine.sample_actions).parameters) == ["self", "actions_dev", "prob"]
    assert list(inspect.signature(gymrs.sample_draw).parameters) == ["seed", "scale", "logits", "global_id", "tick"]
    hpp = (ROOT / "include" / "gymrs_env.hpp").read_text()
    for name in tuple(PROTOTYPES) + ("GYMRS_CLOSED_LOOP_SAMPLE", "gymrs_sampling"):
        assert name in hpp, name
    rs = ROOT / "bindings" / "rust" / "src"
    engine, sharded = (rs / "engine.rs").read_text(), (rs / "sharded.rs").read_text()
    for name in ("gymrs_set_sampling", "gymrs_get_sampling", "gymrs_sample_actions", "gymrs_sample_draw", "GYMRS_CLOSED_LOOP_SAMPLE"):
        assert name in engine, name
    assert "gymrs_sharded_set_sampling" in sharded and "GYMRS_CLOSED_LOOP_SAMPLE" in sharded
    for text, name in ((ROOT / "INTEGRATION.md").read_text(), "INTEGRATION.md"), ((ROOT / "README.md").read_text(), "README.md"):
        assert "gymrs_set_sampling" in text and "GYMRS_CLOSED_LOOP_SAMPLE" in text, name
    assert re.search(r"^#+ Sampling$", (ROOT / "INTEGRATION.md").read_text(), flags=re.M)
    assert (ROOT / "examples" / "policy_gradient_collection.py").exists() and (ROOT / "tools" / "bench_policy_sample.py").exists()
    assert (ROOT / "profiles" / "policy_sample.md").exists()
    build = (ROOT / "gym-rs_amd" / "build.py").read_text()
    for unit in ("gymrs_sample.hip", "gymrs_sample_fitness.hip", "gymrs_table_sample_cartpole.hip", "gymrs_table_sample_mountain_car.hip"):
        assert unit in build and (ROOT / "gym-rs_amd" / "csrc" / unit).exists(), unit


def test_constant_layout_and_host_calls_from_c(tmp_path):
    src = tmp_path / "sample.c"
    src.write_text(r'''
#include "gymrs_amd.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
_Static_assert(GYMRS_CLOSED_LOOP_SAMPLE == 32u, "bit 5");
_Static_assert((GYMRS_CLOSED_LOOP_SAMPLE & (GYMRS_CLOSED_LOOP_FITNESS | GYMRS_CLOSED_LOOP_LANE_PARAMS | GYMRS_CLOSED_LOOP_EXPLORE)) == 0u, "a bit of its own");
_Static_assert(GYMRS_ABI_VERSION == 3, "additive");
_Static_assert(sizeof(gymrs_sampling) == 16, "settings size");
_Static_assert(offsetof(gymrs_sampling, seed) == 0 && offsetof(gymrs_sampling, scale) == 8 && offsetof(gymrs_sampling, reserved) == 12, "settings layout");
int main(void) {
    gymrs_sampling x = {7u, 1.4426950f, 0u};
    const float y[3] = {0.3f, -0.2f, 1.1f}, nan_first[3] = {0.0f / 0.0f, 5.0f, 7.0f};
    float p[3] = {9.0f, 9.0f, 9.0f};
    uint8_t action = 9, again = 9;
    if (gymrs_abi_version() != 3) return 1;
    if (gymrs_set_sampling(NULL, &x) != GYMRS_EINVAL || !strstr(gymrs_last_error(), "gymrs_set_sampling")) return 2;
    if (gymrs_get_sampling(NULL, &x) != GYMRS_EINVAL || !strstr(gymrs_last_error(), "gymrs_get_sampling")) return 3;
    if (gymrs_sample_actions(NULL, p, NULL) != GYMRS_EINVAL || !strstr(gymrs_last_error(), "gymrs_sample_actions")) return 4;
    if (gymrs_sharded_set_sampling(NULL, &x) != GYMRS_EINVAL || !strstr(gymrs_last_error(), "gymrs_sharded_set_sampling")) return 5;
    if (gymrs_sample_draw(NULL, 3, y, 0, 0, &action, p) != GYMRS_EINVAL) return 6;
    if (gymrs_sample_draw(&x, 3, y, 5, 9, &action, p) != GYMRS_OK || action > 2) return 7;
    if (!(p[0] > 0.0f && p[1] > 0.0f && p[2] > p[0] && p[0] > p[1]) || p[0] + p[1] + p[2] < 0.999999f || p[0] + p[1] + p[2] > 1.000001f) return 8;
    if (gymrs_sample_draw(&x, 3, y, 5, 9, &again, NULL) != GYMRS_OK || again != action) return 9; /* reproducible */
    if (gymrs_sample_draw(&x, 3, nan_first, 5, 9, &action, p) != GYMRS_OK || action != 0 || p[0] != 1.0f || p[1] != 0.0f || p[2] != 0.0f) return 10;
    x.scale = 1e30f; /* the argmax wherever there is no exact tie */
    if (gymrs_sample_draw(&x, 3, y, 5, 9, &action, p) != GYMRS_OK || action != 2 || p[2] != 1.0f) return 11;
    x.scale = -1.0f;
    if (gymrs_sample_draw(&x, 3, y, 5, 9, &action, p) != GYMRS_EINVAL || !strstr(gymrs_last_error(), "scale")) return 12;
    x.scale = 1.0f; x.reserved = 1u;
    if (gymrs_sample_draw(&x, 3, y, 5, 9, &action, p) != GYMRS_EINVAL || !strstr(gymrs_last_error(), "reserved")) return 13;
    x.reserved = 0u;
    if (gymrs_sample_draw(&x, 1, y, 5, 9, &action, p) != GYMRS_EINVAL || gymrs_sample_draw(&x, 9, y, 5, 9, &action, p) != GYMRS_EINVAL) return 14;
    if (gymrs_sample_draw(&x, 3, NULL, 5, 9, &action, p) != GYMRS_EINVAL) return 15;
    {
        gymrs_closed_loop_desc d = {100, GYMRS_CLOSED_LOOP_SAMPLE | GYMRS_CLOSED_LOOP_LANE_PARAMS, NULL, 0};
        if (d.flags != 36u || gymrs_rollout_closed_loop(NULL, &d) != GYMRS_EINVAL) return 16;
    }
    printf("SAMPLE_ABI_OK\n");
    return 0;
}
''')
    exe = tmp_path / "sample"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                      f"-L{lib_dir}", "-lgymrs_amd", f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "SAMPLE_ABI_OK" in res.stdout, (res.returncode, res.stdout + res.stderr)


def test_cpp_mirror_members_compile(tmp_path):
    """A small program of its own that names the new members of include/gymrs_env.hpp (their signatures are part of the check); it
    runs no engine: it only has to compile, link and start."""
    src = tmp_path / "sample_mirror.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include "gymrs_env.hpp"
using gymrs::ShardedVecEnv;
using gymrs::VecEnv;
int main() {
    void (VecEnv::*a)(std::uint64_t, float) = &VecEnv::set_sampling;
    void (VecEnv::*b)() = &VecEnv::clear_sampling;
    gymrs_sampling (VecEnv::*c)() const = &VecEnv::sampling;
    void (VecEnv::*d)(void*, float*) = &VecEnv::sample_actions;
    void (VecEnv::*e)(std::uint32_t, bool, bool, const gymrs_trajectory*, bool, bool) = &VecEnv::rollout_closed_loop;
    void (ShardedVecEnv::*f)(std::uint64_t, float) = &ShardedVecEnv::set_sampling;
    void (ShardedVecEnv::*g)() = &ShardedVecEnv::clear_sampling;
    void (ShardedVecEnv::*h)(std::uint32_t, bool, bool, bool, bool) = &ShardedVecEnv::rollout_closed_loop;
    void (VecEnv::*i)(std::uint32_t, const gymrs_trajectory&, float*, float*, bool, bool, bool) = &VecEnv::rollout_transitions;
    // the older overloads are still there
    void (VecEnv::*j)(std::uint32_t, bool, bool, const gymrs_trajectory*, bool) = &VecEnv::rollout_closed_loop;
    void (ShardedVecEnv::*k)(std::uint32_t, bool, bool, bool) = &ShardedVecEnv::rollout_closed_loop;
    static_assert(GYMRS_CLOSED_LOOP_SAMPLE == 32u && sizeof(gymrs_sampling) == 16, "constant, size");
    const float y[3] = {0.3f, -0.2f, 1.1f};
    float p[3] = {0, 0, 0};
    const std::uint8_t action = gymrs::sample_draw(gymrs_sampling{7, 1e30f, 0}, 3, y, 5, 9, p);  // host only
    const bool all = a && b && c && d && e && f && g && h && i && j && k && action == 2 && p[2] == 1.0f;
    std::printf(all ? "SAMPLE_MIRROR_OK\n" : "missing\n");
    return all ? 0 : 1;
}
''')
    exe = tmp_path / "sample_mirror"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib_dir}", "-lgymrs_amd",
                      f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "SAMPLE_MIRROR_OK" in res.stdout, res.stdout + res.stderr
