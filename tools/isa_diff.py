#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of the library, kernel by kernel (no GPU needed).

    python tools/isa_diff.py --lib OLD/libgymrs_amd.so --lib NEW/libgymrs_amd.so [--hsaco OLD.hsaco --hsaco NEW.hsaco] [--out FILE]

For every HIP code object of the library (the clang offload bundles of its .hip_fatbin section, gfx950 entries) and for the
chain kernels' stand-alone code object (gymrs_aql_kernels.hsaco; by default the one the build left in _obj/<lib stem>/ next to
each library) it disassembles every kernel with llvm-objdump and reads its kernel descriptor (<kernel>.kd: register counts,
LDS and kernel-argument sizes).  A kernel counts as identical when both its instruction text (addresses, address comments and
the padding behind it stripped: branch offsets are relative, so a kernel that moved inside its code object compares equal) and
its descriptor bytes (all but the code's offset from the descriptor) are.  The report lists kernels that are identical, that differ, that only the first build has (removed) and that only the
second one has (added), under their demangled names.  Exit status 1 when any kernel differs or was removed.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "gfx950"


def _tool(name: str) -> str:
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and (Path(root) / "llvm" / "bin" / name).exists():
            return str(Path(root) / "llvm" / "bin" / name)
    found = shutil.which(name)
    if not found:
        raise SystemExit(f"{name} not found (looked in $ROCM_PATH/llvm/bin, /opt/rocm/llvm/bin, PATH)")
    return found


def _elf_sections(blob: bytes) -> dict:
    """name -> (addr, offset, size) of a 64-bit little-endian ELF."""
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    heads = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    strtab = heads[shstrndx]
    names = blob[strtab[4]:strtab[4] + strtab[5]]
    out = {}
    for h in heads:
        name = names[h[0]:names.index(b"\0", h[0])].decode()
        out[name] = (h[3], h[4], h[5])
    return out


def code_objects_of_library(lib: Path) -> list[bytes]:
    """The gfx950 code objects of every offload bundle in the library's .hip_fatbin section, in section order."""
    blob = lib.read_bytes()
    secs = _elf_sections(blob)
    if ".hip_fatbin" not in secs:
        raise SystemExit(f"{lib}: no .hip_fatbin section")
    _, off, size = secs[".hip_fatbin"]
    fat = blob[off:off + size]
    objs = []
    for m in re.finditer(re.escape(MAGIC), fat):
        at = m.start()
        n_entries, = struct.unpack_from("<Q", fat, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n_entries):
            e_off, e_size, t_len = struct.unpack_from("<QQQ", fat, p)
            triple = fat[p + 24:p + 24 + t_len].decode()
            p += 24 + t_len
            if triple.endswith(TARGET) or TARGET + ":" in triple:
                objs.append(fat[at + e_off:at + e_off + e_size])
    if not objs:
        raise SystemExit(f"{lib}: no {TARGET} code object found")
    return objs


def kernels_of_code_object(obj: bytes, workdir: Path, tag: str) -> dict:
    """kernel symbol -> sha256 of (instruction text, kernel descriptor bytes); plus the text itself for reports."""
    path = workdir / f"{tag}.co"
    path.write_bytes(obj)
    text = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", str(path)], check=True, capture_output=True,
                          text=True).stdout
    funcs: dict[str, list[str]] = {}
    cur = None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        ins = re.sub(r"\s*//.*$", "", line).strip()  # address comments of branches
        if ins and ins != "...":  # ("..." = the zero padding behind a kernel, which depends on where the next one starts)
            funcs[cur].append(ins)
    # kernel descriptors: <mangled>.kd objects in .rodata
    secs = _elf_sections(obj)
    syms = subprocess.run([_tool("llvm-readelf"), "-s", "--wide", str(path)], check=True, capture_output=True, text=True).stdout
    kds = {}
    for line in syms.splitlines():
        parts = line.split(None, 7)
        if len(parts) == 8 and parts[7].endswith(".kd") and parts[3] == "OBJECT":
            value, size = int(parts[1], 16), int(parts[2])
            for addr, off, sz in secs.values():
                if addr <= value < addr + sz and off:
                    kd = bytearray(obj[off + value - addr:off + value - addr + size])
                    kd[16:24] = bytes(8)  # kernel_code_entry_byte_offset: where the code lies relative to the descriptor, not what it is
                    kds[parts[7][:-3]] = bytes(kd)
                    break
    out = {}
    for name, kd in kds.items():
        body = funcs.get(name, [])
        h = hashlib.sha256(("\n".join(body)).encode() + b"\0" + kd).hexdigest()
        out[name] = (h, body)
    return out


def collect(lib: Path, hsaco: Path | None, workdir: Path, tag: str) -> dict:
    kernels = {}
    for i, obj in enumerate(code_objects_of_library(lib)):
        for name, v in kernels_of_code_object(obj, workdir, f"{tag}_lib{i}").items():
            kernels[f"lib: {name}"] = v
    if hsaco is not None:
        for name, v in kernels_of_code_object(hsaco.read_bytes(), workdir, f"{tag}_chain").items():
            kernels[f"chain: {name}"] = v
    return kernels


def demangle(names: list[str]) -> list[str]:
    """'lib: <mangled>' -> 'lib: <demangled>' (llvm-cxxfilt or c++filt; without either the mangled names stay)."""
    raw = [k.split(": ", 1)[1] for k in names]
    tool = next((t for t in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if t and Path(t).exists()), None)
    if tool is None:
        return list(names)
    out = subprocess.run([tool], input="\n".join(raw) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    return [k.split(": ", 1)[0] + ": " + d for k, d in zip(names, out)]


def default_hsaco(lib: Path) -> Path | None:
    p = lib.parent / "_obj" / lib.stem / "gymrs_aql_kernels.hsaco"
    return p if p.exists() else None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", action="append", required=True, type=Path, help="a build of libgymrs_amd.so (twice: old, new)")
    ap.add_argument("--hsaco", action="append", type=Path, help="the chain code object of each build (twice; default: next to each --lib)")
    ap.add_argument("--out", type=Path, help="also write the report here")
    ap.add_argument("--show", type=int, default=0, help="print the first N lines of difference of each kernel that differs")
    args = ap.parse_args(argv)
    if len(args.lib) != 2:
        ap.error("--lib twice: the old build, then the new one")
    hsacos = args.hsaco or [default_hsaco(args.lib[0]), default_hsaco(args.lib[1])]
    if len(hsacos) != 2:
        ap.error("--hsaco twice, or not at all")
    with tempfile.TemporaryDirectory() as tmp:
        old = collect(args.lib[0], hsacos[0], Path(tmp), "old")
        new = collect(args.lib[1], hsacos[1], Path(tmp), "new")
    names = sorted(set(old) | set(new))
    shown = dict(zip(names, demangle(names)))
    same = sorted(k for k in old if k in new and old[k][0] == new[k][0])
    differ = sorted(k for k in old if k in new and old[k][0] != new[k][0])
    removed = sorted(k for k in old if k not in new)
    added = sorted(k for k in new if k not in old)
    lines = [f"old: {args.lib[0]}" + (f" + {hsacos[0]}" if hsacos[0] else ""),
             f"new: {args.lib[1]}" + (f" + {hsacos[1]}" if hsacos[1] else ""),
             f"kernels: old {len(old)}, new {len(new)}; identical {len(same)}, differ {len(differ)}, removed {len(removed)}, added {len(added)}", ""]
    for title, names in (("DIFFER", differ), ("REMOVED", removed), ("ADDED", added)):
        lines.append(f"== {title} ({len(names)})")
        for k in names:
            lines.append(f"  {shown[k]}")
            if title == "DIFFER" and args.show:
                import difflib
                d = list(difflib.unified_diff(old[k][1], new[k][1], lineterm="", n=0))
                lines.extend("      " + x for x in d[2:2 + args.show])
        lines.append("")
    lines.append(f"== IDENTICAL ({len(same)})")
    lines.extend(f"  {shown[k]}" for k in same)
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if args.out:
        args.out.write_text(report)
    return 1 if differ or removed else 0


if __name__ == "__main__":
    raise SystemExit(main())
