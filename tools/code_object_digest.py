#!/usr/bin/env python
"""Digests of the device code of one build of the library (developer tool, needs no GPU).

    python tools/code_object_digest.py DIR

DIR is where build_hip(out=DIR/libgymrs_amd.so) left a build: the objects of the translation units and the chain kernels'
stand-alone code object lie in DIR/_obj/libgymrs_amd/.  For the gfx950 code object of every translation unit (unbundled with
llvm-objdump --offloading, as tools/isa_path_count.py does) and for gymrs_aql_kernels.hsaco the tool prints one line: the
name, then size and sha256 of the sections .text (the machine code), .rodata (the kernel descriptors) and .note (registers,
scratch, kernel-argument layout).  Two builds whose lines are equal run the same device code; the files as a whole differ
anyway (.dynsym / .dynstr carry a per-unit symbol derived from the source path), which is why sections are compared.
"""
import hashlib
import subprocess
import sys
import tempfile
from pathlib import Path

from isa_path_count import _tool, unbundle

SECTIONS = (".text", ".rodata", ".note")
OBJCOPY_CANDIDATES = ("llvm-objcopy", "/opt/rocm/llvm/bin/llvm-objcopy")


def digest_line(name, code_object, tmp):
    fields = [name]
    for sec in SECTIONS:
        out = Path(tmp) / "section.bin"
        out.unlink(missing_ok=True)
        subprocess.run([_tool(OBJCOPY_CANDIDATES), f"--dump-section={sec}={out}", str(code_object), str(Path(tmp) / "unused.out")], check=True)
        blob = out.read_bytes()
        fields.append(f"{sec} {len(blob)} {hashlib.sha256(blob).hexdigest()}")
    return "  ".join(fields)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    objdir = Path(sys.argv[1]) / "_obj" / "libgymrs_amd"
    units = sorted(objdir.glob("*.o")) + sorted(objdir.glob("*.hsaco"))
    if not units:
        raise SystemExit(f"no objects under {objdir}")
    for unit in units:
        with tempfile.TemporaryDirectory() as tmp:
            objs = unbundle(unit, tmp)
            if objs[0].name == unit.name and unit.suffix == ".o":
                continue  # (a translation unit without device code)
            for i, obj in enumerate(objs):
                print(digest_line(unit.name + (f"#{i}" if len(objs) > 1 else ""), obj, tmp), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
