#!/usr/bin/env python
"""Instruction counts along ONE path through a kernel of a built library (developer tool, needs no GPU).

    python tools/isa_path_count.py LIB KERNEL_SYMBOL_SUBSTRING [--decisions TNNT...] [--show]

The library's gfx950 code objects are unbundled with llvm-objdump --offloading (into a temporary directory), the kernel is
disassembled and cut into basic blocks at the branch targets, and the tool walks from the entry to s_endpgm:

  * s_cbranch_execz is NOT taken and s_cbranch_execnz IS taken (some work-item is active: on the common path of the
    per-step kernel every wave is full, and nearly every wave re-arms a lane of each of its four lane columns), except at the
    offsets of --flip-exec (the skip over the kernel's ragged-tail half, reached by a full wave with no work-item left);
  * every other conditional branch (scc / vcc: wave-uniform decisions on kernel arguments and ballots) takes the next
    letter of --decisions, T(aken) or N(ot taken); --show prints each of them with the instructions in front of it, which
    is how a decision string is written and audited (profiles/cartpole_fastpath_isa.txt keeps the strings it used);
  * a loop's back edge is followed once (the path never enters a block twice).

It prints the counts profiles/cartpole_fastpath_isa.txt records -- v_div_scale, v_div_fmas, v_div_fixup, v_rcp,
VGPR-to-VGPR v_mov, v_cmp, packed (v_pk_*), all VALU, s_nop -- and the kernel's register and scratch figures from the
code object's metadata.
"""
import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

OBJDUMP_CANDIDATES = ("llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump")
READELF_CANDIDATES = ("llvm-readelf", "/opt/rocm/llvm/bin/llvm-readelf")


def _tool(cands):
    for c in cands:
        p = shutil.which(c) or (c if Path(c).exists() else None)
        if p:
            return p
    raise SystemExit(f"none of {cands} found")


def unbundle(lib, tmp):
    """The gfx950 code objects of a library or an object file, unbundled into the directory `tmp` (a bare code object: a copy of it)."""
    copy = Path(tmp) / Path(lib).name
    shutil.copy(lib, copy)
    subprocess.run([_tool(OBJDUMP_CANDIDATES), "--offloading", str(copy)], check=True, stdout=subprocess.DEVNULL, cwd=tmp)
    return sorted(p for p in Path(tmp).iterdir() if "amdgcn" in p.name) or [copy]


def disassemble(lib, needle):
    objdump = _tool(OBJDUMP_CANDIDATES)
    with tempfile.TemporaryDirectory() as tmp:
        for obj in unbundle(lib, tmp):
            syms = subprocess.run([objdump, "-t", str(obj)], check=True, capture_output=True, text=True).stdout
            names = [ln.split()[-1] for ln in syms.splitlines() if " F .text" in ln and needle in ln]
            if not names:
                continue
            if len(names) > 1:
                raise SystemExit("the name matches several kernels:\n  " + "\n  ".join(names))
            text = subprocess.run([objdump, "-d", f"--disassemble-symbols={names[0]}", str(obj)], check=True, capture_output=True, text=True).stdout
            meta = subprocess.run([_tool(READELF_CANDIDATES), "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
            return names[0], text, meta
    raise SystemExit(f"no kernel matching {needle!r} in {lib}")


def parse(text):
    """[(offset, mnemonic, operands, target offset or None)] in address order; offsets relative to the symbol."""
    ins, base = [], None
    for ln in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <", ln)
        if m:
            base = int(m.group(1), 16)
            continue
        m = re.match(r"^\t(\S+)\s*(.*?)\s*// ([0-9A-F]+): \S+( \S+)*?( <[^>]*\+0x([0-9a-f]+)>)?\s*$", ln)
        if not m or base is None:
            continue
        ins.append((int(m.group(3), 16) - base, m.group(1), m.group(2), int(m.group(6), 16) if m.group(6) else None))
    return ins


def is_vgpr_move(mn, ops):
    return mn.startswith(("v_mov_b32", "v_mov_b64")) and re.fullmatch(r"v\d+|v\[\d+:\d+\]", ops.split(",")[-1].strip()) is not None


def walk(ins, decisions, show, flip=()):
    at = {off: i for i, (off, *_rest) in enumerate(ins)}
    counts = dict.fromkeys(("v_div_scale", "v_div_fmas", "v_div_fixup", "v_rcp", "v_mov vgpr->vgpr", "v_cmp", "v_pk", "VALU", "s_nop", "instructions"), 0)
    seen, i, used, dec = set(), 0, 0, list(decisions)
    while i < len(ins):
        off, mn, ops, tgt = ins[i]
        if i in seen:
            raise SystemExit(f"the path re-enters +{off:#x}: a decision is wrong")
        seen.add(i)
        counts["instructions"] += 1
        if mn.startswith("v_"):
            counts["VALU"] += 1
            for k in ("v_div_scale", "v_div_fmas", "v_div_fixup", "v_rcp", "v_cmp", "v_pk"):
                if mn.startswith(k):
                    counts[k] += 1
            if is_vgpr_move(mn, ops):
                counts["v_mov vgpr->vgpr"] += 1
        if mn == "s_nop":
            counts["s_nop"] += 1
        if mn == "s_endpgm":
            break
        nxt = i + 1
        if mn == "s_branch":
            nxt = at[tgt]
        elif mn.startswith("s_cbranch_exec"):
            take = mn.endswith("execnz") != (off in flip)
            if show:
                print(f"    exec branch at +{off:#x}: {mn} -> +{tgt:#x} {'taken' if take else 'not taken'}")
            if take and at[tgt] in seen:
                take = False  # a loop's back edge: once round
            if take:
                nxt = at[tgt]
        elif mn.startswith("s_cbranch_"):
            if at[tgt] in seen:  # back edge of a wave-uniform loop: leave it
                take = False
            else:
                if used >= len(dec):
                    raise SystemExit(f"decision {used + 1} missing: {mn} at +{off:#x} (run with --show)")
                take = dec[used] == "T"
                if show:
                    print(f"--- decision {used + 1} ({'taken' if take else 'not taken'}): {mn} -> +{tgt:#x}, at +{off:#x}; before it:")
                    for o, m2, p2, _t in ins[max(0, i - 6):i]:
                        print(f"      +{o:#x} {m2} {p2}")
                used += 1
            if take:
                nxt = at[tgt]
        i = nxt
    return counts, used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("kernel")
    ap.add_argument("--decisions", default="")
    ap.add_argument("--show", action="store_true")
    ap.add_argument("--flip-exec", default="", help="comma-separated offsets (hex) of exec branches that go the OTHER way: the skip over the "
                    "ragged-tail half of the kernel, which a full wave reaches with no work-item left")
    args = ap.parse_args()
    name, text, meta = disassemble(args.lib, args.kernel)
    ins = parse(text)
    counts, used = walk(ins, args.decisions.upper(), args.show, {int(x, 16) for x in args.flip_exec.split(",") if x})
    print(f"kernel {name}")
    print(f"  {len(ins)} instructions in all; the path: {counts['instructions']}, {used} decisions used ({args.decisions.upper()[:used]})")
    for k, v in counts.items():
        if k != "instructions":
            print(f"  {k:18s} {v}")
    # the metadata entry of the kernel: the keys around its .name
    for key in (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"):
        m = None
        k0 = meta.find(f"{name}.kd")
        if k0 >= 0:
            lo = meta.rfind("- .agpr_count", 0, k0)
            lo = lo if lo >= 0 else meta.rfind("  - .", 0, k0)
            hi = meta.find("\n  - .", k0)
            m = re.search(re.escape(key) + r":\s*(\d+)", meta[lo:hi if hi >= 0 else len(meta)])
        print(f"  {key:28s} {m.group(1) if m else '?'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
