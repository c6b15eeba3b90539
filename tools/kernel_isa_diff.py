"""Compares the gfx950 device code of two builds of libegonerf_hip.so kernel by kernel: a refactor that only moves kernels between
sources must leave every one of them as it was.

    python tools/kernel_isa_diff.py OLD.so NEW.so [-o profiles/rNN/kernel_isa_diff.txt]

Per kernel (matched by demangled name over all code objects of a library, so a kernel may change its translation unit):
  * the resource metadata of its code object note: VGPR / AGPR / SGPR counts, spilled registers, scratch and LDS bytes;
  * its instruction stream as llvm-objdump prints it, without addresses and encodings (the `// addr: words` tail of a line) and with
    the literal of a pc-relative address computation (s_getpc_b64 followed by s_add_u32 / s_addc_u32) masked: those literals are
    distances to other symbols of the code object, which move with the file layout.  Branch targets stay: they are relative to the
    kernel itself.  The padding behind a kernel's last instruction is not part of the stream: zeros (printed as `...`), and the run of
    `s_nop 0` that closes a source's text section behind its last kernel (which kernel that is changes when kernels change sources).
The compiler gives kernels of an anonymous namespace no per-file decoration in this (non-RDC) build, so names compare as they are.
A kernel whose parameter list changed (and nothing else of its name) is matched with its predecessor and compared like any other.
A kernel that differs is listed with the resource line of both builds.  Exit status 1 if the kernel sets differ or any kernel differs."""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from egonerf_amd import build  # noqa: E402

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size")


def _tool(objdump: str, name: str) -> str:
    return os.path.join(os.path.dirname(objdump), name)


def _cxxfilt(objdump: str) -> str:
    for cand in (_tool(objdump, "llvm-cxxfilt"), shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("no demangler found (llvm-cxxfilt or c++filt)")


def _metadata(objdump: str, co: str) -> dict:
    """symbol -> {key: value} from the amdhsa.kernels list of the code object's metadata note"""
    notes = subprocess.run([_tool(objdump, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    entries = []
    for line in notes.splitlines():
        m = re.match(r"^  - (\.\w+):\s*(.*)$", line)   # a new entry of the kernel list (nested lists are indented further)
        if m:
            entries.append({})
        else:
            m = re.match(r"^    (\.\w+):\s*(.*)$", line)
        if m and entries:
            entries[-1][m.group(1)] = m.group(2).strip().strip("'")
    return {k[".symbol"][:-3]: {f: k.get(f, "0") for f in META} for k in entries if k.get(".symbol", "").endswith(".kd")}


def _streams(objdump: str, co: str) -> dict:
    """symbol -> normalised instruction lines"""
    dis = subprocess.run([objdump, "-d", co], capture_output=True, text=True, check=True).stdout
    out, cur, pcrel = {}, None, 0
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = re.sub(r"\s*//.*$", "", line).strip()
        ins = re.sub(r"\s+", " ", ins)
        if ins == "...":   # objdump's mark for the zero padding between two symbols: layout, not code
            continue
        if ins.startswith("s_getpc_b64"):
            pcrel = 3
        elif pcrel:
            pcrel -= 1
            if re.match(r"s_addc?_u32 ", ins):
                ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", ins)
        cur.append(ins)
    for body in out.values():
        while body and body[-1] == "s_nop 0":
            del body[-1]
    return out


def kernels(lib: str) -> dict:
    """demangled kernel name -> list of (metadata, instruction stream), one per code object that holds a kernel of that name"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        objdump, cos = build._code_objects(lib, tmp)
        for co in cos:
            meta, streams = _metadata(objdump, co), _streams(objdump, co)
            names = list(meta)
            dem = subprocess.run([_cxxfilt(objdump)], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            for sym, name in zip(names, dem):
                body = [re.sub(r"<" + re.escape(sym) + r"(\+0x[0-9a-f]+)?>", r"<self\1>", i) for i in streams[sym]]
                out.setdefault(name.strip(), []).append((meta[sym], body))
    for v in out.values():
        v.sort(key=repr)
    return out


def _without_parameters(name: str) -> str:
    """`void k<16, true>(A, B (*)(C))` -> `void k<16, true>`: the demangled name up to its (balanced) trailing parameter list"""
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i] if name.endswith(")") else name
    return name


def pair_changed_signatures(old: dict, new: dict) -> None:
    """A kernel whose parameter list changed keeps its name and template arguments: what is left unmatched on both sides is matched by
    those, and listed under the new build's name."""
    lone = {_without_parameters(n): n for n in old if n not in new}
    for n in [n for n in new if n not in old]:
        o = lone.get(_without_parameters(n))
        if o is not None:
            old[n] = old.pop(o)
    # ... and a kernel template that gained trailing arguments which default to false / 0 (a new switch, off in every instance that
    # existed before): `k<1, true, false>` is the successor of `k<1, true>`
    lone = {_without_parameters(n): n for n in old if n not in new}
    for n in [n for n in new if n not in old]:
        head = _without_parameters(n)
        while re.search(r", (false|0)>$", head) and head not in lone:
            head = re.sub(r", (false|0)>$", ">", head)
        if head in lone:
            old[n] = old.pop(lone.pop(head))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    pair_changed_signatures(old, new)
    lines, n_same, n_diff = [], 0, 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new or len(old[name]) != len(new[name]):
            lines.append(f"differs  {name}: " + ("only in the old build" if name not in new else "only in the new build" if name not in old
                                                  else f"{len(old[name])} copies before, {len(new[name])} after"))
            n_diff += 1
            continue
        for (mo, so), (mn, sn) in zip(old[name], new[name]):
            why = []
            if mo != mn:
                why.append("metadata " + ", ".join(f"{k[1:]} {mo[k]} -> {mn[k]}" for k in META if mo[k] != mn[k]))
            if so != sn:
                first = next((i for i, (x, y) in enumerate(zip(so, sn)) if x != y), min(len(so), len(sn)))
                why.append(f"instructions ({len(so)} -> {len(sn)}, first difference at #{first})")
            n_same += not why
            n_diff += bool(why)
            res = " ".join(f"{k[1:]}={mn[k]}" for k in META)
            lines.append(("differs  " if why else "same     ") + f"{name}  [{len(sn)} instructions; {res}]" + ("  <- " + "; ".join(why) if why else ""))
            if why:   # a kernel that was meant to change is judged by its resources: the old build's line next to the new one
                lines.append(f"  before {name}  [{len(so)} instructions; " + " ".join(f"{k[1:]}={mo[k]}" for k in META) + "]")
    n_old, n_new = sum(map(len, old.values())), sum(map(len, new.values()))
    lines.append(f"kernels: {n_old} before, {n_new} after; same {n_same}, differs {n_diff}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
