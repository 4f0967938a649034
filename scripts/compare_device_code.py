#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libmq_learner.so, kernel by kernel.

    python scripts/compare_device_code.py OLD.so NEW.so [--llvm-bin /opt/rocm/lib/llvm/bin]

Pulls the gfx950 code object out of each library's .hip_fatbin section, disassembles it, and compares every function
symbol of OLD with the symbol of the same name in NEW: the instruction text and the encoded words, addresses removed
(branches are relative, so a kernel that merely moved compares equal; the s_nop padding behind a function's
terminating s_endpgm / s_setpc is dropped: it depends on what follows the function), and every kernel's metadata entry
(argument block, registers, LDS, scratch). Prints one JSON line: how many symbols were identical, which differ, which are
missing from NEW, whose metadata differs, and which NEW adds. Exit status 1 if any OLD symbol is missing or differs.
Needs no GPU.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile


def code_object(lib, llvm, tmp, tag):
    fat = os.path.join(tmp, tag + ".fatbin")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat],
                   check=True)
    bundler = os.path.join(llvm, "clang-offload-bundler")
    targets = subprocess.run([bundler, "--list", "--type=o", "--input=" + fat], check=True, capture_output=True,
                             text=True).stdout.split()
    target = [t for t in targets if "gfx950" in t]
    if len(target) != 1:
        raise SystemExit("{}: expected one gfx950 code object, found {}".format(lib, targets))
    out = os.path.join(tmp, tag + ".co")
    subprocess.run([bundler, "--unbundle", "--type=o", "--input=" + fat, "--targets=" + target[0],
                    "--output=" + out], check=True)
    return out


def functions(co, llvm):
    """{symbol: [instruction text + encoding, ...]} of a code object."""
    text = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True,
                          capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or "//" not in line:
            continue
        ins, enc = line.split("//", 1)
        cur.append(ins.strip() + " | " + enc.split(":", 1)[1].strip())   # drop the address before the encoding
    # the s_nop padding behind a function's terminating s_endpgm / s_setpc depends on what the linker placed after it
    # (the last function of the section is padded to the section's end): not part of the function. Nothing but such
    # padding is dropped: nops anywhere before the terminator stay.
    for body in out.values():
        n = len(body)
        while n and body[n - 1].startswith("s_nop 0 |"):
            n -= 1
        if n and n < len(body) and body[n - 1].startswith(("s_endpgm", "s_setpc")):
            del body[n:]
    return out


def metadata(co, llvm):
    """{kernel name: its amdhsa.kernels entry} (argument block, registers, LDS, scratch) from the code object's note."""
    text = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                          text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("  - ."):
            cur = [line[4:]]
        elif cur is not None and line.startswith("    "):
            cur.append(line[4:])
            m = re.match(r"^    \.name:\s+(\S+)$", line)
            if m:
                out[m.group(1)] = cur
        elif cur is not None:
            cur = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--llvm-bin", default="/opt/rocm/lib/llvm/bin")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        co_old, co_new = code_object(a.old, a.llvm_bin, tmp, "old"), code_object(a.new, a.llvm_bin, tmp, "new")
        fo, fn = functions(co_old, a.llvm_bin), functions(co_new, a.llvm_bin)
        mo, mn = metadata(co_old, a.llvm_bin), metadata(co_new, a.llvm_bin)
    missing = sorted(s for s in fo if s not in fn)
    differ = sorted(s for s in fo if s in fn and fo[s] != fn[s])
    added = sorted(s for s in fn if s not in fo)
    meta_differ = sorted(k for k in mo if mo[k] != mn.get(k))
    print(json.dumps(dict(old_symbols=len(fo), new_symbols=len(fn), identical=len(fo) - len(missing) - len(differ),
                          instructions_compared=sum(len(v) for v in fo.values()), differ=differ, missing=missing,
                          kernels_with_metadata=len(mo), metadata_differ=meta_differ, added=added)))
    return 1 if missing or differ or meta_differ else 0


if __name__ == "__main__":
    sys.exit(main())
