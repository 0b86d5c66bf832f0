#!/usr/bin/env python3
"""Compare the gfx950 code objects inside two objects or shared libraries, kernel by kernel.

    python tools/codeobj_diff.py A B [--json OUT]

A and B are host objects or libraries built by hipcc (build/sots_kernels.o, libsots_hip.so, variants/*.so).  The
device code object is taken out of each (llvm-objcopy: section .hip_fatbin; clang-offload-bundler: the gfx950
entry), its SHA-256 is printed, and where the two differ every kernel is compared on its own:

  * kernels that only one side has;
  * kernels whose code bytes differ (the function symbol's bytes in .text);
  * kernels whose 64-byte descriptor (symbol NAME.kd) differs outside bytes 16-23 - those hold the entry's offset
    from the descriptor and move with the layout, everything else in it is the kernel's own (registers, LDS, flags).

For equal hashes build both sides with the same -cuid=NAME (hipcc otherwise names a symbol after a hash of the source
file and its path, and no edit leaves that alone).  A refactor that moves definitions may reorder the kernels in the
object: the SHA-256 then differs while this report is empty, and that is the statement "no kernel changed".  Exit status 0: equal hashes; 2: the hashes differ but the
kernel sets, every kernel's code and every descriptor are equal; 1: a kernel differs.  Symbol tables and bytes only:
nothing is disassembled.
"""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
STT_OBJECT, STT_FUNC = 1, 2
KD_BYTES = 64
KD_ENTRY_OFFSET = slice(16, 24)  # kernel_code_entry_byte_offset


def extract_code_object(path, workdir, tag):
    """The gfx950 code object (an ELF) of a host object or library, as bytes."""
    fatbin = os.path.join(workdir, tag + ".hipfb")
    out = os.path.join(workdir, tag + ".co")
    subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", path, fatbin],
                   check=True)
    if not os.path.exists(fatbin) or os.path.getsize(fatbin) == 0:
        raise SystemExit(f"{path}: no .hip_fatbin section")
    subprocess.run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                    f"--input={fatbin}", f"--output={out}"], check=True)
    with open(out, "rb") as f:
        return f.read()


def elf_symbols(elf):
    """{name: (type, bytes or None)} for every defined, sized symbol of a little-endian ELF64."""
    if elf[:4] != b"\x7fELF" or elf[4] != 2 or elf[5] != 1:
        raise SystemExit("not a little-endian ELF64 code object")
    e_shoff, = struct.unpack_from("<Q", elf, 0x28)
    e_shentsize, e_shnum = struct.unpack_from("<HH", elf, 0x3A)
    sections = []
    for i in range(e_shnum):
        _, sh_type, _, sh_addr, sh_offset, sh_size, sh_link, _, _, sh_entsize = struct.unpack_from(
            "<IIQQQQIIQQ", elf, e_shoff + i * e_shentsize)
        sections.append((sh_type, sh_addr, sh_offset, sh_size, sh_link, sh_entsize))
    symbols = {}
    for sh_type, _, sh_offset, sh_size, sh_link, sh_entsize in sections:
        if sh_type != 2:  # SHT_SYMTAB
            continue
        str_off = sections[sh_link][2]
        for j in range(sh_size // sh_entsize):
            st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", elf, sh_offset + j * sh_entsize)
            if st_shndx == 0 or st_shndx >= len(sections) or st_size == 0:
                continue
            end = elf.index(b"\0", str_off + st_name)
            name = elf[str_off + st_name:end].decode()
            sec_type, sec_addr, sec_off, _, _, _ = sections[st_shndx]
            data = None if sec_type == 8 else elf[sec_off + st_value - sec_addr:sec_off + st_value - sec_addr + st_size]  # 8: NOBITS
            symbols[name] = (st_info & 0xF, data)
    return symbols


def kernels_of(elf):
    """{kernel name: (code bytes, descriptor bytes)}: every NAME.kd descriptor with its function NAME."""
    symbols = elf_symbols(elf)
    kernels = {}
    for name, (kind, data) in symbols.items():
        if not name.endswith(".kd") or kind != STT_OBJECT or data is None or len(data) != KD_BYTES:
            continue
        func = symbols.get(name[:-3])
        if func is None or func[0] != STT_FUNC:
            raise SystemExit(f"descriptor {name} has no function symbol")
        kernels[name[:-3]] = (func[1], data)
    return kernels


def descriptor_key(kd):
    return kd[:KD_ENTRY_OFFSET.start] + kd[KD_ENTRY_OFFSET.stop:]


def compare(a_path, b_path):
    with tempfile.TemporaryDirectory() as work:
        a, b = extract_code_object(a_path, work, "a"), extract_code_object(b_path, work, "b")
    ka, kb = kernels_of(a), kernels_of(b)
    common = sorted(set(ka) & set(kb))
    report = {
        "a": {"path": a_path, "sha256": hashlib.sha256(a).hexdigest(), "bytes": len(a), "kernels": len(ka)},
        "b": {"path": b_path, "sha256": hashlib.sha256(b).hexdigest(), "bytes": len(b), "kernels": len(kb)},
        "only_in_a": sorted(set(ka) - set(kb)),
        "only_in_b": sorted(set(kb) - set(ka)),
        "code_differs": [k for k in common if ka[k][0] != kb[k][0]],
        "descriptor_differs": [k for k in common if descriptor_key(ka[k][1]) != descriptor_key(kb[k][1])],
        "order_differs": list(ka) != list(kb),
    }
    report["identical"] = report["a"]["sha256"] == report["b"]["sha256"]
    report["kernels_identical"] = not (report["only_in_a"] or report["only_in_b"] or report["code_differs"] or report["descriptor_differs"])
    return report


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--json", help="also write the report to this file")
    args = ap.parse_args()
    r = compare(args.a, args.b)
    for side in ("a", "b"):
        print(f"{r[side]['sha256']}  {r[side]['kernels']:4d} kernels  {r[side]['bytes']:9d} bytes  {r[side]['path']}")
    if r["identical"]:
        print("code objects identical")
    else:
        for title, key in (("only in A", "only_in_a"), ("only in B", "only_in_b"), ("code differs", "code_differs"),
                           ("descriptor differs", "descriptor_differs")):
            print(f"{title}: {len(r[key])}")
            for name in r[key]:
                print(f"  {name}")
        if r["kernels_identical"]:
            print("code objects differ, every kernel's code and descriptor equal" + (" (kernel order differs)" if r["order_differs"] else ""))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(r, f, indent=1)
    return 0 if r["identical"] else 2 if r["kernels_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
