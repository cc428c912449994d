#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of the library, kernel by kernel: machine-code bytes and code-object metadata.

    python tools/compare_kernel_code.py PARENT_BUILD_DIR CHANGE_BUILD_DIR --parent-units spc_select --units spc_select \
        spc_sigma_clip spc_select_global [--title TEXT] > profiles/NAME.txt

Each build directory holds the object files the Makefile leaves in csrc/build/ (UNIT.o).  CPU only: an object file is read as
an ELF file, its .hip_fatbin section as a clang offload bundle, the gfx950 entry of the bundle as the device ELF file; a
kernel's machine code is the bytes of its function symbol in .text, its resources are the entries of the NT_AMDGPU_METADATA
note (.vgpr_count, .agpr_count, .sgpr_count, .private_segment_fixed_size, .group_segment_fixed_size, spill counts).  Nothing
is disassembled.  Kernels are matched by demangled name over ALL units of a side, so a kernel that moved to another unit is
still "present in both".  Exit status 1 when a kernel was added, removed, or differs and is worse in a column.

The layout is that of profiles/retired_switches_resources.txt: "a>b" is parent a, this change b; one number: unchanged."""
import argparse
import os
import struct
import subprocess
import sys

COLS = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"),
        ("lds", ".group_segment_fixed_size"), ("vspill", ".vgpr_spill_count"), ("sspill", ".sgpr_spill_count"))
WIDTHS = {"vgpr": 10, "agpr": 8, "sgpr": 10, "scratch": 10, "lds": 14, "vspill": 10, "sspill": 10, "occ": 6, "bytes": 0}


def elf_sections(data):
    """{name: (offset, size, type)} and the symbol table [(name, value, size, type, shndx)] of a little-endian ELF64 file"""
    assert data[:4] == b"\x7fELF" and data[4] == 2 and data[5] == 1, "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    raw = []
    for i in range(shnum):
        name, typ, _flags, addr, off, size, link, _info, _align, entsize = struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize)
        raw.append((name, typ, addr, off, size, link, entsize))
    strtab = raw[shstrndx]

    def cstr(table_off, at):
        end = data.index(b"\0", table_off + at)
        return data[table_off + at:end].decode()

    sections, by_index, symbols = {}, [], []
    for name, typ, addr, off, size, link, entsize in raw:
        sections[cstr(strtab[3], name)] = (off, size, typ, addr)
        by_index.append((off, size, typ, addr))
    for name, typ, addr, off, size, link, entsize in raw:
        if typ != 2:                                            # SHT_SYMTAB
            continue
        stroff = raw[link][3]
        for i in range(size // entsize):
            st_name, info, _other, shndx, value, ssize = struct.unpack_from("<IBBHQQ", data, off + i * entsize)
            symbols.append((cstr(stroff, st_name), value, ssize, info & 15, shndx))
    return sections, by_index, symbols


def device_elf(obj):
    """the gfx950 code object inside a host object file"""
    data = open(obj, "rb").read()
    sections, _, _ = elf_sections(data)
    off, size = sections[".hip_fatbin"][:2]
    fat = data[off:off + size]
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    assert fat[:len(magic)] == magic, "%s: .hip_fatbin is not an uncompressed clang offload bundle" % obj
    n, = struct.unpack_from("<Q", fat, len(magic))
    at = len(magic) + 8
    for _ in range(n):
        eoff, esize, tlen = struct.unpack_from("<QQQ", fat, at)
        triple = fat[at + 24:at + 24 + tlen].decode()
        at += 24 + tlen
        if "amdgcn" in triple and triple.endswith("gfx950"):
            return fat[eoff:eoff + esize]
    raise SystemExit("%s: no gfx950 entry in the offload bundle" % obj)


def msgpack(data, at=0):
    """(value, next offset): the subset of MessagePack the AMDGPU metadata uses"""
    b = data[at]
    if b <= 0x7F:
        return b, at + 1
    if 0x80 <= b <= 0x8F or b in (0xDE, 0xDF):
        n, at = (b & 15, at + 1) if b <= 0x8F else ((struct.unpack_from(">H", data, at + 1)[0], at + 3) if b == 0xDE else (struct.unpack_from(">I", data, at + 1)[0], at + 5))
        out = {}
        for _ in range(n):
            k, at = msgpack(data, at)
            out[k], at = msgpack(data, at)
        return out, at
    if 0x90 <= b <= 0x9F or b in (0xDC, 0xDD):
        n, at = (b & 15, at + 1) if b <= 0x9F else ((struct.unpack_from(">H", data, at + 1)[0], at + 3) if b == 0xDC else (struct.unpack_from(">I", data, at + 1)[0], at + 5))
        out = []
        for _ in range(n):
            v, at = msgpack(data, at)
            out.append(v)
        return out, at
    if 0xA0 <= b <= 0xBF or b in (0xD9, 0xDA, 0xDB):
        n, at = (b & 31, at + 1) if b <= 0xBF else ((data[at + 1], at + 2) if b == 0xD9 else ((struct.unpack_from(">H", data, at + 1)[0], at + 3) if b == 0xDA else (struct.unpack_from(">I", data, at + 1)[0], at + 5)))
        return data[at:at + n].decode(), at + n
    if b >= 0xE0:
        return b - 256, at + 1
    fixed = {0xC0: (None, 0), 0xC2: (False, 0), 0xC3: (True, 0)}
    if b in fixed:
        return fixed[b][0], at + 1
    nums = {0xCC: ">B", 0xCD: ">H", 0xCE: ">I", 0xCF: ">Q", 0xD0: ">b", 0xD1: ">h", 0xD2: ">i", 0xD3: ">q", 0xCA: ">f", 0xCB: ">d"}
    if b in nums:
        return struct.unpack_from(nums[b], data, at + 1)[0], at + 1 + struct.calcsize(nums[b])
    raise ValueError("MessagePack type 0x%02x" % b)


def kernels_of(obj):
    """{mangled kernel name: (machine-code bytes, metadata dict)} of one object file"""
    dev = device_elf(obj)
    sections, by_index, symbols = elf_sections(dev)
    meta = {}
    for name, (off, size, typ, _addr) in sections.items():
        if typ != 7:                                            # SHT_NOTE
            continue
        at = off
        while at < off + size:
            namesz, descsz, ntype = struct.unpack_from("<III", dev, at)
            desc_at = at + 12 + (namesz + 3) // 4 * 4
            if ntype == 32 and dev[at + 12:at + 12 + namesz].rstrip(b"\0") == b"AMDGPU":
                for k in msgpack(dev, desc_at)[0].get("amdhsa.kernels", []):
                    meta[k[".name"]] = k
            at = desc_at + (descsz + 3) // 4 * 4
    out = {}
    for name, value, size, typ, shndx in symbols:
        if typ == 2 and name in meta:                           # STT_FUNC with a kernel descriptor
            soff, _ssize, _styp, saddr = by_index[shndx]
            out[name] = (dev[soff + value - saddr:soff + value - saddr + size], meta[name])
    assert set(out) == set(meta), "kernels without a function symbol: %s" % sorted(set(meta) - set(out))
    return out


def demangle(names):
    if not names:
        return {}
    text = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, text.splitlines()))


def short(name):
    """the demangled name without its namespace and argument list"""
    name = name.replace("(anonymous namespace)::", "")
    if name.startswith("void "):                               # (a template kernel's name carries its return type)
        name = name[5:]
    depth = 0
    for i, c in enumerate(name):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            return name[:i]
    return name


def occupancy(m):
    """waves per SIMD the unified register file allows"""
    v = (m[".vgpr_count"] + 3) // 4 * 4 + m.get(".agpr_count", 0)
    return min(8, 512 // max(8, (v + 7) // 8 * 8))


def side(build_dir, units):
    found = {}
    for unit in units:
        ks = kernels_of(os.path.join(build_dir, unit + ".o"))
        names = demangle(sorted(ks))
        for mangled, (code, meta) in ks.items():
            assert names[mangled] not in found, "kernel in two units: %s" % names[mangled]
            found[names[mangled]] = (unit, code, meta)
    return found


def cell(a, b):
    return str(a) if a == b else "%s>%s" % (a, b)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent_build")
    ap.add_argument("change_build")
    ap.add_argument("--parent-units", nargs="+", required=True, help="object files of the parent (without .o)")
    ap.add_argument("--units", nargs="+", required=True, help="object files of the change (without .o)")
    ap.add_argument("--title", default="")
    args = ap.parse_args()
    old, new = side(args.parent_build, args.parent_units), side(args.change_build, args.units)
    both = sorted(set(old) & set(new))
    same = [k for k in both if old[k][1] == new[k][1]]
    differ = [k for k in both if old[k][1] != new[k][1]]
    added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
    meta_moved = [k for k in same if any(old[k][2].get(f, 0) != new[k][2].get(f, 0) for _, f in COLS)]
    worse = []
    print("# Kernel resources, parent commit against this change: gfx950 code objects cross-compiled from both trees (hipcc -O3, the")
    print("# Makefile's flags), one row per kernel; every figure from the code object's metadata (.vgpr_count, .agpr_count, .sgpr_count,")
    print("# .private_segment_fixed_size = scratch bytes per lane, .group_segment_fixed_size = static LDS bytes, spill counts) and the size")
    print("# of the kernel's machine code.  occ = waves per SIMD the unified register file allows: min(8, 512 / roundup8(roundup4(vgpr) + agpr)).")
    print("# \"a>b\": parent a, this change b; a single number: unchanged.  Written by tools/compare_kernel_code.py.")
    if args.title:
        print("#\n# " + args.title)
    print()
    print("parent units: %s" % ", ".join("%s.hip (%d kernels)" % (u, sum(1 for v in old.values() if v[0] == u)) for u in args.parent_units))
    print("change units: %s" % ", ".join("%s.hip (%d kernels)" % (u, sum(1 for v in new.values() if v[0] == u)) for u in args.units))
    print()
    print("kernels in the code objects: parent %d, this change %d" % (len(old), len(new)))
    print("present in both and machine code byte-identical: %d (of them with a metadata column that moved: %d)" % (len(same), len(meta_moved)))
    print("present in both, machine code differs: %d" % len(differ))
    print("added: %d" % len(added))
    for k in added:
        print("  " + k)
    print("removed: %d" % len(removed))
    for k in removed:
        print("  " + k)
    families = {}
    for k in both:
        families.setdefault((new[k][0], short(k).split("<")[0]), []).append(k)
    print("\nkernel family                     unit                      kernels  byte-identical  code bytes (sum)")
    for (unit, fam), ks in sorted(families.items()):
        print("%-33s %-25s %-8d %-15d %d" % (fam, unit + ".hip", len(ks), sum(1 for k in ks if k in same), sum(len(new[k][1]) for k in ks)))
    listed = differ + [k for k in meta_moved if k not in differ]
    if listed:
        print("\nKernels whose machine code or metadata differs.")
        header = "%-66s " % "kernel" + "".join(("%-" + str(WIDTHS[c]) + "s") % c for c in WIDTHS)
        for unit in args.units:
            rows = [k for k in listed if new[k][0] == unit]
            if not rows:
                continue
            print("\n### %s.hip\n%s" % (unit, header))
            for k in rows:
                mo, mn = old[k][2], new[k][2]
                vals = [(mo.get(f, 0), mn.get(f, 0)) for _, f in COLS]
                occ = (occupancy(mo), occupancy(mn))
                size = (len(old[k][1]), len(new[k][1]))
                if any(b > a for a, b in vals) or occ[1] < occ[0] or size[1] > size[0]:
                    worse.append(k)
                cells = [cell(a, b) for a, b in vals] + [cell(*occ), cell(*size)]
                print("%-66s " % short(k) + "".join(("%-" + str(WIDTHS[c]) + "s") % v for c, v in zip(WIDTHS, cells)).rstrip())
        print("\nworse in some column: %d" % len(worse))
        for k in worse:
            print("  " + short(k))
    return 1 if (added or removed or worse) else 0


if __name__ == "__main__":
    sys.exit(main())
