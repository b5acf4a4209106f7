#!/usr/bin/env python3
"""Per-kernel resource metadata of libishap_hip.so without a GPU: scratch bytes per lane, VGPRs, SGPRs, LDS, kernarg size.

Reads the gfx950 code objects out of the shared library's `.hip_fatbin` section (clang offload bundles, one per
translation unit) and their NT_AMDGPU_METADATA notes (msgpack).  Why it exists (round 6): removing three unused ints from
`IgemmArgs` moved {alpha, out_mode, stat_out} onto a 16-byte boundary; the compiler then kept those four dwords in a PRIVATE
copy of the argument block -- an s_load + s_waitcnt + scratch_store at kernel entry and a scratch-enabled dispatch: every
LDS-DMA convolution launch got 0.5-1.1 us slower (+3 % per edit, profiles/round6_ab_prune_scratch.txt) with no warning
anywhere.  tests/test_host_cpu.py holds the hot kernels to zero scratch with this module.

    python tools/kernel_meta.py [path/to/libishap_hip.so] [name substring]
    python tools/kernel_meta.py --diff A.so B.so      # one line per kernel whose code or metadata differs; exit status 1 if any
    python tools/kernel_meta.py --diff A.so B.so --ops    # ... and, under each, the metadata fields and the opcodes whose counts
                                                          # differ, as A -> B (llvm-objdump -d of the extracted code objects)
"""
import os
import struct
import sys

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(blob: bytes):
    """every amdgcn ELF image inside the concatenated offload bundles of `blob`"""
    pos = 0
    while True:
        b = blob.find(MAGIC, pos)
        if b < 0:
            return
        n, = struct.unpack_from("<Q", blob, b + len(MAGIC))
        p = b + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "amdgcn" in triple and size > 0:
                yield triple, blob[b + off:b + off + size]
        pos = p


def _notes(elf: bytes):
    """(name, type, desc) of every note in the ELF64 image (section headers)"""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2, "ELF64 image expected"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    for i in range(shnum):
        sh = shoff + i * shentsize
        sh_type, = struct.unpack_from("<I", elf, sh + 4)
        if sh_type != 7:                 # SHT_NOTE
            continue
        off, size = struct.unpack_from("<QQ", elf, sh + 0x18)
        p, end = off, off + size
        while p + 12 <= end:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, p)
            p += 12
            name = elf[p:p + namesz].rstrip(b"\0").decode()
            p += (namesz + 3) & ~3
            desc = elf[p:p + descsz]
            p += (descsz + 3) & ~3
            yield name, ntype, desc


def kernels(lib_path: str):
    """{kernel symbol: metadata dict} over every gfx950 code object of the library"""
    import msgpack
    blob = open(lib_path, "rb").read()
    out = {}
    for triple, elf in _code_objects(blob):
        if "gfx950" not in triple:
            continue
        for name, ntype, desc in _notes(elf):
            if name == "AMDGPU" and ntype == 32:
                md = msgpack.unpackb(desc, raw=False, strict_map_key=False)
                for k in md.get("amdhsa.kernels", []):
                    out[k[".name"]] = k
    return out


def _functions(elf: bytes):
    """{symbol: bytes of the function in its section} for every FUNC symbol of the ELF64 image"""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQII", elf, shoff + i * shentsize) for i in range(shnum)]   # name, type, flags, addr, off, size, link, info
    out = {}
    for _, sh_type, _, _, off, size, link, _ in sec:
        if sh_type != 2:                 # SHT_SYMTAB
            continue
        stroff = sec[link][4]
        for p in range(off, off + size, 24):
            st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", elf, p)
            if st_info & 15 == 2 and 0 < st_shndx < shnum:      # STT_FUNC, defined here
                name = elf[stroff + st_name:elf.index(b"\0", stroff + st_name)].decode()
                start = sec[st_shndx][4] + st_value - sec[st_shndx][3]
                out[name] = elf[start:start + st_size]
    return out


META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def kernel_code(lib_path: str):
    """{kernel symbol: [(metadata tuple, machine code bytes), ...]}: a list, since two translation units may both hold a
    kernel of one (internal-linkage) name"""
    import msgpack
    out = {}
    for triple, elf in _code_objects(open(lib_path, "rb").read()):
        if "gfx950" not in triple:
            continue
        fn = _functions(elf)
        for name, ntype, desc in _notes(elf):
            if name == "AMDGPU" and ntype == 32:
                for k in msgpack.unpackb(desc, raw=False, strict_map_key=False).get("amdhsa.kernels", []):
                    out.setdefault(k[".name"], []).append((tuple(k.get(m, 0) for m in META_KEYS), fn[k[".name"]]))
    return out


def opcodes(lib_path: str):
    """{kernel symbol: Counter of instruction mnemonics}, from llvm-objdump -d of every gfx950 code object of the library
    (two kernels of one internal-linkage name are counted together)"""
    import collections
    import re
    import subprocess
    import tempfile
    out = {}
    for triple, elf in _code_objects(open(lib_path, "rb").read()):
        if "gfx950" not in triple:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(elf)
            f.flush()
            txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", f.name],
                                 capture_output=True, text=True, check=True).stdout
        cur = None
        for line in txt.splitlines():
            m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = out.setdefault(m.group(1), collections.Counter())
            elif cur is not None and re.match(r"\s+[a-z_]", line):
                cur[line.split()[0]] += 1
    return out


def diff(lib_a: str, lib_b: str, ops: bool = False) -> int:
    a, b = kernel_code(lib_a), kernel_code(lib_b)
    oa, ob = (opcodes(lib_a), opcodes(lib_b)) if ops else ({}, {})
    dm = demangle(sorted(set(a) | set(b)))
    bad = 0
    for n in sorted(set(a) | set(b), key=lambda n: dm[n]):
        short = dm[n].split("(")[0].replace("void ", "")
        if n not in a or n not in b:
            what = f"only in {lib_b if n in b else lib_a}"
        elif len(a[n]) != len(b[n]):
            what = f"{len(a[n])} / {len(b[n])} copies"
        else:
            what = ", ".join(w for w, i in (("metadata", 0), ("code", 1)) if [x[i] for x in a[n]] != [x[i] for x in b[n]])
            if "code" in what:
                what += " (" + " / ".join(f"{len(x[1])} -> {len(y[1])} bytes" for x, y in zip(a[n], b[n]) if x[1] != y[1]) + ")"
        if what:
            bad += 1
            print(f"DIFF {short}: {what}")
            if "metadata" in what:
                for x, y in zip(a[n], b[n]):
                    print("    " + ", ".join(f"{m[1:]} {p} -> {q}" for m, p, q in zip(META_KEYS, x[0], y[0]) if p != q))
            if ops and "code" in what:
                ca, cb = oa.get(n, {}), ob.get(n, {})
                for op in sorted(set(ca) | set(cb)):
                    if ca.get(op, 0) != cb.get(op, 0):
                        print(f"    {op:28s} {ca.get(op, 0)} -> {cb.get(op, 0)}")
    na, nb = sum(map(len, a.values())), sum(map(len, b.values()))
    print(f"{na} kernels, {sum(len(c) for v in a.values() for _, c in v)} bytes of kernel code in {lib_a}")
    print(f"{nb} kernels, {sum(len(c) for v in b.values() for _, c in v)} bytes of kernel code in {lib_b}")
    print(f"{bad} kernels differ (compared: the bytes of each kernel's function in .text and its metadata entry: {', '.join(m[1:] for m in META_KEYS)})")
    return 1 if bad else 0


def demangle(names):
    import subprocess
    try:
        r = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    if len(sys.argv) in (4, 5) and sys.argv[1] == "--diff" and sys.argv[4:] in ([], ["--ops"]):
        sys.exit(diff(sys.argv[2], sys.argv[3], ops=len(sys.argv) == 5))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = sys.argv[1] if len(sys.argv) > 1 and os.path.exists(sys.argv[1]) else os.path.join(root, "ishapediting_amd", "libishap_hip.so")
    pat = sys.argv[-1] if len(sys.argv) > 1 and not os.path.exists(sys.argv[-1]) else ""
    ks = kernels(lib)
    dm = demangle(sorted(ks))
    print(f"{len(ks)} kernels in {lib} ({os.path.getsize(lib)} bytes)")
    print(f"{'scratch':>8s} {'vgpr':>5s} {'agpr':>5s} {'sgpr':>5s} {'lds':>7s} {'kernarg':>8s}  kernel")
    for n in sorted(ks, key=lambda n: dm[n]):
        k = ks[n]
        short = dm[n].split("(")[0].replace("void ", "")
        if pat in short:
            print(f"{k.get('.private_segment_fixed_size', 0):8d} {k.get('.vgpr_count', 0):5d} {k.get('.agpr_count', 0):5d} {k.get('.sgpr_count', 0):5d} "
                  f"{k.get('.group_segment_fixed_size', 0):7d} {k.get('.kernarg_segment_size', 0):8d}  {short}")


if __name__ == "__main__":
    main()
