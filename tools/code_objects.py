#!/usr/bin/env python3
"""Kernel resource figures straight from a BUILT library (CPU only): every gfx950 code object embedded in the .so's
`.hip_fatbin` section is unbundled and its AMDGPU metadata note read with llvm-readelf.

  python tools/code_objects.py [path/to/libcpmppi.so] [name-substring]
  python tools/code_objects.py --diff a.so b.so     same device code?  one line per code object for its .text bytes, every
                                                    difference of the kernels() tables; exit status 1 on any difference
  python tools/code_objects.py --diff --by-name a.so b.so   the same question kernel by kernel, whatever unit a kernel sits in
                                                    (after a unit was split or merged): the bytes of every kernel symbol's own
                                                    code and its table without `unit`, the kernels only one side has; also what
                                                    --diff does by itself when the two libraries differ in their number of units

`kernels(path)` -> list of dicts {name, vgpr_count, agpr_count, sgpr_count, sgpr_spill_count, vgpr_spill_count,
private_segment_fixed_size (scratch bytes per lane), group_segment_fixed_size (static LDS), unit (index of the code object)}.
Used by tests/test_abi_and_host.py to keep scratch out of the rollout kernels (round 1 lost 4-15 % to a 28-byte slot)."""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
INT_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
            "group_segment_fixed_size", "kernarg_segment_size")


def code_objects(so_path, target="gfx950"):
    """The device ELF images for `target` inside so_path's .hip_fatbin (one per translation unit)."""
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", so_path,
                        os.path.join(tmp, "discard.so")], check=True)
        data = open(fat, "rb").read()
    out, pos = [], 0
    while True:
        i = data.find(MAGIC, pos)
        if i < 0:
            return out
        n = struct.unpack_from("<Q", data, i + len(MAGIC))[0]
        off = i + len(MAGIC) + 8
        for _ in range(n):
            o, size, tl = struct.unpack_from("<QQQ", data, off)
            off += 24
            triple = data[off:off + tl].decode()
            off += tl
            if target in triple and size:
                out.append(data[i + o:i + o + size])
        pos = i + 1


def kernels(so_path, target="gfx950"):
    res = []
    for unit, elf in enumerate(code_objects(so_path, target)):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(elf)
            f.flush()
            txt = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", f.name], check=True,
                                 capture_output=True, text=True).stdout
        if "amdhsa.kernels:" not in txt:
            continue
        for blk in re.split(r"\n  - \.agpr_count:", txt[txt.index("amdhsa.kernels:"):])[1:]:
            blk = ".agpr_count:" + blk
            k = {"unit": unit, "name": re.search(r"\.name:\s+(\S+)", blk).group(1)}
            for key in INT_KEYS:
                m = re.search(r"\." + key + r":\s+(\d+)", blk)
                k[key] = int(m.group(1)) if m else None
            res.append(k)
    return res


def section(elf, name=".text"):
    """The bytes of section `name` of a device ELF image (whole images differ by the build paths they record)."""
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "in.elf"), os.path.join(tmp, "section.bin")
        open(src, "wb").write(elf)
        subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), "--dump-section", f"{name}={out}", src,
                        os.path.join(tmp, "discard.elf")], check=True)
        return open(out, "rb").read()


def diff(so_a, so_b, sections=(".text",)):
    """Compare two libraries' gfx950 code objects section by section and kernel by kernel; the number of differences."""
    objs_a, objs_b = code_objects(so_a), code_objects(so_b)
    bad = int(len(objs_a) != len(objs_b))
    print(f"code objects: {len(objs_a)} / {len(objs_b)}")
    for unit, (ea, eb) in enumerate(zip(objs_a, objs_b)):
        for name in sections:
            sa, sb = section(ea, name), section(eb, name)
            bad += sa != sb
            print(f"u{unit} {name}: {'identical' if sa == sb else 'DIFFERENT'} ({len(sa)} / {len(sb)} bytes)")
    ka, kb = ({(k["unit"], k["name"]): k for k in kernels(so)} for so in (so_a, so_b))
    for key in sorted(set(ka) | set(kb)):
        if ka.get(key) != kb.get(key):
            bad += 1
            print(f"u{key[0]} {key[1]}: {ka.get(key)} / {kb.get(key)}")
    print(f"kernels: {len(ka)} / {len(kb)}; {'no difference' if not bad else str(bad) + ' differences'}")
    return bad


def kernel_code(so_path):
    """{(kernel name, occurrence): the bytes of the kernel symbol's own range in .text}.  Units that instantiate the same template
    in an anonymous namespace hold kernels of one name: they are numbered in unit order, as kernels_by_name numbers them."""
    res, seen = {}, {}
    for elf in code_objects(so_path):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(elf)
            f.flush()
            txt = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "-S", "-s", "-W", f.name], check=True,
                                 capture_output=True, text=True).stdout
        m = re.search(r"\] \.text\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)", txt)
        if not m:
            continue
        addr, off, size = (int(x, 16) for x in m.groups())
        kds = set(re.findall(r"\s(\S+)\.kd$", txt, re.M))
        funcs = {}                          # (.dynsym and .symtab list a kernel twice)
        for value, n, name in re.findall(r"^\s*\d+: ([0-9a-f]+)\s+(\d+) FUNC\s+\S+\s+\S+\s+\d+ (\S+)$", txt, re.M):
            if name in kds:
                funcs[name] = (int(value, 16), int(n))
        for name, (value, n) in sorted(funcs.items(), key=lambda kv: kv[1]):
            assert addr <= value and value + n <= addr + size, name
            i = seen[name] = seen.get(name, -1) + 1
            res[(name, i)] = elf[off + value - addr:off + value - addr + n]
    return res


def kernels_by_name(so_path):
    """kernels() keyed by (name, occurrence in unit order), without the `unit` field."""
    res, seen = {}, {}
    for k in kernels(so_path):
        i = seen[k["name"]] = seen.get(k["name"], -1) + 1
        res[(k["name"], i)] = {key: v for key, v in k.items() if key != "unit"}
    return res


def diff_by_name(so_a, so_b):
    """Compare two libraries kernel by kernel, whichever code object holds a kernel; the number of differences."""
    ca, cb, ka, kb = kernel_code(so_a), kernel_code(so_b), kernels_by_name(so_a), kernels_by_name(so_b)
    bad = same = 0
    ta, tb = ([section(e) for e in code_objects(so)] for so in (so_a, so_b))
    print(f"code objects: {len(ta)} / {len(tb)}; .text of {sum(t in tb for t in ta)} of the first's found byte for byte in the second")
    for key in sorted(set(ka) | set(kb)):
        tag = key[0] + (f" #{key[1]}" if key[1] else "")
        if key not in ka or key not in kb:
            bad += 1
            print(f"{tag}: only in {'the first' if key in ka else 'the second'}")
        elif ca.get(key) is None or cb.get(key) is None:
            bad += 1
            print(f"{tag}: no function symbol")
        elif ca[key] != cb[key] or ka[key] != kb[key]:
            bad += 1
            print(f"{tag}: code {'identical' if ca[key] == cb[key] else 'DIFFERENT'} ({len(ca[key])} / {len(cb[key])} bytes)"
                  + ("" if ka[key] == kb[key] else f"; {ka[key]} / {kb[key]}"))
        else:
            same += 1
    print(f"kernels by name: {len(ka)} / {len(kb)}, {same} identical; {'no difference' if not bad else str(bad) + ' differences'}")
    return bad


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1:3] == ["--diff", "--by-name"]:
        sys.exit(1 if diff_by_name(sys.argv[3], sys.argv[4]) else 0)
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        if len(code_objects(sys.argv[2])) != len(code_objects(sys.argv[3])):
            sys.exit(1 if diff_by_name(sys.argv[2], sys.argv[3]) else 0)
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] else os.path.join(ROOT, "cartpolesimulation_amd", "libcpmppi.so")
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    for k in kernels(path):
        if flt in k["name"]:
            print(f"u{k['unit']} {k['name'][:100]:100s} vgpr {k['vgpr_count']:>3} agpr {k['agpr_count']:>3} sgpr {k['sgpr_count']:>3} "
                  f"sgpr_spill {k['sgpr_spill_count']:>3} vgpr_spill {k['vgpr_spill_count']:>2} "
                  f"scratch {k['private_segment_fixed_size']:>3} lds {k['group_segment_fixed_size']:>6}")
