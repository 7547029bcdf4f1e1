"""Diff the gfx950 machine code of two builds, kernel by kernel.  No GPU needed.

    python scripts/isa_diff.py <parent> <new>

Each argument is a directory of object files (csrc/build of a tree) or a libcrab_hip.so.  The gfx950 code objects are taken out of the offload
bundles in .hip_fatbin and disassembled with llvm-objdump of the ROCm tree (ROCM_PATH, default /opt/rocm).  Per function symbol: comments (the
addresses and encodings objdump appends) are stripped and local block labels renumbered in order of appearance, a line with the kernel's
resources (LDS, scratch, register counts of its metadata note) is put in front, and the two listings are compared as text.  Printed per kernel:
identical | DIFFERS (first lines of a unified diff, and the per-mnemonic instruction counts that are not equal) | ONLY IN one side.
Exit status 0 iff every kernel is identical.

This is the first check for a change that moves pinned kernel code (a shared header, a template parameter): identical machine code means
identical bits and identical speed, and nothing has to be run.  What differs goes to scripts/ab_bits.py on a GPU."""
import collections
import difflib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
RES_KEYS = (".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count",
            ".sgpr_spill_count")


def _tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def _code_objects(path, tmp):
    """The gfx950 code objects of one host object or shared library (one per translation unit), as files under tmp."""
    fat = os.path.join(tmp, "fatbin")
    if os.path.exists(fat):
        os.remove(fat)
    r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", path, os.path.join(tmp, "copy")],
                       capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(fat):
        if "hip_fatbin" in r.stderr:
            return                                                  # a host-only object: no such section
        sys.exit(f"isa_diff: {path}: {r.stderr.strip()}")
    blob = open(fat, "rb").read()
    at = blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", blob, p)
            ident = blob[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in ident and size:
                co = os.path.join(tmp, f"co{len(os.listdir(tmp))}")
                with open(co, "wb") as f:
                    f.write(blob[at + off:at + off + size])
                yield co
        at = blob.find(MAGIC, at + len(MAGIC))


def _resources(co):
    """{kernel: 'lds=... scratch=...'} from the metadata note (kernel-level keys sit at an indent of four)."""
    out, cur = {}, {}
    for line in _tool("llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"^(?:  - |    )(\.\w+):\s+(\S+)$", line)
        if not m:
            continue
        if line.startswith("  - ") and cur:
            out[cur.get(".name")] = cur
            cur = {}
        cur[m.group(1)] = m.group(2)
    if cur:
        out[cur.get(".name")] = cur
    return {k: ".resources " + " ".join(f"{r[1:]}={v.get(r)}" for r in RES_KEYS) for k, v in out.items()}


def _listing(co):
    """{symbol: [normalised lines]} of one code object."""
    res = _resources(co)
    syms, name = {}, None
    for line in _tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            name = m.group(1)
            syms[name] = [res[name]] if name in res else []
            continue
        line = line.split("//")[0].split(";")[0].strip()
        if name is None or not line:
            continue
        syms[name].append(line)
    for lines in syms.values():                                     # local labels (.LBBn_m of an assembly listing, <Ln> of a symbolised one): by order
        seen = {}
        for i, line in enumerate(lines):
            lines[i] = re.sub(r"\.LBB\d+_\d+|<L\d+>", lambda m: seen.setdefault(m.group(0), f"L{len(seen)}"), line)
        while lines and lines[-1].startswith("s_nop"):              # padding between functions
            lines.pop()
    return syms


def load(arg):
    """{symbol: [listing, ...]} of a build: a symbol of an anonymous namespace may exist in more than one translation unit, in file order."""
    files = sorted(os.path.join(arg, f) for f in os.listdir(arg) if f.endswith(".o")) if os.path.isdir(arg) else [arg]
    if not files:
        sys.exit(f"isa_diff: no object files in {arg}")
    out = collections.defaultdict(list)
    with tempfile.TemporaryDirectory() as tmp:
        for f in files:
            for co in _code_objects(f, tmp):
                for sym, lines in _listing(co).items():
                    out[sym].append(lines)
    return out


def _counts(lines):
    return collections.Counter(l.split()[0] for l in lines if not l.startswith("."))


def _short(sym):
    """kernel<128, 8> for the usual mangled form (a name in the anonymous namespace, integer template arguments); the symbol as it is otherwise."""
    m = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", sym)
    if not m:
        return sym
    at = m.end() + int(m.group(1))
    t = re.match(r"I((?:L[ibjlm]\d+E)+)E", sym[at:])
    return sym[m.end():at] + ("<" + ", ".join(re.findall(r"L[ibjlm](\d+)E", t.group(1))) + ">" if t else "")


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    a, b = load(sys.argv[1]), load(sys.argv[2])
    same = differ = only = 0
    for sym in sorted(set(a) | set(b)):
        short = _short(sym)
        la, lb = a.get(sym, []), b.get(sym, [])
        if len(la) != len(lb):
            only += 1
            print(f"ONLY IN {'parent' if len(la) > len(lb) else 'new'}: {short}")
            continue
        for x, y in zip(la, lb):
            if x == y:
                same += 1
                print(f"identical: {short} ({len(x)} lines)")
                continue
            differ += 1
            d = [l for l in difflib.unified_diff(x, y, "parent", "new", lineterm="", n=1)]
            changed = sum(1 for l in d if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            print(f"DIFFERS: {short} ({len(x)} -> {len(y)} lines, {changed} diff lines)")
            for l in d[:40]:
                print("    " + l)
            ca, cb = _counts(x), _counts(y)
            delta = {k: (ca[k], cb[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]}
            print(f"    instructions {sum(ca.values())} -> {sum(cb.values())}; mnemonic counts that differ: " +
                  (", ".join(f"{k} {u}->{v}" for k, (u, v) in delta.items()) or "none"))
    print(f"{same} identical, {differ} differ, {only} only in one side")
    return 0 if differ == 0 and only == 0 and same > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
