#!/usr/bin/env python3
"""Kernel identity of two builds of csrc/: a plain diff, CPU only, runs no kernel.

    tools/kernel_identity.py PARENT_CSRC NEW_CSRC [--arch gfx950] [--llvm /opt/rocm/llvm/bin] [--rename OLD=NEW ...]

Both directories hold the *.o files of a `make` of csrc/.  The gfx950 code object of every object file is unbundled, every
kernel is keyed by its mangled name across the WHOLE library (kernels may move between object files), and for each name the
two builds are compared in
  - the `llvm-objdump -d` instruction text and encodings (addresses dropped: a kernel may sit elsewhere in its object), and
  - .vgpr_count, .sgpr_count, .agpr_count, .private_segment_fixed_size, .group_segment_fixed_size, .kernarg_segment_size
    of the `llvm-readelf --notes` metadata.
Device functions (code symbols without a kernel descriptor) are listed and compared the same way.  A kernel found in more than
one object file of a build (a template kernel launched from two sources is compiled twice) is counted and named for each build.
--rename OLD=NEW (repeatable) reads the parent's source name OLD as NEW in every mangled name, so that a kernel whose parameter
type was renamed is compared with its successor and not listed as removed and added.
Exit status 0 when the kernel names are the same set, every kernel is identical and no kernel of the new build sits in more than
one object file, 1 otherwise.
"""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
          ".kernarg_segment_size")


def run(cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, arch, llvm, tmp):
    """The unbundled device code object of a host object file, or None when it carries no device code."""
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    r = subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.devnull],
                       capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
         "--targets=hipv4-amdgcn-amd-amdhsa--" + arch, "--output=" + co])
    return co if os.path.getsize(co) > 0 else None


SYM = re.compile(r"^([0-9a-f]+) <(.+)>:$")
INS = re.compile(r"^\s+(.*?)\s*// ([0-9A-F]+): ([0-9A-F ]+?)(?: (<.+>))?\s*$")


def disassembly(co, llvm):
    """{symbol: [instruction text | encoding | symbol-relative branch target]}, each symbol cut at its size: the padding
    that follows the last function of a code object belongs to none"""
    size = {}
    for line in run([os.path.join(llvm, "llvm-readelf"), "-sW", co]).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
    out, cur, end = {}, None, 0
    for line in run([os.path.join(llvm, "llvm-objdump"), "-d", co]).splitlines():
        m = SYM.match(line)
        if m:
            cur = out.setdefault(m.group(2), [])
            end = int(m.group(1), 16) + size.get(m.group(2), 1 << 62)
            continue
        m = INS.match(line)
        if m and cur is not None and int(m.group(2), 16) < end:
            cur.append("%s | %s%s" % (m.group(1), m.group(3), " " + m.group(4) if m.group(4) else ""))
    return out


def metadata(co, llvm):
    """{kernel name: {field: value}} from the AMDGPU metadata note"""
    out, cur = {}, None
    for line in run([os.path.join(llvm, "llvm-readelf"), "--notes", co]).splitlines():
        if line.startswith("  - "):
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"^    (\.[a-z_]+):\s+(\S+)\s*$", line)
        if m and cur is not None:
            if m.group(1) == ".name":
                out[m.group(2)] = cur
            cur[m.group(1)] = m.group(2)
    return out


def renamer(pairs):
    """OLD=NEW options -> a function on text: every mangled source name <len>OLD becomes <len>NEW (type, function and kernel
    names alike; substitutions inside a mangled name keep their positions when a name is only replaced)"""
    subs = []
    for pair in pairs:
        old, _, new = pair.partition("=")
        if not old or not new:
            sys.exit("--rename takes OLD=NEW, got %r" % pair)
        subs.append((re.compile(r"(?<![0-9])%d%s" % (len(old), re.escape(old))), "%d%s" % (len(new), new)))   # the length ends the name

    def apply(text):
        for pat, to in subs:
            text = pat.sub(to, text)
        return text
    return apply


def load(csrc, arch, llvm, rename=lambda text: text):
    """kernels {name: (object, instructions, fields)}, device functions {name: (object, instructions)}, objects without code,
    {kernel name: [objects]} of the kernels found in more than one object file.  rename: applied to every symbol name before it
    is keyed, and to the branch targets of the instruction text, which name their symbol"""
    kernels, funcs, empty, where = {}, {}, [], {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(csrc, "*.o"))):
            base = os.path.basename(obj)
            co = code_object(obj, arch, llvm, tmp)
            if co is None:
                empty.append(base)
                continue
            dis = {rename(name): [rename(line) for line in ins] for name, ins in disassembly(co, llvm).items()}
            meta = {rename(name): fields for name, fields in metadata(co, llvm).items()}
            for name, ins in dis.items():
                if name in meta:
                    if name in kernels and kernels[name][1:] != (ins, {f: meta[name].get(f) for f in FIELDS}):
                        sys.exit("%s: kernel %s differs between %s and %s of the same build" % (csrc, name, kernels[name][0], base))
                    kernels.setdefault(name, (base, ins, {f: meta[name].get(f) for f in FIELDS}))
                    where.setdefault(name, []).append(base)
                else:
                    funcs[name] = (base, ins)
    return kernels, funcs, empty, {n: objs for n, objs in where.items() if len(objs) > 1}


def demangle(names, llvm):
    if not names:
        return {}
    for tool in (os.path.join(llvm, "llvm-cxxfilt"), "c++filt"):     # names only: the comparison never depends on it
        try:
            out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True)
        except OSError:
            continue
        if out.returncode == 0 and len(out.stdout.splitlines()) == len(names):
            return dict(zip(names, out.stdout.splitlines()))
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--llvm", default="/opt/rocm/llvm/bin")
    ap.add_argument("--diff", type=int, default=20, help="lines of instruction diff printed per differing kernel")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="a source name (type, function) that the new build spells NEW: applied to the parent's symbol names before "
                         "they are keyed, so a kernel whose parameter type was renamed meets its successor; repeatable")
    args = ap.parse_args()
    pk, pf, pe, pdup = load(args.parent_csrc, args.arch, args.llvm, renamer(args.rename))
    nk, nf, ne, ndup = load(args.new_csrc, args.arch, args.llvm)
    dm = demangle(sorted(set(pk) | set(nk) | set(pf) | set(nf)), args.llvm)

    print("Kernel identity, parent build against new build: the %s code object of every csrc/*.o unbundled, kernels keyed by mangled"
          % args.arch)
    print("name across the whole library and compared one by one (llvm-readelf --notes metadata, llvm-objdump -d instruction text and")
    print("encodings).")
    if args.rename:
        print("source names of the parent read as the new build spells them: " + ", ".join(r.replace("=", " -> ") for r in args.rename))
    print()
    print("kernels: parent %d, new %d" % (len(pk), len(nk)))
    for title, names, src in (("removed kernels", sorted(set(pk) - set(nk)), pk), ("added kernels", sorted(set(nk) - set(pk)), nk)):
        print(title + ":" + ("" if names else " none"))
        for n in names:
            print("  %s: %s" % (src[n][0], dm.get(n, n)))
    for title, dup in (("parent", pdup), ("new", ndup)):
        print("kernels in more than one object file of the %s build: %d" % (title, len(dup)))
        for n in sorted(dup):
            print("  %s: %s" % (", ".join(dup[n]), dm.get(n, n)))
    moved = sorted(n for n in set(pk) & set(nk) if pk[n][0] != nk[n][0])
    print("kernels in another object file than in the parent: %d" % len(moved))
    routes = {}
    for n in moved:
        routes[(pk[n][0], nk[n][0])] = routes.get((pk[n][0], nk[n][0]), 0) + 1
    for (a, b), c in sorted(routes.items()):
        print("  %s -> %s: %d" % (a, b, c))

    differing = []
    for n in sorted(set(pk) & set(nk)):
        why = []
        if pk[n][1] != nk[n][1]:
            why.append("instructions (%d -> %d)" % (len(pk[n][1]), len(nk[n][1])))
        why += ["%s %s -> %s" % (f, pk[n][2][f], nk[n][2][f]) for f in FIELDS if pk[n][2][f] != nk[n][2][f]]
        if why:
            differing.append((n, why))
    print("per object file of the new build:")
    for base in sorted({v[0] for v in nk.values()} | {v[0] for v in nf.values()} | set(ne)):
        if base in ne:
            print("  %s: no device code" % base)
            continue
        mine = [n for n in nk if nk[n][0] == base]
        surv = [n for n in mine if n in pk]
        bad = [n for n, _ in differing if nk[n][0] == base]
        fn = [n for n in nf if nf[n][0] == base]
        fbad = [n for n in fn if n not in pf or pf[n][1] != nf[n][1]]
        print("  %s: %d kernels, %d of the parent's, %d of %d identical; device functions %d, not in the parent or differing %d"
              % (base, len(mine), len(surv), len(surv) - len(bad), len(surv), len(fn), len(fbad)))
    print("device functions: parent %d, new %d" % (len(pf), len(nf)))
    fbad = sorted(n for n in set(pf) | set(nf) if n not in pf or n not in nf or pf[n][1] != nf[n][1])
    for n in fbad:
        print("  %s: %s" % ("only in parent" if n not in nf else "only in new" if n not in pf else "differs", dm.get(n, n)))
    for n, why in differing:
        print("DIFFERS %s: %s [%s]" % (nk[n][0], dm.get(n, n), "; ".join(why)))
        if args.diff > 0:
            d = list(difflib.unified_diff(pk[n][1], nk[n][1], "parent", "new", lineterm="", n=1))
            for line in d[:args.diff]:
                print("    " + line)
    common = len(set(pk) & set(nk))
    print("%d of %d surviving kernels identical (instruction text and encodings, %s)"
          % (common - len(differing), common, ", ".join(FIELDS)))
    ok = not differing and set(pk) == set(nk) and not fbad and not ndup
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
