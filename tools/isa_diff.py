#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel.  CPU only: runs hipcc, never opens a GPU.

    tools/isa_diff.py OLD NEW

OLD and NEW are each either a source tree (every .hip file of recnn_amd/csrc/Makefile's SRCS is compiled to device assembly with
the Makefile's CXXFLAGS) or a directory of .s files made that way.  For a refactor that must not change a kernel, OLD is a
checkout of the parent (`git worktree add` / `git archive`), NEW the working tree.

Per function symbol (kernels and any device function left out of line) it compares
  * the instruction stream, and
  * the kernel's .amdhsa_* block (VGPRs, SGPRs, scratch, LDS, every other descriptor field),
ignoring only what cannot matter: comments, .file / .ident / .loc / .cfi directives, the order of the symbols in the file and
the names of local labels (.LBB7_3 is renamed by order of first appearance inside its function).
One line per symbol, with one of three verdicts:
  identical   the same instruction stream and the same .amdhsa_* block;
  equivalent  the same .amdhsa_* block and the same count of every instruction mnemonic, in another order or in other registers:
              what moving code into a shared inline function typically gives;
  DIFFERENT   anything else.
Exit status 1 if any symbol is DIFFERENT or exists on one side only.

A kernel whose symbol changes (a template parameter dropped, say) is paired by hand: compile both sides to directories of .s
files, rename the old symbol in a copy, and compare the directories.
"""
import collections
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("recnn_amd", "csrc")
DROP = re.compile(r"^\s*\.(file|ident|loc|cfi_\w+|addrsig|addrsig_sym)\b")
LOCAL = re.compile(r"\.L[\w$.]+")
REPORT = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def makefile_vars(tree):
    """SRCS and CXXFLAGS of the csrc Makefile, $(ARCH) expanded."""
    srcs, flags, arch = [], [], "gfx950"
    for line in open(os.path.join(tree, CSRC, "Makefile")):
        m = re.match(r"^(\w+)\s*(\?=|\+=|=)\s*(.*)$", line.rstrip("\n"))
        if not m:
            continue
        name, _, val = m.groups()
        if name == "ARCH":
            arch = val.strip()
        elif name == "SRCS":
            srcs += val.split()
        elif name == "CXXFLAGS":
            flags += val.split()
    return srcs, [f.replace("$(ARCH)", arch) for f in flags]


def compile_tree(tree, out):
    srcs, flags = makefile_vars(tree)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def one(src):
        dst = os.path.join(out, src[:-4] + ".s")
        r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src, "-o", dst], cwd=os.path.join(tree, CSRC),
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit(f"{tree}: {src} does not compile\n{r.stderr}")
    jobs = int(os.environ.get("MAX_JOBS") or min(16, os.cpu_count() or 4))
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        list(ex.map(one, srcs))


def parse(path):
    """{symbol: (instruction lines, amdhsa lines)} of one .s file."""
    body, hsa, cur, kern, types = {}, {}, None, None, set()
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip() or DROP.match(line):
            continue
        s = line.strip()
        m = re.match(r"\.type\s+([\w$.]+),@function", s)
        if m:
            types.add(m.group(1))
            continue
        m = re.match(r"([\w$.]+):$", s)
        if m and m.group(1) in types and m.group(1) not in body:
            cur = m.group(1)
            body[cur] = []
            continue
        if s.startswith(".amdhsa_kernel "):
            kern = s.split()[1]
            hsa[kern] = []
            continue
        if s == ".end_amdhsa_kernel":
            kern = None
            continue
        if kern is not None:
            hsa[kern].append(" ".join(s.split()))
            continue
        if cur is not None:
            if s.startswith(".size") or s.startswith(".Lfunc_end"):
                cur = None
                continue
            body[cur].append(" ".join(s.split()))
    out = {}
    for sym, lines in body.items():
        names = {}
        ren = lambda m: names.setdefault(m.group(0), f".L{len(names)}")
        out[sym] = ([LOCAL.sub(ren, l) for l in lines], hsa.get(sym, []))
    return out


def mnemonics(lines):
    """How often each mnemonic (a line's first word; labels and directives count as they stand) occurs."""
    return collections.Counter(l.split(None, 1)[0] for l in lines)


def hsa_summary(lines):
    d = dict(l.replace(".amdhsa_", "").split(None, 1) for l in lines if " " in l)
    return " ".join(f"{k}={d[k]}" for k in REPORT if k in d)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        dirs = []
        for i, arg in enumerate(sys.argv[1:]):
            if os.path.isfile(os.path.join(arg, CSRC, "Makefile")):
                d = os.path.join(tmp, str(i))
                os.mkdir(d)
                compile_tree(arg, d)
                dirs.append(d)
            else:
                dirs.append(arg)
        files = [sorted(f for f in os.listdir(d) if f.endswith(".s")) for d in dirs]
        bad = equivalent = total = 0
        for f in sorted(set(files[0]) | set(files[1])):
            if f not in files[0] or f not in files[1]:
                print(f"{f}: only in {'OLD' if f in files[0] else 'NEW'}")
                bad += 1
                continue
            old, new = parse(os.path.join(dirs[0], f)), parse(os.path.join(dirs[1], f))
            for sym in sorted(set(old) | set(new)):
                total += 1
                if sym not in old or sym not in new:
                    print(f"{f} {sym}: only in {'OLD' if sym in old else 'NEW'}")
                    bad += 1
                elif old[sym] == new[sym]:
                    print(f"{f} {sym}: identical ({len(new[sym][0])} lines)")
                elif old[sym][1] == new[sym][1] and mnemonics(old[sym][0]) == mnemonics(new[sym][0]):
                    print(f"{f} {sym}: equivalent ({len(new[sym][0])} lines: the same resources and the same count of every mnemonic)")
                    equivalent += 1
                else:
                    what = [w for w, i in (("instructions", 0), ("resources", 1)) if old[sym][i] != new[sym][i]]
                    first = next((k for k, (a, b) in enumerate(zip(old[sym][0], new[sym][0])) if a != b), min(len(old[sym][0]), len(new[sym][0])))
                    print(f"{f} {sym}: DIFFERENT {' + '.join(what)}; first at line {first}; {len(old[sym][0])} -> {len(new[sym][0])} lines; "
                          f"OLD [{hsa_summary(old[sym][1])}] NEW [{hsa_summary(new[sym][1])}]")
                    bad += 1
        print(f"{total} symbols compared, {total - bad - equivalent} identical, {equivalent} equivalent, {bad} different")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
