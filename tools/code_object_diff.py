#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of the library the same?  The test of a refactor that must not change device code.

Extraction as tools/check_code_objects.py: `llvm-objdump --offloading` unbundles the code objects, `-d --no-show-raw-insn`
disassembles each.  Functions are matched by symbol name across all code objects of a library; reported are the functions present in
one library only, for the others the first differing instruction, and every difference in a kernel's VGPR / AGPR / SGPR / LDS /
scratch figures (the AMDGPU metadata note, `llvm-readelf --notes`).  Addresses are dropped (the listing's `// 0000..:` comments
and branch-target annotations), so a function that merely moved inside its code object compares equal; everything else is
compared as text - the tool knows nothing about particular instructions.  A symbol that ends in a per-compilation hash (a
`.<hex>` / `__<hex>` suffix of eight or more digits, as hipcc gives the symbols it externalises per translation unit under
-fgpu-rdc; this library's build produces none) is matched with the hash stripped.
Exit status 0 only when every function and every figure is identical.
usage: code_object_diff.py OLD.so NEW.so"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

from check_code_objects import LLVM, disassemble

FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
HASH = re.compile(r"(\.|__)[0-9a-f]{8,}$")


def functions(obj):
    """{symbol: [instruction text]} of one code object; labels (L<n>) stay inside their function as lines"""
    out, cur = {}, None
    for ln in disassemble(obj):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln.strip())
        if m and not re.match(r"^L\d+$", m.group(1)):
            cur = out.setdefault(HASH.sub("", m.group(1)), [])
        elif cur is not None:
            s = re.sub(r"\s+", " ", re.sub(r"<[^>]*>", "", ln.split("//")[0])).strip()
            if s:
                cur.append("label:" if m else s)
    return out


def figures(obj):
    """{kernel: {figure: value}} from the metadata note"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], capture_output=True, text=True, check=True).stdout
    out, cur = {}, {}
    for ln in notes.splitlines() + ["  - ."]:
        if re.match(r"^\s{2}- \.", ln) or ln.startswith("amdhsa."):      # the next kernel's entry, or the end of the list
            if ".name" in cur:
                out[HASH.sub("", cur[".name"])] = {k: cur.get(k) for k in FIGURES}
            cur = {}
        m = re.match(r"^\s{2}[- ] (\.\w+):\s*(\S+)\s*$", ln)
        if m:
            cur[m.group(1)] = m.group(2).strip("'\"")
    return out


def load(lib):
    tmp = tempfile.mkdtemp(prefix="codeobj")
    try:
        local = os.path.join(tmp, os.path.basename(lib))
        shutil.copy(lib, local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], capture_output=True, text=True, check=True, cwd=tmp)
        code, figs = {}, {}
        for n, f in enumerate(sorted(f for f in os.listdir(tmp) if "amdgcn" in f)):
            for part, into in ((functions(os.path.join(tmp, f)), code), (figures(os.path.join(tmp, f)), figs)):
                for name, v in part.items():       # file-local kernels of two translation units may share a name
                    into[name if name not in into else "%s (code object %d)" % (name, n)] = v
        return code, figs
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    (old, old_f), (new, new_f) = load(sys.argv[1]), load(sys.argv[2])
    bad = 0
    for name in sorted(set(old) ^ set(new)):
        bad += 1
        print("only in %s: %s" % ("OLD" if name in old else "NEW", name))
    for name in sorted(set(old) & set(new)):
        a, b = old[name], new[name]
        if a != b:
            bad += 1
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("%s: %d / %d instructions, first difference at %d:\n  OLD %s\n  NEW %s"
                  % (name, len(a), len(b), i, a[i] if i < len(a) else "(end)", b[i] if i < len(b) else "(end)"))
        if old_f.get(name) != new_f.get(name):
            bad += 1
            print("%s: figures OLD %s NEW %s" % (name, old_f.get(name), new_f.get(name)))
    print("%d functions in OLD (%d kernels with figures), %d in NEW (%d); %d differences"
          % (len(old), len(old_f), len(new), len(new_f), bad))
    return 1 if bad or not old or not old_f else 0


if __name__ == "__main__":
    sys.exit(main())
