#!/usr/bin/env python3
"""Register, LDS, scratch and code-size table of one translation unit's kernels (dev tool,
no GPU): the unit is compiled for the device alone with the library's own flags
(fleet_amd/build.py) and the figures are read from the code object -- the amdhsa.kernels
metadata note for VGPRs, SGPRs, LDS and scratch, the symbol table for the code size.

usage: kernel_resources.py FILE.hip [--json OUT.json]
       kernel_resources.py --table PARENT.json THIS.json      # the two side by side, markdown
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tool(name):
    from fleet_amd import build as B
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(B.HIPCC)))
    for p in (os.path.join(rocm, "llvm", "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name)):
        if os.path.exists(p):
            return p
    return name


def demangle(names):
    import shutil
    filt = shutil.which(tool("llvm-cxxfilt")) or shutil.which("c++filt")
    if not filt:  # the mangled names then
        return list(names)
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[: len(names)]


def resources(src):
    from fleet_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "unit.co")
        extra = []
        if src.endswith("stream_kernels.hip"):
            extra = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
        B._run([B.HIPCC, "-x", "hip", f"--offload-arch={B.ARCH}", "--cuda-device-only", "--no-gpu-bundle-output", *B.COMMON, *extra, "-c", src, "-o", co])
        notes = subprocess.run([tool("llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        syms = subprocess.run([tool("llvm-readelf"), "-s", "-W", co], capture_output=True, text=True, check=True).stdout
    size = {}
    for line in syms.split("\n"):
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
    rows = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        get = lambda key: re.search(r"\n\s*\.%s:\s*(\S+)" % key, blk).group(1)
        name = get("name")
        rows[name] = {"vgpr": int(get("vgpr_count")), "sgpr": int(get("sgpr_count")),
                      "lds": int(get("group_segment_fixed_size")), "scratch": int(get("private_segment_fixed_size")),
                      "code": size.get(name, -1)}
    names = sorted(rows)
    return {d: rows[n] for n, d in zip(names, demangle(names))}


def short(name):
    return re.sub(r"\(.*", "", name).replace("fleet::", "").replace("void ", "")


def table(parent, this):
    cols = ("vgpr", "sgpr", "lds", "scratch", "code")
    out = ["| kernel | " + " | ".join(f"{c} parent | {c} this" for c in cols) + " | equal |",
           "|---|" + "---|" * (2 * len(cols) + 1)]
    for k in sorted(set(parent) | set(this)):
        a, b = parent.get(k), this.get(k)
        cells = [f"{a[c] if a else '-'} | {b[c] if b else '-'}" for c in cols]
        out.append(f"| `{short(k)}` | " + " | ".join(cells) + f" | {'new' if a is None else 'yes' if a == b else 'NO'} |")
    return "\n".join(out)


def main():
    if sys.argv[1] == "--table":
        print(table(json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))))
        return
    r = resources(os.path.abspath(sys.argv[1]))
    text = json.dumps(r, indent=1, sort_keys=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            f.write(text + "\n")
    for k, v in r.items():
        print(f"{short(k):44s} vgpr {v['vgpr']:3d} sgpr {v['sgpr']:3d} lds {v['lds']:6d} scratch {v['scratch']:3d} code {v['code']:6d}")


if __name__ == "__main__":
    main()
