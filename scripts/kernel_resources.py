#!/usr/bin/env python3
"""Per-kernel resources (VGPRs, SGPRs, LDS, scratch, spills) of every kernel in the SHIPPED liblmc_atomi.so, read from the code-object
metadata notes.  The .so carries one clang offload bundle per translation unit in its .hip_fatbin section; each bundle is split off,
its gfx950 code object unbundled and its AMDGPU metadata note parsed.

    python scripts/kernel_resources.py [path/to/liblmc_atomi.so] [--json]
    python scripts/kernel_resources.py [path/to/liblmc_atomi.so] --code-hash      name and instruction-stream hash of every device function, sorted by
                                                                                  name: `diff` the output of two libraries to see which kernels a change moved

Used by tests/test_kernel_resources.py (the scratch fence: DESIGN section 3.0p "Scratch finding") and for the tables in DESIGN.md."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "lmc_atomi_amd", "lib", "liblmc_atomi.so")


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return [re.sub(r"^void ", "", d).replace("lmc::", "") for d in out]


def _code_objects(lib):
    """Yields the path of the gfx950 code object of every translation unit of `lib` (valid until the next one is asked for)."""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(d, "unused.so")], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, s in enumerate(starts):
            e = starts[i + 1] if i + 1 < len(starts) else len(blob)
            part = os.path.join(d, f"b{i}.bin")
            co = os.path.join(d, f"b{i}.co")
            open(part, "wb").write(blob[s:e])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
            if os.path.getsize(co) > 0:
                yield co


def kernel_resources(lib=DEFAULT_LIB):
    """-> list of dicts {name, vgpr, agpr, sgpr, lds, scratch, vgpr_spill, sgpr_spill, wg_max}"""
    res = []
    for co in _code_objects(lib):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
        if "amdhsa.kernels:" not in notes:
            continue
        md = notes[notes.index("amdhsa.kernels:"):]
        for blk in re.split(r"\n\s+- \.agpr_count:", md)[1:]:
            blk = ".agpr_count:" + blk

            def g(key, default=0):
                m = re.search(r"\.%s:\s+(\d+)" % key, blk)
                return int(m.group(1)) if m else default
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            res.append(dict(name=name, vgpr=g("vgpr_count"), agpr=g("agpr_count"), sgpr=g("sgpr_count"), lds=g("group_segment_fixed_size"),
                            scratch=g("private_segment_fixed_size"), vgpr_spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"),
                            wg_max=g("max_flat_workgroup_size")))
    for r, dm in zip(res, _demangle([r["name"] for r in res])):
        r["demangled"] = dm
    return res


def code_hashes(lib=DEFAULT_LIB):
    """-> sorted list of (demangled name, sha256 of the function's disassembly) for every device function of the library: the instruction text of
    `llvm-objdump -d --no-show-raw-insn --no-leading-addr` without its `//` comments (addresses, encodings), so that equal hashes mean equal instruction streams."""
    names, hashes = [], []
    for co in _code_objects(lib):
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True, check=True).stdout
        h = None
        for line in dis.splitlines():
            m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line)
            if m:
                h = hashlib.sha256()
                names.append(m.group(1))
                hashes.append(h)
            elif h is not None and line.strip() and line.strip() != "...":      # "...": zero padding up to the next function's alignment
                h.update(re.sub(r"//.*$", "", line).strip().encode() + b"\n")
    return sorted(zip(_demangle(names), (h.hexdigest() for h in hashes)))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--code-hash" in sys.argv:
        for name, h in code_hashes(args[0] if args else DEFAULT_LIB):
            print(h, name)
        sys.exit(0)
    rs = kernel_resources(args[0] if args else DEFAULT_LIB)
    if "--json" in sys.argv:
        print(json.dumps(rs, indent=1))
    else:
        for r in sorted(rs, key=lambda r: (-r["scratch"], r["demangled"])):
            print(f"{r['demangled'][:110]:110s} vgpr {r['vgpr']:4d} sgpr {r['sgpr']:4d} lds {r['lds']:6d} scratch {r['scratch']:5d} spill {r['vgpr_spill']:3d}")
        print(f"{len(rs)} kernels; max scratch {max(r['scratch'] for r in rs)} B per lane")
