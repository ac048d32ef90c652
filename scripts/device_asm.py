#!/usr/bin/env python3
"""Device assembly of every HIP unit, for comparing two trees: scripts/device_asm.py --root <tree> --out <dir> [-- flags]

Compiles each entry of HIP_UNITS with the flags of build(), device side only, to <out>/<object name>.s and prints one
`sha256  name` line per file.  -fuse-cuid=none keeps the per-compilation __hip_cuid_<hash> symbol out, so two runs over
the same source are identical and `cmp A/x.s B/x.s` is an exact test that a refactor left the device code alone.
--only picks units by a substring of the object name; flags after `--` go to every compilation (-DCTC_DIAG -DCTC_F6_NS_ONLY).
Needs no GPU.  MAX_JOBS (default 8) compilations run at a time, longest units first."""
import argparse
import hashlib
import importlib.util
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree to compile")
ap.add_argument("--out", required=True)
ap.add_argument("--only", default="")
ap.add_argument("extra", nargs="*")
args = ap.parse_args()
root = os.path.abspath(args.root)
spec = importlib.util.spec_from_file_location("graft_entry_of_root", os.path.join(root, "__graft_entry__.py"))
ge = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ge)  # HIP_UNITS and CSRC of THAT tree
# build()'s flags without --offload-compress (it only packs the fat binary) and with -S on the device side in place of -c
flags = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-I" + os.path.join(root, "include"), "-I" + ge.CSRC,
         "--offload-device-only", "-fuse-cuid=none", "-S"]
os.makedirs(args.out, exist_ok=True)
units = sorted((u for u in ge.HIP_UNITS if args.only in u[2]),
               key=lambda u: 0 if u[0] == "ctc_fused6.hip" else 1 if u[0] == "ctc_fused5.hip" else 2)


def compile_unit(unit):
    src, extra, obj = unit
    dst = os.path.join(args.out, os.path.splitext(obj)[0] + ".s")
    subprocess.run([os.environ.get("HIPCC", "hipcc"), *flags, *extra, *args.extra, os.path.join(ge.CSRC, src), "-o", dst], check=True)
    return dst


with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", 8))) as ex:
    for dst in ex.map(compile_unit, units):
        print(hashlib.sha256(open(dst, "rb").read()).hexdigest() + "  " + os.path.basename(dst), flush=True)
