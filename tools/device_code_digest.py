#!/usr/bin/env python3
"""sha256 of the device code (.hip_fatbin) of every object file of a build: `sha256  name`, one line per object.
Two trees whose listings are equal run the same kernels, whatever changed in their host code.

    python tools/device_code_digest.py [obj_dir]        (default: balf_amd/csrc/obj of this tree)"""
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

OBJCOPY = os.environ.get("LLVM_OBJCOPY", "/opt/rocm/lib/llvm/bin/llvm-objcopy")
obj_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "balf_amd", "csrc", "obj")
with tempfile.TemporaryDirectory() as tmp:
    for o in sorted(glob.glob(os.path.join(obj_dir, "*.o"))):
        fat = os.path.join(tmp, "fatbin")
        open(fat, "wb").close()
        subprocess.run([OBJCOPY, f"--dump-section=.hip_fatbin={fat}", o, os.devnull], stderr=subprocess.DEVNULL)
        data = open(fat, "rb").read()
        if data:                                         # (an object without device code has no such section)
            print(f"{hashlib.sha256(data).hexdigest()}  {os.path.basename(o)}")
