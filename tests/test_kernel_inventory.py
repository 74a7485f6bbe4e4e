"""Every kernel of libhvit.so is compiled once: no kernel name occurs in more
than one of the library's gfx950 code objects.  A template instantiated from two
translation units is compiled (and shipped) twice; the GEMM entry points share
theirs through one translation unit or one non-template host function instead
(csrc/gemm_conv.hip, hvit_gemm_kc_mn in csrc/gemm_linear.hip).

Names only: the code objects are extracted with llvm-objdump --offloading and
their kernel lists read from the notes llvm-readelf prints.  No GPU."""

import os
import re
import shutil
import subprocess

import pytest

LLVM_BIN = "/opt/rocm/llvm/bin"
OBJDUMP = os.path.join(LLVM_BIN, "llvm-objdump")
READELF = os.path.join(LLVM_BIN, "llvm-readelf")

pytestmark = pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)),
                                reason="llvm-objdump / llvm-readelf not under /opt/rocm/llvm/bin")


def kernel_names(code_object):
    notes = subprocess.run([READELF, "--notes", code_object], check=True, capture_output=True, text=True).stdout
    # the amdhsa.kernels list of the metadata note: one item per kernel, its ".name:" at the
    # item's own indent (an argument's ".name:" would sit deeper)
    kernels = notes.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0]
    names = []
    for item in re.split(r"\n  - ", "\n" + kernels):
        m = re.search(r"^    \.name:\s+(\S+)", item, re.M)
        if m:
            names.append(m.group(1).strip("'\""))
    return names


def test_every_kernel_is_compiled_once(hv, tmp_path):
    lib = tmp_path / "libhvit.so"
    shutil.copy(hv._lib.LIB_PATH, lib)
    subprocess.run([OBJDUMP, "--offloading", lib.name], cwd=tmp_path, check=True, capture_output=True)
    objs = sorted(p for p in tmp_path.iterdir() if p.name.endswith("gfx950"))
    assert len(objs) >= 10, [p.name for p in tmp_path.iterdir()]
    where = {}
    for o in objs:
        names = kernel_names(str(o))
        assert names, o.name
        assert len(names) == len(set(names)), o.name
        for n in names:
            where.setdefault(n, []).append(o.name)
    assert len(where) >= 500
    twice = {n: w for n, w in where.items() if len(w) > 1}
    assert not twice, f"{len(twice)} kernels compiled more than once, e.g. {sorted(twice.items())[:3]}"
