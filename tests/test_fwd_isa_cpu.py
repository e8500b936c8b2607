"""CPU: the instruction mix of the headline kernel (mlp_fwd_kernel<1, false, 2>, the exact fp32 inference forward) in
the built library.  fp32 MFMAs run on the SIMD's fp32 lanes, so every VALU instruction costs matrix time: the weight
fragments are read through a buffer descriptor (no 64-bit pointer arithmetic per fragment), and this pins the counts
that follow from that."""
import collections
import os
import re

import pytest

from scade_amd import _lib, build_checks

HEADLINE = "_ZN5scade14mlp_fwd_kernelILi1ELb0ELi2EEEvNS_10MlpFwdArgsE"


def headline_ops():
    if not os.path.exists(build_checks.OBJDUMP):
        pytest.skip("llvm-objdump is not installed")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the library is not built")
    for elf in build_checks.code_objects(_lib.LIB_PATH):
        lines = build_checks.disassemble(elf).split("\n")
        start = [i for i, l in enumerate(lines) if l.endswith("<" + HEADLINE + ">:")]
        if not start:
            continue
        body = []
        for l in lines[start[0] + 1:]:
            if re.match(r"^[0-9a-f]+ <", l):
                break
            tok = l.split("//")[0].split()
            if tok and not tok[0].endswith(":"):
                body.append(tok[0])
        return collections.Counter(body)
    pytest.fail(f"{HEADLINE} not found in the library")


def test_headline_forward_instruction_mix():
    c = headline_ops()
    mfma = sum(v for k, v in c.items() if k.startswith("v_mfma"))
    valu = sum(v for k, v in c.items() if k.startswith("v_") and not k.startswith("v_mfma"))
    assert mfma == 4376                      # the layers' k-blocks: fixed by the network and the tiling
    assert c["s_barrier"] == 21              # two per MFMA layer boundary (in-place epilogue), one after the prologue
    assert valu <= 1690, valu                # 1,944 when each weight fragment had its own 64-bit address
    assert c["v_add_co_u32_e32"] + c["v_addc_co_u32_e32"] <= 12   # 264 before; what is left is outside the k-loops
    assert sum(v for k, v in c.items() if k.startswith("buffer_load")) == 528   # every weight fragment of the k-loops
