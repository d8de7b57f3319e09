"""Codegen guard for the weight ring of the four-wave f16x3 field kernels (csrc/mlp_h3n.hip, ARing): a weight fragment costs no vector-ALU
instruction.  The ring's address is `scalar base + the lane's 16 bytes as a 32-bit offset + immediate`, which the compiler can issue as
global_load_dwordx4 v[..], v_off, s[base:base+1] offset:imm -- but only where it sees the 32-bit offset being widened in the block of
the load.  Hoisted out of the tile loop as a 64-bit value the offset cost one v_lshl_add_u64 per pair of fragments in the three per-view
instances (397 / 397 / 428 between the first and the last MFMA); the post kernels, whose rings start right in front of their GEMMs,
never had them.  Compiled the way tests/test_boundary_cpu.py::test_no_spill_code_inside_nsplit_gemms compiles the file."""
import os
import re
import shutil
import subprocess

import pytest

# v_lshl_add_u64 between the first and the last MFMA.  Per-view instances: the cap of 16 is the allowance of the packed-fp32 guard in
# test_no_spill_code_inside_nsplit_gemms, a condition and not a measurement -- reached: 1 / 1 / 1 (k_train_fwd_pre: its other 31 were the
# per-lane row addresses of save_block, which now takes a scalar base there).  Post instances: no more than before the change (2 / 12;
# reached: 2 / 12).
LIMIT = {"k_field_pre_h3n": 16, "k_field_views_h3n": 16, "k_train_fwd_pre": 16, "k_field_post_h3n": 2, "k_train_fwd_post": 12}
POLICY = set()           # cache-policy bits of the shipped weight loads: none (non-temporal loads lost 16.6 %, profiles/weight_ring_ab_runs.txt)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from diner_amd import build as B
    hipcc = B._hipcc()
    if not (hipcc and (shutil.which(hipcc) or os.path.exists(hipcc))):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("weight_ring") / "mlp_h3n.s"
    subprocess.check_call([hipcc] + B.FLAGS + ["-x", "hip", "-S", "--cuda-device-only", os.path.join(B.CSRC, "mlp_h3n.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def mfma_span(txt, name):
    m = list(re.finditer(r"^(\w*\d" + name + r"I?\w*):.*?\n(.*?)\.Lfunc_end", txt, re.S | re.M))      # (Itanium mangling: <length><name>[I<template args>]E...)
    assert len(m) == 1, f"expected one instance of {name}"
    body = [l.split(";")[0].split("//")[0].strip() for l in m[0].group(2).split("\n")]
    idx = [i for i, l in enumerate(body) if l.startswith("v_mfma")]
    assert len(idx) > 1000, (name, len(idx))
    return [l for l in body[idx[0]:idx[-1] + 1] if l]


@pytest.mark.parametrize("name", sorted(LIMIT))
def test_no_vector_alu_instruction_per_weight_fragment(listing, name):
    span = mfma_span(listing, name)
    adds = [l for l in span if l.startswith("v_lshl_add_u64")]
    print(f"{name}: {len(adds)} v_lshl_add_u64 between the first and the last MFMA")
    assert len(adds) <= LIMIT[name], (name, len(adds))
    # The weight loads: a fragment sits at a non-zero multiple of 1 KB from the ring's base (eight fragments per half-step at -4096 .. 3072;
    # the one at offset 0 cannot be told from a tap and is left out).  Each is the scalar-base form -- a 32-bit vector offset and an SGPR
    # pair -- and carries the shipped cache-policy bits and no others.
    at_kb = lambda l: (o := re.search(r"offset:(-?\d+)", l)) is not None and int(o.group(1)) % 1024 == 0
    loads = [l for l in span if l.startswith("global_load_dwordx4") and at_kb(l)]
    form = re.compile(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\] offset:-?\d+((?: \w+)*)$")
    frag = [l for l in loads if form.match(l)]
    per_gemm = 32 * 7          # half-steps x fragments with a non-zero offset, of one 512-wide GEMM
    assert len(frag) >= 2 * per_gemm, (name, len(frag))
    other_form = [l for l in loads if l not in frag]      # e.g. a 64-bit vector address: global_load_dwordx4 v[..], v[a:b], off offset:1024
    assert not other_form, f"{name}: {len(other_form)} weight loads in another form, e.g. {other_form[:2]}"
    for l in frag:
        assert set(form.match(l).group(1).split()) == POLICY, f"{name}: cache policy of a weight load: {l}"
