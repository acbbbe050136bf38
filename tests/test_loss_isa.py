"""Compiled-code checks of the exact-f32 in-batch passes (CPU only: cross-compiles loss.hip for gfx950).

The G.Y products of the item pass (inbatch_gt_kernel) and of the user pass (inbatch_sweep_kernel) must keep their
LDS B operands in flight ahead of the MFMAs: no `s_waitcnt lgkmcnt(0)` in front of each MFMA group, and no scratch
traffic inside the tile loop.
"""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "recommendit_amd" / "csrc"
HIPCC = shutil.which("hipcc") or next((p for p in ["/opt/rocm/bin/hipcc"] if os.path.exists(p)), None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not available")

GT = [(d, nw) for d in (32, 64, 128) for nw in (8, 4)]
SWEEP = [(d, mu, go, nw) for d in (32, 64, 128) for (mu, go) in ((1, 1), (1, 0), (0, 0)) for nw in (8, 4)]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "loss.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    "--cuda-device-only", "-S", "-o", str(out), str(CSRC / "loss.hip")],
                   check=True, capture_output=True, timeout=600)
    return out.read_text()


def _kernel(asm, sym):
    start = asm.index(f"\n{sym}:")
    return asm[start:asm.index("s_endpgm", start)]


def _meta(asm, sym, key):
    """A field of the kernel's metadata record (the records start with .agpr_count)."""
    at = asm.index(f".name:           {sym}")
    start = asm.rindex("- .agpr_count:", 0, at)
    nxt = asm.find("- .agpr_count:", at)
    m = re.search(rf"\.{key}:\s+(\d+)", asm[start:nxt if nxt > 0 else len(asm)])
    return int(m.group(1))


def _loop(body):
    """Instructions of the tile loop (header label .. last branch back to it)."""
    m = re.search(r"^(\.LBB\d+_\d+):\s+; =>This Inner Loop Header", body, re.M)
    assert m, "no loop found"
    end = max(x.end() for x in re.finditer(rf"s_c?branch\w*\s+{re.escape(m.group(1))}\b", body))
    lines = (ln.strip() for ln in body[m.start():end].split("\n"))
    return [ln for ln in lines if ln and ln[0] not in ";."]


def _waits_before_mfma(ins):
    return sum(1 for a, b in zip(ins, ins[1:]) if a == "s_waitcnt lgkmcnt(0)" and b.startswith("v_mfma"))


@pytest.mark.parametrize("d,nw", GT)
def test_item_pass_operands_prefetched(asm, d, nw):
    sym = f"_ZN12_GLOBAL__N_117inbatch_gt_kernelILi{d}ELi{nw}EEEv9SweepArgs"
    ins = _loop(_kernel(asm, sym))
    assert sum(1 for x in ins if x.startswith("v_mfma")) == 16 * (d // 32)
    assert _waits_before_mfma(ins) == 0
    assert _meta(asm, sym, "private_segment_fixed_size") == 0
    if d == 128:  # one ds_read_b128 per k-row
        assert sum(1 for x in ins if x.startswith("ds_read_b128")) == 16


@pytest.mark.parametrize("d,mu,go,nw", SWEEP)
def test_user_pass_operands_prefetched(asm, d, mu, go, nw):
    sym = (f"_ZN12_GLOBAL__N_120inbatch_sweep_kernelILi{d}ELb{mu}ELb{go}ELi{nw}EEEv9SweepArgs")
    ins = _loop(_kernel(asm, sym))
    kb, ct = d // 8, d // 32
    # the S chain (row-major reads, unchanged) may wait before its MFMAs; the G.Y block would add 8 * ct more if
    # it waited before every MFMA pair
    assert _waits_before_mfma(ins) <= 2 * kb + ct
    if not (d == 128 and mu == 0):  # the d = 128 recompute form still reloads two spilled values per tile
        assert not any(x.startswith("scratch_") for x in ins)
    if d == 128:
        assert not any(x.startswith("ds_read2_b32") for x in ins)
