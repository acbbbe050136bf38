"""Compiled-code checks of the steady-state tile loops of the exact-f32 in-batch passes (CPU only: cross-compiles
loss.hip for gfx950).

Full tiles off the diagonal band, with two more full tiles to come, run in a loop unrolled by the period of the rings
(three tiles in the item pass, six in the user pass).  Its body must hold the MFMAs, their LDS operands, the element
arithmetic and the unconditional loads and stores, and none of the bookkeeping of the one-tile loop: no register
copies, no compares, no exec-masked regions, no scratch, no packed f32.  These are conditions read off the design, not
tuned thresholds.  tests/test_loss_isa.py keeps watching the one-tile loop, which stays first in each kernel.
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

# Which instantiations take the steady loop, and how many tiles one trip of it runs.  Mirrors GT_STEADY / SWEEP_STEADY
# in csrc/loss_sweep_args.h; every other instantiation keeps the one-tile loop for all its tiles and is exempt.
GT_STEADY = {(128, 8): 3}
SWEEP_STEADY = {(128, 1, 1, 8): 6}

# private_segment_fixed_size (bytes of scratch per lane) of every kernel at the parent commit bd0d023
PARENT_SCRATCH_GT = {k: 0 for k in GT}
PARENT_SCRATCH_SWEEP = {k: 0 for k in SWEEP if k[0] < 128}
PARENT_SCRATCH_SWEEP.update({(128, 1, 1, 8): 12, (128, 1, 0, 8): 12, (128, 0, 0, 8): 12,
                             (128, 1, 1, 4): 12, (128, 1, 0, 4): 12, (128, 0, 0, 4): 28})


def gt_sym(d, nw):
    return f"_ZN12_GLOBAL__N_117inbatch_gt_kernelILi{d}ELi{nw}EEEv9SweepArgs"


def sweep_sym(d, mu, go, nw):
    return f"_ZN12_GLOBAL__N_120inbatch_sweep_kernelILi{d}ELb{mu}ELb{go}ELi{nw}EEEv9SweepArgs"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_steady") / "loss.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    "--cuda-device-only", "-S", "-o", str(out), str(CSRC / "loss.hip")],
                   check=True, capture_output=True, timeout=600)
    return out.read_text()


def _kernel(asm, sym):
    start = asm.index(f"\n{sym}:")
    return asm[start:asm.index("s_endpgm", start)]


def _meta(asm, sym, key):
    at = asm.index(f".name:           {sym}")
    start = asm.rindex("- .agpr_count:", 0, at)
    nxt = asm.find("- .agpr_count:", at)
    return int(re.search(rf"\.{key}:\s+(\d+)", asm[start:nxt if nxt > 0 else len(asm)]).group(1))


def _inner_loops(body):
    """Instruction lists of the innermost loops, in code order.  The compiler annotates the header block of such a
    loop with `This Inner Loop Header` (on the label's line at depth 1, on a comment line after it when the loop is
    nested) and every other block of the loop with `in Loop: Header=BBn_m`."""
    blocks = []  # [label or None, annotation, instructions]
    for ln in body.split("\n"):
        t = ln.strip()
        m = re.match(r"^\.LBB(\d+_\d+):(.*)", t)
        if m:
            blocks.append([m.group(1), m.group(2), []])
        elif t.startswith("; %bb."):
            blocks.append([None, t, []])
        elif blocks and t.startswith(";"):
            blocks[-1][1] += " " + t
        elif blocks and t and t[0] != ".":
            blocks[-1][2].append(t)
    loops = {label: [] for label, note, _ in blocks if label and "This Inner Loop Header" in note}
    for label, note, ins in blocks:
        h = re.search(r"in Loop: Header=BB(\d+_\d+)\b", note)
        owner = label if label in loops else (h.group(1) if h else None)
        if owner in loops:
            loops[owner] += ins
    return list(loops.values())


def _steady_loop(asm, sym):
    """The steady loop is the inner loop with the most MFMAs."""
    loops = _inner_loops(_kernel(asm, sym))
    assert loops, "no loop found"
    return max(loops, key=lambda ins: sum(1 for x in ins if x.startswith("v_mfma")))


def _count(ins, prefix):
    return sum(1 for x in ins if x.startswith(prefix))


def _waits_before_mfma(ins):
    return sum(1 for a, b in zip(ins, ins[1:]) if a == "s_waitcnt lgkmcnt(0)" and b.startswith("v_mfma"))


def _no_bookkeeping(ins):
    assert not [x for x in ins if x.startswith("v_cmp")], "compares in the steady loop"
    assert not [x for x in ins if re.match(r"s_\w*saveexec", x) or x.startswith("s_cbranch_exec")
                or re.match(r"s_\w+\s+exec\b", x)], "exec-mask instructions in the steady loop"
    assert not [x for x in ins if x.startswith("scratch_")], "scratch traffic in the steady loop"


def test_table_matches_source():
    src = (CSRC / "loss_sweep_args.h").read_text()
    assert "constexpr bool GT_STEADY(int d, int nw) { return d == 128 && nw == 8; }" in src
    assert ("constexpr bool SWEEP_STEADY(int d, bool mode_user, bool gout, int nw) "
            "{ return d == 128 && mode_user && gout && nw == 8; }") in src


@pytest.mark.parametrize("d,nw", sorted(GT_STEADY))
def test_item_pass_steady_loop(asm, d, nw):
    unroll, ct = GT_STEADY[(d, nw)], d // 32
    ins = _steady_loop(asm, gt_sym(d, nw))
    assert _count(ins, "v_mfma") == 16 * ct * unroll       # 64 per tile at d = 128
    assert _count(ins, "v_mov") == 0 and _count(ins, "v_accvgpr") == 0
    _no_bookkeeping(ins)
    assert _waits_before_mfma(ins) == 0
    assert _count(ins, "ds_read_b128") == 16 * unroll      # one per k-row
    # a plain GEMM: nothing on the VALU but the MFMAs
    assert [x for x in ins if x.startswith("v_") and not x.startswith("v_mfma")] == []


@pytest.mark.parametrize("d,mu,go,nw", sorted(SWEEP_STEADY))
def test_user_pass_steady_loop(asm, d, mu, go, nw):
    unroll, kb, ct = SWEEP_STEADY[(d, mu, go, nw)], d // 8, d // 32
    ins = _steady_loop(asm, sweep_sym(d, mu, go, nw))
    assert _count(ins, "v_mfma") == (4 * kb + 16 * ct) * unroll   # S chain + G.Y: 128 per tile at d = 128
    # the element definition and nothing more: 16 elements and two logs per tile
    assert _count(ins, "v_exp_f32") == 16 * unroll
    assert _count(ins, "v_rcp_f32") == 16 * unroll
    assert _count(ins, "v_log_f32") == 2 * unroll
    assert _count(ins, "v_pk_") == 0
    assert _count(ins, "v_mov_b64") == 0                   # no st = sn accumulator copies
    _no_bookkeeping(ins)
    assert _waits_before_mfma(ins) <= (2 * kb + ct) * unroll   # only the S chain waits on its operands


@pytest.mark.parametrize("d,nw", GT)
def test_item_pass_scratch_not_above_parent(asm, d, nw):
    assert _meta(asm, gt_sym(d, nw), "private_segment_fixed_size") <= PARENT_SCRATCH_GT[(d, nw)]


@pytest.mark.parametrize("d,mu,go,nw", SWEEP)
def test_user_pass_scratch_not_above_parent(asm, d, mu, go, nw):
    assert _meta(asm, sweep_sym(d, mu, go, nw), "private_segment_fixed_size") <= PARENT_SCRATCH_SWEEP[(d, mu, go, nw)]
