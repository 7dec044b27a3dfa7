"""Where the step loops of the prologue form of the pair rollout kernel lie in the shipped library (no GPU needed).

The compiler aligns no loop of these kernels, and the pair kernel's speed depends on where its step loops lie: moved by 4, 16 or
48 bytes the headline generation takes 5 % longer, moved by 32 or 64 bytes it does not (NOTES.md, "the serial path between two
rollouts").  perturb_prologue (csrc/ses_perturb_prologue.h) therefore ends on a 256-byte line plus a per-instance number of
no-ops (csrc/ses_rollout.hip, k_rollout_cartpole_mlp_handover_perturb) that puts the loops where they were measured.  An edit of
the prologue cannot move them any more, but one that changes the code BEHIND it (or the prologue's register allocation, which
that code inherits) can: this test then fails, and the constants are to be set again so that every loop head is back at its
offset mod 32 -- or, after a change of the loops themselves, measured anew.

A loop here is a backward branch that spans more than 900 bytes.  The last ones of a kernel, in address order, are the loops
behind the prologue -- the light wave's step loop, the heavy wave's, their twins behind the hand-over -- and only those are
compared, as offsets mod 32: the loops inside the prologue may lie anywhere.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_hash  # noqa: E402

LIB = os.path.join(ROOT, "simple-es_amd", "libses_hip.so")

# instance (mangled-name fragment) -> offsets mod 32 of its loop heads, in address order: <true, true>, the headline's, as measured
# (profiles/r12_serial_path.txt); <true, false> as the instance was placed before the prologue's rows came from registers (its
# placement was never measured on its own)
PLACED = {
    "k_rollout_cartpole_mlp_handover_perturbILb1ELb1E": [4, 0, 8, 4, 28, 16],
    "k_rollout_cartpole_mlp_handover_perturbILb1ELb0E": [12, 20, 4, 0, 16, 0, 20, 0],
}


def loop_heads(frag):
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
    assert os.path.exists(objdump), "llvm-objdump (ROCm's LLVM) is needed to read where the loops lie: the pin must not go unchecked"
    for co in kernel_hash._code_objects(open(LIB, "rb").read()):
        if frag.encode() not in co:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            text = subprocess.run([objdump, "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, timeout=300).stdout
        body = re.search(r"<[^>]*" + frag + r"[^>]*>:(.*?)s_endpgm", text, flags=re.S)
        if not body:
            continue
        heads = set()
        for line in body.group(1).splitlines():
            m = re.search(r"^\s*(s_cbranch\w*|s_branch)\s.*//\s*([0-9A-Fa-f]{12}):\s*([0-9A-Fa-f]{8})", line)
            if not m:
                continue
            at, simm = int(m.group(2), 16), int(m.group(3), 16) & 0xFFFF
            target = at + 4 + 4 * (simm - 0x10000 if simm >= 0x8000 else simm)
            if at - target > 900:
                heads.add(target)
        return sorted(heads)
    raise AssertionError(f"no kernel named *{frag}* in {LIB}")


@pytest.mark.parametrize("frag", list(PLACED))
def test_step_loops_of_the_prologue_form_lie_where_they_were_measured(frag):
    assert os.path.exists(LIB), "build the library first (python __graft_entry__.py)"
    heads = loop_heads(frag)
    got = [h % 32 for h in heads][-len(PLACED[frag]):]
    print(frag, [hex(h) for h in heads], got)
    assert got == PLACED[frag], (f"{frag}: loop heads at {got} mod 32, measured at {PLACED[frag]}: set the no-op count of this instance "
                                 "again (csrc/ses_rollout.hip) -- 4 bytes per no-op")
