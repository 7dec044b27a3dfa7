#!/usr/bin/env python3
"""Serial-issue model of the headline rollout kernel, written next to the profiles (no GPU needed).

    python tools/issue_model.py profiles/r05_issue_model.json

Compiles csrc/ses_rollout.hip to a gfx950 listing with the build's flags, prices the two loop bodies the headline job
runs (fully observed CartPole: the light wave at 16 lanes per env, the heavy wave at 4 in its packed form, in
k_rollout_cartpole_mlp_handover_perturb<true, true> -- the step loops are the ones k_rollout_cartpole_mlp_handover<true, true> compiles; the
prologue in front of them is not priced) with tools/loop_issue_cost.py --
every VALU instruction at the issue cadence tools/valu_issue.hip / vgpr_bank.hip measured on MI355X (2, 4 or 8 cycles) --
and records them with the hash of the kernel's machine code in the built library.  bench.py turns it into
`rollout_kernel.valu_issue_model_frac`: SIMD cycles the loops need if every instruction issued alone at its measured
cadence, over the SIMD cycles the kernel had.  It says how far the kernel is from the ceiling of its own instruction MIX;
`valu_issue_frac` beside it is the nominal one (every instruction at 2 cycles)."""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kernel_hash  # noqa: E402
import loop_issue_cost  # noqa: E402

KERNEL = "k_rollout_cartpole_mlp_handover_perturbILb1ELb1"   # <fixed_length = true, heavy_pk = true>, the form that draws its own rows: what the headline launches for every generation of a call but the first (round 8), with the packed heavy wave (round 9)


def build_flags():
    text = open(os.path.join(ROOT, "simple-es_amd", "csrc", "build.sh")).read()
    m = re.search(r"FLAGS=\((.*?)\)", text, re.S)
    return m.group(1).split()


def main():
    out_path = sys.argv[1]
    src = os.path.join(ROOT, "simple-es_amd", "csrc", "ses_rollout.hip")
    with tempfile.TemporaryDirectory() as tmp:
        lst = os.path.join(tmp, "rollout.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + build_flags() + ["--cuda-device-only", "-S", src, "-o", lst],
                              stderr=subprocess.DEVNULL)
        name, found = loop_issue_cost.loops(open(lst).read().splitlines(), KERNEL)
    # step loops by lanes per env: 4 (the heavy wave, packed: the loops with v_pk_fma_f32, ~132 VALU), 8 (the hand-over's second
    # phase, ~104), 16 (the light wave, ~83); the loop that nests the heavy wave's two priority segments (> 200 VALU) is not a step
    # loop, and neither is the scalar loop a heavy wave with a wild initial angle falls back to
    packed = lambda lp: lp["kinds"].get("v_pk_fma_f32", 0) > 0   # noqa: E731
    heavy = [lp for lp in found if packed(lp) and lp["valu"] <= 200]
    split = [lp for lp in found if not packed(lp) and 95 <= lp["valu"] < 140]
    light = [lp for lp in found if not packed(lp) and lp["valu"] < 95]
    assert len(heavy) == 2 and len(split) == 2 and len(light) == 2, [(lp["label"], lp["valu"]) for lp in found]
    # each body exists twice: with the observation mask applied (POMDP: four more v_cndmask_b32) and without -- the headline is fully observed
    pick = lambda pair: min(pair, key=lambda lp: lp["kinds"].get("v_cndmask_b32", 0))   # noqa: E731
    h, s8, l = pick(heavy), pick(split), pick(light)
    lib = os.path.join(ROOT, "simple-es_amd", "libses_hip.so")
    model = {
        "kernel": name,
        "kernel_match": "k_rollout_cartpole_mlp",
        "kernel_code_sha256": kernel_hash.hash_kernels(lib, "k_rollout_cartpole_mlp"),
        "workload": "4096 offspring x 5 episodes x 500 fixed-length steps: 1024 light waves (4 envs at 16 lanes per env) + 1024 heavy "
                    "waves (16 envs at 4 lanes per env, the packed step), paired one of each per SIMD, no hand-over (the default)",
        "issue_cycles_per_step": {"lanes_per_env_16": {"waves": 1024, "cycles": l["cycles"], "valu": l["valu"]},
                                  "lanes_per_env_4": {"waves": 1024, "cycles": h["cycles"], "valu": h["valu"]}},
        "handover_phase2_loop": {"lanes_per_env_8": {"cycles": s8["cycles"], "valu": s8["valu"],
                                                     "note": "runs only with rollout_handover_step < max_step; not in the sum"}},
        "clock_ghz_under_load": 2.4,
        "clock_source": "DESIGN 6: 2394-2400 MHz sampled during the bench",
        "pricing": "tools/loop_issue_cost.py: 2 cycles for mul/add/sub/mov/and/lshr and fma forms with <= 2 register sources or three "
                   "registers of mixed parity, 8 for v_rcp_f32, 4 for everything else, v_pk_* included (profiles/r01_valu_issue.txt, r01_vgpr_bank.txt)",
        "instructions_per_step": {"lanes_per_env_16": l["valu"] + l["lds"] + l["salu"], "lanes_per_env_4": h["valu"] + h["lds"] + h["salu"],
                                  "note": "VALU + LDS + SALU of the loop body (s_waitcnt / s_nop not counted): what the wave that is served "
                                          "first pays for (profiles/r09_heavy_stream.txt)"},
    }
    json.dump(model, open(out_path, "w"), indent=1)
    print(json.dumps(model["issue_cycles_per_step"]))


if __name__ == "__main__":
    main()
