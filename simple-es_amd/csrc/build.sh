#!/bin/bash
# Builds libses_hip.so for gfx950 (cross-compiles without a GPU).  Usage: csrc/build.sh [extra hipcc flags]
# The translation units are compiled side by side (one hipcc each) and linked; objects land in csrc/_obj (git-ignored).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${SES_OUT:-$HERE/../libses_hip.so}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
OBJ="${SES_OBJ:-$HERE/_obj}"
mkdir -p "$OBJ"
# -fno-slp-vectorize: v_pk_fma_f32 has no throughput advantage on gfx950 (a packed op costs two issue slots)
# and SLP packing adds v_mov traffic; measured 0.357 -> 0.311 ms on the 4096x5x500 rollout.
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize
       -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function -I/opt/rocm/include)
UNITS=(ses_core ses_rollout ses_strategy ses_comm ses_envs ses_generations ses_f64_envs ses_pgpe ses_spread_gru ses_sepcma ses_lmma ses_lander_discrete ses_waterworld ses_maes ses_batch ses_batch_elite ses_batch_sepcma ses_pursuit ses_render ses_ars ses_obs_norm ses_batch_ars ses_hopper ses_walker2d ses_walker_hardcore)
pids=()
for u in "${UNITS[@]}"; do
  "$HIPCC" "${FLAGS[@]}" "$@" -c "$HERE/$u.hip" -o "$OBJ/$u.o" &
  pids+=($!)
done
fail=0
for p in "${pids[@]}"; do wait "$p" || fail=1; done
[ "$fail" = 0 ] || { echo "build failed" >&2; exit 1; }
objs=()
for u in "${UNITS[@]}"; do objs+=("$OBJ/$u.o"); done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -ldl -o "$OUT"
echo "built $OUT"
