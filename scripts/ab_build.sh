#!/bin/bash
# A/B build of the step kernel: evariants/libeng_<name>.so from zb_engine.hip of a git revision
# (or the working tree with REV=cur), linked with the product's other objects. Diagnostic only.
#   scripts/ab_build.sh <name> [REV | cur | file <path>] [extra hipcc flags]   (SCHED= for the default scheduler)      then on the GPU: python tests/diag_variants.py evariants/libeng_*.so
# Both compilation units of the product are built (csrc/Makefile: the collider sets XG_MASK_A under the
# iterative-ilp scheduler, XG_MASK_B = XG 2 and 5 under the default one), so a variant holds every
# kernel the product does. SCHED= and the extra flags apply to the first unit; the second keeps the
# product's flags.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=$ROOT/ksim-gym-zbot_amd/csrc
OUT=$ROOT/evariants
NAME=$1; REV=${2:-cur}; shift 2 || true
mkdir -p "$OUT"
make -C "$CSRC" -s
SRC=$CSRC/zb_engine.hip
if [ "$REV" = cur ] && [ $# -eq 0 ] && [ -z "${SLP+x}" ] && [ -z "${SCHED+x}" ]; then
  # the working tree with the product flags: the product library just built is that variant
  cp "$ROOT/ksim-gym-zbot_amd/zbot_amd/libzbot_hip.so" "$OUT/libeng_$NAME.so"
  echo "built $OUT/libeng_$NAME.so (the product build)"
  exit 0
fi
if [ "$REV" = file ]; then SRC=$1; shift;
elif [ "$REV" != cur ]; then SRC=$OUT/zb_engine_$NAME.hip; git -C "$ROOT" show "$REV:ksim-gym-zbot_amd/csrc/zb_engine.hip" > "$SRC"; fi
MASK_A=$(sed -n 's/^XG_MASK_A *= *//p' "$CSRC/Makefile")
MASK_B=$(sed -n 's/^XG_MASK_B *= *//p' "$CSRC/Makefile")
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$ROOT/include -I$CSRC -fno-signed-zeros -freciprocal-math -fno-math-errno -fapprox-func"
/opt/rocm/bin/hipcc $FLAGS ${SLP--fno-slp-vectorize} ${SCHED--mllvm -amdgpu-sched-strategy=iterative-ilp} "$@" \
  -DZB_XG_MASK=$MASK_A -c -o "$OUT/eng_$NAME.o" "$SRC" &
/opt/rocm/bin/hipcc $FLAGS -fno-slp-vectorize -DZB_ENGINE_TU_B -DZB_XG_MASK=$MASK_B -c -o "$OUT/eng_${NAME}_b.o" "$SRC" &
wait -n
wait -n
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libeng_$NAME.so" "$OUT/eng_$NAME.o" "$OUT/eng_${NAME}_b.o" \
  "$CSRC/build/zb_capi.o" "$CSRC/build/zb_ppo.o" "$CSRC/build/zb_policy.o" "$CSRC/build/zb_policy_train.o" "$CSRC/build/zb_learner.o" "$CSRC/build/zb_minibatch.o" "$CSRC/build/zb_host.o"
echo "built $OUT/libeng_$NAME.so"
