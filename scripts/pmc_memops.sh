#!/bin/bash
# Executed memory instructions of the step kernel by class (run on the GPU box): one rocprofv3 --pmc pass of
# the SQ instruction counters (vector-memory reads and writes, scalar-memory reads, LDS, SALU, VALU) per
# (solver, env count) over scripts/variant_driver.py, summarised per wave and per physics substep by
# scripts/pmc_memops_summary.py into $OUT/pmc_memops.json (OUT: build/pmc_memops unless set). The static counts of
# scripts/phase_waits.py say where a load stands; these say how many a wave executes. A pass of its own, no
# tracing beside it.
# LIB=<another build of the library> SOLVERS="cg" SIZES="512" as in scripts/pmc_latency.sh.
set -e -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT:-build/pmc_memops}
mkdir -p $OUT
LIB=${LIB:-ksim-gym-zbot_amd/zbot_amd/libzbot_hip.so}
for solver in ${SOLVERS:-cg}; do
  for n in ${SIZES:-512}; do
    d=$OUT/pmcmem_${solver}_$n
    rm -rf $d
    SOLVER=$solver N=$n timeout -k 10 120 rocprofv3 --pmc SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_INSTS_LDS \
      SQ_INSTS_SALU SQ_INSTS_VALU SQ_WAVES --output-format csv -d $d -o run -- \
      python3 scripts/variant_driver.py $LIB 6 > $d.log 2>&1
  done
done
python3 scripts/pmc_memops_summary.py $OUT/pmcmem > $OUT/pmc_memops.json
cat $OUT/pmc_memops.json
