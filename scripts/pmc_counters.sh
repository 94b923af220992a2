#!/bin/bash
# A counter pass of the step kernel over a list of SQ / SQC counters chosen by the caller (run on the GPU box):
# one rocprofv3 --pmc run per env count over scripts/variant_driver.py, nothing traced beside it, summarised per
# wave and per physics substep by scripts/pmc_memops_summary.py into $OUT/<TAG>.json.
#   TAG=insts COUNTERS="SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS SQ_INSTS_BRANCH SQ_ACTIVE_INST_MISC" scripts/pmc_counters.sh
#   TAG=icache COUNTERS="SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE" scripts/pmc_counters.sh
#   TAG=ifetch COUNTERS="SQ_IFETCH SQ_IFETCH_LEVEL SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS" scripts/pmc_counters.sh
# SQ_WAVES is added to every pass (the summary divides by it). As many counters as one pass holds: split a longer
# list over several calls. LIB=<another build of the library> SOLVER=cg SIZES="512 8192" as in scripts/pmc_latency.sh.
set -e -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT:-build/pmc_counters}
TAG=${TAG:?TAG}
mkdir -p $OUT
LIB=${LIB:-ksim-gym-zbot_amd/zbot_amd/libzbot_hip.so}
solver=${SOLVER:-cg}
for n in ${SIZES:-512 8192}; do
  d=$OUT/${TAG}_${solver}_$n
  rm -rf $d
  SOLVER=$solver N=$n timeout -k 10 120 rocprofv3 --pmc ${COUNTERS:?COUNTERS} SQ_WAVES --output-format csv -d $d -o run -- \
    python3 scripts/variant_driver.py $LIB 6 > $d.log 2>&1
done
python3 scripts/pmc_memops_summary.py $OUT/$TAG > $OUT/$TAG.json
cat $OUT/$TAG.json
