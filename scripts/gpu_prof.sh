#!/bin/bash
# PMC passes (force-free and Kerr) + kernel-trace summaries of both benches.  TAG names outputs,
# which go under $OUT (default prof_out/).
set -o pipefail
T=${TAG:-x}
export OUT=${OUT:-prof_out}
mkdir -p $OUT
export TMPDIR=/tmp
# --full: the traced runs' bench lines carry pass_ms and the roofline (scripts/show_bench.py)
B="python bench.py --full --steps 3 --warmup 1 --no-cpu --no-extras"
PMC_TAG=_${T}_ff PROBLEM=force_free bash scripts/gpu_pmc.sh > $OUT/${T}_pmc_ff_chain.log 2>&1
grep -q PMC_RC=0 $OUT/${T}_pmc_ff_chain.log || exit 6
python scripts/pmc_summary.py $OUT/pmc_${T}_ff $OUT/${T}_ff_pmc.json > $OUT/${T}_ff_pmc_summary.log 2>&1 || exit 7
PMC_TAG=_${T}_kerr PROBLEM=kerr_magnetosphere bash scripts/gpu_pmc.sh > $OUT/${T}_pmc_kerr_chain.log 2>&1
grep -q PMC_RC=0 $OUT/${T}_pmc_kerr_chain.log || exit 8
python scripts/pmc_summary.py $OUT/pmc_${T}_kerr $OUT/${T}_kerr_pmc.json > $OUT/${T}_kerr_pmc_summary.log 2>&1 || exit 9
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${T}_prof_ff -o run -- $B > $OUT/${T}_prof_ff.log 2>&1 || exit 10
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${T}_prof_kerr -o run -- $B --problem kerr_magnetosphere > $OUT/${T}_prof_kerr.log 2>&1 || exit 11
echo "PROF_RC=0"
