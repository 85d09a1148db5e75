#!/bin/bash
# Runs on the GPU box (via gpurun): rocprofv3 kernel-trace stats + separate PMC passes over tools/pmc_workload.py (the non-LDPC
# kernels of the path).  tools/summarize_kernels_pmc.py condenses the outputs into profiles/<tag>_kernels_pmc.md.
# Six passes, each a run of its own (counters are never collected together with a trace) under a time limit of its own; the script stops at the first pass
# that fails or runs into its limit and returns that pass's exit status (124 / 137: the limit), so nothing more is started on a GPU that has just faulted or hung.
# PASS_LIMIT: the plain workload (no profiler) takes 3 s on the MI355X and the slowest of the six passes 4 s (results/rx_device/README.md); 60 s is fifteen times
# that: room for a cold start and a busy host.
set -u
REPO="${GRAFT_REPO_ROOT:-$(pwd)}"
OUT="$REPO/gpurun_out"
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
W="$REPO/tools/pmc_workload.py"
PASS_LIMIT="${PROFILE_PASS_LIMIT:-60}"      # seconds per pass

pass() {      # pass NAME rocprofv3-options...
    local name=$1; shift
    local t0=$SECONDS
    timeout -k 10 "$PASS_LIMIT" rocprofv3 "$@" --output-format csv -d "$OUT/pk_$name" -- python3 "$W" > "$OUT/pk_$name.log" 2>&1
    local rc=$?
    echo "pass $name: exit status $rc after $((SECONDS - t0)) s (limit $PASS_LIMIT s)"
    if [ $rc -ne 0 ]; then tail -5 "$OUT/pk_$name.log"; fi
    return $rc
}

pass stats --kernel-trace --stats &&
pass fetch --pmc FETCH_SIZE &&
pass write --pmc WRITE_SIZE &&
pass sq1 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_WAIT_ANY &&
pass sq2 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_ANY SQ_BUSY_CYCLES TCC_HIT_sum TCC_MISS_sum &&
pass sq3 --pmc SQ_INSTS_VALU_TRANS_F32 SQ_ACTIVE_INST_VMEM SQ_INST_CYCLES_VMEM_RD SQ_INST_CYCLES_VMEM_WR SQ_WAIT_INST_LDS SQ_INSTS_VALU_MFMA_MOPS_BF16
rc=$?
if [ $rc -ne 0 ]; then echo "profile_kernels.sh: stopped at the first failed pass, exit status $rc"; exit $rc; fi
tail -2 "$OUT/pk_stats.log"; ls "$OUT"/pk_*/*/ | head
