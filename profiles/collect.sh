#!/bin/bash
# Re-collect the rocprofv3 evidence kept under profiles/ (run on the GPU box from the repo root):
#   bash profiles/collect.sh                 -> gpurun_out/prof_<prec>/{trace,pmc_sq,pmc_fetch,pmc_write}         (render, per precision)
#                                               gpurun_out/prof_train_<prec>/{trace,pmc_sq,pmc_fetch,pmc_write}    (BASELINE configs[2])
#   python profiles/summarize.py gpurun_out/prof_<prec> r03_<prec>
#   python profiles/summarize.py gpurun_out/prof_train_<prec> r03_train_<prec>
# Counters are collected in their own passes (never together with trace domains), FETCH_SIZE and
# WRITE_SIZE separately (TCC slot limit), as MI355X_MICROARCH.md prescribes.
#   PASSES="trace" bash profiles/collect.sh  -> only the kernel trace (a before/after timing comparison needs no counters);
#                                               PASSES is any subset of: trace pmc_sq pmc_fetch pmc_write
#   OUT=dir                                     where prof_* goes instead of the default (absolute, or relative to the repo root)
# Every rocprofv3 pass is a step of its own under a time limit (STEP_TIMEOUT seconds, default 600), and the first step that
# fails or runs out of time ends the script (set -e): nothing more is started on a GPU that has just faulted or hung.
set -e
cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:-/root/repo}"
PASSES=${PASSES-trace pmc_sq pmc_fetch pmc_write}
LIMIT="timeout -k 10 ${STEP_TIMEOUT:-600}"
want() { case " $PASSES " in *" $1 "*) return 0;; esac; return 1; }
SQ="SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE SQ_LDS_BANK_CONFLICT"
for P in ${PRECS-f32 f16 f32x}; do
  if [ -z "$OUT" ]; then
  D=gpurun_out/prof_$P; mkdir -p $D
  else D="$OUT/prof_$P"; mkdir -p "$D"; fi
  A="--full --cpu-sample 0 --no-extras --no-full-network-compare --precision $P"     # --full: the HIP-event pass of the roofline too
  if want trace; then $LIMIT rocprofv3 --kernel-trace --stats --output-format csv -d $D/trace -- python3 bench.py --steps 3 --warmup 1 $A > $D/bench_trace.log 2>&1; fi
  if want pmc_sq; then $LIMIT rocprofv3 --pmc $SQ --output-format csv -d $D/pmc_sq -- python3 bench.py --steps 1 --warmup 0 $A > $D/bench_pmc_sq.log 2>&1; fi
  if want pmc_fetch; then $LIMIT rocprofv3 --pmc FETCH_SIZE --output-format csv -d $D/pmc_fetch -- python3 bench.py --steps 1 --warmup 0 $A > $D/bench_pmc_fetch.log 2>&1; fi
  if want pmc_write; then $LIMIT rocprofv3 --pmc WRITE_SIZE --output-format csv -d $D/pmc_write -- python3 bench.py --steps 1 --warmup 0 $A > $D/bench_pmc_write.log 2>&1; fi
  if want trace; then tail -1 $D/bench_trace.log | cut -c1-200; fi
done
for P in ${TRAIN_PRECS-f32 f32x}; do
  if [ -z "$OUT" ]; then
  D=gpurun_out/prof_train_$P${TRAIN_TAG-}; mkdir -p $D      # TRAIN_TAG=_dense with NERF_DEAD_TILE_SKIP=0 in the environment: every tile computed
  else D="$OUT/prof_train_$P${TRAIN_TAG-}"; mkdir -p "$D"; fi
  A="--mode train --precision $P --no-dense-compare"
  if want trace; then $LIMIT rocprofv3 --kernel-trace --stats --output-format csv -d $D/trace -- python3 bench.py --steps 10 --warmup 2 $A > $D/bench_trace.log 2>&1; fi
  if want pmc_sq; then $LIMIT rocprofv3 --pmc $SQ --output-format csv -d $D/pmc_sq -- python3 bench.py --steps 2 --warmup 0 $A > $D/bench_pmc_sq.log 2>&1; fi
  if want pmc_fetch; then $LIMIT rocprofv3 --pmc FETCH_SIZE --output-format csv -d $D/pmc_fetch -- python3 bench.py --steps 2 --warmup 0 $A > $D/bench_pmc_fetch.log 2>&1; fi
  if want pmc_write; then $LIMIT rocprofv3 --pmc WRITE_SIZE --output-format csv -d $D/pmc_write -- python3 bench.py --steps 2 --warmup 0 $A > $D/bench_pmc_write.log 2>&1; fi
  if want trace; then tail -1 $D/bench_trace.log | cut -c1-200; fi
done
