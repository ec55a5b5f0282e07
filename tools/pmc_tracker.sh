#!/bin/bash
# SQ and memory counters of the dense tracker's two launches at the bench batch (profiles/tracker_sweep.md): one rocprofv3 --pmc run per group, nothing traced in the
# same run, counting restricted to the tracker kernels.  The SQ block has eight slots, FETCH_SIZE and WRITE_SIZE do not fit one pass: four runs.
#   bash tools/pmc_tracker.sh <outdir> [library]      (library: another build of libscavislam_hip.so, through SVS_LIB_PATH)
out=${1:-/tmp/pmc_tracker}
[ -n "$2" ] && export SVS_LIB_PATH=$(realpath $2)
mkdir -p $out
export TMPDIR=/tmp
i=0
for grp in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY" \
           "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY" \
           "FETCH_SIZE" \
           "WRITE_SIZE"; do
  i=$((i+1))
  SVS_BENCH_TRACE_STOP=1 timeout -k 10 170 rocprofv3 --pmc $grp --kernel-include-regex dense_track_batch_kernel --output-format csv -d $out/g$i -o pmc -- \
    python bench.py --gpus 1 --no-cpu --steps 6 --warmup 2 > $out/g$i.log 2>&1
  rc=$?
  echo "group $i rc=$rc"
  if [ $rc -ne 0 ]; then tail -20 $out/g$i.log; exit $rc; fi      # (a run that failed: nothing more is started on the device)
  python tools/pmc_csv.py 'dense_track_batch_kernel<[^>]*>' $(find $out/g$i -name "*counter_collection.csv") > $out/g$i.txt 2>&1
  rm -rf $out/g$i
done
cat $out/g*.txt
