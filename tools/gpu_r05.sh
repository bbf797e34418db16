#!/bin/bash
# Round-5 GPU runs, one parameterised runner (no more one-off scripts):   gpurun --timeout N -- 'bash tools/gpu_r05.sh <step> [tag]'
# Everything a step writes goes to gpurun_out/<tag>_*; what is to be judged is copied to profiles/ by hand afterwards.
#   probe     tools/micro/fault_probe.bin in every mode (which host-memory life cycle makes a later pageable copy fault)
#   stress    tools/reader_fault_stress.py under the A/B environments of the reader-fault investigation
#   suite     the GPU suite in the driver's order, once ($REPEAT times)
#   bench     bench.py (default flags)
#   evidence  what profiles/ holds at the end of the round, all at the SAME code: bench lines, kernel stats + step timeline (rocprofv3 --kernel-trace --stats),
#             the four PMC passes (separate runs, no trace domains beside --kernel-trace), reader rates with and without the registered file mapping,
#             small-batch latency, the strong-scaling line on one and on two ranks (one GPU, gloo)
set -u
step=${1:-probe}; tag=${2:-r05}
out=gpurun_out; mkdir -p $out
export TMPDIR=/tmp
case "$step" in
probe)
  B=tools/micro/fault_probe.bin
  TL=$(python -c "import torch,os;print(os.path.join(os.path.dirname(torch.__file__),'lib'))")
  {
    echo "=== with torch's bundled HIP runtime ($TL: what the GPU suite runs on, torch being imported first)"
    for m in pincache_sync pincache_async pincache_h2d reg_file_ro reg_file reg_anon; do
      for sl in 20000 0; do LD_LIBRARY_PATH=$TL timeout 120 $B $m 1239008 $sl 40 2>&1 | tail -2; done
    done
    echo "=== with /opt/rocm's HIP runtime"
    for m in pincache_sync pincache_async pincache_h2d reg_file_ro reg_file reg_anon reg_file_keep; do
      for sl in 20000 0; do timeout 120 $B $m 1239008 $sl 40 2>&1 | tail -2; done
    done
    echo "--- below the in-place pinning threshold (staged copies): control"
    timeout 120 $B pincache_sync 900000 20000 40 2>&1 | tail -1
    timeout 120 $B reg_file_ro 900000 20000 40 2>&1 | tail -1
    echo "--- larger copies"
    timeout 120 $B pincache_sync 8000000 20000 40 2>&1 | tail -1
    timeout 120 $B reg_file_ro 8000000 20000 40 2>&1 | tail -1
    echo "--- GPU_PINNED_MIN_XFER_SIZE=4096 (MB): is in-place pinning the mechanism?"
    GPU_PINNED_MIN_XFER_SIZE=4096 timeout 120 $B pincache_sync 1239008 20000 40 2>&1 | tail -1
    GPU_PINNED_MIN_XFER_SIZE=4096 timeout 120 $B reg_file_ro 1239008 20000 40 2>&1 | tail -1
  } > $out/${tag}_fault_probe.txt 2>&1
  cat $out/${tag}_fault_probe.txt
  ;;
stress)
  {
    for seed in 1 2 3; do echo "== default env, seed $seed"; timeout 600 python tools/reader_fault_stress.py --iters ${ITERS:-150} --seed $seed 2>&1 | tail -3; done
    echo "== SVX_BAM_DEV_MAPFILE=0"; SVX_BAM_DEV_MAPFILE=0 timeout 600 python tools/reader_fault_stress.py --iters ${ITERS:-150} --seed 1 2>&1 | tail -3
    echo "== GPU_PINNED_MIN_XFER_SIZE=4096"; GPU_PINNED_MIN_XFER_SIZE=4096 timeout 600 python tools/reader_fault_stress.py --iters ${ITERS:-150} --seed 1 2>&1 | tail -3
    echo "== no torch (/opt/rocm runtime)"; timeout 600 python tools/reader_fault_stress.py --iters ${ITERS:-150} --seed 1 --no-torch 2>&1 | tail -3
    TL=$(python -c "import torch,os;print(os.path.join(os.path.dirname(torch.__file__),'lib'))")
    echo "== no torch, torch's bundled runtime"; LD_LIBRARY_PATH=$TL timeout 600 python tools/reader_fault_stress.py --iters ${ITERS:-150} --seed 1 --no-torch 2>&1 | tail -3
  } > $out/${tag}_reader_stress.txt 2>&1
  cat $out/${tag}_reader_stress.txt
  ;;
oldway)
  # the round-4 behaviour with the round-5 diagnostics: direct pageable copies, registered file mapping and reader windows, the round-4 test order - a fault would now be
  # NAMED by the clean-device check that follows every GPU test (tests/conftest.py).  CAREFUL: its one run hung in the 64th test of that order and sat there until gpurun's
  # limit (profiles/r05_reader_fault_old_behaviour_AB_run_hung.txt) - run it with a short --timeout; the per-test watchdog of tests/conftest.py (15 min) did not exist yet
  export SVX_COPY_DIRECT=1 SVX_BAM_DEV_MAPFILE=1 SVX_READER_REGISTER=1 SVX_TEST_ORDER=collection AMD_LOG_LEVEL=1
  for k in $(seq 1 ${REPEAT:-2}); do
    timeout 1500 python -m pytest tests/ -x -q -m gpu --deselect tests/test_gpu_reader_stress.py > $out/${tag}_oldway_$k.txt 2>&1
    echo "old-way suite run $k: rc=$? $(tail -1 $out/${tag}_oldway_$k.txt)"
  done
  ;;
suite)
  for k in $(seq 1 ${REPEAT:-1}); do
    timeout 1500 python -m pytest tests/ -x -q -m gpu --durations=8 > $out/${tag}_pytest_$k.txt 2>&1
    echo "suite run $k: rc=$? $(tail -1 $out/${tag}_pytest_$k.txt)"
  done
  ;;
probe2)
  B=tools/micro/fault_probe.bin
  TL=$(python -c "import torch,os;print(os.path.join(os.path.dirname(torch.__file__),'lib'))")
  {
    for rt in torch rocm; do
      echo "=== HIP runtime: $rt"
      for how in sync event query none; do for where in null other same; do
        for sl in 20000 0; do
          if [ $rt = torch ]; then LD_LIBRARY_PATH=$TL timeout 120 $B cross_${how}_${where} 1239008 $sl 30 2>&1 | tail -1; else timeout 120 $B cross_${how}_${where} 1239008 $sl 30 2>&1 | tail -1; fi
        done
      done; done
    done
  } > $out/${tag}_fault_probe2.txt 2>&1
  cat $out/${tag}_fault_probe2.txt
  ;;
guard)
  # SVX_ALLOC_GUARD=1: every device buffer ends at the end of its own mapping (unmapped space behind it) - an overrun of a kernel is a fault at once.
  # Groups run in separate processes (a fault is sticky); the first failing test of a group is run again with the runtime's launch log, serialised,
  # so that the LAST kernel named in the log is the one that faulted.
  export SVX_ALLOC_GUARD=1
  declare -A G
  G[reader]="device_bam or queryname or device_batches or long_cigar or foreign"
  G[readerpipe]="bam_path or through_bam or bam_pipeline or bench_harness or gpu_inflate or bgzf"
  G[collect]="cigar_indel or collect_golden or dropin or per_read or resident or g6_ or genotype"
  G[cluster]="cluster_golden or sampling or partition or linkage or cluster_scheduling or combine or writers or radix"
  G[edit]="edit_distance"
  G[exchange]="rank_exchange or multigpu_step"
  G[workloads]="c2_hifi or c4_clr"
  for g in ${GROUPS_TO_RUN:-reader readerpipe collect cluster edit exchange workloads}; do
    f=$out/${tag}_guard_$g.txt
    timeout 900 python -m pytest tests/ -x -q -m gpu -k "${G[$g]}" > $f 2>&1
    echo "guard group $g: rc=$? $(tail -1 $f)"
    bad=$(grep -m1 "^FAILED" $f | awk '{print $2}')
    if [ -n "$bad" ]; then
      echo "  first failure: $bad -> again with the launch log"
      AMD_SERIALIZE_KERNEL=3 AMD_LOG_LEVEL=3 timeout 600 python -m pytest "$bad" -x -q -m gpu > $out/${tag}_guard_${g}_trace_full.txt 2>&1
      grep -a "ShaderName\\|illegal\\|fault\\|rror" $out/${tag}_guard_${g}_trace_full.txt | tail -60 | cut -c1-400 > $out/${tag}_guard_${g}_trace.txt
      rm -f $out/${tag}_guard_${g}_trace_full.txt
      tail -25 $out/${tag}_guard_${g}_trace.txt
    fi
  done
  ;;
tailrepro)
  # the tail of the suite in front of the test that faulted in GPUTEST_r04 (tests 85..99 of the driver's order), repeated: a cheap reproducer?
  K="bench_harness or bench_under_torchrun or bgzf_inflate or gpu_inflate or combine_consumers or writers_on_gpu or full_size_through or rank_exchange or two_ranks or test_device_bam_decode_equals_host_reader"
  for k in $(seq 1 ${REPEAT:-6}); do
    timeout 600 python -m pytest tests/ -x -q -m gpu -k "$K" > $out/${tag}_tail_$k.txt 2>&1
    echo "tail run $k: rc=$? $(tail -1 $out/${tag}_tail_$k.txt)"
  done
  ;;
evidence)
  export HSA_DISABLE_COREDUMP_ON_EXCEPTION=1; ulimit -c 0
  R=$PWD
  python bench.py --full --steps 20 --warmup 5 > $out/${tag}_bench_c1.json 2> $out/${tag}_bench_c1.err; echo "bench c1 rc=$?"
  B="--steps 4 --warmup 2 --no-cpu-baseline --no-end-to-end"
  rm -rf /tmp/kt && (cd /tmp && rocprofv3 --kernel-trace --stats -d /tmp/kt -o p -- python $R/bench.py $B > /dev/null 2> /tmp/kt.err)
  db=$(find /tmp/kt -name "*.db" | head -1)
  python tools/rocpd_stats.py $db $out/${tag}_kernel_stats.csv > /dev/null
  python tools/rocpd_timeline.py $db > $out/${tag}_step_timeline.txt
  for pass in "SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE" "SQ_ACTIVE_INST_VALU SQ_INSTS_SALU SQ_WAIT_INST_ANY SQ_WAIT_ANY" "FETCH_SIZE" "WRITE_SIZE"; do
    t=$(echo $pass | tr ' ' '_' | cut -c1-24)
    rm -rf /tmp/pmc_$t
    (cd /tmp && timeout 300 rocprofv3 --kernel-trace --pmc $pass -d /tmp/pmc_$t -o p -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-end-to-end > /dev/null 2> /tmp/pmc_$t.err)
    db=$(find /tmp/pmc_$t -name "*.db" | head -1)
    [ -n "$db" ] && python tools/pmc_summary.py $db $out/${tag}_pmc_$t.csv > /dev/null
  done
  python bench.py --full --steps 10 --warmup 3 --workload c2 --no-cpu-baseline > $out/${tag}_bench_c2.json 2>/dev/null
  for pmd in 1000 100000; do python bench.py --full --steps 5 --warmup 2 --workload c4 --partition-max-distance $pmd --no-cpu-baseline > $out/${tag}_bench_c4_pmd$pmd.json 2>/dev/null; done
  python bench.py --scaling strong --steps 5 --warmup 2 > $out/${tag}_bench_strong_1rank.json 2> $out/${tag}_bench_strong_1rank.err
  SVX_BENCH_BACKEND=gloo SVX_BENCH_ONE_GPU=1 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29577 bench.py --gpus 2 --scaling strong --steps 5 --warmup 2 > $out/${tag}_bench_strong_2ranks_one_gpu.json 2> $out/${tag}_bench_strong_2ranks_one_gpu.err
  python tools/device_reader_rate.py 180000 8192 2>&1 | grep -v "amdgpu.ids\|bamio pass\|   pass\|bamio 64" > $out/${tag}_device_reader_rate.txt
  SVX_BAM_DEV_MAPFILE=1 python tools/device_reader_rate.py 180000 8192 2>&1 | grep -v "amdgpu.ids\|bamio pass\|   pass\|bamio 64" > $out/${tag}_device_reader_rate_registered_file.txt
  python tools/small_batch_latency.py 2>&1 | grep -v amdgpu.ids > $out/${tag}_small_batch_latency.txt
  bash tools/host_probe.sh > $out/${tag}_host_probe.txt 2>&1
  git rev-parse HEAD > $out/${tag}_evidence_commit.txt 2>/dev/null || true
  ls -la $out/${tag}_* | head -40
  ;;
bench)
  python bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err; echo "bench rc=$?"; cut -c1-1500 $out/${tag}_bench.json
  ;;
*) echo "unknown step $step"; exit 2;;
esac
