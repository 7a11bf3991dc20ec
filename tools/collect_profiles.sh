#!/bin/bash
# GPU box: the round's committed measurements.  Writes under $OUT (default out/; copy into profiles/ afterwards).
# usage: bash tools/collect_profiles.sh <tag>
set -e
tag=${1:-r1}
part=${2:-all}      # core | workloads | all (two gpurun calls when the whole list does not fit one call's time limit)
cd /root/repo; export TMPDIR=/tmp
out=${OUT:-out}; mkdir -p $out
if [ "$part" != "workloads" ]; then
python3 bench.py --full > $out/${tag}_bench_default.json 2> $out/${tag}_bench_default.err
rocprofv3 --kernel-trace --stats -d $out/prof_${tag}_w -- python3 bench.py --full --steps 3 --warmup 2 --no-cpu-baseline > $out/prof_${tag}_w.log 2>&1
python3 tools/prof_summary.py $(ls $out/prof_${tag}_w/*/*.db | head -1) $out/${tag}_w_bench_kernel_stats.csv 8 > $out/prof_${tag}_w.txt
python3 tools/collect_traffic.py ${tag} > $out/${tag}_traffic.log 2>&1
rm -rf $out/prof_${tag}_w $out/pmc_${tag}_FETCH_SIZE $out/pmc_${tag}_WRITE_SIZE
OCTSEG_PROFILE_DUMP=$out/${tag}_layers_alone.csv python3 bench.py --full --steps 4 --warmup 2 --no-cpu-baseline > /dev/null 2>&1
python3 tools/group_layers.py $out/${tag}_layers_alone.csv 2 > $out/${tag}_layer_groups.txt
python3 bench.py --full --workload ensemble_704_fp16 --steps 30 > $out/${tag}_ensemble_b1.json 2> /dev/null
python3 bench.py --full --workload ensemble_704_fp16 --steps 20 --batch 8 > $out/${tag}_ensemble_b8.json 2> /dev/null
fi
if [ "$part" != "core" ]; then
for w in linknet_r50_704 unet_r50_704 fpn_r50_704 deeplabv3plus_r50_704 pspnet_r50_704 deeplabv3_r50_704 manet_r50_704 pan_r50_704 unet_regnetx064_704 unet_regnety120_704 \
         fpn_regnetx002_704 unet_effb0_704 fpn_effb5_704; do
  OCTSEG_PROFILE_DUMP=$out/${tag}_layers_$w.csv python3 bench.py --full --workload $w --steps 10 --warmup 3 --no-cpu-baseline > $out/${tag}_bench_$w.json 2> /dev/null
  python3 tools/group_layers.py $out/${tag}_layers_$w.csv 2 > $out/${tag}_layer_groups_$w.txt; rm -f $out/${tag}_layers_$w.csv
done
for b in 2 4; do python3 bench.py --full --batch $b --steps 20 --warmup 5 --no-cpu-baseline > $out/${tag}_bench_batch$b.json 2> /dev/null; done
python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --force-exchange > $out/${tag}_bench_force_exchange.json 2> /dev/null
python3 bench.py --full --batch 2 --steps 20 --warmup 5 --no-cpu-baseline --train-graph > $out/${tag}_bench_batch2_train_graph.json 2> /dev/null
tail -c 600 $out/${tag}_bench_default.err
fi
