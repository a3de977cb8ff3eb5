# The round's profile set: (1) rocprofv3 --kernel-trace --stats of the default bench, (2) the bench JSON line of a --full
# run (with its in-run PMC traffic), (3) the PMC passes (tools/gpu_pmc.sh) folded into one summary.  Argument: tag.  Run
# from the repository root; output under $SLAM_PROFILE_OUT (default profile_out/).
tag=${1:-r02}
OUT=${SLAM_PROFILE_OUT:-profile_out}
export SLAM_PROFILE_OUT=$OUT
mkdir -p $OUT
bash tools/gpu_prof.sh $tag > $OUT/prof_$tag.sh.log 2>&1
timeout -k 10 500 python bench.py --full > $OUT/bench_$tag.json 2> $OUT/bench_$tag.err
echo "bench exit $?"
python tools/show_bench.py $OUT/bench_$tag.json
rm -rf $OUT/pmc
bash tools/gpu_pmc.sh > $OUT/pmc_$tag.log 2>&1
python tools/pmc_summary.py $OUT/pmc > $OUT/pmc_${tag}_summary.txt 2>&1
cut -c1-230 $OUT/pmc_${tag}_summary.txt | grep -E "downdate|pf_auto_step"
rm -rf $OUT/pmc                                   # (the raw counter files are large; the summary is what profiles/ keeps)
# the other configurations' bench lines (C2: 1k landmarks, 16 obs; C5: 50k landmarks, fp64, Joseph form, 8 obs)
timeout -k 10 300 python bench.py --full --landmarks 1000 --obs 16 --steps 200 --warmup 20 --no-fastslam > $OUT/bench_${tag}_c2.json 2>/dev/null
timeout -k 10 400 python bench.py --full --landmarks 50000 --obs 8 --dtype f64 --form joseph --steps 20 --warmup 3 --no-fastslam > $OUT/bench_${tag}_c5.json 2>/dev/null
python tools/show_bench.py $OUT/bench_${tag}_c2.json | head -4
python tools/show_bench.py $OUT/bench_${tag}_c5.json | head -4
