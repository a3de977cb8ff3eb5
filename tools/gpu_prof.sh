# rocprofv3 kernel trace + stats of the bench (argument: profile tag; the rest goes to bench.py).  Run from the repository
# root; the summary lands in $SLAM_PROFILE_OUT (default profile_out/)/prof_<tag>_stats.csv.
tag=${1:-r02}
shift
ROOT=$(pwd)
OUT=$(realpath -m ${SLAM_PROFILE_OUT:-profile_out})
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$tag -o bench -- python3 $ROOT/bench.py --full --no-cpu-baseline --no-pmc --no-configs "$@" > $OUT/prof_$tag.log 2>&1
echo "rocprof exit $?"
f=$(find $OUT/prof_$tag -name '*kernel_stats.csv' | head -1)
cp "$f" $OUT/prof_${tag}_stats.csv
rm -rf $OUT/prof_$tag          # (the raw trace is large; the stats are what profiles/ keeps)
cut -c1-150 $OUT/prof_${tag}_stats.csv | head -30
tail -c 3000 $OUT/prof_$tag.log | grep -o '"regimes".*"weak_scaling"' | head -3
