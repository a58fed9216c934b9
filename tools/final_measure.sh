# usage: bash tools/final_measure.sh <outdir>
export TMPDIR=/tmp
R=$PWD
O=$(realpath -m "${1:?usage: bash tools/final_measure.sh <outdir>}")
mkdir -p $O
timeout 500 python -m pytest tests -m gpu -q --no-header --timeout 300 -p no:cacheprovider 2>&1 | grep -vE "Extension modules" | tail -3 > $O/pytest.log
timeout 400 python bench.py --full > $O/bench.json 2> $O/bench.err
(cd /tmp && timeout 280 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o b -- python $R/bench.py --full --steps 3 --warmup 2 --no-cpu-baseline > $O/stats.log 2>&1)
cat $O/pytest.log; tail -c 600 $O/bench.json; find $O/stats -name "*kernel_stats.csv"
