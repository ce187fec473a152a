V=${1:-v7}
O=${2:-profile_runs/$V}   # output directory (relative to the repository root, or absolute)
export TMPDIR=/tmp
R=$PWD
mkdir -p $O && O=$(cd $O && pwd)
python bench.py --full > $O/bench.json 2> $O/bench.err
tail -c 600 $O/bench.json
(cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o $V -- python3 $R/bench.py --full --no-cpu-baseline > $O/stats.log 2>&1)
for c in FETCH_SIZE WRITE_SIZE; do (cd /tmp && rocprofv3 --pmc $c --kernel-trace --output-format csv -d $O/pmc_$c -o p -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/pmc_$c.log 2>&1); done
(cd /tmp && rocprofv3 --pmc SQ_INSTS_VALU GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $O/pmc_SQ_INSTS_VALU -o p -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/pmc_valu.log 2>&1)
find $O -name "*.csv" | head -20
